"""Time seed-and-extend (csrc/fmextend.hip) on a benchmark workload; prints one JSON line and writes it to --out (default
profiles/extend_time.json).

    python tools/extend_time.py [--workload c3] [--reads 1000000] [--len 150] [--reps 3] [--k 8] [--seed-len 20] [--ks 0,2,8,32] [--out FILE]

The workload's text (big-bwt_amd/synth.py) and its .bwt / .ssa / .esa (-s -e) are built on the device, then, on a context of its
own, an index with text and thresholds, and --reads reads of --len bytes drawn from the text with about 2 % substituted bytes and
0.5 % indels (half insertions, half deletions).  In the same process, warm, the minimum of --reps timed calls each:
  mems     pfp_fm_ms_dev + pfp_fm_mems_dev (offsets, then the triples) alone, with PHONI
  align    pfp_fm_align_dev with its outputs, at k = --k and min_seed = --seed-len, with PHONI and with thresholds; from one more
           call under the kernel trace (not timed) the time per phase: ms (every kernel of the matching statistics), mems, seeds
           (candidates, their sort and the distinct diagonals), extend, sort (keys, their sort, cap and scatter)
  extend   pfp_fm_extend_dev alone on the reads' true diagonals, for every k of --ks
Rates: candidates/s = distinct diagonals extended per second of the extend phase (or of the extend call); cell updates/s counts
the cells the kernel updates: per candidate m rows of 16 * CPL cells forward, and as many backward where it aligned (CPL = 1, 2,
3, 6, 11 cells per lane for k <= 3, 6, 9, 19, 32); k = 0 is a compare and has none."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def band_cells(k):
    w = 5 * k + 1
    return 0 if k == 0 else 16 * (1 if w <= 16 else 2 if w <= 32 else 3 if w <= 48 else 6 if w <= 96 else 11)


def sample_reads(torch, text, nreads, m, seed, sub=0.02, indel=0.005):
    """nreads reads of m bytes: windows of the text copied byte by byte, where an output byte is a random base instead of the next
    source byte (insertion) or a source byte is skipped first (deletion), each with probability indel / 2, then substitutions"""
    dev = text.device
    n = text.numel()
    g = torch.Generator(device="cpu").manual_seed(seed)
    pad = 32
    start = torch.randint(0, n - m - pad, (nreads,), generator=g).to(dev)
    u = torch.rand((nreads, m), generator=g).to(dev)
    ins = u < indel / 2
    dele = (u >= indel / 2) & (u < indel)
    src = torch.cumsum((~ins).to(torch.int64), 1) - (~ins).to(torch.int64) + torch.cumsum(dele.to(torch.int64), 1)
    src = torch.clamp(src, max=m + pad - 1)
    P = text[start[:, None] + src]
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
    r4 = torch.randint(0, 4, (nreads, m), generator=g).to(dev)
    rnd = acgt[r4]
    P = torch.where(ins, rnd, P)
    subs = torch.rand((nreads, m), generator=g).to(dev) < sub
    P = torch.where(subs, torch.where(P == rnd, acgt[(r4 + 1) % 4], rnd), P)      # (another base than the one that stands there)
    off = torch.arange(0, nreads * m + 1, m, dtype=torch.int64, device=dev)
    edits = (ins | dele | subs).sum(1)
    return P.reshape(-1).contiguous(), off, start, edits


def timed(torch, call, reps):
    times = []
    for r in range(reps + 1):          # the first call warms up
        torch.cuda.synchronize()
        t0 = time.time()
        call()
        if r:
            times.append(time.time() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--seed-len", type=int, default=20)
    ap.add_argument("--ks", default="0,2,8,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extend_time.json"))
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    synth = __import__("bigbwt_amd.synth", fromlist=["x"])
    dev = torch.device("cuda", 0)
    cfg = synth.WORKLOADS[a.workload]
    text = synth.workload_text_torch(dev, a.workload)
    n = text.numel()
    bwt = torch.empty(n + 17, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()            # (the library works on a stream of its own: torch's writes must be done)
    b = pkg.Context(0)
    used, outs = b.bigbwt_formats_dev(text.data_ptr(), n, bwt.data_ptr(), cfg["w"], cfg["p"], pkg.FLAG_SSA | pkg.FLAG_ESA)
    assert used == n
    (ssa, ssa_b), (esa, esa_b) = outs["ssa"], outs["esa"]
    npat, m = a.reads, a.len
    out = {"tool": "extend_time", "workload": a.workload, "n": n, "reads": npat, "read_len": m, "reps": a.reps,
           "planted": "2 % substitutions, 0.5 % indels", "align": {}, "extend": {}}
    with pkg.Context(0) as c:
        fm = c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr())
        for ptr, _ in outs.values():
            b.dev_free(ptr)
        b.close()
        fm.add_thresholds()
        pat, off, start, edits = sample_reads(torch, text, npat, m, seed=m)
        out["mean_edits_per_read"] = round(float(edits.to(torch.float64).mean()), 3)
        z = lambda cnt, dt=torch.int64: torch.zeros(cnt, dtype=dt, device=dev)
        ln, pos, moff, aoff = z(npat * m + 1, torch.int32), z(npat * m + 1), z(npat + 1), z(npat + 1)
        torch.cuda.synchronize()
        P, O = pat.data_ptr(), off.data_ptr()

        # MEMs alone
        def mems_sizes():
            fm.matching_statistics_dev(P, O, npat, ln.data_ptr(), pos.data_ptr())
            fm.mems_dev(O, npat, ln.data_ptr(), pos.data_ptr(), a.seed_len, moff.data_ptr())
        mems_sizes()
        M = int(moff[-1])
        mem = z(3 * M + 1)
        torch.cuda.synchronize()

        def mems():
            mems_sizes()
            fm.mems_dev(O, npat, ln.data_ptr(), pos.data_ptr(), a.seed_len, moff.data_ptr(), mem.data_ptr())
        s = timed(torch, mems, a.reps)
        tri = mem[:3 * M].reshape(M, 3)
        owner = torch.repeat_interleave(torch.arange(npat, device=dev), moff[1:] - moff[:-1])
        distinct = int(torch.unique(torch.stack([owner, tri[:, 2] - tri[:, 0]], 1), dim=0).shape[0])
        out["mems"] = {"ms": round(s * 1e3, 2), "mems": M, "distinct_diagonals": distinct, "reads_per_s": round(npat / s)}
        del mem, tri, owner

        cells = band_cells(a.k)
        for label, thr in (("phoni", False), ("thresholds", True)):
            fm.align_dev(P, O, npat, a.k, a.seed_len, aoff.data_ptr(), thresholds=thr)
            A = int(aoff[-1])
            st, en, di = z(A + 1), z(A + 1), z(A + 1, torch.uint8)
            torch.cuda.synchronize()
            call = lambda: fm.align_dev(P, O, npat, a.k, a.seed_len, aoff.data_ptr(), st.data_ptr(), en.data_ptr(), di.data_ptr(), thresholds=thr)
            s = timed(torch, call, a.reps)
            c.set_kernel_trace(True)
            call()
            rows = c.kernel_trace()
            c.set_kernel_trace(False)
            by = {r["name"]: r["total_ms"] for r in rows}
            own = ("fm_mems", "fm_align_seeds", "fm_extend", "fm_align_sort")
            phase = {"ms": round(sum(v for k_, v in by.items() if k_.startswith("fm_") and k_ not in own), 2), "mems": round(by.get("fm_mems", 0), 2),
                     "seeds": round(by.get("fm_align_seeds", 0), 2), "extend": round(by.get("fm_extend", 0), 2),
                     "sort": round(by.get("fm_align_sort", 0), 2)}
            aligned = int((aoff[1:] > aoff[:-1]).sum())
            at_home = int((torch.repeat_interleave(start, aoff[1:] - aoff[:-1]) - st[:A]).abs().le(a.k).sum())
            ext_s = max(phase["extend"], 1e-6) / 1e3
            out["align"][label] = {"k": a.k, "min_seed": a.seed_len, "ms": round(s * 1e3, 2), "reads_per_s": round(npat / s), "alignments": A,
                                   "reads_aligned": aligned, "alignments_near_true_start": at_home, "phase_ms": phase,
                                   "candidates_per_s": round(distinct / ext_s) if not thr else None,
                                   "cell_updates_per_s_at_least": round(distinct * m * cells / ext_s) if not thr else None}
            del st, en, di

        # the kernel alone, on the true diagonals
        cp = torch.arange(npat, dtype=torch.int32, device=dev)
        cd = start.clone()
        st, en, di = z(npat), z(npat), z(npat, torch.uint8)
        torch.cuda.synchronize()
        for k in (int(x) for x in a.ks.split(",")):
            call = lambda: fm.extend_dev(P, O, npat, cp.data_ptr(), cd.data_ptr(), npat, k, di.data_ptr(), st.data_ptr(), en.data_ptr())
            s = timed(torch, call, a.reps)
            hit = int((di != 0xFF).sum())
            out["extend"][str(k)] = {"ms": round(s * 1e3, 2), "aligned": hit, "candidates_per_s": round(npat / s),
                                     "cell_updates_per_s": round((npat + hit) * m * band_cells(k) / s)}
        fm.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
