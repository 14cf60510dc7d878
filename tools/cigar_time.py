"""Time the edit scripts (csrc/fmcigar.hip) on a benchmark workload; prints one JSON line and writes it to --out (default
profiles/cigar_time.json).

    python tools/cigar_time.py [--workload c3] [--reads 1000000] [--len 150] [--reps 3] [--seed-len 20] [--ks 8,32] [--out FILE]

The text, the index and the reads are tools/extend_time.py's: --reads reads of --len bytes drawn from the text with about 2 %
substituted bytes and 0.5 % indels.  For every k of --ks, in the same process, warm, the minimum of --reps timed calls each:
  align    pfp_fm_align_dev with its outputs (PHONI, min_seed = --seed-len): it finds the alignments (pattern, start, end)
  cigar    pfp_fm_cigar_dev over those alignments, offsets only and with the runs; from one more call under the kernel trace (not
           timed) the time of the pass with its walk (fm_cigar), of sizing the records (fm_cigar_plan) and of placing the runs
  extend   pfp_fm_extend_dev at the same k on the same candidates - every alignment's pattern along the diagonal of its start -
           as the yardstick: the ratio cigar / extend says what the script costs next to finding the alignment
Rates: alignments/s of the cigar call with the runs; cell updates/s counts m rows of 16 * CPL cells per alignment (CPL = 1, 2, 3, 5
cells per lane for k <= 7, 15, 23, 32)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as entry  # noqa: E402
from extend_time import sample_reads, timed  # noqa: E402


def band_cells(k):
    w = 2 * k + 1
    return 0 if k == 0 else 16 * (1 if w <= 16 else 2 if w <= 32 else 3 if w <= 48 else 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed-len", type=int, default=20)
    ap.add_argument("--ks", default="8,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cigar_time.json"))
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
    out = {"tool": "cigar_time", "workload": a.workload, "n": n, "reads": npat, "read_len": m, "reps": a.reps,
           "planted": "2 % substitutions, 0.5 % indels", "min_seed": a.seed_len, "k": {}}
    with pkg.Context(0) as c:
        fm = c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr())
        for ptr, _ in outs.values():
            b.dev_free(ptr)
        b.close()
        pat, off, start, edits = sample_reads(torch, text, npat, m, seed=m)
        out["mean_edits_per_read"] = round(float(edits.to(torch.float64).mean()), 3)
        z = lambda cnt, dt=torch.int64: torch.zeros(cnt, dtype=dt, device=dev)
        aoff = z(npat + 1)
        torch.cuda.synchronize()
        P, O = pat.data_ptr(), off.data_ptr()
        for k in (int(x) for x in a.ks.split(",")):
            fm.align_dev(P, O, npat, k, a.seed_len, aoff.data_ptr())
            A = int(aoff[-1])
            st, en, di = z(A + 1), z(A + 1), z(A + 1, torch.uint8)
            torch.cuda.synchronize()
            s_align = timed(torch, lambda: fm.align_dev(P, O, npat, k, a.seed_len, aoff.data_ptr(), st.data_ptr(), en.data_ptr(), di.data_ptr()), a.reps)
            ap_ = torch.repeat_interleave(torch.arange(npat, dtype=torch.int32, device=dev), aoff[1:] - aoff[:-1])
            cdist, coff = z(A + 1, torch.uint8), z(A + 1)
            torch.cuda.synchronize()
            sizes = lambda: fm.cigar_dev(P, O, npat, ap_.data_ptr(), st.data_ptr(), en.data_ptr(), A, k, cdist.data_ptr(), coff.data_ptr())
            s_sizes = timed(torch, sizes, a.reps)
            R = int(coff[A])
            cig = z(R + 1, torch.int32)
            torch.cuda.synchronize()
            fill = lambda: fm.cigar_dev(P, O, npat, ap_.data_ptr(), st.data_ptr(), en.data_ptr(), A, k, cdist.data_ptr(), coff.data_ptr(), cig.data_ptr())
            s_fill = timed(torch, fill, a.reps)
            c.set_kernel_trace(True)
            fill()
            by = {r["name"]: (r["total_ms"], r["launches"]) for r in c.kernel_trace()}
            c.set_kernel_trace(False)
            assert bool((cdist[:A] == di[:A]).all()), "the scripts' costs differ from the alignments' distances"
            # the yardstick: one extension per alignment, its pattern along the diagonal of its start
            ed, es, ee = z(A + 1, torch.uint8), z(A + 1), z(A + 1)
            torch.cuda.synchronize()
            s_ext = timed(torch, lambda: fm.extend_dev(P, O, npat, ap_.data_ptr(), st.data_ptr(), A, k, ed.data_ptr(), es.data_ptr(), ee.data_ptr()), a.reps)
            ms = lambda name: round(by.get(name, (0, 0))[0], 2)
            out["k"][str(k)] = {"alignments": A, "runs": R, "mean_distance": round(float(di[:A].to(torch.float64).mean()), 3) if A else None,
                                "align_ms": round(s_align * 1e3, 2), "cigar_offsets_only_ms": round(s_sizes * 1e3, 2), "cigar_ms": round(s_fill * 1e3, 2),
                                "extend_ms": round(s_ext * 1e3, 2), "cigar_over_extend": round(s_fill / s_ext, 2),
                                "phase_ms": {"plan": ms("fm_cigar_plan"), "pass_and_walk": ms("fm_cigar"), "place": ms("fm_cigar_place")},
                                "launches": by.get("fm_cigar", (0, 0))[1], "alignments_per_s": round(A / s_fill),
                                "cell_updates_per_s": round(A * m * band_cells(k) / s_fill)}
            del st, en, di, ap_, cdist, coff, cig, ed, es, ee
        fm.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
