"""Time the read-mapping layer (csrc/fmmap.hip) on a benchmark workload; prints one JSON line and writes it to --out (default
profiles/map_time.json).

    python tools/map_time.py [--workload c3] [--reads 1000000] [--len 150] [--reps 3] [--seed-len 20] [--k 8] [--records 64] [--out FILE]

The text, the index and the reads are tools/extend_time.py's: --reads reads of --len bytes drawn from the text with about 2 %
substituted bytes and 0.5 % indels; every second read is then replaced by its reverse complement, so both strands are asked.  The
text is cut into --records records of equal length for the sequence table.  In the same process, warm, the minimum of --reps
timed calls each:
  map      pfp_fm_map_dev with every output (max_sec = 0)
  align    pfp_fm_align_dev with its outputs on the 2 x reads interleaved patterns (read, reverse complement) - what the mapper
           runs inside
  cigar    pfp_fm_cigar_dev with the runs over ALL of those alignments (the mapper asks it for the returned hits only, which is
           why the layer can cost less than nothing next to this sum)
The figure: layer = map - (align + cigar), in ms and as a fraction of align + cigar.  From one more map call under the kernel
trace (not timed) the time of the layer's own kernels: strands (reverse complement), inside, shadow, select, hits and md; the
library's segmented sorts are a row of their own, which also holds the sorts of the alignment step."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as entry  # noqa: E402
from extend_time import sample_reads, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed-len", type=int, default=20)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_time.json"))
    a = ap.parse_args()
    import numpy as np
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
    npat, m, k = a.reads, a.len, a.k
    out = {"tool": "map_time", "workload": a.workload, "n": n, "reads": npat, "read_len": m, "reps": a.reps, "records": a.records,
           "planted": "2 % substitutions, 0.5 % indels, every second read reverse-complemented", "min_seed": a.seed_len, "k": k}
    with pkg.Context(0) as c:
        fm = c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr())
        for ptr, _ in outs.values():
            b.dev_free(ptr)
        b.close()
        fm.set_sequences(np.linspace(0, n, a.records + 1).astype(np.uint64))
        pat, off, _, edits = sample_reads(torch, text, npat, m, seed=m)
        out["mean_edits_per_read"] = round(float(edits.to(torch.float64).mean()), 3)
        # the reverse complement of every read, by a table: the timed calls' own input, not the feature
        comp = torch.arange(256, dtype=torch.uint8, device=dev)
        for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
            comp[x] = y
        fw = pat.reshape(npat, m)
        rc = comp[fw.flip(1).to(torch.int64)]
        reads = torch.where((torch.arange(npat, device=dev) % 2 == 1)[:, None], rc, fw).contiguous()
        both = torch.stack([reads, comp[reads.flip(1).to(torch.int64)]], 1).reshape(-1).contiguous()      # 2p = read p, 2p + 1 = its reverse complement
        off2 = torch.arange(0, 2 * npat * m + 1, m, dtype=torch.int64, device=dev)
        reads = reads.reshape(-1)
        z = lambda cnt, dt=torch.int64: torch.zeros(cnt, dtype=dt, device=dev)
        hoff, mapq, nh = z(npat + 1), z(npat, torch.uint8), z(npat)
        torch.cuda.synchronize()
        P, O, P2, O2 = reads.data_ptr(), off.data_ptr(), both.data_ptr(), off2.data_ptr()
        fm.map_reads_dev(P, O, npat, k, a.seed_len, hoff.data_ptr(), mapq.data_ptr(), nh.data_ptr())
        H = int(hoff[-1])
        strand, dist, seq = z(H + 1, torch.uint8), z(H + 1, torch.uint8), z(H + 1, torch.int32)
        soff, start, coff, moff = z(H + 1), z(H + 1), z(H + 2), z(H + 2)
        torch.cuda.synchronize()

        def map_call():
            d_cig, d_md = fm.map_reads_dev(P, O, npat, k, a.seed_len, hoff.data_ptr(), mapq.data_ptr(), nh.data_ptr(), strand.data_ptr(), seq.data_ptr(),
                                           soff.data_ptr(), start.data_ptr(), dist.data_ptr(), coff.data_ptr(), moff.data_ptr())
            for p in (d_cig, d_md):
                if p:
                    c.dev_free(p)
        s_map = timed(torch, map_call, a.reps)
        c.set_kernel_trace(True)
        map_call()
        by = {r["name"]: (r["total_ms"], r["launches"]) for r in c.kernel_trace()}
        c.set_kernel_trace(False)
        # the two existing calls on the same patterns
        aoff = z(2 * npat + 1)
        fm.align_dev(P2, O2, 2 * npat, k, a.seed_len, aoff.data_ptr())
        A = int(aoff[-1])
        st, en, di = z(A + 1), z(A + 1), z(A + 1, torch.uint8)
        torch.cuda.synchronize()
        s_align = timed(torch, lambda: fm.align_dev(P2, O2, 2 * npat, k, a.seed_len, aoff.data_ptr(), st.data_ptr(), en.data_ptr(), di.data_ptr()), a.reps)
        ap_ = torch.repeat_interleave(torch.arange(2 * npat, dtype=torch.int32, device=dev), aoff[1:] - aoff[:-1])
        cdist, acoff = z(A + 1, torch.uint8), z(A + 1)
        torch.cuda.synchronize()
        fm.cigar_dev(P2, O2, 2 * npat, ap_.data_ptr(), st.data_ptr(), en.data_ptr(), A, k, cdist.data_ptr(), acoff.data_ptr())
        cig = z(int(acoff[A]) + 1, torch.int32)
        torch.cuda.synchronize()
        s_cigar = timed(torch, lambda: fm.cigar_dev(P2, O2, 2 * npat, ap_.data_ptr(), st.data_ptr(), en.data_ptr(), A, k, cdist.data_ptr(),
                                                    acoff.data_ptr(), cig.data_ptr()), a.reps)
        ms = lambda name: round(by.get(name, (0, 0))[0], 2)
        base = s_align + s_cigar
        out.update({"alignments_of_both_strands": A, "hits_returned": H, "reads_mapped": int((nh > 0).sum()),
                    "reads_on_their_planted_strand": int(((strand[hoff[:-1].clamp(max=max(H - 1, 0))] == (torch.arange(npat, device=dev) % 2)) & (nh > 0)).sum()),
                    "mapq_60": int((mapq == 60).sum()), "mapq_0_mapped": int(((mapq == 0) & (nh > 0)).sum()),
                    "map_ms": round(s_map * 1e3, 2), "align_ms": round(s_align * 1e3, 2), "cigar_all_alignments_ms": round(s_cigar * 1e3, 2),
                    "layer_ms": round((s_map - base) * 1e3, 2), "layer_over_align_plus_cigar": round((s_map - base) / base, 4),
                    "kernel_ms": {"strands": ms("fm_map_strands"), "inside": ms("fm_map_inside"), "shadow": ms("fm_map_shadow"),
                                  "select": ms("fm_map_select"), "hits": ms("fm_map_hits"), "md": ms("fm_map_md"),
                                  "cigar_of_the_hits": round(ms("fm_cigar_plan") + ms("fm_cigar") + ms("fm_cigar_place"), 2),
                                  "segmented_sorts_of_the_whole_call": ms("rocprim::segmented_radix_sort_pairs<u64,u32>")},
                    "reads_per_s": round(npat / s_map)})
        fm.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
