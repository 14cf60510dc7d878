"""Time long-read mapping by chaining (csrc/fmchain.hip) on a benchmark workload; prints one JSON line and writes it to --out
(default profiles/chain_time.json).

    python tools/chain_time.py [--workload c3] [--reads 100000] [--len 10000] [--batch 2000] [--seed-len 20] [--max-occ 500]
                               [--gap 5000] [--band 500] [--min-score 40] [--records 64] [--out FILE]

The text and the index are tools/extend_time.py's (c3 is BASELINE configs[2]: 64 mutated copies of a yeast-shaped genome), cut
into --records records of equal length.  --reads reads of --len bytes are drawn from it with 1 % substituted bytes and 0.2 %
indels (extend_time.sample_reads); every second one is replaced by its reverse complement, so both strands are asked.  A read of
10 kb brings some ten thousand anchors per strand on this text, so the reads go through pfp_fm_map_long_dev in batches of --batch
(the host call cuts its groups by the same budget rule).  The first batch runs once untimed; then every batch runs once under
the kernel trace, and the rows are summed into the split of the call:
  matching statistics (fm_ms), MEM count (fm_mems, the spans, fm_count), locate (the plan, the expansion and the phi^-1 chains),
  sort (the three segmented sorts of a call with the key, count and write kernels around them, and the strand merge), programme
  (fm_chain_dp) and peel (fm_chain_peel),
next to the wall time of the calls, anchors per second (of the call, and of the programme alone) and predecessor evaluations per
second: 64 per anchor over the programme's time."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as entry  # noqa: E402
from extend_time import sample_reads  # noqa: E402

SPLIT = {"matching_statistics": ("fm_ms",), "mem_count": ("fm_mems", "fm_anchor_spans", "fm_count"), "locate": ("fm_anchor_locate",),
         "sort": ("fm_anchor_sort", "fm_chain_sort", "fm_chain_write", "fm_long_select", "fm_long_hits"), "programme": ("fm_chain_dp",),
         "peel": ("fm_chain_peel",), "strands": ("fm_map_strands",)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--len", type=int, default=10_000)
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--seed-len", type=int, default=20)
    ap.add_argument("--max-occ", type=int, default=500)
    ap.add_argument("--gap", type=int, default=5000)
    ap.add_argument("--band", type=int, default=500)
    ap.add_argument("--min-score", type=int, default=40)
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_time.json"))
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
    m = a.len
    out = {"tool": "chain_time", "workload": a.workload, "n": n, "reads": a.reads, "read_len": m, "batch": a.batch, "records": a.records,
           "planted": "1 % substitutions, 0.2 % indels, every second read reverse-complemented", "min_seed": a.seed_len,
           "max_occ": a.max_occ, "max_gap": a.gap, "band": a.band, "min_score": a.min_score}
    comp = torch.arange(256, dtype=torch.uint8, device=dev)
    for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
        comp[x] = y
    with pkg.Context(0) as c:
        fm = c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr())
        for ptr, _ in outs.values():
            b.dev_free(ptr)
        b.close()
        fm.set_sequences(np.linspace(0, n, a.records + 1).astype(np.uint64))
        z = lambda cnt, dt=torch.int64: torch.zeros(cnt, dtype=dt, device=dev)
        wall, anchors, chains, mapped, on_strand, mapq60 = 0.0, 0, 0, 0, 0, 0
        by = {}
        done, first = 0, True
        while done < a.reads:
            k = min(a.batch, a.reads - done)
            pat, off, _, _ = sample_reads(torch, text, k, m, seed=m + done, sub=0.01, indel=0.002)
            fw = pat.reshape(k, m)
            odd = ((torch.arange(k, device=dev) + done) % 2 == 1)
            reads = torch.where(odd[:, None], comp[fw.flip(1).to(torch.int64)], fw).contiguous().reshape(-1)
            hoff, mapq, nc = z(k + 1), z(k, torch.uint8), z(k)
            outs_ = [z(k, torch.uint8), z(k, torch.int32)] + [z(k) for _ in range(3)] + [z(k, torch.int32) for _ in range(5)]
            aoff = z(k + 1)
            torch.cuda.synchronize()
            call = lambda: fm.map_long_dev(reads.data_ptr(), off.data_ptr(), k, a.seed_len, hoff.data_ptr(), mapq.data_ptr(), nc.data_ptr(),
                                           *[t.data_ptr() for t in outs_], max_occ=a.max_occ, max_gap=a.gap, band=a.band,
                                           min_score=a.min_score, max_sec=0)
            if first:
                call()                                      # warms up
                first = False
            c.set_kernel_trace(True)
            torch.cuda.synchronize()
            t0 = time.time()
            call()
            wall += time.time() - t0
            for r in c.kernel_trace():
                t, l = by.get(r["name"], (0.0, 0))
                by[r["name"]] = (t + r["total_ms"], l + r["launches"])
            c.set_kernel_trace(False)
            # the anchors the call chained, counted apart: those of the reads as given and of their reverse complements
            other = comp[reads.reshape(k, m).flip(1).to(torch.int64)].contiguous().reshape(-1)
            torch.cuda.synchronize()
            for strand in (reads, other):
                fm.anchors_dev(strand.data_ptr(), off.data_ptr(), k, a.seed_len, aoff.data_ptr(), max_occ=a.max_occ)
                anchors += int(aoff[-1])
            chains += int(nc.sum())
            mapped += int((nc > 0).sum())
            on_strand += int(((outs_[0] == odd.to(torch.uint8)) & (nc > 0)).sum())
            mapq60 += int((mapq == 60).sum())
            done += k
            del pat, off, fw, reads, other, hoff, mapq, nc, outs_, aoff
        ms = {key: round(sum(by.get(nm, (0.0, 0))[0] for nm in names), 2) for key, names in SPLIT.items()}
        launches = {key: sum(by.get(nm, (0.0, 0))[1] for nm in names) for key, names in SPLIT.items()}
        prog = max(ms["programme"], 1e-9) / 1e3
        out.update({"call_ms": round(wall * 1e3, 2), "kernel_ms": ms, "launches": launches, "anchors_both_strands": anchors,
                    "chains": chains, "reads_mapped": mapped, "reads_on_their_planted_strand": on_strand, "mapq_60": mapq60,
                    "reads_per_s": round(a.reads / wall), "anchors_per_s": round(anchors / wall),
                    "anchors_per_s_of_the_programme": round(anchors / prog),
                    "predecessor_evaluations_per_s": round(64 * anchors / prog)})
        fm.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
