"""Time the base-level alignment of chains (csrc/fmfill.hip) on the workload of tools/chain_time.py; prints one JSON line and writes
it to --out (default profiles/fill_time.json).

    python tools/fill_time.py [--workload c3] [--reads 100000] [--len 10000] [--batch 2000] [--seed-len 20] [--max-occ 500]
                              [--gap 5000] [--band 500] [--min-score 40] [--fill 500] [--records 64] [--out FILE]

The text, the index and the reads are chain_time.py's: --reads reads of --len bytes with 1 % substituted bytes and 0.2 % indels,
every second one reverse-complemented, in batches of --batch.  Per batch, in one process: pfp_fm_map_long_aln_dev once without the
runs, untimed, under PFP_FM_MS_STATS=1 - it sizes the runs and counts the gaps (pfp_fm_fill_stats); then pfp_fm_map_long_dev and
pfp_fm_map_long_aln_dev with the runs, each once under the wall clock, the second also under the kernel trace.  Reported: both
calls' wall time and what alignment adds; the gap kernel alone by band width (fm_fill_16 .. fm_fill_4160: launches, time, the gaps
that went through a pass of that width, gaps/s and cell updates/s - a pass that stops early counts all its cells); the share of
trivial gaps; the other passes (plan, members, gaps, stitch); and edits, unfilled gaps and runs of the primary chains."""
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

OTHER = {"plan": ("fm_fill_plan",), "members": ("fm_aln_members",), "gaps": ("fm_aln_gaps",), "stitch": ("fm_aln_stitch",)}


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
    ap.add_argument("--fill", type=int, default=500)
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_time.json"))
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
    out = {"tool": "fill_time", "workload": a.workload, "n": n, "reads": a.reads, "read_len": m, "batch": a.batch, "records": a.records,
           "planted": "1 % substitutions, 0.2 % indels, every second read reverse-complemented", "min_seed": a.seed_len,
           "max_occ": a.max_occ, "max_gap": a.gap, "band": a.band, "min_score": a.min_score, "max_fill": a.fill}
    comp = torch.arange(256, dtype=torch.uint8, device=dev)
    for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
        comp[x] = y
    os.environ.pop("PFP_FM_MS_STATS", None)
    with pkg.Context(0) as c:
        fm = c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr())
        for ptr, _ in outs.values():
            b.dev_free(ptr)
        b.close()
        fm.set_sequences(np.linspace(0, n, a.records + 1).astype(np.uint64))
        z = lambda cnt, dt=torch.int64: torch.zeros(cnt, dtype=dt, device=dev)
        wall_map, wall_aln, chains, edits, unfilled, runs, same_first = 0.0, 0.0, 0, 0, 0, 0, True
        by, stats = {}, None
        done = 0
        while done < a.reads:
            k = min(a.batch, a.reads - done)
            pat, off, _, _ = sample_reads(torch, text, k, m, seed=m + done, sub=0.01, indel=0.002)
            fw = pat.reshape(k, m)
            odd = ((torch.arange(k, device=dev) + done) % 2 == 1)
            reads = torch.where(odd[:, None], comp[fw.flip(1).to(torch.int64)], fw).contiguous().reshape(-1)
            kinds = [torch.uint8, torch.int32, torch.int64, torch.int64, torch.int64] + [torch.int32] * 5
            more = [torch.int32, torch.int64, torch.int32, torch.int32]
            head = lambda: (z(k + 1), z(k, torch.uint8), z(k))
            kw = dict(max_occ=a.max_occ, max_gap=a.gap, band=a.band, min_score=a.min_score, max_sec=0)
            ptrs = lambda ts: [t.data_ptr() for t in ts]
            # sizes the runs and counts the gaps (also the warm-up)
            h0, o0, g0 = head(), [z(k, t) for t in kinds + more], z(k + 1)
            os.environ["PFP_FM_MS_STATS"] = "1"
            fm.fill_stats()
            torch.cuda.synchronize()
            fm.map_long_aln_dev(reads.data_ptr(), off.data_ptr(), k, a.seed_len, *ptrs(h0), *ptrs(o0), g0.data_ptr(), None, max_fill=a.fill, **kw)
            st = fm.fill_stats()
            del os.environ["PFP_FM_MS_STATS"]
            stats = st if stats is None else {key: [x + y for x, y in zip(stats[key], st[key])] if isinstance(st[key], list) else
                                              (st[key] if key == "widths" else stats[key] + st[key]) for key in st}
            H = int(h0[0][-1])
            total = int(g0[H])
            # map_long alone
            h1, o1 = head(), [z(k, t) for t in kinds]
            torch.cuda.synchronize()
            t0 = time.time()
            fm.map_long_dev(reads.data_ptr(), off.data_ptr(), k, a.seed_len, *ptrs(h1), *ptrs(o1), **kw)
            wall_map += time.time() - t0
            # map_long_aln with the runs
            h2, o2, g2, cig = head(), [z(k, t) for t in kinds + more], z(k + 1), z(total + 1, torch.int32)
            c.set_kernel_trace(True)
            torch.cuda.synchronize()
            t0 = time.time()
            fm.map_long_aln_dev(reads.data_ptr(), off.data_ptr(), k, a.seed_len, *ptrs(h2), *ptrs(o2), g2.data_ptr(), cig.data_ptr(), max_fill=a.fill,
                                **kw)
            wall_aln += time.time() - t0
            for r in c.kernel_trace():
                t, l = by.get(r["name"], (0.0, 0))
                by[r["name"]] = (t + r["total_ms"], l + r["launches"])
            c.set_kernel_trace(False)
            same_first &= all(bool((x[:H] == y[:H]).all()) for x, y in zip(o1, o2)) and all(bool((x == y).all()) for x, y in zip(h1, h2))
            chains += H
            edits += int(o2[12][:H].sum())
            unfilled += int(o2[13][:H].sum())
            runs += total
            done += k
            print("%d reads: map_long %.2f s, map_long_aln %.2f s" % (done, wall_map, wall_aln), file=sys.stderr, flush=True)
            del pat, off, fw, reads, h0, o0, g0, h1, o1, h2, o2, g2, cig
        rows = []
        for bk, w in enumerate(stats["widths"]):
            ms, launches = by.get("fm_fill_%d" % w, (0.0, 0))
            sec = max(ms, 1e-9) / 1e3
            rows.append({"cells": w, "launches": launches, "ms": round(ms, 2), "gap_passes": stats["passes"][bk],
                         "gaps_per_s": round(stats["passes"][bk] / sec) if launches else 0,
                         "cell_updates_per_s": round(stats["cells"][bk] / sec) if launches else 0})
        out.update({"map_long_ms": round(wall_map * 1e3, 2), "map_long_aln_ms": round(wall_aln * 1e3, 2),
                    "added_ms": round((wall_aln - wall_map) * 1e3, 2), "added_share": round((wall_aln - wall_map) / wall_map, 4),
                    "reads_per_s_map_long": round(a.reads / wall_map), "reads_per_s_map_long_aln": round(a.reads / wall_aln),
                    "first_arrays_equal": bool(same_first), "chains_aligned": chains, "edits": edits, "unfilled_gaps": unfilled, "runs": runs,
                    "gaps": stats["gaps"], "trivial_gaps": stats["trivial"], "trivial_share": round(stats["trivial"] / max(stats["gaps"], 1), 4),
                    "gap_kernel": rows,
                    "other_ms": {key: round(sum(by.get(nm, (0.0, 0))[0] for nm in names), 2) for key, names in OTHER.items()}})
        fm.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
