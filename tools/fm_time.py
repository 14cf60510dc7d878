"""Time pattern count and locate over a BWT and its run samples (csrc/fmsearch.hip) on benchmark workloads; prints one JSON line
and writes it to --out (default profiles/fm_time.json).

    python tools/fm_time.py [--workloads c3,huge_s] [--npat 1000000] [--lengths 32,100,1000] [--reps 3] [--out FILE]

For every workload: its text (big-bwt_amd/synth.py) and .bwt / .ssa / .esa (-s -e, whatever the workload's own flags) are built
on the device, then, on a context of its own (so that its peak is the index's alone): the index build (pfp_fm_build_dev, after
one warm-up build), count of npat patterns of each length sampled from the text with 10 % of them mutated in one byte (warm,
min of reps), and locate of the patterns of the shortest length, capped by --max-occ positions per pattern (0: all).  Reported:
build time, the index's device bytes and the build's peak per row, count throughput in patterns/s and pattern bytes/s, locate
throughput in positions/s."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402

NEED_GB = {"c3": 20, "huge_s": 200}


def sample_patterns(torch, text, npat, m, seed):
    dev = text.device
    n = text.numel()
    g = torch.Generator(device="cpu").manual_seed(seed)
    start = torch.randint(0, n - m, (npat,), generator=g).to(dev)
    P = text[start[:, None] + torch.arange(m, device=dev)[None, :]]
    mut = (torch.rand(npat, generator=g) < 0.1).to(dev)
    col = torch.randint(0, m, (npat,), generator=g).to(dev)
    rows = torch.arange(npat, device=dev)[mut]
    P[rows, col[mut]] = torch.where(P[rows, col[mut]] == ord("A"), ord("C"), ord("A")).to(torch.uint8)
    off = torch.arange(0, npat * m + 1, m, dtype=torch.int64, device=dev)
    return P.reshape(-1).contiguous(), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,huge_s")
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--lengths", default="32,100,1000")
    ap.add_argument("--max-occ", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_time.json"))
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    synth = __import__("bigbwt_amd.synth", fromlist=["x"])
    dev = torch.device("cuda", 0)
    out = {"tool": "fm_time", "npat": a.npat, "mutated": 0.1, "reps": a.reps, "max_occ": a.max_occ, "workloads": {}}
    for name in a.workloads.split(","):
        free, _ = torch.cuda.mem_get_info(dev)
        if free < NEED_GB.get(name, 40) * (1 << 30):
            out["workloads"][name] = {"skipped": "free device memory %.0f GB" % (free / 2**30)}
            continue
        cfg = synth.WORKLOADS[name]
        text = synth.workload_text_torch(dev, name)
        n = text.numel()
        bwt = torch.empty(n + 17, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()            # (the library works on a stream of its own: torch's writes must be done)
        b = pkg.Context(0)
        used, outs = b.bigbwt_formats_dev(text.data_ptr(), n, bwt.data_ptr(), cfg["w"], cfg["p"], pkg.FLAG_SSA | pkg.FLAG_ESA)
        assert used == n
        (ssa, ssa_b), (esa, esa_b) = outs["ssa"], outs["esa"]
        b.pool_trim()
        torch.cuda.empty_cache()
        row = {"n": n}
        with pkg.Context(0) as c:
            fm = c.fm_index_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b)          # warm-up
            fm.close()
            torch.cuda.synchronize()
            t0 = time.time()
            fm = c.fm_index_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b)
            row["build_ms"] = round((time.time() - t0) * 1e3, 2)
            for ptr, _ in outs.values():
                b.dev_free(ptr)
            b.close()
            inf = fm.info()
            row.update(runs=inf["runs"], sigma=inf["sigma"], row_bits=inf["row_bits"],
                       index_bytes_per_row=round(inf["device_bytes"] / (n + 1), 4),
                       build_peak_bytes_per_row=round(c.mem_stats()["peak"] / (n + 1), 4))
            row["count"] = {}
            for m in [int(x) for x in a.lengths.split(",")]:
                pat, off = sample_patterns(torch, text, a.npat, m, seed=m)
                sp, ep, first = (torch.zeros(a.npat, dtype=torch.int64, device=dev) for _ in range(3))
                times = []
                for r in range(a.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.time()
                    fm.count_dev(pat.data_ptr(), off.data_ptr(), a.npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr())
                    if r:
                        times.append(time.time() - t0)
                s = min(times)
                row["count"][str(m)] = {"ms": round(s * 1e3, 2), "patterns_per_s": round(a.npat / s), "pattern_bytes_per_s": round(a.npat * m / s),
                                        "found": int((ep > sp).sum()), "occurrences": int((ep - sp).sum())}
                if m == min(int(x) for x in a.lengths.split(",")):
                    out_off = torch.zeros(a.npat + 1, dtype=torch.int64, device=dev)
                    torch.cuda.synchronize()
                    fm.locate_dev(a.npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr(), a.max_occ, out_off.data_ptr())
                    total = int(out_off[-1])
                    pos = torch.empty(total + 1, dtype=torch.int64, device=dev)
                    lt = []
                    for r in range(a.reps + 1):
                        torch.cuda.synchronize()
                        t0 = time.time()
                        fm.locate_dev(a.npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr(), a.max_occ, out_off.data_ptr(), pos.data_ptr())
                        if r:
                            lt.append(time.time() - t0)
                    s = min(lt)
                    row["locate"] = {"pattern_len": m, "positions": total, "ms": round(s * 1e3, 2), "positions_per_s": round(total / s)}
                    del pos
                del pat, off, sp, ep, first
            row["peak_bytes_per_row"] = round(c.mem_stats()["peak"] / (n + 1), 4)
            fm.close()
        out["workloads"][name] = row
        del text, bwt
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
