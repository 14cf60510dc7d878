"""Time matching statistics (csrc/fmsearch.hip: PHONI) on benchmark workloads; prints one JSON line and writes it to --out
(default profiles/ms_time.json).

    python tools/ms_time.py [--workloads c3,huge_s] [--npat 1000000] [--lengths 32,100,1000] [--reps 3] [--out FILE]

For every workload: its text (big-bwt_amd/synth.py) and .bwt / .ssa / .esa (-s -e) are built on the device, then, on a context
of its own: the index build with the text given and by inversion (after one warm-up build each: ms and the context's peak per
row), matching statistics of the pattern sets of tools/fm_time.py (npat patterns of each length sampled from the text, 10 %
mutated in one byte) with count timed on the same patterns in the same run, and one read-like set: --reads patterns of
--read-len bytes with 1 % of the bytes changed.  Warm, min of reps, a host clock around synchronising calls.  One more pass per
set under PFP_FM_MS_STATS=1 gives the share of steps that jumped (step 3) and the bytes matched per such step."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as entry  # noqa: E402
from fm_time import NEED_GB, sample_patterns  # noqa: E402


def read_patterns(torch, text, npat, m, seed):
    dev = text.device
    n = text.numel()
    g = torch.Generator(device="cpu").manual_seed(seed)
    start = torch.randint(0, n - m, (npat,), generator=g).to(dev)
    P = text[start[:, None] + torch.arange(m, device=dev)[None, :]]
    mut = (torch.rand(npat, m, generator=g) < 0.01).to(dev)
    P[mut] = torch.where(P[mut] == ord("A"), ord("C"), ord("A")).to(torch.uint8)
    off = torch.arange(0, npat * m + 1, m, dtype=torch.int64, device=dev)
    return torch.cat([P.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)]).contiguous(), off


def timed(torch, reps, fn):
    times = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.time()
        fn()
        if r:
            times.append(time.time() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,huge_s")
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--lengths", default="32,100,1000")
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_time.json"))
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    synth = __import__("bigbwt_amd.synth", fromlist=["x"])
    dev = torch.device("cuda", 0)
    out = {"tool": "ms_time", "npat": a.npat, "mutated": 0.1, "reps": a.reps, "workloads": {}}
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
        row = {"n": n, "build": {}}
        for how, d_text in (("inverted", None), ("text_given", text.data_ptr())):
            with pkg.Context(0) as c:
                build = lambda: c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, d_text)
                build().close()             # warm-up
                torch.cuda.synchronize()
                t0 = time.time()
                fm = build()
                row["build"][how] = {"ms": round((time.time() - t0) * 1e3, 2), "peak_bytes_per_row": round(c.mem_stats()["peak"] / (n + 1), 4)}
                if how == "inverted":
                    fm.close()
                    continue
                for ptr, _ in outs.values():
                    b.dev_free(ptr)
                b.close()
                inf = fm.info()
                row.update(runs=inf["runs"], sigma=inf["sigma"], row_bits=inf["row_bits"], index_bytes_per_row=round(inf["device_bytes"] / (n + 1), 4))
                row["sets"] = {}
                sets = [(str(m), a.npat, m, False) for m in (int(x) for x in a.lengths.split(","))] + [("reads", a.reads, a.read_len, True)]
                for label, npat, m, reads in sets:
                    pat, off = read_patterns(torch, text, npat, m, 7) if reads else sample_patterns(torch, text, npat, m, seed=m)
                    ln = torch.zeros(npat * m, dtype=torch.int32, device=dev)
                    pos = torch.zeros(npat * m, dtype=torch.int64, device=dev)
                    sp, ep, first = (torch.zeros(npat, dtype=torch.int64, device=dev) for _ in range(3))
                    ms = lambda: fm.matching_statistics_dev(pat.data_ptr(), off.data_ptr(), npat, ln.data_ptr(), pos.data_ptr())
                    s_cnt = timed(torch, a.reps, lambda: fm.count_dev(pat.data_ptr(), off.data_ptr(), npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr()))
                    fm.ms_stats()
                    s_ms = timed(torch, a.reps, ms)
                    launches = fm.ms_stats()["launches"] // (a.reps + 1)
                    os.environ["PFP_FM_MS_STATS"] = "1"
                    ms()
                    st = fm.ms_stats()
                    del os.environ["PFP_FM_MS_STATS"]
                    row["sets"][label] = {
                        "patterns": npat, "pattern_len": m, "ms_ms": round(s_ms * 1e3, 2), "ms_pattern_bytes_per_s": round(npat * m / s_ms),
                        "count_ms": round(s_cnt * 1e3, 2), "count_pattern_bytes_per_s": round(npat * m / s_cnt),
                        "ms_rate_over_count_rate": round(s_cnt / s_ms, 3), "launches": launches,
                        "jump_share": round(st["jumps"] / (npat * m), 5), "bytes_matched_per_jump": round(st["matched"] / max(st["jumps"], 1), 2),
                        "mean_len": round(float(ln.to(torch.float64).mean()), 2)}
                    del pat, off, ln, pos, sp, ep, first
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
