"""Time the BWT check / inversion of csrc/unbwt.hip on benchmark workloads; prints one JSON line.

    python tools/unbwt_time.py [--workloads c3,huge_s] [--reps 3] [--trace]

For every workload: its text (big-bwt_amd/synth.py) and outputs are built on the device (pfp_bigbwt_formats_dev with the
workload's flags), then, on a context of its own (so that its peak is the check's alone), pfp_check_bwt_dev of the .bwt and
.ssa / .esa against the text and pfp_unbwt_dev, each `reps` times after one warm-up.  Reported: warm times (min / median),
the library's peak device memory per BWT byte and, with --trace, the per-kernel device times of the last check."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402

NEED_GB = {"c3": 20, "huge_s": 230}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,huge_s")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    synth = __import__("bigbwt_amd.synth", fromlist=["x"])
    dev = torch.device("cuda", 0)
    out = {"tool": "unbwt_time", "reps": a.reps, "workloads": {}}
    for name in a.workloads.split(","):
        free, _ = torch.cuda.mem_get_info(dev)
        if free < NEED_GB.get(name, 40) * (1 << 30):
            out["workloads"][name] = {"skipped": "free device memory %.0f GB" % (free / 2**30)}
            continue
        cfg = synth.WORKLOADS[name]
        w, p, flags = cfg["w"], cfg["p"], cfg["flags"]
        text = synth.workload_text_torch(dev, name)
        n = text.numel()
        bwt = torch.empty(n + 17, dtype=torch.uint8, device=dev)
        b = pkg.Context(0)              # the builder's context: holds the .ssa / .esa device buffers during the check
        t0 = time.time()
        used, outs = b.bigbwt_formats_dev(text.data_ptr(), n, bwt.data_ptr(), w, p, flags)
        build_s = time.time() - t0
        assert used == n
        b.pool_trim()
        torch.cuda.empty_cache()
        row = {"n": n, "flags": flags, "build_s_cold": round(build_s, 3)}
        ssa, ssa_b = outs.get("ssa", (None, 0))
        esa, esa_b = outs.get("esa", (None, 0))
        with pkg.Context(0) as c:
            times, dtimes = [], []
            for r in range(a.reps + 1):
                if a.trace and r == a.reps:
                    c.set_kernel_trace(True)
                res = c.check_bwt_dev(bwt.data_ptr(), n + 1, text.data_ptr(), None, ssa, ssa_b, esa, esa_b)
                assert all(res[k] is None for k in ("text_mismatch", "sa_mismatch", "ssa_mismatch", "esa_mismatch")), res
                if r:
                    times.append(res["ms"])
            if a.trace:
                row["kernels"] = [dict(name=k["name"], launches=k["launches"], ms=round(k["total_ms"], 3)) for k in c.kernel_trace()]
                c.set_kernel_trace(False)
            row["check_ms_min"] = round(min(times), 2)
            row["check_ms_median"] = round(statistics.median(times), 2)
            row["ssa_runs"] = res["ssa_runs"]
            row["esa_runs"] = res["esa_runs"]
            st = c.mem_stats()
            row["check_peak_bytes_per_bwt_byte"] = round(st["peak"] / (n + 1), 3)
            dec = torch.empty(n + 16, dtype=torch.uint8, device=dev)
            for r in range(a.reps + 1):
                torch.cuda.synchronize()
                t0 = time.time()
                c.unbwt_dev(bwt.data_ptr(), n + 1, dec.data_ptr())
                el = (time.time() - t0) * 1e3
                if r:
                    dtimes.append(el)
            row["unbwt_ms_min"] = round(min(dtimes), 2)
            row["unbwt_equal"] = bool(torch.equal(dec[:n], text))
            row["peak_bytes_per_bwt_byte"] = round(c.mem_stats()["peak"] / (n + 1), 3)
        out["workloads"][name] = row
        for ptr, _ in outs.values():
            b.dev_free(ptr)
        b.close()
        del text, bwt, dec
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
