"""Time windowed alignment (csrc/fmwindow.hip) on a benchmark workload; prints one JSON line and writes it to --out (default
profiles/window_time.json).

    python tools/window_time.py [--workload c3] [--reads 200000] [--len 150] [--reps 3] [--k 8] [--widths 500,4000] [--out FILE]

The text, the index and the reads are tools/extend_time.py's: --reads reads of --len bytes drawn from the text with about 2 %
substituted bytes and 0.5 % indels.  Every read gets one window of each of --widths bytes that holds the place it was drawn from, at
a pseudo-random offset in the window.  In the same process, warm, the minimum of --reps timed calls of pfp_fm_window_dev per width;
the figure is cell updates per second, cells = read bytes x window bytes, as the header counts them.  From one more call under the
kernel trace (not timed): the time of the plan, of the forward kernel and of the start kernel.  Next to it pfp_fm_extend_dev on
the reads' own diagonals, the call that already existed: what a banded look at one diagonal costs on the same reads."""
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
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--widths", default="500,4000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_time.json"))
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
    npat, m, k = a.reads, a.len, a.k
    out = {"tool": "window_time", "workload": a.workload, "n": n, "reads": npat, "read_len": m, "reps": a.reps, "k": k,
           "planted": "2 % substitutions, 0.5 % indels", "widths": {}}
    with pkg.Context(0) as c:
        fm = c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr())
        for ptr, _ in outs.values():
            b.dev_free(ptr)
        b.close()
        pat, off, start, _ = sample_reads(torch, text, npat, m, seed=m)
        cp = torch.arange(npat, dtype=torch.int32, device=dev)
        z = lambda cnt, dt=torch.int64: torch.zeros(cnt, dtype=dt, device=dev)
        dist, s, e = z(npat, torch.uint8), z(npat), z(npat)
        P, O = pat.data_ptr(), off.data_ptr()
        for width in (int(x) for x in a.widths.split(",")):
            room = max(width - m - 2 * k, 1)
            lo = (start - (torch.arange(npat, device=dev) * 7919) % room - k).clamp(min=0)
            hi = (lo + width).clamp(max=n)
            torch.cuda.synchronize()
            call = lambda: fm.window_dev(P, O, npat, cp.data_ptr(), lo.data_ptr(), hi.data_ptr(), npat, k, dist.data_ptr(), s.data_ptr(), e.data_ptr())
            sec = timed(torch, call, a.reps)
            c.set_kernel_trace(True)
            call()
            by = {r["name"]: (round(r["total_ms"], 2), r["launches"]) for r in c.kernel_trace()}
            c.set_kernel_trace(False)
            cells = int(((hi - lo) * m).sum())
            out["widths"][str(width)] = {"call_ms": round(sec * 1e3, 2), "cells": cells, "cell_updates_per_s": round(cells / sec),
                                         "aligned": int((dist != 0xFF).sum()),
                                         "kernel_ms": {name: by.get(name, (0, 0))[0] for name in ("fm_window_plan", "fm_window", "fm_window_start")},
                                         "launches_of_the_forward_kernel": by.get("fm_window", (0, 0))[1]}
        diag = start.clone()
        torch.cuda.synchronize()
        sec = timed(torch, lambda: fm.extend_dev(P, O, npat, cp.data_ptr(), diag.data_ptr(), npat, k, dist.data_ptr(), s.data_ptr(), e.data_ptr()), a.reps)
        out["extend_on_the_own_diagonal_ms"] = round(sec * 1e3, 2)
        fm.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
