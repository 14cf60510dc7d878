"""Time sequence-aware locate and document listing (csrc/seqmap.hip) next to plain locate on a benchmark workload; prints one JSON
line and writes it to --out (default profiles/seq_time.json).

    python tools/seq_time.py [--workload c3] [--npat 1000000] [--len 32] [--reps 3] [--tables natural,1000000] [--out FILE]

The workload's text (big-bwt_amd/synth.py) and its .bwt / .ssa / .esa (-s -e) are built on the device, then, on a context of its
own, an index, and npat patterns of --len bytes sampled from the text as tools/fm_time.py samples them (10 % mutated in one byte).
For every table - "natural": one sequence per record of the collection, cut at its '>' bytes; a number K: K sequences cut at sorted
random positions - in the same process, warm, the minimum of --reps timed calls each: pfp_fm_locate_dev (the baseline: the code the
other two start with), pfp_fm_locate_seqs_dev and pfp_fm_doclist_dev, as milliseconds and located positions per second, the regime
document listing took, and, from one more traced call of each (pfp_set_kernel_trace: event pairs around the launches, so not part
of the timed calls), the split by kernel."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as entry  # noqa: E402
from fm_time import sample_patterns  # noqa: E402

DOC_LDS = 4096          # csrc/seqmap.hip: kDocLds


def timed(torch, call, reps):
    times = []
    for r in range(reps + 1):          # the first call warms up
        torch.cuda.synchronize()
        t0 = time.time()
        call()
        if r:
            times.append(time.time() - t0)
    return min(times)


def traced(ctx, call):
    ctx.set_kernel_trace(True)
    call()
    rows = ctx.kernel_trace()
    ctx.set_kernel_trace(False)
    return {r["name"]: {"launches": r["launches"], "ms": round(r["total_ms"], 3)} for r in sorted(rows, key=lambda r: -r["total_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tables", default="natural,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_time.json"))
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
    out = {"tool": "seq_time", "workload": a.workload, "n": n, "npat": a.npat, "pattern_len": a.len, "mutated": 0.1, "reps": a.reps, "tables": {}}
    with pkg.Context(0) as c:
        fm = c.fm_index_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b)
        for ptr, _ in outs.values():
            b.dev_free(ptr)
        b.close()
        npat = a.npat
        pat, off = sample_patterns(torch, text, npat, a.len, seed=a.len)
        z = lambda k, dt=torch.int64: torch.zeros(k, dtype=dt, device=dev)
        sp, ep, first, uoff = z(npat), z(npat), z(npat), z(npat + 1)
        torch.cuda.synchronize()
        fm.count_dev(pat.data_ptr(), off.data_ptr(), npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr())
        fm.locate_dev(npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr(), 0, uoff.data_ptr())
        U = int(uoff[-1])
        out["positions"] = U
        pos, seq, offs = z(U + 1), z(U + 1, torch.int32), z(U + 1)
        ooff, doff = z(npat + 1), z(npat + 1)
        torch.cuda.synchronize()
        rng_args = (npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr())
        locate = lambda: fm.locate_dev(*rng_args, 0, uoff.data_ptr(), pos.data_ptr())
        s = timed(torch, locate, a.reps)
        out["locate"] = {"ms": round(s * 1e3, 2), "positions_per_s": round(U / s), "kernels": traced(c, locate)}
        for spec in a.tables.split(","):
            if spec == "natural":
                starts = torch.nonzero(text == ord(">")).reshape(-1).cpu().numpy().astype(np.uint64)
                if len(starts) == 0 or starts[0] != 0:
                    starts = np.concatenate([np.zeros(1, dtype=np.uint64), starts])
                starts = np.concatenate([starts, np.array([n], dtype=np.uint64)])
            else:
                cuts = np.sort(np.random.default_rng(7).integers(0, n + 1, int(spec) - 1)).astype(np.uint64)
                starts = np.concatenate([np.zeros(1, dtype=np.uint64), cuts, np.array([n], dtype=np.uint64)])
            before = fm.info()["device_bytes"]
            t0 = time.time()
            fm.set_sequences(starts)
            row = {"nseq": len(starts) - 1, "set_ms": round((time.time() - t0) * 1e3, 2), "table_bytes": fm.info()["device_bytes"] - before}
            seqs_call = lambda: fm.locate_seqs_dev(off.data_ptr(), *rng_args, 0, ooff.data_ptr(), seq.data_ptr(), offs.data_ptr())
            s = timed(torch, seqs_call, a.reps)
            kept = int(ooff[-1])
            row["locate_seqs"] = {"ms": round(s * 1e3, 2), "positions_per_s": round(U / s), "kept": kept,
                                  "over_locate": round(s * 1e3 / out["locate"]["ms"], 3), "kernels": traced(c, seqs_call)}
            only = lambda: fm.doclist_dev(off.data_ptr(), *rng_args, doff.data_ptr())
            only()
            D = int(doff[-1])
            doc, cnt = z(D + 1, torch.int32), z(D + 1)
            torch.cuda.synchronize()
            docs_call = lambda: fm.doclist_dev(off.data_ptr(), *rng_args, doff.data_ptr(), doc.data_ptr(), cnt.data_ptr())
            s = timed(torch, docs_call, a.reps)
            row["doclist"] = {"ms": round(s * 1e3, 2), "positions_per_s": round(U / s), "documents": D,
                              "regime": "histogram" if row["nseq"] <= DOC_LDS else "sort", "over_locate": round(s * 1e3 / out["locate"]["ms"], 3),
                              "kernels": traced(c, docs_call)}
            assert int(cnt[:D].sum()) == kept          # every kept hit is counted in exactly one document
            out["tables"][spec] = row
            del doc, cnt
        out["peak_bytes_per_position"] = round(c.mem_stats()["peak"] / max(U, 1), 2)
        fm.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
