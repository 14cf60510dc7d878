"""Time the LCP array, thresholds and matching statistics with thresholds (csrc/lcp.hip) on benchmark workloads; prints one JSON
line and writes it to --out (default profiles/thr_time.json).

    python tools/thr_time.py [--workloads c3] [--npat 1000000] [--lengths 32,100,1000] [--reps 3] [--out FILE]

For every workload: its text (big-bwt_amd/synth.py) and .bwt / .ssa / .esa (-s -e) are built on the device, then, on a context
of its own: LCP + thresholds through pfp_lcp_dev (after one warm-up: ms, the context's peak per row, sum and maximum of the
irreducible values read from the array at the run starts), an index with text that loads those thresholds, and matching
statistics by PHONI and by the two passes with thresholds, timed in the same run on the pattern sets of tools/ms_time.py plus
adversarial ones: chimeras (reads whose halves come from different places) and a^k b a^k over the text a^n.  Warm, min of
reps, a host clock around synchronising calls.  One more pass per set and algorithm under PFP_FM_MS_STATS=1 gives the jumps and the
bytes matched (PHONI: by the extensions of its jumps; thresholds: by pass 2, at most the pattern bytes)."""
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
from ms_time import read_patterns, timed  # noqa: E402


def chimeras(torch, text, npat, m, seed):
    """npat patterns of m bytes: two halves sampled from different places"""
    dev = text.device
    n = text.numel()
    g = torch.Generator(device="cpu").manual_seed(seed)
    h = m // 2
    a = torch.randint(0, n - h, (npat,), generator=g).to(dev)
    b = torch.randint(0, n - h, (npat,), generator=g).to(dev)
    ar = torch.arange(h, device=dev)
    P = torch.cat([text[a[:, None] + ar[None, :]], text[b[:, None] + ar[None, :]]], dim=1)
    off = torch.arange(0, npat * 2 * h + 1, 2 * h, dtype=torch.int64, device=dev)
    return torch.cat([P.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)]).contiguous(), off


def run_sets(torch, fm, sets, reps, dev):
    """{label: figures} for [(label, pat, off, npat, total bytes)]"""
    res = {}
    for label, pat, off, npat, total in sets:
        ln, ln0 = (torch.zeros(total + 1, dtype=torch.int32, device=dev) for _ in range(2))
        pos = torch.zeros(total + 1, dtype=torch.int64, device=dev)
        phoni = lambda: fm.matching_statistics_dev(pat.data_ptr(), off.data_ptr(), npat, ln0.data_ptr(), pos.data_ptr())
        thr = lambda: fm.matching_statistics_dev(pat.data_ptr(), off.data_ptr(), npat, ln.data_ptr(), pos.data_ptr(), thresholds=True)
        row = {"patterns": npat, "pattern_bytes": total}
        for name, fn in (("phoni", phoni), ("thresholds", thr)):
            fm.ms_stats()
            s = timed(torch, reps, fn)
            launches = fm.ms_stats()["launches"] // (reps + 1)
            os.environ["PFP_FM_MS_STATS"] = "1"
            fn()
            st = fm.ms_stats()
            del os.environ["PFP_FM_MS_STATS"]
            row[name] = {"ms": round(s * 1e3, 2), "pattern_bytes_per_s": round(total / s), "launches": launches, "jumps": st["jumps"],
                         "bytes_matched": st["matched"]}
        row["thresholds_rate_over_phoni_rate"] = round(row["phoni"]["ms"] / max(row["thresholds"]["ms"], 1e-9), 3)
        row["same_lengths"] = bool(torch.equal(ln, ln0))
        res[label] = row
        del ln, ln0, pos
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3")
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--lengths", default="32,100,1000")
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--a-n", type=int, default=1_000_000, help="n of the text a^n of the adversarial set")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thr_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = entry.load_package()
    synth = __import__("bigbwt_amd.synth", fromlist=["x"])
    dev = torch.device("cuda", 0)
    out = {"tool": "thr_time", "npat": a.npat, "mutated": 0.1, "reps": a.reps, "workloads": {}}
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
        r = ssa_b // 10
        starts = torch.from_numpy(pkg.unpack5(b.fetch_dev(ssa, ssa_b)).reshape(-1, 2)[:, 0].astype(np.int64)).to(dev)
        b.pool_trim()
        torch.cuda.empty_cache()
        row = {"n": n, "runs": r}
        with pkg.Context(0) as c:
            d_lcp = torch.zeros(n + 2, dtype=torch.int64, device=dev)
            d_thr = torch.zeros(r + 1, dtype=torch.int64, device=dev)
            args = (bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr())
            torch.cuda.synchronize()
            c.lcp_dev(*args, d_lcp=d_lcp.data_ptr(), d_thr=d_thr.data_ptr())          # warm-up
            t0 = time.time()
            c.lcp_dev(*args, d_lcp=d_lcp.data_ptr(), d_thr=d_thr.data_ptr())
            row["lcp_and_thresholds"] = {"ms": round((time.time() - t0) * 1e3, 2), "peak_bytes_per_row": round(c.mem_stats()["peak"] / (n + 1), 4)}
            irr = d_lcp[starts]
            row["irreducible"] = {"sum": int(irr.sum()), "max": int(irr.max()), "mean": round(float(irr.to(torch.float64).mean()), 2)}
            del d_lcp, irr, starts
            thr5 = torch.zeros(5 * r + 16, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            c.pack5_dev(d_thr.data_ptr(), r, thr5.data_ptr())
            fm = c.fm_index_ms_dev(*args)
            for ptr, _ in outs.values():
                b.dev_free(ptr)
            b.close()
            fm.add_thresholds_dev(thr5.data_ptr(), 5 * r)
            inf = fm.info()
            row.update(sigma=inf["sigma"], row_bits=inf["row_bits"], index_bytes_per_row=round(inf["device_bytes"] / (n + 1), 4))
            sets = []
            for m in (int(x) for x in a.lengths.split(",")):
                pat, off = sample_patterns(torch, text, a.npat, m, seed=m)
                sets.append((str(m), pat, off, a.npat, a.npat * m))
            pat, off = read_patterns(torch, text, a.reads, a.read_len, 7)
            sets.append(("reads", pat, off, a.reads, a.reads * a.read_len))
            pat, off = chimeras(torch, text, a.reads, a.read_len, 9)
            sets.append(("chimeras", pat, off, a.reads, a.reads * (a.read_len // 2) * 2))
            row["sets"] = run_sets(torch, fm, sets, a.reps, dev)
            fm.close()
        out["workloads"][name] = row
        del text, bwt
        torch.cuda.empty_cache()
    # a^k b a^k over a^n: every step of PHONI after the b re-compares what it holds
    tx = np.full(a.a_n, ord("a"), dtype=np.uint8)
    with pkg.Context(0) as c:
        got = c.bigbwt(tx, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
        with c.fm_index_ms(got["bwt"], got["ssa"], got["esa"], tx) as fm:
            t0 = time.time()
            fm.add_thresholds()
            row = {"n": a.a_n, "thresholds_ms": round((time.time() - t0) * 1e3, 2)}
            k = a.a_n // 20
            p = np.concatenate([np.full(k, ord("a"), dtype=np.uint8), [ord("b")], np.full(k, ord("a"), dtype=np.uint8)]).astype(np.uint8)
            pat = torch.from_numpy(p).to(dev)
            off = torch.tensor([0, len(p)], dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            row["sets"] = run_sets(torch, fm, [("a^k b a^k, k = %d" % k, pat, off, 1, len(p))], a.reps, dev)
    out["a_n"] = row
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
