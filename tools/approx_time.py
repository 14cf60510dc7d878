"""Time the k-mismatch search (csrc/fmapprox.hip) next to plain count on a benchmark workload; prints one JSON line and writes it
to --out (default profiles/approx_time.json).

    python tools/approx_time.py [--workload c3] [--npat 1000000] [--len 100] [--reps 3] [--ks 0,1,2,3] [--out FILE]

The workload's text (big-bwt_amd/synth.py) and its .bwt / .ssa / .esa (-s -e) are built on the device, then, on a context of its
own, an index, and npat patterns of --len bytes sampled from the text: half verbatim, a quarter with one substituted byte and a
quarter with two.  In the same process, warm, the minimum of --reps timed calls each: pfp_fm_count_dev (the baseline) and, for every
k, pfp_fm_approx_dev offsets-only (one walk) and with the hits and their toeholds (two walks, the scan, the sort).  Per k also the
hits, and from one more call under PFP_FM_MS_STATS=1 (not timed) the LF pairs and launches that pfp_fm_approx_stats reports.
`over_count` of k = 0 is the figure to watch: the same LF pairs as count, plus the record, the second walk and the scan."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def sample_patterns(torch, text, npat, m, seed):
    """npat windows of the text: the first half as they are, then a quarter with one and a quarter with two substituted bytes"""
    dev = text.device
    n = text.numel()
    g = torch.Generator(device="cpu").manual_seed(seed)
    start = torch.randint(0, n - m, (npat,), generator=g).to(dev)
    P = text[start[:, None] + torch.arange(m, device=dev)[None, :]]
    rows = torch.arange(npat, device=dev)
    for lo in (npat // 2, npat - npat // 4):          # rows from lo on get one more substitution
        col = torch.randint(0, m, (npat,), generator=g).to(dev)
        r = rows[lo:]
        P[r, col[lo:]] = torch.where(P[r, col[lo:]] == ord("A"), ord("C"), ord("A")).to(torch.uint8)
    off = torch.arange(0, npat * m + 1, m, dtype=torch.int64, device=dev)
    return P.reshape(-1).contiguous(), off


def timed(torch, call, reps):
    times = []
    for r in range(reps + 1):          # the first call warms up
        torch.cuda.synchronize()
        t0 = time.time()
        call()
        if r:
            times.append(time.time() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="0,1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "approx_time.json"))
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
    out = {"tool": "approx_time", "workload": a.workload, "n": n, "npat": a.npat, "pattern_len": a.len, "reps": a.reps,
           "patterns": "1/2 verbatim, 1/4 one substitution, 1/4 two", "k": {}}
    with pkg.Context(0) as c:
        fm = c.fm_index_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b)
        for ptr, _ in outs.values():
            b.dev_free(ptr)
        b.close()
        npat = a.npat
        pat, off = sample_patterns(torch, text, npat, a.len, seed=a.len)
        z = lambda k, dt=torch.int64: torch.zeros(k, dtype=dt, device=dev)
        sp, ep, first, hoff = z(npat), z(npat), z(npat), z(npat + 1)
        torch.cuda.synchronize()
        count = lambda: fm.count_dev(pat.data_ptr(), off.data_ptr(), npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr())
        s = timed(torch, count, a.reps)
        out["count"] = {"ms": round(s * 1e3, 2), "found": int((ep > sp).sum())}
        for k in (int(x) for x in a.ks.split(",")):
            offsets = lambda: fm.approx_dev(pat.data_ptr(), off.data_ptr(), npat, k, hoff.data_ptr())
            s1 = timed(torch, offsets, a.reps)
            H = int(hoff[-1])
            hsp, hep, hfirst, hd = z(H + 1), z(H + 1), z(H + 1), z(H + 1, torch.uint8)
            torch.cuda.synchronize()
            fill = lambda: fm.approx_dev(pat.data_ptr(), off.data_ptr(), npat, k, hoff.data_ptr(), hsp.data_ptr(), hep.data_ptr(),
                                         hd.data_ptr(), hfirst.data_ptr())
            s2 = timed(torch, fill, a.reps)
            os.environ["PFP_FM_MS_STATS"] = "1"          # (read per call)
            fm.approx_stats()
            fill()
            st = fm.approx_stats()
            del os.environ["PFP_FM_MS_STATS"]
            out["k"][str(k)] = {"offsets_ms": round(s1 * 1e3, 2), "ms": round(s2 * 1e3, 2), "hits": H,
                                "occurrences": int((hep[:H] - hsp[:H]).sum()), "lf_pairs": st["pairs"], "launches": st["launches"],
                                "over_count": round(s2 * 1e3 / out["count"]["ms"], 3),
                                "offsets_over_count": round(s1 * 1e3 / out["count"]["ms"], 3)}
            del hsp, hep, hfirst, hd
        fm.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
