"""Time the mapping of read pairs (csrc/fmpair.hip) on a benchmark workload; prints one JSON line and writes it to --out (default
profiles/pair_time.json).

    python tools/pair_time.py [--workload c3] [--pairs 1000000] [--len 150] [--reps 3] [--seed-len 20] [--k 8] [--anchors 8]
                              [--records 64] [--ins 300:500] [--out FILE]

The text and the index are tools/map_time.py's, the text cut into --records records.  --pairs fragments of a length drawn evenly
from --ins give two reads of --len bytes each, the fragment's first bytes and the reverse complement of its last, with about 2 %
substituted bytes and 0.5 % indels; in one pair of ten one mate (mates 1 and 2 in turn) also gets a substitution every 15 bytes,
which leaves it no seed of 20 bytes.  In the same process, warm, the minimum of --reps timed calls each:
  pairs    pfp_fm_map_pairs_dev with min_ins = 0 and max_ins = the largest fragment + 2k
  map      pfp_fm_map_dev (max_sec = 0, every output) on the same 2 x pairs reads: the call that already existed, the baseline on
           the same commit
From one more pairs call under the kernel trace (not timed): the time of the pairing kernels and of the window kernel inside it.
The share of ANCHORS that needed rescue is not exported by the library; recorded instead: the reads reported as rescued."""
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
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed-len", type=int, default=20)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--anchors", type=int, default=8)
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--ins", default="300:500")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_time.json"))
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
    npair, m, k = a.pairs, a.len, a.k
    f_lo, f_hi = (int(x) for x in a.ins.split(":"))
    out = {"tool": "pair_time", "workload": a.workload, "n": n, "pairs": npair, "read_len": m, "reps": a.reps, "records": a.records,
           "fragments": [f_lo, f_hi], "planted": "2 % substitutions, 0.5 % indels; in one pair of ten one mate has a substitution every 15 bytes",
           "min_seed": a.seed_len, "k": k, "anchors": a.anchors}
    with pkg.Context(0) as c:
        fm = c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr())
        for ptr, _ in outs.values():
            b.dev_free(ptr)
        b.close()
        fm.set_sequences(np.linspace(0, n, a.records + 1).astype(np.uint64))
        # fragments as reads of f_hi bytes; mate 1 = the first m bytes, mate 2 = the reverse complement of the m bytes that end at F
        frag, _, _, _ = sample_reads(torch, text, npair, f_hi, seed=m)
        frag = frag.reshape(npair, f_hi)
        g = torch.Generator(device="cpu").manual_seed(5)
        F = torch.randint(f_lo, f_hi + 1, (npair,), generator=g).to(dev)
        comp = torch.arange(256, dtype=torch.uint8, device=dev)
        for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
            comp[x] = y
        col = torch.arange(m, device=dev)
        m1 = frag[:, :m].clone()
        m2 = comp[torch.gather(frag, 1, (F[:, None] - 1 - col[None, :])).to(torch.int64)]
        q = torch.arange(npair, device=dev)
        every15 = (col % 15 == 7)[None, :]
        flip = lambda x: torch.where(x == 65, torch.full_like(x, 67), torch.full_like(x, 65))     # (A -> C, every other byte -> A)
        m1 = torch.where(every15 & (q % 20 == 0)[:, None], flip(m1), m1)
        m2 = torch.where(every15 & (q % 20 == 10)[:, None], flip(m2), m2)
        reads = torch.stack([m1, m2], 1).reshape(-1).contiguous()
        nread = 2 * npair
        off = torch.arange(0, nread * m + 1, m, dtype=torch.int64, device=dev)
        z = lambda cnt, dt=torch.int64: torch.zeros(cnt, dtype=dt, device=dev)
        u8 = torch.uint8
        proper, npairs = z(npair, u8), z(npair)
        mapped, resc, mapq, nh, strand, seq = z(nread, u8), z(nread, u8), z(nread, u8), z(nread), z(nread, u8), z(nread, torch.int32)
        soff, start, dist, tlen, coff, moff = z(nread), z(nread), z(nread, u8), z(nread), z(nread + 1), z(nread + 1)
        torch.cuda.synchronize()
        P, O = reads.data_ptr(), off.data_ptr()

        def pairs_call():
            d_cig, d_md = fm.map_pairs_dev(P, O, nread, k, a.seed_len, 0, f_hi + 2 * k, proper.data_ptr(), npairs.data_ptr(), mapped.data_ptr(),
                                           resc.data_ptr(), mapq.data_ptr(), nh.data_ptr(), strand.data_ptr(), seq.data_ptr(), soff.data_ptr(),
                                           start.data_ptr(), dist.data_ptr(), tlen.data_ptr(), coff.data_ptr(), moff.data_ptr(), anchors=a.anchors)
            for p in (d_cig, d_md):
                if p:
                    c.dev_free(p)
        s_pairs = timed(torch, pairs_call, a.reps)
        c.set_kernel_trace(True)
        pairs_call()
        by = {r["name"]: (r["total_ms"], r["launches"]) for r in c.kernel_trace()}
        c.set_kernel_trace(False)
        out.update({"proper_pairs": int(proper.sum()), "reads_mapped": int(mapped.sum()), "reads_rescued": int(resc.sum()),
                    "pair_mapq_60": int(((mapq == 60) & (mapped == 1)).sum())})
        hoff, smapq, snh = z(nread + 1), z(nread, u8), z(nread)
        fm.map_reads_dev(P, O, nread, k, a.seed_len, hoff.data_ptr(), smapq.data_ptr(), snh.data_ptr())
        H = int(hoff[-1])
        hs, hd, hq = z(H + 1, u8), z(H + 1, u8), z(H + 1, torch.int32)
        ho, hst, hc, hm = z(H + 1), z(H + 1), z(H + 2), z(H + 2)
        torch.cuda.synchronize()

        def map_call():
            d_cig, d_md = fm.map_reads_dev(P, O, nread, k, a.seed_len, hoff.data_ptr(), smapq.data_ptr(), snh.data_ptr(), hs.data_ptr(), hq.data_ptr(),
                                           ho.data_ptr(), hst.data_ptr(), hd.data_ptr(), hc.data_ptr(), hm.data_ptr())
            for p in (d_cig, d_md):
                if p:
                    c.dev_free(p)
        s_map = timed(torch, map_call, a.reps)
        ms = lambda name: round(by.get(name, (0, 0))[0], 2)
        out.update({"pairs_ms": round(s_pairs * 1e3, 2), "map_same_reads_ms": round(s_map * 1e3, 2),
                    "pairs_over_map": round(s_pairs / s_map, 4), "single_end_reads_mapped": int((snh > 0).sum()),
                    "kernel_ms": {"need": ms("fm_pair_need"), "windows": ms("fm_pair_windows"), "reduce": ms("fm_pair_reduce"),
                                  "window_plan": ms("fm_window_plan"), "window": ms("fm_window"), "window_start": ms("fm_window_start")},
                    "pairs_per_s": round(npair / s_pairs)})
        fm.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
