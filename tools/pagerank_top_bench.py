"""The k highest-ranked vertices of a PageRank run: selected on the device (jg_pagerank_top + a full
jg_pagerank_top_read) against the route it replaces, jg_pagerank_end with its hand-back of two n-element
arrays, then numpy.argpartition and a sort of the k on the host.  Same process, same graph, same session.

One process per scale (a fresh child each; --scale N runs one scale in this process): RMAT-<scale>, ef 16, IN
adjacency, one GPU, after pagerank_begin + 9 steps.  Per scale and k (10, 1000, 2^20 by default), median and
range of --reps calls after one warm-up:
  handback[k]   wall_ms of pagerank_end() + the host select, the call's wall alone
  top[k]        wall_ms of pagerank_top(k) (select + full read), select_ms (the select, order and emit kernels
                alone), kernel launches, the byte model and its share of 8 TB/s over select_ms, the bytes read
                back, the peak temporary footprint
The host select is tie-exact (ties by index ascending): argpartition finds the k-th rank, the ranks above it
and the smallest indices of the ranks equal to it are the candidates, a lexsort of those k orders them.  The
two routes' lists are compared, indices and rank bits, before any time is printed.  One JSON line per scale.
Usage: python tools/pagerank_top_bench.py [--scales 20 24 26] [--scale N] [--ks 10 1000 1048576] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
TOP_BINS = 2048      # kTopBins (csrc/jg_top.hip)
TOP_SMALL = 4096     # kTopSmall
RADIX_TILE = 4096    # kRadixTile (csrc/jg_prim.hip)


def med(xs):
    return round(float(np.median(xs)), 3)


def rng_of(xs):
    return [round(float(min(xs)), 3), round(float(max(xs)), 3)]


def host_top(rank, k):
    """Indices of the k highest ranks, rank descending, ties by index ascending (finite ranks)."""
    n = len(rank)
    k = min(k, n)
    if k < n:
        kth = rank[np.argpartition(-rank, k - 1)[k - 1]]
        above = np.flatnonzero(rank > kth)
        cand = np.concatenate([above, np.flatnonzero(rank == kth)[:k - len(above)]])
    else:
        cand = np.arange(n)
    return cand[np.lexsort((cand, -rank[cand]))]


def temporary_bytes(n, k):
    """Peak device temporaries of one select: the records and output arrays (28 B per record), the state
    slots and histograms of the passes, and past kTopSmall records the radix sort's second copy and digit
    counts."""
    passes = 6 + -(-max((n - 1).bit_length(), 1) // 11)
    b = 28 * k + 48 * (passes + 1) + 4 * TOP_BINS * passes + 8
    if k > TOP_SMALL:
        b += 12 * k + -(-k // RADIX_TILE) * 256 * 12
    return b


def one_scale(scale, edgefactor, ks, reps):
    import janusgraph_amd as jg
    ctx = jg.Context((0,))
    n = 1 << scale
    g = ctx.build_rmat(scale, edgefactor, 0x5EED + scale, flags=jg.ADJ_IN)
    g.pagerank_begin(0.85, n)
    g.pagerank_step(9)
    g.pagerank_end(want=False)
    line = {"workload": f"pagerank_top_rmat{scale}_ef{edgefactor}", "vertices": n, "reps": reps, "steps": 9}
    out = {}
    for k in ks:
        # ---- the parent route ----
        wall, call = [], []
        rank = idx = None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            rank, ec = g.pagerank_end()
            t1 = time.perf_counter()
            idx = host_top(rank, k)
            top_a = (idx, rank[idx], ec[idx])
            t2 = time.perf_counter()
            if rep:
                wall.append((t2 - t0) * 1e3)
                call.append((t1 - t0) * 1e3)
        hand = {"wall_ms": med(wall), "wall_ms_range": rng_of(wall), "call_wall_ms": med(call),
                "call_wall_ms_range": rng_of(call), "bytes_handed_back": 16 * n}
        # ---- the device select ----
        wall, sms = [], []
        got = st = None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            got = g.pagerank_top(k)
            t1 = time.perf_counter()
            if rep:
                wall.append((t1 - t0) * 1e3)
        for rep in range(reps + 1):  # the device time of the call alone (the stats are the last call's)
            listed, ms = g.pagerank_top_build(k)
            st = ctx.stats()
            if rep:
                sms.append(ms)
        g.pagerank_top_release()
        vid, gi, gr, ge = got
        assert np.array_equal(gi, top_a[0]), "the two routes list different vertices"
        assert np.array_equal(gr.view(np.uint64), top_a[1].view(np.uint64)), "the two routes' ranks differ"
        assert np.array_equal(ge, top_a[2]) and np.array_equal(vid, gi), "edge counts / ids differ"
        out[k] = (hand, wall, sms, st, len(gi))
    for k, (hand, wall, sms, st, listed) in out.items():
        s = med(sms)
        model = st["algorithmic_bytes"]
        line[f"handback_{k}"] = hand
        line[f"top_{k}"] = {
            "wall_ms": med(wall), "wall_ms_range": rng_of(wall), "select_ms": s, "select_ms_range": rng_of(sms),
            "listed": listed, "kernel_launches": st["kernel_launches"], "bytes_read_back": 32 * listed,
            "roofline": {"bound": "hbm", "bytes": model, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "achieved": round(model / (s * 1e-3) / 1e9, 1),
                         "frac": round(model / (s * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
            "temporary_bytes": temporary_bytes(n, listed),
            "wall_below_handback_by_ms": round(hand["wall_ms"] - med(wall), 3),
            "handback_over_top": round(hand["wall_ms"] / med(wall), 1)}
    print(json.dumps(line), flush=True)
    g.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[20, 24, 26])
    ap.add_argument("--scale", type=int, default=0, help="run this one scale in this process")
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--ks", type=int, nargs="*", default=[10, 1000, 1 << 20])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.scale:
        one_scale(args.scale, args.edgefactor, args.ks, args.reps)
        return
    for s in args.scales:  # one fresh process per scale
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--scale", str(s), "--edgefactor",
                               str(args.edgefactor), "--reps", str(args.reps), "--ks"] + [str(k) for k in args.ks])


if __name__ == "__main__":
    main()
