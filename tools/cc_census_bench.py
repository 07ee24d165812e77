"""The component census of ConnectedComponentVertexProgram: counted on the device (jg_cc_census + a full
jg_cc_census_read) against the route it replaces for "how many components, how big" — jg_connected_components
with its hand-back of n ids, then numpy.unique(return_counts=True) on the host.  Same process, same graph.

One process per scale (a fresh child each; --scale N runs one scale in this process): RMAT-<scale>, ef 16,
BOTH adjacency, one GPU.  Per scale, median and range of --reps calls after one warm-up:
  handback        wall_ms of connected_components() + numpy.unique, the call's wall alone, compute_ms
  census[mp]      for min_population 1 and 2: wall_ms of jg_cc_census + a full read, census_ms (the census
                  kernels alone), compute_ms (program + census), components / listed / largest, bytes read back,
                  the census byte model and its share of 8 TB/s over census_ms, the peak temporary footprint
The two routes' censuses are compared, order included (population descending, ties by the label's String),
before any time is printed.  One JSON line per scale.
Usage: python tools/cc_census_bench.py [--scales 20 24 26] [--scale N] [--reps 5]
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
CENSUS_TILE = 2048   # kCensusTile (csrc/jg_census.hip)
RADIX_TILE = 4096    # kRadixTile (csrc/jg_prim.hip)


def med(xs):
    return round(float(np.median(xs)), 3)


def rng_of(xs):
    return [round(float(min(xs)), 3), round(float(max(xs)), 3)]


def string_order(ids):
    """Sort keys of non-negative ids in decimal String order: the left-aligned 19-digit decimal, then the
    digit count (a prefix sorts first), as jg_cc.hip ranks them."""
    ids = ids.astype(np.uint64)
    digits = np.ones(len(ids), np.int64)
    for k in range(1, 19):
        digits += ids >= np.uint64(10 ** k)
    padded = ids * (np.uint64(10) ** (19 - digits).astype(np.uint64))
    return padded, digits


def host_census(comp, min_population):
    ids, pops = np.unique(comp, return_counts=True)
    padded, digits = string_order(ids)
    order = np.lexsort((digits, padded, -pops))
    ids, pops = ids[order], pops[order].astype(np.int64)
    keep = pops >= min_population
    return len(order), int(pops[0]), ids[keep], pops[keep]


def census_bytes(n, lrows, listed, largest, min_population):
    """The census byte model (jg_census.hip, census_of_labels)."""
    passes = (max(int(largest).bit_length(), 1) + 7) // 8
    suffix = 8.0 * (n - lrows) if min_population == 1 else 0.0
    return 12.0 * n + 4.0 * lrows + suffix + listed * (48.0 + 32.0 * passes)


def temporary_bytes(n, listed):
    """Peak device temporaries of the census: the counters, the tile counts and offsets, the sort records and
    the radix sort's second copy and digit counts.  (The held pairs, 16 B per listed component, stay.)"""
    tiles = -(-n // CENSUS_TILE)
    rtiles = -(-listed // RADIX_TILE)
    return 4 * n + 12 * tiles + 24 + 24 * listed + rtiles * 256 * 12


def one_scale(scale, edgefactor, reps):
    import janusgraph_amd as jg
    ctx = jg.Context((0,))
    n = 1 << scale
    g = ctx.build_rmat(scale, edgefactor, 0x5EED + scale, flags=jg.ADJ_BOTH)
    line = {"workload": f"cc_census_rmat{scale}_ef{edgefactor}", "vertices": n, "reps": reps}
    # ---- the parent route ----
    wall, call, comp_ms = [], [], []
    comp = it0 = None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        comp, it0 = g.connected_components()
        t1 = time.perf_counter()
        st = ctx.stats()
        ids, pops = np.unique(comp, return_counts=True)
        t2 = time.perf_counter()
        if rep:
            wall.append((t2 - t0) * 1e3)
            call.append((t1 - t0) * 1e3)
            comp_ms.append(st["compute_ms"])
    line["handback"] = {"wall_ms": med(wall), "wall_ms_range": rng_of(wall), "call_wall_ms": med(call),
                        "call_wall_ms_range": rng_of(call), "compute_ms": med(comp_ms),
                        "compute_ms_range": rng_of(comp_ms), "bytes_handed_back": 8 * n, "iterations": it0}
    # ---- the census ----
    for mp in (1, 2):
        want = host_census(comp, mp)
        wall, cms, cmp_ms = [], [], []
        got = st = None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            got = g.cc_census(mp)
            t1 = time.perf_counter()
            if rep:
                wall.append((t1 - t0) * 1e3)
        for rep in range(reps + 1):  # the device times of the call alone (the stats are the last call's)
            it, nc, nl, largest, ms = g.cc_census_build(mp)
            st = ctx.stats()
            if rep:
                cms.append(ms)
                cmp_ms.append(st["compute_ms"])
        g.cc_census_release()
        it, nc, largest, vids, pops = got
        assert (it, nc, largest) == (it0, want[0], want[1]), "the two routes disagree on the totals"
        assert np.array_equal(vids, want[2]) and np.array_equal(pops, want[3]), "the two routes' censuses differ"
        listed = len(vids)
        # rows the program labelled: every vertex with an edge (the others are the edgeless suffix)
        lrows = n - int(np.count_nonzero(g.degrees() == 0)) if mp == 1 else line["census_1"]["labelled_rows"]
        model = census_bytes(n, lrows, listed, largest, mp)
        c = med(cms)
        line[f"census_{mp}"] = {
            "wall_ms": med(wall), "wall_ms_range": rng_of(wall), "census_ms": c, "census_ms_range": rng_of(cms),
            "compute_ms": med(cmp_ms), "compute_ms_range": rng_of(cmp_ms), "components": nc, "listed": listed,
            "largest": largest, "labelled_rows": lrows, "bytes_read_back": 16 * listed,
            "roofline": {"bound": "hbm", "bytes": model, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "achieved": round(model / (c * 1e-3) / 1e9, 1),
                         "frac": round(model / (c * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
            "temporary_bytes": temporary_bytes(n, listed),
            "wall_below_handback_by_ms": round(line["handback"]["wall_ms"] - med(wall), 3),
            "combined_ranges_ms": round((max(wall) - min(wall)) + (line["handback"]["wall_ms_range"][1]
                                                                    - line["handback"]["wall_ms_range"][0]), 3)}
    print(json.dumps(line), flush=True)
    g.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[20, 24, 26])
    ap.add_argument("--scale", type=int, default=0, help="run this one scale in this process")
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.scale:
        one_scale(args.scale, args.edgefactor, args.reps)
        return
    for s in args.scales:  # one fresh process per scale
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--scale", str(s), "--edgefactor",
                               str(args.edgefactor), "--reps", str(args.reps)])


if __name__ == "__main__":
    main()
