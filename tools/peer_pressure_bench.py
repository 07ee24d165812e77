"""PeerPressureVertexProgram on the device (jg_peer_pressure) against the floor a pull superstep has: a
jg_combine_steps MIN superstep over the same IN adjacency, the fold with the same column stream and the same
kind of gather and a trivial reduction.  Same process, same graph.

One process per scale (a fresh child each; --scale N runs one scale in this process): RMAT-<scale>, ef 16, IN
adjacency, one GPU, outE votes, maxIterations 30.  Per scale, for unit and for distributed strength, median and
range over --reps calls after one warm-up:
  vote_ms        HIP-event time of the vote kernels per vote superstep (kernel_ms_total / levels)
  votes, iterations, clusters
  roofline       the unit's byte model (csrc/jg_peer.hip) per second of vote kernel time, as a share of 8 TB/s
  compute_ms     the whole device run (ranks, row classes, supersteps, output)
and once per scale
  fold_ms        ms per jg_combine_steps MIN superstep (compute_ms / steps), --fold-steps supersteps
  vote_over_fold the ratio of the two
One JSON line per scale.
Usage: python tools/peer_pressure_bench.py [--scales 20 24] [--scale N] [--reps 3] [--fold-steps 10]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def med(xs):
    return round(float(np.median(xs)), 4)


def rng_of(xs):
    return [round(float(min(xs)), 4), round(float(max(xs)), 4)]


def one_scale(scale, edgefactor, reps, fold_steps, cap):
    import janusgraph_amd as jg
    ctx = jg.Context((0,))
    n = 1 << scale
    g = ctx.build_rmat(scale, edgefactor, 0x5EED + scale, flags=jg.ADJ_IN)
    info = g.info()
    line = {"workload": f"peer_pressure_rmat{scale}_ef{edgefactor}", "vertices": n, "edges": info["num_edges"],
            "reps": reps, "max_iterations": cap}
    # ---- the floor: a MIN fold over the same adjacency ----
    fold = []
    init = np.arange(n, dtype=np.int64)
    for rep in range(reps + 1):
        g.combine_steps(jg.DIR_IN, jg.COMBINE_MIN, fold_steps, init, int32_wrap=False)
        if rep:
            fold.append(ctx.stats()["compute_ms"] / fold_steps)
    line["fold_ms"] = med(fold)
    line["fold_ms_range"] = rng_of(fold)
    # ---- the vote supersteps ----
    for name, distribute in (("unit", False), ("distribute", True)):
        per_vote, whole, st, clusters, it = [], [], None, None, 0
        for rep in range(reps + 1):
            clusters, it = g.peer_pressure(jg.DIR_OUT, distribute, cap)
            st = ctx.stats()
            if rep:
                per_vote.append(st["kernel_ms_total"] / max(st["levels"], 1))
                whole.append(st["compute_ms"])
        v = med(per_vote)
        model = st["algorithmic_bytes"] / max(st["levels"], 1)
        line[name] = {
            "vote_ms": v, "vote_ms_range": rng_of(per_vote), "votes": st["levels"], "iterations": it,
            "clusters": int(len(np.unique(clusters))), "compute_ms": med(whole), "compute_ms_range": rng_of(whole),
            "kernel_launches": st["kernel_launches"],
            "roofline": {"bound": "hbm", "bytes_per_vote": model, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "achieved": round(model / (v * 1e-3) / 1e9, 1),
                         "frac": round(model / (v * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
            "vote_over_fold": round(v / line["fold_ms"], 2)}
    print(json.dumps(line), flush=True)
    g.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--scale", type=int, default=0, help="run this one scale in this process")
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fold-steps", type=int, default=10)
    ap.add_argument("--max-iterations", type=int, default=30)
    args = ap.parse_args()
    if args.scale:
        one_scale(args.scale, args.edgefactor, args.reps, args.fold_steps, args.max_iterations)
        return
    for s in args.scales:  # one fresh process per scale
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--scale", str(s), "--edgefactor",
                               str(args.edgefactor), "--reps", str(args.reps), "--fold-steps", str(args.fold_steps),
                               "--max-iterations", str(args.max_iterations)])


if __name__ == "__main__":
    main()
