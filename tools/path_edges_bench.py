"""The edge-listing predecessor DAG (jg_bfs_kept_dag_edges) against the plain one (jg_bfs_kept_dag), and the
snapshot build with and without edge ordinals (JG_ADJ_EDGE_INDEX), alternated in one process.  One JSON line.

The graph is the test fixtures': RMAT (Graph500 Kronecker) edges from the oracle's generator as host arrays,
seed 11, built with JG_ADJ_BOTH; the source is the vertex of highest out-degree, the traversal JG_DIR_BOTH.
  build   --reps times, after one warm-up pair: a build without the flag, then one with it (build_ms of jg_stats,
          HIP events); the device bytes of each.
  dag     one kept depth row on each graph.  Per target set (1000 random reached vertices; every reached vertex),
          --reps rounds after one warm-up round, each round: the plain DAG on the flag-less graph, the plain DAG
          on the flagged graph, the edge-listing DAG on the flagged graph (compute_ms of jg_stats: the build of
          the DAG on the device, no read-back).  Reported: medians and ranges, the edges-to-plain ratio of the
          medians on the flagged graph, and the ratio of the two calls' byte models (algorithmic_bytes).
On a tree without the flag (an earlier commit) only the figures that exist there are measured: the flag-less
build and the plain DAG on it.  --plain-only measures just those on this tree too: the like-for-like process
to lay beside an earlier commit's (a process that also holds the flagged graph and alternates three calls
leaves each call a colder cache than one that repeats a single call on a single graph).
Usage: python tools/path_edges_bench.py [--scale 20] [--ef 16] [--reps 9] [--plain-only]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    return round(float(np.median(xs)), 4)


def rng_of(xs):
    return [round(float(min(xs)), 4), round(float(max(xs)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--plain-only", action="store_true", help="only the figures a tree without the flag has")
    a = ap.parse_args()
    import janusgraph_amd as jg
    from oracle import oracle
    oracle.build()
    E = jg._lib
    index = 0 if a.plain_only else getattr(E, "ADJ_EDGE_INDEX", 0)  # 0: a tree without the flag
    n = 1 << a.scale
    s, t = oracle.rmat_edges(a.scale, a.ef, 11)
    vid = (np.random.default_rng(a.scale).permutation(n).astype(np.int64) + 1) << 8
    src, dst = vid[s], vid[t]
    source = int(np.bincount(s, minlength=n).argmax())
    ctx = jg.Context((0,))
    line = {"workload": f"path_edges_rmat{a.scale}_ef{a.ef}", "n": n, "m": int(len(s)), "source_row": source,
            "direction": "both", "reps": a.reps, "edge_index": bool(index)}

    # ---- build ----
    kinds = [("plain", E.ADJ_BOTH)] + ([("edge_index", E.ADJ_BOTH | index)] if index else [])
    build_ms = {k: [] for k, _ in kinds}
    dev_bytes = {}
    for rep in range(a.reps + 1):
        for k, flags in kinds:
            g = ctx.build(vid, src, dst, flags=flags)
            if rep:
                build_ms[k].append(ctx.stats()["build_ms"])
            dev_bytes[k] = int(g.info()["device_bytes"])
            g.close()
    line["build"] = {k: {"build_ms": med(v), "build_ms_range": rng_of(v), "device_bytes": dev_bytes[k]}
                     for k, v in build_ms.items()}
    if index:
        line["build"]["edge_index_over_plain"] = round(med(build_ms["edge_index"]) / med(build_ms["plain"]), 4)

    # ---- dag ----
    graphs = {k: ctx.build(vid, src, dst, flags=flags) for k, flags in kinds}
    for g in graphs.values():
        g.bfs_keep([vid[source]], jg.DIR_BOTH)
    depth = graphs["plain"].bfs_kept_row(0)
    some = np.zeros(n, bool)
    some[np.random.default_rng(a.scale).choice(np.flatnonzero(depth > 0), 1000, replace=False)] = True
    calls = [("plain", "plain", "bfs_kept_dag_build")]
    if index:
        calls += [("plain_on_indexed", "edge_index", "bfs_kept_dag_build"),
                  ("edges", "edge_index", "bfs_kept_dag_edges_build")]
    for name, target in (("targets_1000", some), ("target_none", None)):
        ms = {c: [] for c, _, _ in calls}
        last = {}
        for rep in range(a.reps + 1):
            for c, k, fn in calls:
                nv, ne, deepest = getattr(graphs[k], fn)(0, target)
                st = ctx.stats()
                if rep:
                    ms[c].append(st["compute_ms"])
                last[c] = {"dag_vertices": int(nv), "dag_entries": int(ne), "deepest": int(deepest),
                           "row_entries_walked": int(st["edges_traversed"]), "launches": int(st["kernel_launches"]),
                           "model_bytes": st["algorithmic_bytes"]}
        cell = {}
        for c, _, _ in calls:
            cell[c] = dict(last[c], compute_ms=med(ms[c]), compute_ms_range=rng_of(ms[c]),
                           model_gbs=round(last[c]["model_bytes"] / (med(ms[c]) * 1e-3) / 1e9, 1))
        if index:
            cell["edges_over_plain"] = round(cell["edges"]["compute_ms"] / cell["plain_on_indexed"]["compute_ms"], 4)
            cell["model_edges_over_plain"] = round(cell["edges"]["model_bytes"] / cell["plain_on_indexed"]["model_bytes"], 4)
        line[name] = cell
    print(json.dumps(line), flush=True)
    for g in graphs.values():
        g.close()
    ctx.close()


if __name__ == "__main__":
    main()
