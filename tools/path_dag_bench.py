"""The shortest-path predecessor DAG of one kept BFS row: built on the device (jg_bfs_kept_dag) against the
host walk-back it replaces (jg_bfs_kept_row + PathDag.predecessors over jg_graph_neighbors), same process,
same graph, same kept row.  One JSON line out.

Cells: RMAT-<scale> (ef 16, BOTH), one source, target=None (every reached vertex) and 60 random reached
targets.  Per cell:
  device_wall_ms   host clock from the kept row to host arrays of predecessors (Graph.bfs_kept_dag: build +
                   read-back), median and range of --reps calls after one warm-up;
  compute_ms       the build alone (HIP events, jg_stats), and its byte model over it as a share of 8 TB/s;
  host_wall_ms     the parent route, --host-reps times; with --host-budget S a run is cut at the first
                   jg_graph_neighbors batch after S seconds and reported as "partial": the rows it finished of
                   the DAG's rows (deepest levels first) — a lower bound of the route's time.
  The lists are compared (every vertex the host route finished: the same predecessors in the same order).
--path N: the work-bound case instead — a path of N vertices with a chord every 7, the far end the only
  target (~6N/7 levels of one or two rows): compute_ms of the device build, to show that a level costs a
  launch and not a pass over the rows.
Usage: python tools/path_dag_bench.py [--scale 20] [--reps 5] [--host-reps 2] [--host-budget 60] [--path 1048576]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


class Budget(Exception):
    pass


def host_route(g, n, target, budget):
    """(predecessor dict or None when cut, wall seconds, rows finished)."""
    from janusgraph_amd.computer import PathDag
    t0 = time.perf_counter()
    done = [0]

    def neighbors(rows):
        if budget and time.perf_counter() - t0 > budget:
            raise Budget()
        out = g.neighbors(rows)
        done[0] += len(rows)  # counted when asked for: the batch's host loop follows
        return out
    try:
        depth = g.bfs_kept_row(0)
        pred, _, _ = PathDag(neighbors, n).predecessors(depth, target)
        return pred, time.perf_counter() - t0, len(pred)
    except Budget:
        return None, time.perf_counter() - t0, done[0]


def med(xs):
    return round(float(np.median(xs)), 3)


def rng_of(xs):
    return [round(float(min(xs)), 3), round(float(max(xs)), 3)]


def cell(g, ctx, n, target, reps, host_reps, budget):
    wall, comp = [], []
    st = dag = None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        dag = g.bfs_kept_dag(0, target)
        t1 = time.perf_counter()
        st = ctx.stats()
        if rep:
            wall.append((t1 - t0) * 1e3)
            comp.append(st["compute_ms"])
    vertex, vdepth, off, pred = dag
    host, finished, partial, hp = [], 0, False, None
    for _ in range(host_reps):
        hp, secs, finished = host_route(g, n, target, budget)
        host.append(secs * 1e3)
        partial = hp is None
        if partial:
            break
    checked = 0
    if hp is not None:
        assert set(hp) == set(vertex[vdepth >= 1].tolist()), "the two routes found other vertices"
        for j in np.random.default_rng(1).choice(len(vertex), min(len(vertex), 20000), replace=False).tolist():
            if vdepth[j] >= 1:
                assert pred[off[j]:off[j + 1]].tolist() == hp[int(vertex[j])].tolist(), int(vertex[j])
                checked += 1
    c = med(comp)
    out = {"dag_vertices": int(len(vertex)), "dag_entries": int(len(pred)), "deepest": int(st["levels"]),
           "row_entries_walked": int(st["edges_traversed"]), "launches": int(st["kernel_launches"]),
           "device_wall_ms": med(wall), "device_wall_ms_range": rng_of(wall),
           "compute_ms": c, "compute_ms_range": rng_of(comp),
           "roofline": {"bound": "hbm", "bytes": st["algorithmic_bytes"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "achieved": round(st["algorithmic_bytes"] / (c * 1e-3) / 1e9, 1),
                        "frac": round(st["algorithmic_bytes"] / (c * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
           "host_runs": len(host)}
    if host:
        out.update({"host_wall_ms": med(host), "host_wall_ms_range": rng_of(host), "host_partial": partial,
                    "host_rows_finished": int(finished), "lists_compared": checked,
                    "host_over_device": round(med(host) / med(wall), 1)})
    return out


def path_case(ctx, n):
    import janusgraph_amd as jg
    i = np.arange(n - 1, dtype=np.int64)
    chords = np.arange(0, n - 2, 7, dtype=np.int64)
    g = ctx.build(np.arange(n, dtype=np.int64), np.concatenate([i, chords]), np.concatenate([i + 1, chords + 2]),
                  flags=jg.ADJ_BOTH)
    t0 = time.perf_counter()
    g.bfs_keep([0])
    keep_s = time.perf_counter() - t0
    target = np.zeros(n, bool)
    target[n - 1] = True
    t0 = time.perf_counter()
    nv, ne, deepest = g.bfs_kept_dag_build(0, target)
    wall = time.perf_counter() - t0
    st = ctx.stats()
    g.close()
    return {"workload": f"path_dag_path{n}_chord7", "vertices": n, "deepest": deepest, "dag_vertices": nv,
            "dag_entries": ne, "bfs_keep_wall_ms": round(keep_s * 1e3, 1), "build_wall_ms": round(wall * 1e3, 1),
            "compute_ms": round(st["compute_ms"], 3), "launches": int(st["kernel_launches"]),
            "us_per_level": round(st["compute_ms"] * 1e3 / max(deepest, 1), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--host-budget", type=float, default=0, help="seconds after which a host run is cut (0: never)")
    ap.add_argument("--path", type=int, default=0, help="run the path-graph work-bound case of this many vertices instead")
    args = ap.parse_args()
    import janusgraph_amd as jg
    ctx = jg.Context((0,))
    if args.path:
        print(json.dumps(path_case(ctx, args.path)), flush=True)
        ctx.close()
        return
    n = 1 << args.scale
    g = ctx.build_rmat(args.scale, args.edgefactor, 0x5EED + args.scale, flags=jg.ADJ_BOTH)
    rng = np.random.default_rng(args.scale)
    cand = rng.choice(n, 256, replace=False).astype(np.int64)
    source = int(cand[np.flatnonzero(g.degrees(rows=cand) > 0)[0]])
    g.bfs_keep([source])
    keep_ms = ctx.stats()["compute_ms"]
    depth = g.bfs_kept_row(0)
    some = np.zeros(n, bool)
    some[rng.choice(np.flatnonzero(depth >= 1), 60, replace=False)] = True
    line = {"workload": f"path_dag_rmat{args.scale}_ef{args.edgefactor}", "source": source,
            "reached": int((depth >= 0).sum()), "bfs_keep_compute_ms": round(keep_ms, 3), "reps": args.reps,
            "host_budget_s": args.host_budget,
            "targets_60": cell(g, ctx, n, some, args.reps, args.host_reps, args.host_budget),
            "target_none": cell(g, ctx, n, None, args.reps, min(1, args.host_reps) if args.host_budget else args.host_reps,
                                args.host_budget)}
    print(json.dumps(line), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
