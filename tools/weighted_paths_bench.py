"""Weighted shortest paths on the device: (a) jg_sssp_keep against jg_shortest_distance over the same
adjacency, (b) the tight-edge predecessor DAG (jg_sssp_kept_dag) against the host alternative in the same
process, jg_sssp_kept_row plus a host walk-back over jg_graph_neighbors and the edge weights.  One JSON line.

The graph is tools/sd_bench.py's: Graph500 Kronecker edges, weights uniform in [1, wmax], the seed the row of
largest in-degree, so (a) can be laid beside sd_bench lines of other commits.  Built with JG_ADJ_IN |
JG_ADJ_OUT; direction IN (the adjacency jg_shortest_distance relaxes).
  (a) `runs` calls each of jg_shortest_distance (automatic delta, unbounded hops) and jg_sssp_keep, interleaved,
      after one warm call each: HIP-event compute_ms (jg_stats), the near passes, and whether the kept row
      equals the distances.
  (b) targets: 1000 random reached vertices, and target=None.  Per cell:
      device_wall_ms  host clock of Graph.sssp_kept_dag (build + read-back), median and range of --reps calls
                      after one warm-up;
      compute_ms      the build alone (HIP events), its byte model over it as a share of 8 TB/s, its rounds;
      host_wall_ms    sssp_kept_row + the walk-back: from the targets, the reverse (OUT) rows of the frontier
                      read through jg_graph_neighbors, an entry u of v tight when dist[u] + w == dist[v] with w
                      the smallest weight of the u -> v edges (a host dictionary of the edge list, built outside
                      the timed part), --host-reps times;
      the vertex sets and (sampled) predecessor lists of the two routes are compared.
--f64: the double-weight route beside the integer one, in one process (one JSON line): the same graph over BOTH and
over IN, weights 1..wmax as int32 and as the same values in doubles (jg_graph_set_weights_f64) on one graph.
  keep    `runs` calls each of jg_sssp_keep and jg_sssp_keep_f64, interleaved, after one warm call each;
  dags    jg_sssp_kept_dag and jg_sssp_kept_dag_f64 to 1000 random reached targets and to every reached vertex,
          `reps` builds each after one warm-up (HIP-event compute_ms, the library's byte model);
  checks  the two planes are equal (integer-valued doubles below 2^53 add exactly) and so are the two DAGs'
          predecessor lists, vertex by vertex.
  Byte model of a keep: every entry of the relaxed adjacency read once (4 B column, 4 or 8 B weight, an 8 B
  distance probe) and 32 B per row (the distance's init, the kept plane, a queue entry with its edge offset); the
  re-relaxed rows and the atomics are not counted, so it is a floor.
Usage: python tools/weighted_paths_bench.py [--scale 20] [--runs 5] [--reps 5] [--host-reps 1] [--wmax 255] [--f64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0
DEPTH_INF = 2**31 - 1
ROWS_PER_CALL = 1 << 16


def med(xs):
    return round(float(np.median(xs)), 3)


def rng_of(xs):
    return [round(float(min(xs)), 3), round(float(max(xs)), 3)]


def host_walk_back(g, jg, n, target, minw_key, minw_val):
    """(predecessor dict, DAG vertex count, wall seconds): the kept row copied out, then rounds of
    jg_graph_neighbors over the reverse rows; minw_key (sorted v * n + u) / minw_val: the lightest u -> v edge
    as the reverse row of v sees it."""
    t0 = time.perf_counter()
    dist = g.sssp_kept_row()
    on = dist != jg.DIST_ABSENT
    if target is not None:
        on &= target
    queued = on.copy()
    cur = np.flatnonzero(on)
    pred = {}
    while len(cur):
        nxt = []
        for f in range(0, len(cur), ROWS_PER_CALL):
            rows = cur[f:f + ROWS_PER_CALL]
            off, nbr = g.neighbors(rows, jg.DIR_OUT)
            owner = np.repeat(rows, np.diff(off))
            key = owner * n + nbr
            w = minw_val[np.searchsorted(minw_key, key)]
            tight = (dist[nbr] != jg.DIST_ABSENT) & (dist[nbr] + w == dist[owner])
            for i, v in enumerate(rows.tolist()):
                nb = nbr[off[i]:off[i + 1]][tight[off[i]:off[i + 1]]]
                _, first = np.unique(nb, return_index=True)
                pred[v] = nb[np.sort(first)]
            new = np.unique(nbr[tight])
            new = new[~queued[new]]
            queued[new] = True
            nxt.append(new)
        cur = np.concatenate(nxt) if nxt else np.zeros(0, np.int64)
    return pred, int(queued.sum()), time.perf_counter() - t0


def cell(g, ctx, jg, n, target, reps, host_reps, minw):
    wall, comp = [], []
    st = dag = None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        dag = g.sssp_kept_dag(target)
        t1 = time.perf_counter()
        st = ctx.stats()
        if rep:
            wall.append((t1 - t0) * 1e3)
            comp.append(st["compute_ms"])
    vertex, vdist, off, pred = dag
    host, hp, hv = [], None, 0
    for _ in range(host_reps):
        hp, hv, secs = host_walk_back(g, jg, n, target, *minw)
        host.append(secs * 1e3)
    checked = 0
    if hp is not None:
        assert hv == len(vertex) and set(hp) == set(vertex.tolist()), "the two routes found other vertices"
        for j in np.random.default_rng(1).choice(len(vertex), min(len(vertex), 20000), replace=False).tolist():
            assert pred[off[j]:off[j + 1]].tolist() == hp[int(vertex[j])].tolist(), int(vertex[j])
            checked += 1
    c = med(comp)
    out = {"dag_vertices": int(len(vertex)), "dag_entries": int(len(pred)), "rounds": int(st["levels"]),
           "row_entries_walked": int(st["edges_traversed"]), "launches": int(st["kernel_launches"]),
           "device_wall_ms": med(wall), "device_wall_ms_range": rng_of(wall),
           "compute_ms": c, "compute_ms_range": rng_of(comp),
           "roofline": {"bound": "hbm", "bytes": st["algorithmic_bytes"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "achieved": round(st["algorithmic_bytes"] / (c * 1e-3) / 1e9, 1),
                        "frac": round(st["algorithmic_bytes"] / (c * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
           "host_runs": len(host)}
    if host:
        out.update({"host_wall_ms": med(host), "host_wall_ms_range": rng_of(host), "lists_compared": checked,
                    "host_over_device": round(med(host) / med(wall), 1)})
    return out


def lists_by_vertex(dag):
    """(per-vertex predecessor counts, the predecessors concatenated) in vertex order: the DAG without the order
    of its equal distances."""
    vertex, _, off, pred = dag
    perm = np.argsort(vertex, kind="stable")
    cnt = np.diff(off)[perm]
    start = np.repeat(off[:-1][perm] - np.r_[0, np.cumsum(cnt)[:-1]], cnt)
    return vertex[perm], cnt, pred[start + np.arange(int(cnt.sum()))]


def f64_mode(a, jg, n, s, t, w, vid, seed):
    E = jg._lib
    ctx = jg.Context((0,))
    line = {"workload": f"f64_paths_rmat{a.scale}_ef{a.ef}_w1-{a.wmax}", "n": n, "m": len(s), "seed_row": seed,
            "runs": a.runs, "reps": a.reps}
    wf = w.astype(np.float64)
    for name, direction in (("both", jg.DIR_BOTH), ("in", jg.DIR_IN)):
        both = direction == jg.DIR_BOTH
        g = ctx.build(vid, vid[s], vid[t], weight=w,
                      flags=((jg.ADJ_BOTH | E.ADJ_WEIGHT_BOTH) if both else (jg.ADJ_IN | jg.ADJ_OUT)) | E.ADJ_EDGE_INDEX)
        g.set_weights_f64(wf)
        entries = int(g.info()["num_edges"]) * (2 if both else 1)
        g.sssp_keep(vid[seed], direction)
        g.sssp_keep_f64(vid[seed], direction)
        ms = {"int": [], "f64": []}
        passes = {}
        for _ in range(a.runs):
            for kind, keep in (("int", g.sssp_keep), ("f64", g.sssp_keep_f64)):
                keep(vid[seed], direction)
                st = ctx.stats()
                ms[kind].append(st["compute_ms"])
                passes[kind] = int(st["levels"])
        out = {"entries": entries}
        for kind, wbytes in (("int", 4), ("f64", 8)):
            b = entries * (12.0 + wbytes) + 32.0 * n
            c = med(ms[kind])
            out["keep_" + kind] = {"ms": [round(x, 4) for x in ms[kind]], "ms_median": c, "ms_range": rng_of(ms[kind]),
                                   "passes": passes[kind], "model_bytes": b,
                                   "frac_of_8TBs": round(b / (c * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        out["keep_f64_over_int"] = round(med(ms["f64"]) / med(ms["int"]), 3)
        out["keep_model_ratio"] = round((entries * 20.0 + 32.0 * n) / (entries * 16.0 + 32.0 * n), 3)
        g.sssp_keep(vid[seed], direction)
        row_i = g.sssp_kept_row()
        reached = (row_i != jg.DIST_ABSENT) & (row_i > 0)
        some = np.zeros(n, bool)
        some[np.random.default_rng(a.scale).choice(np.flatnonzero(reached), 1000, replace=False)] = True
        dags = {}
        for kind in ("int", "f64"):
            if kind == "f64":
                g.sssp_keep_f64(vid[seed], direction)
                row_f = g.sssp_kept_row_f64()
                out["planes_equal"] = bool(np.array_equal(
                    row_f, np.where(row_i == jg.DIST_ABSENT, np.inf, row_i.astype(np.float64))))
            build = g.sssp_kept_dag_build if kind == "int" else g.sssp_kept_dag_f64_build
            for cname, target in (("targets_1000", some), ("target_none", None)):
                comp = []
                for rep_ in range(a.reps + 1):
                    nv, ne, _ = build(target)
                    st = ctx.stats()
                    if rep_:
                        comp.append(st["compute_ms"])
                c = med(comp)
                out[f"dag_{kind}_{cname}"] = {
                    "dag_vertices": int(nv), "dag_entries": int(ne), "rounds": int(st["levels"]),
                    "row_entries_walked": int(st["edges_traversed"]), "compute_ms": c, "compute_ms_range": rng_of(comp),
                    "model_bytes": st["algorithmic_bytes"],
                    "frac_of_8TBs": round(st["algorithmic_bytes"] / (c * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
                dags[kind, cname] = lists_by_vertex((g.sssp_kept_dag if kind == "int" else g.sssp_kept_dag_f64)(target))
        for cname in ("targets_1000", "target_none"):
            out["dags_equal_" + cname] = bool(all(np.array_equal(x, y) for x, y in zip(dags["int", cname], dags["f64", cname])))
            out[f"dag_f64_over_int_{cname}"] = round(out[f"dag_f64_{cname}"]["compute_ms"] / out[f"dag_int_{cname}"]["compute_ms"], 3)
        assert out["planes_equal"] and out["dags_equal_targets_1000"] and out["dags_equal_target_none"], out
        line[name] = out
        g.close()
    print(json.dumps(line), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--wmax", type=int, default=255)
    ap.add_argument("--no-dag", action="store_true", help="part (a) only")
    ap.add_argument("--f64", action="store_true", help="the double-weight route beside the integer one")
    a = ap.parse_args()
    import janusgraph_amd as jg
    from sd_bench import kronecker
    n = 1 << a.scale
    s, t = kronecker(a.scale, a.ef, 0x55D + a.scale)
    w = np.random.default_rng(a.scale).integers(1, a.wmax + 1, len(s)).astype(np.int32)
    vid = (np.arange(n, dtype=np.int64) + 1) << 8
    seed = int(np.bincount(t, minlength=n).argmax())
    if a.f64:
        return f64_mode(a, jg, n, s, t, w, vid, seed)
    ctx = jg.Context((0,))
    g = ctx.build(vid, vid[s], vid[t], weight=w, flags=jg.ADJ_IN | (0 if a.no_dag else jg.ADJ_OUT))
    line = {"workload": f"weighted_paths_rmat{a.scale}_ef{a.ef}_w1-{a.wmax}", "n": n, "m": len(s), "seed_row": seed,
            "direction": "in", "runs": a.runs}
    # ---- (a) ----
    dist = g.shortest_distance(vid[seed], DEPTH_INF)
    g.sssp_keep(vid[seed], jg.DIR_IN)
    sd_ms, keep_ms, sd_passes, keep_passes = [], [], 0, 0
    for _ in range(a.runs):
        dist = g.shortest_distance(vid[seed], DEPTH_INF)
        st = ctx.stats()
        sd_ms.append(st["compute_ms"])
        sd_passes = st["levels"]
        g.sssp_keep(vid[seed], jg.DIR_IN)
        st = ctx.stats()
        keep_ms.append(st["compute_ms"])
        keep_passes = st["levels"]
    row = g.sssp_kept_row()
    line["sssp"] = {"shortest_distance_ms": [round(x, 4) for x in sd_ms], "shortest_distance_ms_median": med(sd_ms),
                    "sssp_keep_ms": [round(x, 4) for x in keep_ms], "sssp_keep_ms_median": med(keep_ms),
                    "passes": [int(sd_passes), int(keep_passes)], "reached": int((row != jg.DIST_ABSENT).sum()),
                    "kept_row_equals_distances": bool(np.array_equal(row, dist))}
    # ---- (b) ----
    if not a.no_dag:
        # the lightest u -> v edge, keyed as the OUT row of ... the reverse rows of direction IN are the OUT rows:
        # row v = an edge's source, entry u = its target
        key = s.astype(np.int64) * n + t
        order = np.argsort(key, kind="stable")
        ks, ws = key[order], w[order].astype(np.int64)
        start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        minw = (ks[start], np.minimum.reduceat(ws, start))
        rng = np.random.default_rng(a.scale)
        some = np.zeros(n, bool)
        some[rng.choice(np.flatnonzero((row != jg.DIST_ABSENT) & (row > 0)), 1000, replace=False)] = True
        line["reps"] = a.reps
        line["targets_1000"] = cell(g, ctx, jg, n, some, a.reps, a.host_reps, minw)
        line["target_none"] = cell(g, ctx, jg, n, None, a.reps, a.host_reps, minw)
    print(json.dumps(line), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
