"""ShortestPathVertexProgram's distanceProperty / edgeDirection knobs (configuration parsing), and the host
model of weighted shortest paths that tests/test_gpu_weighted_paths.py checks the device against.

The model (weighted_dag: heapq Dijkstra over the edge list, then the tight edges; model_paths: the
enumeration) is itself pinned here against brute-force enumeration of all simple paths on small seeded
multigraphs with self-loops, parallel edges and many ties.  No GPU.
"""
import heapq

import numpy as np
import pytest

DIR_OUT, DIR_IN, DIR_BOTH = 1, 2, 3
REVERSE = {DIR_OUT: DIR_IN, DIR_IN: DIR_OUT, DIR_BOTH: DIR_BOTH}


def followed(src, dst, w, direction):
    """The (from, to, weight) triples a path may follow: u->v along (OUT), against (IN) or either way (BOTH)."""
    out = []
    for a, b, x in zip(np.asarray(src).tolist(), np.asarray(dst).tolist(), np.asarray(w).tolist()):
        if direction in (DIR_OUT, DIR_BOTH):
            out.append((a, b, x))
        if direction in (DIR_IN, DIR_BOTH):
            out.append((b, a, x))
    return out


def weighted_dag(n, src, dst, w, direction, source):
    """(dist, pred): dist[v] = the smallest summed weight of a path source -> v following `direction` (None:
    unreached); pred[v] = the set of u with a followed edge u -> v of weight x and dist[u] + x == dist[v]."""
    adj = [[] for _ in range(n)]
    arcs = followed(src, dst, w, direction)
    for a, b, x in arcs:
        adj[a].append((b, x))
    dist = [None] * n
    heap = [(0, source)]
    while heap:
        d, v = heapq.heappop(heap)
        if dist[v] is not None:
            continue
        dist[v] = d
        for u, x in adj[v]:
            if dist[u] is None:
                heapq.heappush(heap, (d + x, u))
    pred = [set() for _ in range(n)]
    for a, b, x in arcs:
        if dist[a] is not None and dist[b] is not None and dist[a] + x == dist[b]:
            pred[b].add(a)
    return dist, pred


def model_paths(n, src, dst, w, direction, sources, targets=None, max_distance=None, order=None):
    """Every minimum-weight path from each source (in the given order) to each target (ascending index) within
    max_distance (inclusive), as vertex-index lists, first predecessor first.  order(v) -> v's reverse
    neighbours in the order predecessors are listed (default: ascending index)."""
    out = []
    for s in sources:
        dist, pred = weighted_dag(n, src, dst, w, direction, s)
        for t in (range(n) if targets is None else sorted(set(targets))):
            if dist[t] is None or (max_distance is not None and dist[t] > max_distance):
                continue

            def walk(v, suffix):
                if v == s:
                    out.append(list(reversed(suffix)))
                    return
                seen = set()
                for u in (sorted(pred[v]) if order is None else order(v)):
                    if u in pred[v] and u not in seen:
                        seen.add(u)
                        walk(u, suffix + [u])

            walk(t, [t])
    return out


def brute_force(n, src, dst, w, direction, source):
    """{target: (smallest weight, sorted list of every simple path of that weight)} by enumerating all simple
    paths (weights >= 1: a minimum-weight path is simple)."""
    adj = [[] for _ in range(n)]
    for a, b, x in followed(src, dst, w, direction):
        adj[a].append((b, x))
    best = {}

    def go(path, total):
        v = path[-1]
        cur = best.get(v)
        if cur is None or total < cur[0]:
            best[v] = (total, {tuple(path)})
        elif total == cur[0]:
            cur[1].add(tuple(path))
        for u, x in adj[v]:
            if u not in path:
                go(path + [u], total + x)

    go([source], 0)
    return {v: (d, sorted(p)) for v, (d, p) in best.items()}


def random_multigraph(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 8))
    m = int(rng.integers(1, 15))
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n, m)          # self-loops as they fall
    k = int(rng.integers(0, m + 1))      # and some parallel edges (same or reversed endpoints)
    for i in range(min(k, 3)):
        j = int(rng.integers(0, m))
        src[i], dst[i] = (src[j], dst[j]) if rng.integers(0, 2) else (dst[j], src[j])
    w = rng.integers(1, 5, m)
    return n, src.astype(np.int64), dst.astype(np.int64), w.astype(np.int32)


@pytest.mark.parametrize("seed", range(36))
def test_model_against_brute_force(seed):
    n, src, dst, w = random_multigraph(seed)
    assert n <= 7 and len(src) <= 14 and w.min() >= 1 and w.max() <= 4
    for direction in (DIR_OUT, DIR_IN, DIR_BOTH):
        for source in range(n):
            dist, pred = weighted_dag(n, src, dst, w, direction, source)
            want = brute_force(n, src, dst, w, direction, source)
            assert {v: d for v, d in enumerate(dist) if d is not None} == {v: d for v, (d, _) in want.items()}
            for v in range(n):
                last_hops = {p[-2] for p in want[v][1] if len(p) > 1} if v in want else set()
                assert pred[v] == last_hops, (direction, source, v)
            paths = model_paths(n, src, dst, w, direction, [source])
            assert sorted(map(tuple, paths)) == sorted(p for _, ps in want.values() for p in ps)
            assert len(set(map(tuple, paths))) == len(paths)
            # targets ascending, and the inclusive bound on the summed weight
            assert [p[-1] for p in paths] == sorted(p[-1] for p in paths)
            reached = sorted(d for d in dist if d is not None)
            bound = reached[len(reached) // 2]
            cut = model_paths(n, src, dst, w, direction, [source], max_distance=bound)
            assert cut == [p for p in paths if dist[p[-1]] <= bound]
            assert any(dist[p[-1]] == bound for p in cut)


def test_model_kats():
    # s - a - t with weights 1, 1 and a direct s - t: 3 leaves the two-hop path alone, 2 ties with it
    s, a, t = 0, 1, 2
    for direct, want in ((3, [[s, a, t]]), (2, [[s, a, t], [s, t]])):
        got = model_paths(3, [s, a, s], [a, t, t], [1, 1, direct], DIR_BOTH, [s], [t])
        assert sorted(got) == want
        dist, pred = weighted_dag(3, [s, a, s], [a, t, t], [1, 1, direct], DIR_BOTH, s)
        assert dist == [0, 1, 2] and pred[t] == ({a} if direct == 3 else {a, s}) and pred[s] == set()
    assert model_paths(3, [s, a], [a, t], [1, 1], DIR_OUT, [s], [s]) == [[s]]
    assert model_paths(3, [s, a], [a, t], [1, 1], DIR_IN, [s], [t]) == []


# ---------------- the program's configuration ----------------

def test_builder_stores_the_two_knobs():
    import janusgraph_amd as jg
    P = jg.ShortestPathVertexProgram
    vp = P.build().source(1).target(2).maxDistance(9).distanceProperty("weight").edgeDirection("out").create()
    assert vp.configuration["distanceProperty"] == "weight" and vp.configuration["edgeDirection"] == "out"
    assert (vp.distance_property, vp.edge_direction, vp.max_distance) == ("weight", "out", 9)
    assert P.build().edgeDirection("IN").create().edge_direction == "in"
    again = P(vp.store_state())  # storeState / loadState round trip
    assert (again.distance_property, again.edge_direction) == ("weight", "out")


def test_defaults_are_the_hop_program():
    import janusgraph_amd as jg
    vp = jg.ShortestPathVertexProgram.build().source(1).create()
    assert vp.distance_property is None and vp.edge_direction == "both"
    assert "distanceProperty" not in vp.configuration and "edgeDirection" not in vp.configuration


@pytest.mark.parametrize("bad", ["up", "", None, 3, "outE"])
def test_bad_direction_is_refused(bad):
    import janusgraph_amd as jg
    P = jg.ShortestPathVertexProgram
    with pytest.raises((ValueError, TypeError)):
        P.build().edgeDirection(bad)
    with pytest.raises(ValueError):
        P({"edgeDirection": bad})


@pytest.mark.parametrize("bad", ["", 7, ("a",)])
def test_bad_distance_property_is_refused(bad):
    import janusgraph_amd as jg
    P = jg.ShortestPathVertexProgram
    with pytest.raises(ValueError):
        P.build().distanceProperty(bad)
    with pytest.raises(ValueError):
        P({"distanceProperty": bad})


def test_include_edges_is_still_refused():
    import janusgraph_amd as jg
    with pytest.raises(ValueError):
        jg.ShortestPathVertexProgram({"includeEdges": True, "distanceProperty": "weight"})


def test_bindings_declare_the_new_entry_points():
    from janusgraph_amd import _lib
    assert _lib.ADJ_WEIGHT_BOTH == 8
    for f in ("jg_sssp_keep", "jg_sssp_kept_row", "jg_sssp_kept_release", "jg_sssp_kept_dag", "jg_sssp_kept_dag_read"):
        assert f in _lib.EXPORTS
    for m in ("sssp_keep", "sssp_kept_row", "sssp_kept_dag", "sssp_kept_release"):
        assert callable(getattr(_lib.Graph, m))
