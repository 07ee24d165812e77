"""ShortestPathVertexProgram's includeEdges knob (configuration parsing), and the host model of edge-listing
shortest paths that tests/test_gpu_path_edges.py checks the device against.

The model (edge_dag: per vertex the (predecessor, edge ordinal) entries of the hop or weighted predecessor DAG;
model_edge_paths: the enumeration v, e, v, ..., v) is pinned here against brute-force enumeration of every
simple edge sequence on the small seeded multigraphs of test_weighted_paths_host (self-loops, parallel edges,
mixed orientations, many ties), and against the vertex paths of that file's model.  No GPU.
"""
import os
import re
from collections import deque

import numpy as np
import pytest

from test_weighted_paths_host import DIR_BOTH, DIR_IN, DIR_OUT, model_paths, random_multigraph, weighted_dag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def followed_edges(src, dst, w, direction):
    """The (from, to, weight, ordinal) arcs a path may follow; the ordinal is the edge's position in src/dst."""
    out = []
    for e, (a, b, x) in enumerate(zip(np.asarray(src).tolist(), np.asarray(dst).tolist(), np.asarray(w).tolist())):
        if direction in (DIR_OUT, DIR_BOTH):
            out.append((a, b, x, e))
        if direction in (DIR_IN, DIR_BOTH):
            out.append((b, a, x, e))
    return out


def hop_depths(n, src, dst, direction, source):
    """depth[v] = edges of a shortest path source -> v following `direction` (None: unreached), by a plain BFS."""
    adj = [[] for _ in range(n)]
    for a, b, _, _ in followed_edges(src, dst, np.ones(len(src), np.int64), direction):
        adj[a].append(b)
    depth = [None] * n
    depth[source] = 0
    queue = deque([source])
    while queue:
        v = queue.popleft()
        for u in adj[v]:
            if depth[u] is None:
                depth[u] = depth[v] + 1
                queue.append(u)
    return depth


def edge_dag(n, src, dst, w, direction, source):
    """(val, entries).  w None: the hop DAG, val = depths and every followed arc u -> v with depth[u] == depth[v] - 1
    is an entry of v; else the weighted DAG, val = the smallest summed weights and every arc with
    val[u] + weight == val[v] is one.  entries[v] = the (u, ordinal) pairs, sorted: one per arc, so parallel
    edges each have their own and a self-loop (weights >= 1) never has one."""
    if w is None:
        val = hop_depths(n, src, dst, direction, source)
        x = np.ones(len(src), np.int64)
    else:
        val, _ = weighted_dag(n, src, dst, w, direction, source)
        x = w
    entries = [[] for _ in range(n)]
    for a, b, k, e in followed_edges(src, dst, x, direction):
        if val[a] is not None and val[b] is not None and val[a] + k == val[b]:
            entries[b].append((a, e))
    return val, [sorted(es) for es in entries]


def model_edge_paths(n, src, dst, w, direction, sources, targets=None, max_distance=None, order=None):
    """Every shortest path (w None: fewest edges; else smallest summed weight) from each source (in the given
    order) to each target (ascending index) within max_distance (inclusive), as [v, e, v, ..., v] of vertex
    indices and edge ordinals, first entry first.  order(v) -> the (u, ordinal) pairs of v's reverse row in the
    order entries are listed (default: sorted)."""
    out = []
    for s in sources:
        val, entries = edge_dag(n, src, dst, w, direction, s)
        for t in (range(n) if targets is None else sorted(set(targets))):
            if val[t] is None or (max_distance is not None and val[t] > max_distance):
                continue
            stack = [(t, [t])]
            while stack:
                v, suffix = stack.pop()
                if v == s:
                    out.append(list(reversed(suffix)))
                    continue
                have = set(entries[v])
                row = entries[v] if order is None else [ue for ue in order(v) if ue in have]
                for u, e in reversed(row):
                    stack.append((u, suffix + [e, u]))
    return out


def brute_force_edges(n, src, dst, w, direction, source):
    """{target: (smallest total, set of every simple edge sequence (v, e, v, ..., v) of that total)} by
    enumerating all simple paths, parallel edges apart (weights >= 1: a shortest path is simple)."""
    adj = [[] for _ in range(n)]
    for a, b, x, e in followed_edges(src, dst, w, direction):
        adj[a].append((b, x, e))
    best = {}

    def go(seq, on, total):
        v = seq[-1]
        cur = best.get(v)
        if cur is None or total < cur[0]:
            best[v] = (total, {tuple(seq)})
        elif total == cur[0]:
            cur[1].add(tuple(seq))
        for u, x, e in adj[v]:
            if u not in on:
                go(seq + [e, u], on | {u}, total + x)

    go([source], {source}, 0)
    return best


@pytest.mark.parametrize("seed", range(36))
def test_model_against_brute_force(seed):
    n, src, dst, w = random_multigraph(seed)
    ones = np.ones(len(src), np.int64)
    for direction in (DIR_OUT, DIR_IN, DIR_BOTH):
        for source in range(n):
            for weights, brute_w in ((None, ones), (w, w)):  # the hop DAG is the unit-weight one
                want = brute_force_edges(n, src, dst, brute_w, direction, source)
                val, entries = edge_dag(n, src, dst, weights, direction, source)
                assert {v: d for v, d in enumerate(val) if d is not None} == {v: d for v, (d, _) in want.items()}
                for v in range(n):  # each vertex's entries are the last hops of its shortest edge sequences
                    last = sorted({(p[-3], p[-2]) for p in want[v][1] if len(p) > 1}) if v in want else []
                    assert entries[v] == last, (direction, source, v)
                    assert all(u != v for u, _ in entries[v])  # no self-loop
                paths = model_edge_paths(n, src, dst, weights, direction, [source])
                assert sorted(map(tuple, paths)) == sorted(p for _, ps in want.values() for p in ps)
                assert len(set(map(tuple, paths))) == len(paths)
                assert [p[-1] for p in paths] == sorted(p[-1] for p in paths)  # targets ascending
                for p in paths:  # every listed edge joins the vertices beside it, in a followed orientation
                    for i in range(1, len(p), 2):
                        a, b = int(src[p[i]]), int(dst[p[i]])
                        assert (p[i - 1], p[i + 1]) in {DIR_OUT: [(a, b)], DIR_IN: [(b, a)],
                                                        DIR_BOTH: [(a, b), (b, a)]}[direction]


@pytest.mark.parametrize("seed", range(36))
def test_consistent_with_the_vertex_paths(seed):
    """The number of edge paths is the sum, over the vertex paths, of the product of the numbers of qualifying
    parallel edges between consecutive vertices; and dropping the edges gives the vertex paths, each that often."""
    n, src, dst, w = random_multigraph(seed)
    ones = np.ones(len(src), np.int64)
    for direction in (DIR_OUT, DIR_IN, DIR_BOTH):
        for source in range(n):
            for weights, vertex_w in ((None, ones), (w, w)):
                _, entries = edge_dag(n, src, dst, weights, direction, source)
                vertex_paths = model_paths(n, src, dst, vertex_w, direction, [source])
                edge_paths = model_edge_paths(n, src, dst, weights, direction, [source])
                total = 0
                for p in vertex_paths:
                    ways = 1
                    for u, v in zip(p, p[1:]):
                        ways *= sum(1 for a, _ in entries[v] if a == u)
                    assert ways >= 1
                    assert sum(1 for q in edge_paths if q[::2] == p) == ways
                    total += ways
                assert len(edge_paths) == total


def test_model_kats():
    # a diamond 0 -> {1, 2} -> 3 with the 1 -> 3 side doubled: three edge paths, two vertex paths
    src, dst = [0, 0, 1, 2, 1], [1, 2, 3, 3, 3]
    assert model_edge_paths(4, src, dst, None, DIR_OUT, [0], [3]) == [[0, 0, 1, 2, 3], [0, 0, 1, 4, 3], [0, 1, 2, 3, 3]]
    assert model_edge_paths(4, src, dst, None, DIR_OUT, [0], [0]) == [[0]]
    assert model_edge_paths(4, src, dst, None, DIR_IN, [0], [3]) == []
    # weighted: of three parallel edges 2, 3, 2 the two lightest are listed
    got = model_edge_paths(2, [0, 0, 0], [1, 1, 1], np.asarray([2, 3, 2]), DIR_OUT, [0], [1])
    assert got == [[0, 0, 1], [0, 2, 1]]
    # a u -> v / v -> u pair under BOTH lists both edges, a self-loop on the way none
    assert model_edge_paths(2, [0, 1, 1], [1, 0, 1], None, DIR_BOTH, [0], [1]) == [[0, 0, 1], [0, 1, 1]]


# ---------------- the program's configuration ----------------

def test_builder_stores_include_edges():
    import janusgraph_amd as jg
    P = jg.ShortestPathVertexProgram
    vp = P.build().source(1).target(2).includeEdges(True).edgeDirection("out").create()
    assert vp.configuration["includeEdges"] is True and vp.include_edges is True
    again = P(vp.store_state())  # storeState / loadState round trip
    assert again.include_edges is True and again.edge_direction == "out" and again.distance_property is None
    assert P.build().includeEdges(False).create().include_edges is False
    assert P({"includeEdges": True}).include_edges is True  # accepted without a distanceProperty


def test_include_edges_is_absent_by_default():
    import janusgraph_amd as jg
    vp = jg.ShortestPathVertexProgram.build().source(1).create()
    assert vp.include_edges is False and "includeEdges" not in vp.configuration


def test_include_edges_with_a_distance_property_is_still_refused():
    import janusgraph_amd as jg
    P = jg.ShortestPathVertexProgram
    with pytest.raises(ValueError):
        P({"includeEdges": True, "distanceProperty": "weight"})
    with pytest.raises(ValueError):
        P.build().includeEdges(True).distanceProperty("weight").create()
    assert P({"includeEdges": False, "distanceProperty": "weight"}).include_edges is False


def test_bindings_declare_the_new_entry_points():
    from janusgraph_amd import _lib
    assert _lib.ADJ_EDGE_INDEX == 16
    for f in ("jg_graph_neighbor_edges", "jg_bfs_kept_dag_edges", "jg_bfs_kept_dag_read_edges",
              "jg_sssp_kept_dag_edges", "jg_sssp_kept_dag_read_edges"):
        assert f in _lib.EXPORTS
    for m in ("neighbor_edges", "bfs_kept_dag_edges_build", "bfs_kept_dag_read_edges", "bfs_kept_dag_edges",
              "sssp_kept_dag_edges_build", "sssp_kept_dag_read_edges", "sssp_kept_dag_edges"):
        assert callable(getattr(_lib.Graph, m))


def test_header_declares_the_flag_and_keeps_abi_3():
    text = open(os.path.join(ROOT, "include", "janusgpu.h")).read()
    assert re.search(r"^#define\s+JG_ABI_VERSION\s+3\s*$", text, re.M)
    assert re.search(r"^#define\s+JG_ADJ_EDGE_INDEX\s+16u\s*$", text, re.M)
    from janusgraph_amd import _lib
    assert _lib.ABI_VERSION == 3
