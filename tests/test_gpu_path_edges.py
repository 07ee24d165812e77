"""JG_ADJ_EDGE_INDEX (edge ordinals in the snapshot, jg_graph_neighbor_edges), the edge-listing predecessor DAGs
(jg_bfs_kept_dag_edges, jg_sssp_kept_dag_edges; janusgraph_amd/csrc/jg_build.hip, jg_pathdag.hip) and
ShortestPathVertexProgram's includeEdges through the computer.

What is expected comes from the caller's edge list and the host model of tests/test_path_edges_host.py (pinned
there against brute force).  Every DAG is checked three ways: against the plain DAG of the same inputs (same
vertices, order and values; collapsing each run of equal predecessors gives the plain lists), entry for entry
and in order against the reverse rows (jg_graph_neighbors + jg_graph_neighbor_edges) filtered by the model's
predicate, and as a set of (vertex, predecessor, ordinal) triples against the edge list alone.  Integers,
compared exactly.
"""
import json
import os

import numpy as np
import pytest

from test_path_edges_host import edge_dag, hop_depths, model_edge_paths
from test_weighted_paths_host import DIR_BOTH, DIR_IN, DIR_OUT, REVERSE, model_paths, weighted_dag

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = -(1 << 60)  # an unreached vertex in the model's value arrays


def flags_for(direction, weighted=False, index=True):
    import janusgraph_amd as jg
    E = jg._lib
    f = (E.ADJ_BOTH | (E.ADJ_WEIGHT_BOTH if weighted else 0)) if direction == DIR_BOTH else (E.ADJ_IN | E.ADJ_OUT)
    return f | (E.ADJ_EDGE_INDEX if index else 0)


def mask(n, *on):
    t = np.zeros(n, bool)
    t[list(on)] = True
    return t


def code(fn, *a, **k):
    import janusgraph_amd as jg
    with pytest.raises(jg.JanusGpuError) as e:
        fn(*a, **k)
    return e.value.code


def values(val):
    return np.asarray([NONE if x is None else x for x in val], np.int64)


def model_values(n, src, dst, w, direction, source):
    if w is None:
        return values(hop_depths(n, src, dst, direction, source))
    return values(weighted_dag(n, src, dst, w, direction, source)[0])


@pytest.fixture(scope="module")
def ctx():
    import janusgraph_amd as jg
    c = jg.Context((0,))
    yield c
    c.close()


def reverse_rows(g, rows, src, dst, direction):
    """(off, nbr, edge) of the rows predecessors are read from, every entry checked against the caller's edge
    list: its edge joins its neighbour to its row in an orientation a path may follow."""
    off, nbr = g.neighbors(rows, REVERSE[direction])
    eoff, edge = g.neighbor_edges(rows, REVERSE[direction])
    np.testing.assert_array_equal(off, eoff)
    owner = np.repeat(np.asarray(rows, np.int64), np.diff(off))
    e = edge.astype(np.int64)
    along = (src[e] == nbr) & (dst[e] == owner)
    against = (dst[e] == nbr) & (src[e] == owner)
    assert {DIR_OUT: along, DIR_IN: against, DIR_BOTH: along | against}[direction].all()
    return off, nbr, e, owner


def check_edge_dag(g, vid, n, src, dst, w, direction, source, target=None, max_distance=-1, keep=True, val=None):
    """Builds the plain and then the edge-listing DAG from `source` (vertex index; w None: the hop DAG of kept row
    0, else the weighted DAG) and checks the latter as the module docstring says.  Returns
    (vertex, value, off, pred, edge, plain entries)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    x = np.ones(len(src), np.int64) if w is None else np.asarray(w, np.int64)
    if w is None:
        if keep:
            g.bfs_keep([vid[source]], direction)
        plain_build, plain_read = (lambda: g.bfs_kept_dag_build(0, target)), g.bfs_kept_dag_read
        edges_build, read_edges = (lambda: g.bfs_kept_dag_edges_build(0, target)), g.bfs_kept_dag_read_edges
    else:
        if keep:
            g.sssp_keep(vid[source], direction)
        plain_build, plain_read = (lambda: g.sssp_kept_dag_build(target, max_distance)), g.sssp_kept_dag_read
        edges_build, read_edges = (lambda: g.sssp_kept_dag_edges_build(target, max_distance)), g.sssp_kept_dag_read_edges
    pnv, pne, pfar = plain_build()
    plain = plain_read(0, pnv)
    nv, ne, far = edges_build()
    stats = g.ctx.stats()
    print(f"edge dag: nv {nv} ne {ne} (plain {pne}) far {far} compute_ms {stats['compute_ms']:.3f} "
          f"launches {stats['kernel_launches']} edges {stats['edges_traversed']:.0f}")
    assert (nv, far) == (pnv, pfar) and ne >= pne
    vertex, value, off, pred = plain_read(0, nv)  # the plain read serves both kinds
    edge = read_edges(0, nv).astype(np.int64)
    assert len(vertex) == nv and len(off) == nv + 1 and off[0] == 0 and off[-1] == ne == len(pred) == len(edge)
    if nv == 0:
        assert (ne, far) == (0, -1)
        return vertex, value, off, pred, edge, pne
    # the plain DAG's vertices, order and values; each run of equal predecessors collapses to the plain entry
    np.testing.assert_array_equal(vertex, plain[0])
    np.testing.assert_array_equal(value, plain[1])
    grp = np.repeat(np.arange(nv), np.diff(off))
    first = np.ones(ne, bool)
    first[1:] = (pred[1:] != pred[:-1]) | (grp[1:] != grp[:-1])
    np.testing.assert_array_equal(pred[first], plain[3])
    np.testing.assert_array_equal(np.concatenate([[0], np.cumsum(np.bincount(grp[first], minlength=nv))]), plain[2])
    # the model's values, and the source's empty range
    val = model_values(n, src, dst, w, direction, source) if val is None else val
    np.testing.assert_array_equal(value, val[vertex])
    assert vertex[-1] == source and value[-1] == 0 and off[-1] == off[-2]
    # entry for entry, in order: the reverse rows filtered by the model's predicate
    roff, rnbr, redge, owner = reverse_rows(g, vertex, src, dst, direction)
    ok = (val[rnbr] != NONE) & (val[rnbr] + x[redge] == val[owner])
    rgrp = np.repeat(np.arange(nv), np.diff(roff))
    want_off = np.concatenate([[0], np.cumsum(np.bincount(rgrp[ok], minlength=nv))])
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(pred, rnbr[ok])
    np.testing.assert_array_equal(edge, redge[ok])
    assert not (pred == vertex[grp]).any()  # no self-loop
    # as a set, against the edge list alone: every followed arc u -> v of a DAG vertex v that the predicate passes
    on = np.zeros(n, bool)
    on[vertex] = True
    arcs = ([(src, dst)] if direction != DIR_IN else []) + ([(dst, src)] if direction != DIR_OUT else [])
    want = []
    for a, b in arcs:
        k = np.flatnonzero(on[b] & (val[a] != NONE) & (val[b] != NONE) & (val[a] + x == val[b]))
        want.append(np.stack([b[k], a[k], k], 1))
    want = np.concatenate(want)
    got = np.stack([vertex[grp].astype(np.int64), pred.astype(np.int64), edge], 1)
    order = lambda t: t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]  # noqa: E731
    np.testing.assert_array_equal(order(got), order(want))
    # the same call again: the same output
    assert edges_build() == (nv, ne, far)
    for a, b in zip(plain_read(0, nv), (vertex, value, off, pred)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(read_edges(0, nv), edge)
    return vertex, value, off, pred, edge, pne


def build(ctx, n, edges, direction, weighted=False):
    """edges: (u, v) or (u, v, w) rows over vertex indices.  Returns (graph, vid, src, dst, w or None)."""
    e = np.asarray(edges, np.int64).reshape(len(edges), -1)
    vid = (np.arange(n, dtype=np.int64) + 1) * 10
    w = e[:, 2].astype(np.int32) if weighted else None
    g = ctx.build(vid, vid[e[:, 0]], vid[e[:, 1]], w, flags=flags_for(direction, weighted))
    return g, vid, e[:, 0], e[:, 1], w


def lists_of(dag):
    vertex, _, off, pred, edge = dag[:5]
    return {int(v): list(zip(pred[off[j]:off[j + 1]].tolist(), edge[off[j]:off[j + 1]].tolist()))
            for j, v in enumerate(vertex)}


def device_order(g, direction):
    """order(v) for model_edge_paths: the (u, ordinal) pairs of v's reverse row as the device lists them."""
    def order(v):
        _, nbr = g.neighbors([v], REVERSE[direction])
        _, edge = g.neighbor_edges([v], REVERSE[direction])
        return list(zip(nbr.tolist(), edge.tolist()))
    return order


# ---------------- ordinals, edge for edge ----------------

GHOST = 999  # no vertex has this id


def multigraph9():
    """9 vertices; a triple 0 -> 1 (ordinals 0, 1, 7) and its reverse 1 -> 0 (3), self-loops on 2 and 6, two edges
    with a ghost endpoint in the middle chunk; three chunks, the last of one edge."""
    vid = (np.arange(9, dtype=np.int64) + 1) * 10
    v = lambda i: GHOST if i < 0 else int(vid[i])  # noqa: E731
    chunks = [[(0, 1), (0, 1), (2, 2), (1, 0), (3, 4)],
              [(4, 5), (-1, 3), (0, 1), (5, -1), (6, 6), (6, 7)],
              [(7, 8)]]
    ids = [(np.asarray([v(a) for a, _ in c], np.int64), np.asarray([v(b) for _, b in c], np.int64)) for c in chunks]
    flat = np.asarray([p for c in chunks for p in c], np.int64)
    return vid, ids, flat[:, 0], flat[:, 1]


def test_ordinals_edge_for_edge(ctx):
    import janusgraph_amd as jg
    E = jg._lib
    vid, chunks, si, di = multigraph9()
    flags = E.ADJ_IN | E.ADJ_OUT | E.ADJ_BOTH | E.ADJ_EDGE_INDEX
    b = ctx.builder()
    b.add_vertices(vid)
    for s, d in chunks:
        b.add_edges(s, d)
    g = b.finish(flags)
    b.close()
    g2 = ctx.build(vid, np.concatenate([s for s, _ in chunks]), np.concatenate([d for _, d in chunks]), flags=flags)
    assert g.info()["ghost_edges"] == 2 and g.info()["self_loops"] == 2 and g.info()["flags"] & E.ADJ_EDGE_INDEX
    real = np.flatnonzero((si >= 0) & (di >= 0))
    rows = np.arange(9)
    for direction in (DIR_OUT, DIR_IN, DIR_BOTH):
        off, nbr = g.neighbors(rows, direction)
        eoff, edge = g.neighbor_edges(rows, direction)
        np.testing.assert_array_equal(off, eoff)
        assert edge.dtype == np.uint32 and len(edge) == len(nbr) == len(real) * (2 if direction == DIR_BOTH else 1)
        e = edge.astype(np.int64)
        owner = np.repeat(rows, np.diff(off))
        out_entry = (si[e] == owner) & (di[e] == nbr)  # the row's vertex is the edge's source
        in_entry = (di[e] == owner) & (si[e] == nbr)
        assert {DIR_OUT: out_entry, DIR_IN: in_entry, DIR_BOTH: out_entry | in_entry}[direction].all()
        # exactly the non-ghost edges, twice each on BOTH (a self-loop: both entries in its one row)
        np.testing.assert_array_equal(np.sort(e), np.sort(np.tile(real, 2 if direction == DIR_BOTH else 1)))
        same_run = (owner[1:] == owner[:-1]) & (nbr[1:] == nbr[:-1])
        assert (e[1:][same_run] >= e[:-1][same_run]).all()              # inside a run ordinals ascend
        assert (e[1:][same_run & (owner[1:] != nbr[1:])] > e[:-1][same_run & (owner[1:] != nbr[1:])]).all()
        if direction == DIR_BOTH:
            assert e[off[2]:off[3]].tolist() == [2, 2] and e[off[6]:off[7]].tolist().count(9) == 2
            assert list(zip(nbr[off[1]:off[2]].tolist(), e[off[1]:off[2]].tolist())) == [(0, 0), (0, 1), (0, 3), (0, 7)]
        # the same graph in one call: identical arrays
        for a, c in zip(g2.neighbors(rows, direction) + g2.neighbor_edges(rows, direction), (off, nbr, eoff, edge)):
            np.testing.assert_array_equal(a, c)
        # size first, then fill; a subset of rows in the caller's order
        sub = np.asarray([6, 1, 1, 8])
        soff, sedge = g.neighbor_edges(sub, direction)
        assert np.diff(soff).tolist() == np.diff(off)[sub].tolist()
        assert sedge.tolist() == np.concatenate([edge[off[r]:off[r + 1]] for r in sub]).tolist()
    g.close()
    g2.close()


# ---------------- KATs on 4 vertices ----------------

S, A, B, T = 0, 1, 2, 3


def test_kat_diamond_with_a_doubled_side(ctx):
    import janusgraph_amd as jg
    edges = [(S, A), (S, B), (A, T), (B, T), (A, T)]
    for direction in (DIR_OUT, DIR_BOTH):
        g, vid, s, d, _ = build(ctx, 4, edges, direction)
        dag = check_edge_dag(g, vid, 4, s, d, None, direction, S, mask(4, T))
        assert sorted(lists_of(dag)[T]) == [(A, 2), (A, 4), (B, 3)] and dag[5] == 4 and len(dag[3]) == 5
        got, deepest = jg.computer.DevicePathDag(4).edge_paths(dag[:5], S, mask(4, T))
        want = model_edge_paths(4, s, d, None, direction, [S], [T], order=device_order(g, direction))
        assert got == want and deepest == 2
        assert sorted(got) == [[S, 0, A, 2, T], [S, 0, A, 4, T], [S, 1, B, 3, T]]
        g.close()


def test_kat_source_is_its_own_target(ctx):
    import janusgraph_amd as jg
    g, vid, s, d, _ = build(ctx, 4, [(S, A), (A, T), (A, T)], DIR_OUT)
    dag = check_edge_dag(g, vid, 4, s, d, None, DIR_OUT, S, mask(4, S))
    assert dag[0].tolist() == [S] and dag[1].tolist() == [0] and len(dag[3]) == len(dag[4]) == 0
    assert jg.computer.DevicePathDag(4).edge_paths(dag[:5], S, mask(4, S)) == ([[S]], 0)
    g.close()


def test_kat_nothing_reached(ctx):
    """An unreachable target (B is isolated) and an empty target mask: (0, 0, -1), and empty reads."""
    for weighted in (False, True):
        g, vid, s, d, w = build(ctx, 4, [(S, A, 1), (A, T, 2), (A, T, 2)], DIR_BOTH, weighted)
        for target in (mask(4, B), mask(4)):
            if weighted:
                g.sssp_keep(vid[S], DIR_BOTH)
                assert g.sssp_kept_dag_edges_build(target) == (0, 0, -1)
                dag = g.sssp_kept_dag_edges(target)
                assert len(g.sssp_kept_dag_read_edges(0, 0)) == 0
            else:
                g.bfs_keep([vid[S]], DIR_BOTH)
                assert g.bfs_kept_dag_edges_build(0, target) == (0, 0, -1)
                dag = g.bfs_kept_dag_edges(0, target)
                assert len(g.bfs_kept_dag_read_edges(0, 0)) == 0
            assert [len(a) for a in dag] == [0, 0, 1, 0, 0] and dag[2].tolist() == [0]
        g.close()


def test_kat_self_loop_on_the_way_is_never_listed(ctx):
    edges = [(S, A, 1), (A, A, 1), (A, T, 1), (T, T, 2)]
    for direction in (DIR_OUT, DIR_BOTH):
        for weighted in (False, True):
            g, vid, s, d, w = build(ctx, 4, edges, direction, weighted)
            dag = check_edge_dag(g, vid, 4, s, d, w, direction, S)
            assert lists_of(dag) == {T: [(A, 2)], A: [(S, 0)], S: []}
            g.close()


def test_kat_mixed_orientation_pair_under_both(ctx):
    """S -> A and A -> S: under BOTH both are edges from S to A; under OUT only the first is."""
    edges = [(S, A, 3), (A, S, 3), (A, T, 1)]
    for weighted in (False, True):
        g, vid, s, d, w = build(ctx, 4, edges, DIR_BOTH, weighted)
        assert lists_of(check_edge_dag(g, vid, 4, s, d, w, DIR_BOTH, S)) == {T: [(A, 2)], A: [(S, 0), (S, 1)], S: []}
        g.close()
        g, vid, s, d, w = build(ctx, 4, edges, DIR_OUT, weighted)
        assert lists_of(check_edge_dag(g, vid, 4, s, d, w, DIR_OUT, S)) == {T: [(A, 2)], A: [(S, 0)], S: []}
        g.close()


def test_kat_of_parallel_edges_only_the_lightest_are_tight(ctx):
    g, vid, s, d, w = build(ctx, 2, [(0, 1, 2), (0, 1, 3), (0, 1, 2), (0, 1, 4)], DIR_OUT, True)
    assert lists_of(check_edge_dag(g, vid, 2, s, d, w, DIR_OUT, 0)) == {1: [(0, 0), (0, 2)], 0: []}
    assert lists_of(check_edge_dag(g, vid, 2, s, d, None, DIR_OUT, 0)) == {1: [(0, 0), (0, 1), (0, 2), (0, 3)], 0: []}
    g.close()


# ---------------- a hub row across ranges ----------------

@pytest.mark.parametrize("direction", [DIR_OUT, DIR_BOTH])
def test_hub_row_across_ranges(ctx, direction):
    """Source -> 1500 middles -> sink, every middle -> sink edge tripled: the sink's 4500-entry row spans more
    than 4 ranges of 1024 entries, and its runs of 3 straddle the 64-lane steps (64 = 3 * 21 + 1) and the range
    ends (1024 = 3 * 341 + 1).  Hop: all 4500 are listed; weighted, with the middle one of each triple heavier:
    2 of 3."""
    k = 1500
    mid = np.arange(1, k + 1)
    sink = k + 1
    n = k + 2
    first = np.stack([np.zeros(k, np.int64), mid, np.ones(k, np.int64)], 1)
    triple = np.stack([np.repeat(mid, 3), np.full(3 * k, sink), np.tile([2, 3, 2], k)], 1)
    edges = np.concatenate([first, triple])
    g, vid, s, d, w = build(ctx, n, edges, direction, True)
    assert 3 * k > 4 * 1024
    for weights, per in ((None, 3), (w, 2)):
        dag = check_edge_dag(g, vid, n, s, d, weights, direction, 0, mask(n, sink))
        vertex, value, off, pred, edge, plain_ne = dag
        assert len(vertex) == n and vertex[0] == sink and plain_ne == 2 * k and len(pred) == k + per * k
        got_p, got_e = pred[off[0]:off[1]], edge[off[0]:off[1]]
        assert len(got_p) == per * k
        # runs of `per` equal predecessors with ascending ordinals, every middle once
        runs = got_p.reshape(k, per)
        assert (runs == runs[:, :1]).all() and len(np.unique(runs[:, 0])) == k
        want_e = k + 3 * (runs[:, :1] - 1) + (np.asarray([[0, 1, 2]]) if per == 3 else np.asarray([[0, 2]]))
        np.testing.assert_array_equal(got_e.reshape(k, per), want_e)
        _, entries = edge_dag(n, s, d, weights, direction, 0)
        assert sorted(zip(got_p.tolist(), got_e.tolist())) == entries[sink]
    g.close()


# ---------------- RMAT-14 against the model ----------------

@pytest.fixture(scope="module")
def rmat14(oracle_lib):
    """RMAT-14 (edgefactor 16) with random weights in [1, 255], the source its vertex of highest out-degree.
    Counted on the CPU from the generator's edges: to every reached vertex the hop DAGs list 53309 (OUT) and
    78366 (BOTH) entries against 49227 and 69419 distinct predecessors, the weighted ones 11244 and 13066 against
    11242 and 13058, so the parallel edges on shortest paths are there without doubling any."""
    from test_gpu_vdev import rmat_graph
    n, vid, s, t, _ = rmat_graph(oracle_lib, 14)
    w = np.random.default_rng(14).integers(1, 256, len(s)).astype(np.int32)
    source = int(np.bincount(s, minlength=n).argmax())
    vals = {}

    def val(direction, weighted):  # one model run per case, shared and left unchanged
        if (direction, weighted) not in vals:
            vals[direction, weighted] = model_values(n, s, t, w if weighted else None, direction, source)
            vals[direction, weighted].setflags(write=False)
        return vals[direction, weighted]

    return n, vid, s.astype(np.int64), t.astype(np.int64), w, source, val


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("direction", [DIR_OUT, DIR_BOTH])
def test_rmat14(ctx, rmat14, direction, weighted):
    n, vid, s, t, w, source, val = rmat14
    g = ctx.build(vid, vid[s], vid[t], w, flags=flags_for(direction, True))
    v = val(direction, weighted)
    every = check_edge_dag(g, vid, n, s, t, w if weighted else None, direction, source, val=v)
    assert len(every[0]) > n // 4
    assert len(every[3]) > every[5]  # ne_edges > ne_plain: parallel edges lie on shortest paths
    tg = mask(n, *np.random.default_rng(direction).choice(np.flatnonzero(v > 0), 1000, replace=False))
    some = check_edge_dag(g, vid, n, s, t, w if weighted else None, direction, source, tg, keep=False, val=v)
    assert 1000 < len(some[0]) < len(every[0]) and len(some[3]) >= some[5]
    g.close()


# ---------------- reads and lifetime ----------------

def test_ranged_reads(ctx, rmat14):
    n, vid, s, t, w, source, _ = rmat14
    g = ctx.build(vid, vid[s], vid[t], w, flags=flags_for(DIR_OUT, True))
    g.bfs_keep([vid[source]], DIR_OUT)
    g.sssp_keep(vid[source], DIR_OUT)
    for build_, read, read_edges, whole in (
            (lambda: g.bfs_kept_dag_edges_build(0), g.bfs_kept_dag_read, g.bfs_kept_dag_read_edges,
             lambda: g.bfs_kept_dag_edges(0)),
            (g.sssp_kept_dag_edges_build, g.sssp_kept_dag_read, g.sssp_kept_dag_read_edges, g.sssp_kept_dag_edges)):
        nv, ne, _ = build_()
        vertex, value, off, pred = read(0, nv)
        edge = read_edges(0, nv)
        assert len(edge) == ne == len(pred)
        cuts = [0, nv // 3, nv // 3 + 1, nv]
        parts = [read_edges(a, b - a) for a, b in zip(cuts, cuts[1:])]
        np.testing.assert_array_equal(np.concatenate(parts), edge)
        for (a, b), p in zip(zip(cuts, cuts[1:]), parts):
            np.testing.assert_array_equal(p, edge[off[a]:off[b]])
        assert len(read_edges(nv, 0)) == 0 and len(read_edges(0, 0)) == 0
        g.DAG_READ_ENTRIES = 1000  # Graph.*_kept_dag_edges' own ranges: dozens of reads here
        try:
            for a, b in zip(whole(), (vertex, value, off, pred, edge)):
                np.testing.assert_array_equal(a, b)
        finally:
            del g.DAG_READ_ENTRIES
    g.close()


def test_lifetime_and_errors(ctx):
    import janusgraph_amd as jg
    E = jg._lib
    edges = [(S, A, 1), (A, T, 2), (A, T, 2)]
    g, vid, s, d, w = build(ctx, 4, edges, DIR_BOTH, True)
    # nothing held
    assert code(g.bfs_kept_dag_read_edges, 0, 0) == E.JG_ERR_STATE
    assert code(g.sssp_kept_dag_read_edges, 0, 0) == E.JG_ERR_STATE
    assert code(g.bfs_kept_dag_edges_build, 0) == E.JG_ERR_ARG          # no kept row: as jg_bfs_kept_dag
    assert code(g.sssp_kept_dag_edges_build) == E.JG_ERR_STATE          # no plane: as jg_sssp_kept_dag
    g.bfs_keep([vid[S]], DIR_BOTH)
    g.sssp_keep(vid[S], DIR_BOTH)
    for plain_build, edges_build, read, read_edges in (
            (lambda: g.bfs_kept_dag_build(0), lambda: g.bfs_kept_dag_edges_build(0), g.bfs_kept_dag_read,
             g.bfs_kept_dag_read_edges),
            (g.sssp_kept_dag_build, g.sssp_kept_dag_edges_build, g.sssp_kept_dag_read, g.sssp_kept_dag_read_edges)):
        assert code(read_edges, 0, 0) == E.JG_ERR_STATE                 # a row / plane, no DAG yet
        assert plain_build()[:2] == (3, 2)
        assert code(read_edges, 0, 3) == E.JG_ERR_STATE                 # a plain DAG lists no edges
        assert edges_build()[:2] == (3, 3)                              # ... and is replaced by an edge DAG
        assert read(0, 3)[3].tolist() == [A, A, S] and read_edges(0, 3).tolist() == [1, 2, 0]
        assert read_edges(0, 1).tolist() == [1, 2] and read_edges(1, 2).tolist() == [0]
        for first, count in ((0, 4), (3, 1), (-1, 1), (0, -1)):
            assert code(read_edges, first, count) == E.JG_ERR_ARG
        assert plain_build()[:2] == (3, 2)                              # and the reverse
        assert read(0, 3)[3].tolist() == [A, S] and code(read_edges, 0, 3) == E.JG_ERR_STATE
        edges_build()
    # the two families hold their DAGs independently; a new keep or a release drops its family's
    assert g.bfs_kept_dag_read_edges(0, 3).tolist() == [1, 2, 0] == g.sssp_kept_dag_read_edges(0, 3).tolist()
    g.bfs_keep([vid[A]], DIR_BOTH)
    assert code(g.bfs_kept_dag_read_edges, 0, 0) == E.JG_ERR_STATE
    assert g.sssp_kept_dag_read_edges(0, 3).tolist() == [1, 2, 0]
    g.sssp_kept_release()
    assert code(g.sssp_kept_dag_read_edges, 0, 0) == E.JG_ERR_STATE
    g.close()
    # a graph built without the flag
    e = np.asarray(edges, np.int64)
    g = ctx.build(vid, vid[e[:, 0]], vid[e[:, 1]], e[:, 2].astype(np.int32), flags=flags_for(DIR_BOTH, True, index=False))
    g.bfs_keep([vid[S]], DIR_BOTH)
    g.sssp_keep(vid[S], DIR_BOTH)
    assert code(g.neighbor_edges, [0], DIR_BOTH) == E.JG_ERR_UNSUPPORTED
    assert code(g.bfs_kept_dag_edges_build, 0) == E.JG_ERR_UNSUPPORTED
    assert code(g.sssp_kept_dag_edges_build) == E.JG_ERR_UNSUPPORTED
    assert g.bfs_kept_dag_build(0)[:2] == (3, 2) and g.sssp_kept_dag_build()[:2] == (3, 2)
    assert code(g.bfs_kept_dag_read_edges, 0, 0) == E.JG_ERR_UNSUPPORTED
    assert code(g.sssp_kept_dag_read_edges, 0, 0) == E.JG_ERR_UNSUPPORTED
    g.close()
    # an adjacency that was not built, a bad direction, a row outside the graph
    g = ctx.build(vid, vid[e[:, 0]], vid[e[:, 1]], flags=E.ADJ_OUT | E.ADJ_EDGE_INDEX)
    assert g.neighbor_edges([S], DIR_OUT)[1].tolist() == [0]
    assert code(g.neighbor_edges, [S], DIR_IN) == E.JG_ERR_UNSUPPORTED
    assert code(g.neighbor_edges, [S], 0) == E.JG_ERR_ARG and code(g.neighbor_edges, [4], DIR_OUT) == E.JG_ERR_ARG
    g.close()


def test_build_refusals():
    import janusgraph_amd as jg
    E = jg._lib
    vid = (np.arange(4, dtype=np.int64) + 1) * 10
    src, dst = vid[[0, 1]], vid[[1, 2]]
    flags = E.ADJ_BOTH | E.ADJ_EDGE_INDEX
    ctx2 = jg.Context((0, 0))  # two logical shards
    try:
        assert code(ctx2.build, vid, src, dst, None, flags) == E.JG_ERR_UNSUPPORTED
        b = ctx2.builder()
        b.add_vertices(vid)
        b.add_edges(src, dst)
        assert code(b.finish, flags) == E.JG_ERR_UNSUPPORTED
        g = b.finish(E.ADJ_BOTH)  # the refusal left the builder usable
        assert g.info()["num_shards"] == 2 and g.info()["num_edges"] == 2
        g.close()
        b.close()
    finally:
        ctx2.close()
    ctx = jg.Context((0,))
    try:
        b = ctx.builder()  # edgestore rows
        b.add_rows(np.zeros(0, np.uint64), [0], b"", [0], [])
        assert code(b.finish, flags) == E.JG_ERR_UNSUPPORTED
        b.finish(E.ADJ_BOTH).close()
        b.close()
        assert code(ctx.build_edgestore, np.zeros(0, np.uint64), [0], b"", [0], [], flags=flags) == E.JG_ERR_UNSUPPORTED
        b = ctx.builder()  # a label scope
        b.keep_labels()
        b.add_vertices(vid)
        b.add_edges(src, dst, label=[7, 9])
        assert code(b.finish_labels, [7], flags) == E.JG_ERR_UNSUPPORTED
        g = b.finish_labels([7], E.ADJ_BOTH)
        assert g.info()["num_edges"] == 1
        g.close()
        b.close()
        assert code(ctx.build_rmat, 4, 4, 1, flags) == E.JG_ERR_UNSUPPORTED
        assert code(ctx.build, vid, src, dst, None, E.ADJ_EDGE_INDEX) == E.JG_ERR_ARG   # no adjacency asked for
        assert code(ctx.build, vid, src, dst, None, flags | 32) == E.JG_ERR_ARG        # an unknown bit
    finally:
        ctx.close()


def test_no_flag_no_change(ctx, rmat14):
    """Without the flag the snapshot and the plain DAGs are what the flagged build gives beside its ordinals: the
    same rows, the same DAG arrays, no ordinal bytes on the device."""
    import janusgraph_amd as jg
    n, vid, s, t, w, source, val = rmat14
    got = []
    for index in (False, True):
        g = ctx.build(vid, vid[s], vid[t], w, flags=flags_for(DIR_BOTH, True, index))
        info = g.info()
        assert bool(info["flags"] & jg._lib.ADJ_EDGE_INDEX) == index
        g.bfs_keep([vid[source]], DIR_BOTH)
        g.sssp_keep(vid[source], DIR_BOTH)
        rows = np.arange(0, n, 37)
        got.append((info["device_bytes"], g.neighbors(rows, DIR_BOTH), g.bfs_kept_dag(0), g.sssp_kept_dag()))
        g.close()
    (bytes0, nb0, hop0, wd0), (bytes1, nb1, hop1, wd1) = got
    assert bytes1 - bytes0 == 4 * 2 * int(((s >= 0) & (t >= 0)).sum())  # one uint32 per BOTH entry
    for a, b in zip(nb0 + hop0 + wd0, nb1 + hop1 + wd1):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(hop0[1], val(DIR_BOTH, False)[hop0[0]])
    np.testing.assert_array_equal(wd0[1], val(DIR_BOTH, True)[wd0[0]])


@pytest.mark.parametrize("pattern", ["ff", "2a"])
def test_poison(oracle_lib, monkeypatch, pattern):
    """The hop and weighted edge DAGs on RMAT-12 with every device allocation filled with a poison byte first:
    nothing the build, the passes or the reads touch is left unwritten."""
    import janusgraph_amd as jg
    from test_gpu_vdev import rmat_graph
    monkeypatch.setenv("JG_DEV_POISON", pattern)
    n, vid, s, t, _ = rmat_graph(oracle_lib, 12)
    w = np.random.default_rng(12).integers(1, 256, len(s)).astype(np.int32)
    source = int(np.bincount(s, minlength=n).argmax())
    c = jg.Context((0,))
    try:
        g = c.build(vid, vid[s], vid[t], w, flags=flags_for(DIR_BOTH, True))
        check_edge_dag(g, vid, n, s, t, None, DIR_BOTH, source)
        check_edge_dag(g, vid, n, s, t, w, DIR_BOTH, source)
        g.close()
    finally:
        c.close()


# ---------------- through the computer ----------------

def small_multigraph():
    """40 vertices, 120 edges: 100 seeded pairs (self-loops as they fall) and 20 repeats of earlier ones, half of
    them reversed."""
    import janusgraph_amd as jg
    rng = np.random.default_rng(7)
    graph = jg.InMemoryGraph()
    v = [graph.add_vertex() for _ in range(40)]
    pairs = [(int(a), int(b)) for a, b in zip(rng.integers(0, 40, 100), rng.integers(0, 40, 100))]
    for k in range(20):
        a, b = pairs[int(rng.integers(0, 100))]
        pairs.append((a, b) if k % 2 else (b, a))
    for a, b in pairs:
        graph.add_edge(v[a], v[b], "E")
    return graph, v


@pytest.mark.parametrize("max_distance", [None, 2])
@pytest.mark.parametrize("name,direction", [("both", DIR_BOTH), ("out", DIR_OUT)])
def test_computer_include_edges(ctx, name, direction, max_distance):
    import janusgraph_amd as jg
    graph, v = small_multigraph()
    assert len(graph.edges) == 120
    vid, src, dst, _ = graph.snapshot()
    index = {int(x): i for i, x in enumerate(vid.tolist())}
    si = np.asarray([index[int(x)] for x in src]), np.asarray([index[int(x)] for x in dst])
    sources = [v[3].id, v[17].id, v[0].id]
    targets = [x.id for x in v[::3]]

    def submit(include):
        b = jg.ShortestPathVertexProgram.build().source(*sources).target(*targets).edgeDirection(name)
        if include:
            b = b.includeEdges(True)
        if max_distance is not None:
            b = b.maxDistance(max_distance)
        return jg.GpuGraphComputer(graph, context=ctx).program(b.create(graph)).submit().result().memory()

    memory, plain = submit(True), submit(False)
    g = ctx.build(vid, src, dst, flags=flags_for(direction))  # the order entries are listed in
    order = device_order(g, direction)
    args = (len(vid), si[0], si[1])
    rest = ([index[x] for x in sources], [index[x] for x in targets], max_distance)
    want = model_edge_paths(*args, None, direction, *rest, order)
    want_plain = model_paths(*args, np.ones(len(src), np.int64), direction, *rest, lambda x: [u for u, _ in order(x)])
    g.close()
    got = memory.get(jg.ShortestPathVertexProgram.SHORTEST_PATHS)
    assert len(got) == len(want) > len(want_plain) >= 3  # parallel edges lie on these paths
    for p, q in zip(got, want):
        assert len(p) == len(q) and p[::2] == [int(vid[x]) for x in q[::2]]
        assert all(a is graph.edges[k] for a, k in zip(p[1::2], q[1::2]))  # the graph's own Edge objects
        for a, e, b in zip(p[::2], p[1::2], p[2::2]):
            assert (a, b) in {DIR_OUT: [(e.out_id, e.in_id)], DIR_BOTH: [(e.out_id, e.in_id), (e.in_id, e.out_id)]}[direction]
    assert plain.get(jg.ShortestPathVertexProgram.SHORTEST_PATHS) == [[int(vid[x]) for x in p] for p in want_plain]
    assert memory.getIteration() == plain.getIteration() == 1 + max(len(p) - 1 for p in want_plain)


def test_computer_golden_diamond_lists_its_one_edge(ctx):
    """OLAPTest.testShortestPath's diamond (tests/golden/spvp_diamond): v1, e, v2 with the one v1 -> v2 edge; a
    path from a vertex to itself is [vid]."""
    import janusgraph_amd as jg
    z = np.load(os.path.join(GOLD, "spvp_diamond.npz"))
    meta = json.load(open(os.path.join(GOLD, "spvp_diamond.json")))
    graph = jg.InMemoryGraph()
    v = {x: graph.add_vertex() for x in z["vid"].astype(np.int64).tolist()}
    edges = [graph.add_edge(v[a], v[b], "E") for a, b in zip(z["src"].tolist(), z["dst"].tolist())]
    s, t = v[meta["source_vid"]].id, v[meta["target_vid"]].id
    vp = jg.ShortestPathVertexProgram.build().source(s).target(t).includeEdges(True)
    memory = jg.GpuGraphComputer(graph, context=ctx).program(vp.create(graph)).submit().result().memory()
    got = memory.get(jg.ShortestPathVertexProgram.SHORTEST_PATHS)
    assert meta["expected_paths"] == [[256, 512]] and len(got) == 1 and len(got[0]) == 3
    assert got[0][0] == s and got[0][2] == t and got[0][1] is edges[0]
    assert (edges[0].out_id, edges[0].in_id) == (s, t) and memory.getIteration() == 2
    vp = jg.ShortestPathVertexProgram.build().source(s).target(s).includeEdges(True)
    memory = jg.GpuGraphComputer(graph, context=ctx).program(vp.create(graph)).submit().result().memory()
    assert memory.get(jg.ShortestPathVertexProgram.SHORTEST_PATHS) == [[s]] and memory.getIteration() == 1


def test_computer_refuses_a_sharded_context():
    import janusgraph_amd as jg
    graph, v = small_multigraph()
    c2 = jg.Context((0, 0))
    try:
        vp = jg.ShortestPathVertexProgram.build().source(v[0].id).includeEdges(True).create(graph)
        with pytest.raises(jg.ProgramNotSupported):
            jg.GpuGraphComputer(graph, context=c2).program(vp).submit().result()
    finally:
        c2.close()
