"""jg_sssp_keep / jg_sssp_kept_dag: weighted shortest distances kept on the device and their tight-edge
predecessor DAG (janusgraph_amd/csrc/jg_sssp.hip, jg_pathdag.hip), the weighted BOTH rows
(JG_ADJ_WEIGHT_BOTH), and ShortestPathVertexProgram's distanceProperty / edgeDirection through the computer.

What is expected comes from the host model of tests/test_weighted_paths_host.py (heapq Dijkstra over the edge
list; pinned there against brute force): the kept row against its distances, the DAG's vertex set against a
walk-back over its tight sets, and every predecessor LIST, order included, against the first occurrences of
jg_graph_neighbors(v, reverse direction) filtered by the model's tight set.  Integers, compared exactly.
"""
import json
import os

import numpy as np
import pytest

from test_weighted_paths_host import DIR_BOTH, DIR_IN, DIR_OUT, REVERSE, model_paths, weighted_dag

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ABSENT = np.iinfo(np.int64).min


def flags_for(direction):
    import janusgraph_amd as jg
    return (jg._lib.ADJ_BOTH | jg._lib.ADJ_WEIGHT_BOTH) if direction == DIR_BOTH else (jg.ADJ_IN | jg.ADJ_OUT)


def build(ctx, n, edges, direction, vid=None):
    """edges: (u, v, w) triples over vertex indices.  Returns (graph, vid, src, dst, w)."""
    e = np.asarray(edges, np.int64).reshape(-1, 3)
    vid = np.arange(n, dtype=np.int64) if vid is None else vid
    g = ctx.build(vid, vid[e[:, 0]], vid[e[:, 1]], e[:, 2].astype(np.int32), flags=flags_for(direction))
    return g, vid, e[:, 0], e[:, 1], e[:, 2]


def mask(n, *on):
    t = np.zeros(n, bool)
    t[list(on)] = True
    return t


def model_dag(n, dist, pred, target, max_distance):
    """(DAG vertex set as a sorted array, farthest) by a walk-back from the targets over the tight sets."""
    d = np.asarray([ABSENT if x is None else x for x in dist], np.int64)
    on = d != ABSENT
    if max_distance >= 0:
        on &= d <= max_distance
    if target is not None:
        on &= np.asarray(target, bool)
    if not on.any():
        return d, np.zeros(0, np.int64), -1
    farthest = int(d[on].max())
    seen = set(np.flatnonzero(on).tolist())
    stack = list(seen)
    while stack:
        for u in pred[stack.pop()]:
            if u not in seen:
                seen.add(u)
                stack.append(u)
    return d, np.asarray(sorted(seen), np.int64), farthest


def check_wdag(g, vid, n, model, direction, source, target=None, max_distance=-1, keep=True):
    """Keeps the distances from `source` (vertex index), builds and reads the DAG, and checks all of it against
    model = weighted_dag(...)'s (dist, pred).  Returns (vertex, vdist, off, pred)."""
    dist, tight = model
    if keep:
        g.sssp_keep(vid[source], direction)
    want_d, want_v, want_far = model_dag(n, dist, tight, target, max_distance)
    np.testing.assert_array_equal(g.sssp_kept_row(), want_d)
    nv, ne, far = g.sssp_kept_dag_build(target, max_distance)
    stats = g.ctx.stats()
    vertex, vdist, off, pred = g.sssp_kept_dag_read(0, nv)
    print(f"wdag: nv {nv} ne {ne} farthest {far} compute_ms {stats['compute_ms']:.3f} rounds {stats['levels']} "
          f"launches {stats['kernel_launches']} edges {stats['edges_traversed']:.0f}")
    assert (nv, far) == (len(want_v), want_far)
    assert len(vertex) == nv and len(off) == nv + 1 and off[0] == 0 and off[-1] == ne == len(pred)
    if nv == 0:
        assert ne == 0 and far == -1
        return vertex, vdist, off, pred
    np.testing.assert_array_equal(np.sort(vertex), want_v)            # the vertex set, each once
    np.testing.assert_array_equal(vdist, want_d[vertex])
    assert np.all(np.diff(vdist) <= 0) and vertex[-1] == source and vdist[0] == far and vdist[-1] == 0
    assert np.all(np.diff(off) >= 0) and off[-1] - off[-2] == 0       # the source: an empty range
    # every list with its order: the reverse rows' first occurrences, filtered by the model's tight set
    roff, rnbr = g.neighbors(vertex, REVERSE[direction])
    pairs = np.asarray(sorted(v * n + u for v in vertex.tolist() for u in tight[v]), np.int64)
    owner = np.repeat(vertex.astype(np.int64), np.diff(roff))
    is_tight = np.isin(owner * n + rnbr, pairs)
    for j, v in enumerate(vertex.tolist()):
        nb = rnbr[roff[j]:roff[j + 1]][is_tight[roff[j]:roff[j + 1]]]
        _, first = np.unique(nb, return_index=True)
        want = nb[np.sort(first)]
        assert pred[off[j]:off[j + 1]].tolist() == want.tolist(), v
        assert set(want.tolist()) == tight[v]
    # the same call again: the same output
    assert g.sssp_kept_dag_build(target, max_distance) == (nv, ne, far)
    for a, b in zip(g.sssp_kept_dag_read(0, nv), (vertex, vdist, off, pred)):
        np.testing.assert_array_equal(a, b)
    return vertex, vdist, off, pred


def lists_of(dag):
    vertex, _, off, pred = dag
    return {int(v): pred[off[j]:off[j + 1]].tolist() for j, v in enumerate(vertex)}


@pytest.fixture(scope="module")
def ctx():
    import janusgraph_amd as jg
    c = jg.Context((0,))
    yield c
    c.close()


def run_case(ctx, n, edges, direction, source, target=None, max_distance=-1):
    g, vid, s, d, w = build(ctx, n, edges, direction)
    try:
        model = weighted_dag(n, s, d, w, direction, source)
        return check_wdag(g, vid, n, model, direction, source, target, max_distance)
    finally:
        g.close()


S, A, T, X = 0, 1, 2, 3  # vertex 3 is isolated


def triangle(direct):
    return [(S, A, 1), (A, T, 1), (S, T, direct)]


def test_kat_heavier_direct_edge_is_not_a_path(ctx):
    dag = run_case(ctx, 4, triangle(3), DIR_BOTH, S, mask(4, T))
    assert lists_of(dag) == {T: [A], A: [S], S: []} and dag[1].tolist() == [2, 1, 0]


def test_kat_tie_spans_two_hop_levels(ctx):
    """t's predecessors are a (hop depth 1) and s (hop depth 0): a sweep by hop levels cannot list both."""
    dag = run_case(ctx, 4, triangle(2), DIR_BOTH, S, mask(4, T))
    lists = lists_of(dag)
    assert sorted(lists[T]) == [S, A] and lists[A] == [S] and lists[S] == [] and len(dag[3]) == 3


def test_kat_source_is_a_target(ctx):
    dag = run_case(ctx, 4, triangle(3), DIR_BOTH, S, mask(4, S))
    assert dag[0].tolist() == [S] and dag[1].tolist() == [0] and len(dag[3]) == 0


def test_kat_unreachable_target(ctx):
    dag = run_case(ctx, 4, triangle(3), DIR_BOTH, S, mask(4, X, A))
    assert sorted(dag[0].tolist()) == [S, A]


def test_kat_no_target_reached(ctx):
    for target, bound in ((mask(4, X), -1), (mask(4), -1), (mask(4, T), 1)):
        g, vid, s, d, w = build(ctx, 4, triangle(3), DIR_BOTH)
        g.sssp_keep(vid[S], DIR_BOTH)
        assert g.sssp_kept_dag_build(target, bound) == (0, 0, -1)
        vertex, vdist, off, pred = g.sssp_kept_dag_read(0, 0)
        assert len(vertex) == 0 and off.tolist() == [0] and len(pred) == 0
        g.close()


def test_kat_max_distance_is_inclusive(ctx):
    kept = run_case(ctx, 4, triangle(3), DIR_BOTH, S, mask(4, T), max_distance=2)
    assert kept[0].tolist()[0] == T and len(kept[0]) == 3
    cut = run_case(ctx, 4, triangle(3), DIR_BOTH, S, mask(4, T), max_distance=1)
    assert len(cut[0]) == 0
    every = run_case(ctx, 4, triangle(3), DIR_BOTH, S, None, max_distance=1)
    assert sorted(every[0].tolist()) == [S, A]


def test_kat_three_directions_three_dags(ctx):
    #   0 -> 1 (1), 1 -> 2 (1), 2 -> 0 (1), 0 -> 2 (5), 3 -> 0 (1)
    edges = [(0, 1, 1), (1, 2, 1), (2, 0, 1), (0, 2, 5), (3, 0, 1)]
    out = lists_of(run_case(ctx, 4, edges, DIR_OUT, 0))
    inn = lists_of(run_case(ctx, 4, edges, DIR_IN, 0))
    both = lists_of(run_case(ctx, 4, edges, DIR_BOTH, 0))
    assert out == {2: [1], 1: [0], 0: []}
    assert inn == {1: [2], 2: [0], 3: [0], 0: []}
    assert both == {1: [0], 2: [0], 3: [0], 0: []}


def test_multi_edge_run(ctx):
    """Three parallel u - v edges 3, 5, 3 with 3 tight: u once.  And a run whose only tight entry is its last
    (weights 5, 4, 3 in edge order), under each direction's rows."""
    U, V = 0, 1
    for direction in (DIR_OUT, DIR_BOTH):
        dag = run_case(ctx, 3, [(U, V, 3), (U, V, 5), (U, V, 3), (V, 2, 1)], direction, U)
        assert lists_of(dag) == {2: [V], V: [U], U: []}
        dag = run_case(ctx, 3, [(U, V, 5), (U, V, 4), (U, V, 3), (V, 2, 1)], direction, U)
        assert lists_of(dag) == {2: [V], V: [U], U: []} and dag[1].tolist() == [4, 3, 0]
    # mixed orientations of the same pair under BOTH, and a self-loop on the way (never tight)
    dag = run_case(ctx, 3, [(V, U, 4), (U, V, 2), (V, V, 1), (V, U, 2), (2, V, 1)], DIR_BOTH, U)
    assert lists_of(dag) == {2: [V], V: [U], U: []}


def test_hub_row_spans_many_waves(ctx):
    """Source -> 5000 middles -> sink, every total equal (w and 20 - w), every middle -> sink edge doubled with a
    heavier twin alternately before and after it: the sink's 10000-entry row spans ~10 ranges of 1024 entries
    and lists 5000 predecessors, each once."""
    k = 5000
    mid = np.arange(1, k + 1)
    sink = k + 1
    w1 = mid % 9 + 1
    first = np.stack([np.zeros(k, np.int64), mid, w1], 1)
    tight = np.stack([mid, np.full(k, sink), 20 - w1], 1)
    twin = np.stack([mid, np.full(k, sink), 20 - w1 + 1 + mid % 3], 1)
    pair = np.where((mid % 2 == 0)[:, None, None], np.stack([twin, tight], 1), np.stack([tight, twin], 1))
    edges = np.concatenate([first, pair.reshape(-1, 3)])
    n = k + 2
    for direction in (DIR_OUT, DIR_BOTH):
        dag = run_case(ctx, n, edges, direction, 0, mask(n, sink))
        vertex, vdist, off, pred = dag
        assert len(vertex) == n and len(pred) == 2 * k and vertex[0] == sink and vdist[0] == 20
        got = pred[off[0]:off[1]]
        assert len(got) == k and len(np.unique(got)) == k
        assert 2 * k >= 9 * 1024  # the sink's row: >= 10 ranges


def test_many_rounds(ctx):
    """A 3000-vertex weighted path with a tight chord every 7 vertices (i -> i + 2 weighing what the two path
    edges weigh), the far end the only target: ~2600 rounds of one or two rows, many control batches."""
    n = 3000
    i = np.arange(n - 1)
    w = i % 5 + 1
    chords = np.arange(0, n - 2, 7)
    edges = np.concatenate([np.stack([i, i + 1, w], 1), np.stack([chords, chords + 2, w[chords] + w[chords + 1]], 1)])
    g, vid, s, d, ww = build(ctx, n, edges, DIR_OUT)
    model = weighted_dag(n, s, d, ww, DIR_OUT, 0)
    vertex, vdist, off, pred = check_wdag(g, vid, n, model, DIR_OUT, 0, mask(n, n - 1))
    st = g.ctx.stats()
    assert len(vertex) == n and len(pred) == n - 1 + len(chords)
    assert st["levels"] > 2000 and st["kernel_launches"] > 2000
    g.close()


@pytest.fixture(scope="module")
def rmat14(oracle_lib):
    from test_gpu_vdev import rmat_graph
    n, vid, s, t, _ = rmat_graph(oracle_lib, 14)
    w = np.random.default_rng(14).integers(1, 256, len(s)).astype(np.int32)
    source = int(np.bincount(s, minlength=n).argmax())
    models = {}

    def model(direction):  # one Dijkstra per direction, shared and left unchanged
        if direction not in models:
            models[direction] = weighted_dag(n, s, t, w, direction, source)
        return models[direction]

    return n, vid, s, t, w, source, model


@pytest.mark.parametrize("dist32", [2, 0])
@pytest.mark.parametrize("direction", [DIR_OUT, DIR_BOTH])
def test_rmat14(ctx, rmat14, direction, dist32):
    import janusgraph_amd as jg
    n, vid, s, t, w, source, model = rmat14
    jg._lib.tune_set("sd_dist32", dist32)
    try:
        g = ctx.build(vid, vid[s], vid[t], w, flags=flags_for(direction))
        m = model(direction)
        every = check_wdag(g, vid, n, m, direction, source)
        assert len(every[0]) > n // 4
        reached = np.flatnonzero(np.asarray([x is not None and x > 0 for x in m[0]]))
        tg = mask(n, *np.random.default_rng(direction).choice(reached, 1000, replace=False))
        some = check_wdag(g, vid, n, m, direction, source, tg, keep=False)
        assert 1000 < len(some[0]) < len(every[0])
        g.close()
    finally:
        jg._lib.tune_set("sd_dist32", 1)


def test_distances_past_32_bits(ctx):
    big = 2**31 - 1
    edges = [(i, i + 1, big) for i in range(6)] + [(0, 6, big)]
    dag = run_case(ctx, 7, edges, DIR_OUT, 0)
    assert dag[1].tolist()[0] == 5 * big > 2**32 and dag[0].tolist()[0] == 5
    assert lists_of(dag)[6] == [0]


def test_ranged_read(ctx, rmat14):
    n, vid, s, t, w, source, model = rmat14
    g = ctx.build(vid, vid[s], vid[t], w, flags=flags_for(DIR_OUT))
    g.sssp_keep(vid[source], DIR_OUT)
    nv, ne, _ = g.sssp_kept_dag_build()
    vertex, vdist, off, pred = g.sssp_kept_dag_read(0, nv)
    cuts = [0, nv // 3, nv // 3 + 1, nv]
    parts = [g.sssp_kept_dag_read(a, b - a) for a, b in zip(cuts, cuts[1:])]
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), vertex)
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), vdist)
    np.testing.assert_array_equal(np.concatenate([p[3] for p in parts]), pred)
    for (a, b), p in zip(zip(cuts, cuts[1:]), parts):  # absolute offsets
        np.testing.assert_array_equal(p[2], off[a:b + 1])
    empty = g.sssp_kept_dag_read(nv, 0)
    assert len(empty[0]) == 0 and empty[2].tolist() == [ne] and len(empty[3]) == 0
    g.DAG_READ_ENTRIES = 1000  # Graph.sssp_kept_dag's own ranges: dozens of reads here
    try:
        for a, b in zip(g.sssp_kept_dag(), (vertex, vdist, off, pred)):
            np.testing.assert_array_equal(a, b)
    finally:
        del g.DAG_READ_ENTRIES
    g.close()


def code(fn, *a, **k):
    import janusgraph_amd as jg
    with pytest.raises(jg.JanusGpuError) as e:
        fn(*a, **k)
    return e.value.code


def test_lifetime_and_errors(ctx):
    import janusgraph_amd as jg
    E = jg._lib
    g, vid, s, d, w = build(ctx, 4, triangle(3), DIR_BOTH)
    assert code(g.sssp_kept_row) == E.JG_ERR_STATE                 # before any keep
    assert code(g.sssp_kept_dag_build) == E.JG_ERR_STATE
    assert code(g.sssp_kept_dag_read, 0, 0) == E.JG_ERR_STATE
    g.sssp_keep(S, DIR_BOTH)
    assert code(g.sssp_kept_dag_read, 0, 0) == E.JG_ERR_STATE      # a plane, no DAG yet
    nv, ne, far = g.sssp_kept_dag_build()
    assert (nv, ne, far) == (3, 2, 2)
    assert code(g.sssp_kept_dag_read, 0, nv + 1) == E.JG_ERR_ARG
    assert code(g.sssp_kept_dag_read, nv, 1) == E.JG_ERR_ARG
    assert code(g.sssp_kept_dag_read, -1, 1) == E.JG_ERR_ARG
    assert code(g.sssp_keep, S, 0) == E.JG_ERR_ARG                 # a bad direction
    g.sssp_keep(A, DIR_BOTH)
    assert code(g.sssp_kept_dag_read, 0, 0) == E.JG_ERR_STATE      # dropped by a new keep
    assert g.sssp_kept_row().tolist() == [1, 0, 1, ABSENT]
    g.sssp_keep(12345, DIR_BOTH)                                   # not a vertex: every distance absent
    assert g.sssp_kept_row().tolist() == [ABSENT] * 4 and g.sssp_kept_dag_build() == (0, 0, -1)
    g.sssp_kept_release()
    assert code(g.sssp_kept_row) == E.JG_ERR_STATE                 # after the release
    assert code(g.sssp_kept_dag_build) == E.JG_ERR_STATE
    g.sssp_kept_release()                                          # nothing held: still JG_OK
    # BOTH rows without weights on them, and a direction whose rows were not built
    assert code(g.sssp_keep, S, DIR_OUT) == E.JG_ERR_UNSUPPORTED
    g.close()
    e = np.asarray(triangle(3), np.int64)
    v4 = np.arange(4, dtype=np.int64)
    g = ctx.build(v4, e[:, 0], e[:, 1], e[:, 2].astype(np.int32), flags=jg.ADJ_BOTH | jg.ADJ_OUT)
    assert code(g.sssp_keep, S, DIR_BOTH) == E.JG_ERR_UNSUPPORTED  # BOTH built without ADJ_WEIGHT_BOTH
    g.sssp_keep(S, DIR_OUT)
    assert g.sssp_kept_row().tolist() == [0, 1, 2, ABSENT]
    assert code(g.sssp_kept_dag_build) == E.JG_ERR_UNSUPPORTED     # the reverse (IN) rows were not built
    g.close()
    g = ctx.build(v4, e[:, 0], e[:, 1], flags=jg.ADJ_BOTH | jg.ADJ_OUT)
    assert code(g.sssp_keep, S, DIR_OUT) == E.JG_ERR_UNSUPPORTED   # an unweighted graph
    g.close()
    assert code(ctx.build, v4, e[:, 0], e[:, 1], None, jg.ADJ_BOTH | E.ADJ_WEIGHT_BOTH) == E.JG_ERR_ARG
    assert code(ctx.build, v4, e[:, 0], e[:, 1], e[:, 2].astype(np.int32), jg.ADJ_IN | E.ADJ_WEIGHT_BOTH) == E.JG_ERR_ARG
    assert code(ctx.build_rmat, 4, 4, 1, jg.ADJ_BOTH | E.ADJ_WEIGHT_BOTH) == E.JG_ERR_ARG
    zero = e.copy()
    zero[1, 2] = 0
    g = ctx.build(v4, zero[:, 0], zero[:, 1], zero[:, 2].astype(np.int32), flags=flags_for(DIR_BOTH))
    assert code(g.sssp_keep, S, DIR_BOTH) == E.JG_ERR_ARG          # a zero weight
    assert code(g.sssp_kept_row) == E.JG_ERR_STATE
    g.close()
    absent = e.copy().astype(np.int32)
    absent[1, 2] = E.WEIGHT_ABSENT
    g = ctx.build(v4, e[:, 0], e[:, 1], absent[:, 2], flags=flags_for(DIR_OUT))
    assert code(g.sssp_keep, S, DIR_OUT) == E.JG_ERR_ARG           # a crossed edge without the weight
    g.sssp_keep(T, DIR_OUT)                                        # not crossed from here: harmless
    assert g.sssp_kept_row().tolist() == [ABSENT, ABSENT, 0, ABSENT]
    g.close()


def test_weighted_both_rows_through_the_builder(ctx):
    """ADJ_WEIGHT_BOTH with a builder: chunks that carry weights give weighted BOTH rows (one chunk per edge
    here, and a label-scoped finish), chunks without are JG_ERR_ARG; a failed finish leaves the builder usable."""
    import janusgraph_amd as jg
    E = jg._lib
    e = np.asarray(triangle(2), np.int64)
    v4 = np.arange(4, dtype=np.int64)
    b = ctx.builder()
    b.add_vertices(v4)
    b.add_edges(e[:, 0], e[:, 1])
    assert code(b.finish, jg.ADJ_BOTH | E.ADJ_WEIGHT_BOTH) == E.JG_ERR_ARG
    b.finish(jg.ADJ_BOTH).close()
    b.close()
    for labelled in (False, True):
        b = ctx.builder()
        if labelled:
            b.keep_labels()
        b.add_vertices(v4)
        for k in range(len(e)):
            b.add_edges(e[k:k + 1, 0], e[k:k + 1, 1], e[k:k + 1, 2].astype(np.int32),
                        label=[7 if k < 2 else 9] if labelled else None)
        assert code(b.finish_labels if labelled else b.finish, *([[7]] if labelled else []),
                    jg.ADJ_IN | E.ADJ_WEIGHT_BOTH) == E.JG_ERR_ARG
        g = b.finish_labels([7], flags_for(DIR_BOTH)) if labelled else b.finish(flags_for(DIR_BOTH))
        edges = e[:2] if labelled else e  # the scope drops the direct s - t edge
        model = weighted_dag(4, edges[:, 0], edges[:, 1], edges[:, 2], DIR_BOTH, S)
        dag = check_wdag(g, v4, 4, model, DIR_BOTH, S, mask(4, T))
        assert sorted(lists_of(dag)[T]) == ([A] if labelled else [S, A])
        g.close()
        b.close()


def test_two_logical_shards_are_unsupported():
    import janusgraph_amd as jg
    E = jg._lib
    ctx2 = jg.Context((0, 0))
    g, vid, s, d, w = build(ctx2, 4, triangle(3), DIR_BOTH)
    assert g.info()["num_shards"] == 2
    assert code(g.sssp_keep, S, DIR_BOTH) == E.JG_ERR_UNSUPPORTED
    assert code(g.sssp_kept_dag_build) == E.JG_ERR_UNSUPPORTED
    assert code(g.sssp_kept_row) == E.JG_ERR_STATE
    g.close()
    ctx2.close()


def test_bfs_and_sssp_holdings_are_independent(ctx):
    import janusgraph_amd as jg
    g, vid, s, d, w = build(ctx, 4, triangle(2), DIR_BOTH)
    g.bfs_keep([S], jg.DIR_BOTH)
    hop = g.bfs_kept_dag(0)
    g.sssp_keep(S, DIR_BOTH)
    wdag = g.sssp_kept_dag(mask(4, T))
    # each family's row and DAG are still readable, and unchanged
    assert g.bfs_kept_row(0).tolist() == [0, 1, 1, -1]
    for a, b in zip(g.bfs_kept_dag_read(0, len(hop[0])), hop):
        np.testing.assert_array_equal(a, b)
    g.bfs_keep([A], jg.DIR_BOTH)             # a new BFS keep drops the BFS DAG only
    assert code(g.bfs_kept_dag_read, 0, 0) == jg._lib.JG_ERR_STATE
    for a, b in zip(g.sssp_kept_dag_read(0, len(wdag[0])), wdag):
        np.testing.assert_array_equal(a, b)
    assert g.sssp_kept_row().tolist() == [0, 1, 2, ABSENT]
    g.bfs_kept_dag_build(0)
    g.sssp_kept_release()                    # and the other way round
    assert len(g.bfs_kept_dag_read(0, 3)[0]) == 3 and g.bfs_kept_row(0).tolist() == [1, 0, 1, -1]
    g.close()


@pytest.mark.parametrize("pattern", ["ff", "2a"])
def test_poison(oracle_lib, monkeypatch, pattern):
    """Keep and DAG on RMAT-12 with every device allocation filled with a poison byte first: nothing either
    reads is left unwritten."""
    import janusgraph_amd as jg
    from test_gpu_vdev import rmat_graph
    monkeypatch.setenv("JG_DEV_POISON", pattern)
    n, vid, s, t, _ = rmat_graph(oracle_lib, 12)
    w = np.random.default_rng(12).integers(1, 256, len(s)).astype(np.int32)
    source = int(np.bincount(s, minlength=n).argmax())
    c = jg.Context((0,))
    try:
        g = c.build(vid, vid[s], vid[t], w, flags=flags_for(DIR_BOTH))
        check_wdag(g, vid, n, weighted_dag(n, s, t, w, DIR_BOTH, source), DIR_BOTH, source)
        g.close()
    finally:
        c.close()


# ---------------- through the computer ----------------

def small_weighted_graph():
    import janusgraph_amd as jg
    rng = np.random.default_rng(5)
    graph = jg.InMemoryGraph()
    v = [graph.add_vertex() for _ in range(40)]
    pairs = [(int(a), int(b), int(x)) for a, b, x in zip(rng.integers(0, 40, 120), rng.integers(0, 40, 120),
                                                         rng.integers(1, 5, 120))]
    for a, b, x in pairs:
        graph.add_edge(v[a], v[b], "E", weight=x)
    return graph, v, pairs


@pytest.mark.parametrize("max_distance", [None, 4])
@pytest.mark.parametrize("name,direction", [("out", DIR_OUT), ("both", DIR_BOTH)])
def test_computer_weighted(ctx, name, direction, max_distance):
    import janusgraph_amd as jg
    graph, v, pairs = small_weighted_graph()
    vid, src, dst, w = graph.snapshot(weight_property="weight")
    index = {int(x): i for i, x in enumerate(vid.tolist())}
    si = np.asarray([index[int(x)] for x in src]), np.asarray([index[int(x)] for x in dst])
    sources = [v[3].id, v[17].id, v[0].id]
    targets = [x.id for x in v[::3]]
    b = jg.ShortestPathVertexProgram.build().source(*sources).target(*targets).distanceProperty("weight")
    b = b.edgeDirection(name)
    if max_distance is not None:
        b = b.maxDistance(max_distance)
    memory = jg.GpuGraphComputer(graph, context=ctx).program(b.create(graph)).submit().result().memory()
    g = ctx.build(vid, src, dst, w, flags=flags_for(direction))  # the order predecessors are listed in

    def order(x):
        return g.neighbors([x], REVERSE[direction])[1].tolist()

    want = model_paths(len(vid), si[0], si[1], w, direction, [index[x] for x in sources],
                       [index[x] for x in targets], max_distance, order)
    g.close()
    got = memory.get(jg.ShortestPathVertexProgram.SHORTEST_PATHS)
    assert got == [[int(vid[x]) for x in p] for p in want] and len(want) >= 3
    assert memory.getIteration() == 1 + max(len(p) - 1 for p in want)


def host_bfs_paths(n, src, dst, sources, targets, order):
    """Hop-count shortest paths along u -> v by a plain host BFS and walk-back (unit weights in the model)."""
    return model_paths(n, src, dst, np.ones(len(src), np.int64), DIR_OUT, sources, targets, None, order)


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_computer_edge_direction_without_weights(devices):
    import janusgraph_amd as jg
    graph, v, pairs = small_weighted_graph()
    vid, src, dst, _ = graph.snapshot()
    index = {int(x): i for i, x in enumerate(vid.tolist())}
    si = np.asarray([index[int(x)] for x in src]), np.asarray([index[int(x)] for x in dst])
    sources = [v[3].id, v[17].id]
    targets = [x.id for x in v[::2]]
    c = jg.Context(devices)
    try:
        b = jg.ShortestPathVertexProgram.build().source(*sources).target(*targets).edgeDirection("out")
        memory = jg.GpuGraphComputer(graph, context=c).program(b.create(graph)).submit().result().memory()
        g = c.build(vid, src, dst, flags=jg.ADJ_IN | jg.ADJ_OUT)
        assert g.info()["num_shards"] == len(devices)

        def order(x):
            return g.neighbors([x], jg.DIR_IN)[1].tolist()

        want = host_bfs_paths(len(vid), si[0], si[1], [index[x] for x in sources], [index[x] for x in targets], order)
        g.close()
    finally:
        c.close()
    assert memory.get(jg.ShortestPathVertexProgram.SHORTEST_PATHS) == [[int(vid[x]) for x in p] for p in want]
    assert len(want) >= 3 and memory.getIteration() == 1 + max(len(p) - 1 for p in want)


def test_computer_refuses_what_it_cannot_run(ctx):
    import janusgraph_amd as jg
    for bad in ({"weight": 0}, {}):
        graph, v, _ = small_weighted_graph()
        graph.add_edge(v[0], v[1], "E", **bad)
        vp = jg.ShortestPathVertexProgram.build().source(v[0].id).distanceProperty("weight").create(graph)
        with pytest.raises(jg.ProgramNotSupported):
            jg.GpuGraphComputer(graph, context=ctx).program(vp).submit().result()
    graph, v, _ = small_weighted_graph()
    c2 = jg.Context((0, 0))
    try:
        vp = jg.ShortestPathVertexProgram.build().source(v[0].id).distanceProperty("weight").create(graph)
        with pytest.raises(jg.ProgramNotSupported):
            jg.GpuGraphComputer(graph, context=c2).program(vp).submit().result()
    finally:
        c2.close()


def test_default_program_is_unchanged_on_the_golden_diamond(ctx):
    """No new knob: OLAPTest.testShortestPath's diamond (tests/golden/spvp_diamond) gives its one path v1, v2
    and iteration 2, as before."""
    import janusgraph_amd as jg
    z = np.load(os.path.join(GOLD, "spvp_diamond.npz"))
    meta = json.load(open(os.path.join(GOLD, "spvp_diamond.json")))
    gvid = z["vid"].astype(np.int64).tolist()
    graph = jg.InMemoryGraph()
    v = {x: graph.add_vertex() for x in gvid}
    for a, b in zip(z["src"].tolist(), z["dst"].tolist()):
        graph.add_edge(v[a], v[b], "E")
    vp = jg.ShortestPathVertexProgram.build().source(v[meta["source_vid"]].id).target(v[meta["target_vid"]].id)
    memory = jg.GpuGraphComputer(graph, context=ctx).program(vp.create(graph)).submit().result().memory()
    want = [[v[x].id for x in p] for p in meta["expected_paths"]]
    assert memory.get(jg.ShortestPathVertexProgram.SHORTEST_PATHS) == want == [[v[256].id, v[512].id]]
    assert memory.getIteration() == 2
