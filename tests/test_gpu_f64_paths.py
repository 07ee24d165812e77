"""jg_graph_set_weights_f64 / jg_sssp_keep_f64 / jg_sssp_kept_dag_f64 (janusgraph_amd/csrc/jg_sssp.hip,
jg_pathdag.hip): shortest distances over double edge weights kept on the device, their tight-edge predecessor
DAGs, and ShortestPathVertexProgram with a Double distanceProperty through the computer.

What is expected comes from the host model of tests/test_weighted_paths_host.py fed Python floats (pinned against
brute force in tests/test_f64_paths_host.py): distances are the smallest left-to-right IEEE binary64 sums, an
edge is tight on an exact ==.  Planes are compared bit for bit (view(np.int64)); every predecessor list is
compared with its order (the reverse rows' first occurrences, filtered by the model's tight set), every
edge-listing DAG entry for entry.
"""
import numpy as np
import pytest

from test_weighted_paths_host import DIR_BOTH, DIR_IN, DIR_OUT, REVERSE, model_paths, weighted_dag

pytestmark = pytest.mark.gpu

INF = np.inf
NAMES = {DIR_OUT: "out", DIR_IN: "in", DIR_BOTH: "both"}


def flags_for(direction):
    import janusgraph_amd as jg
    E = jg._lib
    return (E.ADJ_BOTH if direction == DIR_BOTH else E.ADJ_IN | E.ADJ_OUT) | E.ADJ_EDGE_INDEX


def build(ctx, n, src, dst, w, direction, vid=None):
    vid = np.arange(n, dtype=np.int64) if vid is None else vid
    src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
    g = ctx.build(vid, vid[src], vid[dst], flags=flags_for(direction))
    g.set_weights_f64(np.asarray(w, np.float64))
    return g, vid


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def mask(n, *on):
    t = np.zeros(n, bool)
    t[list(on)] = True
    return t


def model_plane(dist):
    return np.asarray([INF if x is None else float(x) for x in dist], np.float64)


def model_dag(d, pred, target, max_distance):
    """(DAG vertex set as a sorted array, farthest) by a walk-back from the targets over the tight sets."""
    on = np.isfinite(d)
    if max_distance >= 0:
        on &= d <= max_distance
    if target is not None:
        on &= np.asarray(target, bool)
    if not on.any():
        return np.zeros(0, np.int64), -1.0
    seen = set(np.flatnonzero(on).tolist())
    stack = list(seen)
    while stack:
        for u in pred[stack.pop()]:
            if u not in seen:
                seen.add(u)
                stack.append(u)
    return np.asarray(sorted(seen), np.int64), float(d[on].max())


def check_fdag(g, vid, n, model, w, direction, source, target=None, max_distance=-1.0, keep=True, edges=True):
    """Keeps the distances from `source` (vertex index), builds and reads the DAG (and its edge-listing twin) and
    checks all of it against model = weighted_dag(...)'s (dist, pred).  Returns (vertex, vdist, off, pred)."""
    dist, tight = model
    if keep:
        g.sssp_keep_f64(vid[source], direction)
    want_d = model_plane(dist)
    want_v, want_far = model_dag(want_d, tight, target, max_distance)
    np.testing.assert_array_equal(bits(g.sssp_kept_row_f64()), bits(want_d))
    nv, ne, far = g.sssp_kept_dag_f64_build(target, max_distance)
    stats = g.ctx.stats()
    vertex, vdist, off, pred = g.sssp_kept_dag_f64_read(0, nv)
    print(f"fdag: nv {nv} ne {ne} farthest {far!r} compute_ms {stats['compute_ms']:.3f} rounds {stats['levels']} "
          f"launches {stats['kernel_launches']} edges {stats['edges_traversed']:.0f}")
    assert nv == len(want_v) and bits([far])[0] == bits([want_far])[0]
    assert len(vertex) == nv and len(off) == nv + 1 and off[0] == 0 and off[-1] == ne == len(pred)
    if nv == 0:
        assert ne == 0 and far == -1.0
        return vertex, vdist, off, pred
    np.testing.assert_array_equal(np.sort(vertex), want_v)            # the vertex set, each once
    np.testing.assert_array_equal(bits(vdist), bits(want_d[vertex]))
    assert np.all(np.diff(vdist) <= 0) and vertex[-1] == source and vdist[0] == far and vdist[-1] == 0
    assert np.all(np.diff(off) >= 0) and off[-1] - off[-2] == 0       # the source: an empty range
    rev = REVERSE[direction]
    roff, rnbr = g.neighbors(vertex, rev)
    owner = np.repeat(vertex.astype(np.int64), np.diff(roff))
    pairs = np.asarray(sorted(v * n + u for v in vertex.tolist() for u in tight[v]), np.int64)
    is_tight = np.isin(owner * n + rnbr, pairs)
    for j, v in enumerate(vertex.tolist()):
        nb = rnbr[roff[j]:roff[j + 1]][is_tight[roff[j]:roff[j + 1]]]
        _, first = np.unique(nb, return_index=True)
        want = nb[np.sort(first)]
        assert pred[off[j]:off[j + 1]].tolist() == want.tolist(), v
        assert set(want.tolist()) == tight[v]
    # the same call again: the same output
    assert g.sssp_kept_dag_f64_build(target, max_distance) == (nv, ne, far)
    for a, b in zip(g.sssp_kept_dag_f64_read(0, nv), (vertex, vdist, off, pred)):
        np.testing.assert_array_equal(a, b)
    if edges:
        # the edge-listing twin: every tight entry of the reverse rows, in row order, with its ordinal
        ev, ed, eoff, epred, eedge = g.sssp_kept_dag_edges_f64(target, max_distance)
        np.testing.assert_array_equal(ev, vertex)
        np.testing.assert_array_equal(bits(ed), bits(vdist))
        _, redge = g.neighbor_edges(vertex, rev)
        w = np.asarray(w, np.float64)
        du, dv = want_d[rnbr], want_d[owner]
        t = np.isfinite(du) & (du < dv) & (du + w[redge] == dv)
        np.testing.assert_array_equal(epred, rnbr[t])
        np.testing.assert_array_equal(eedge, redge[t])
        np.testing.assert_array_equal(eoff, np.concatenate([[0], np.cumsum(t)])[roff])
        # back to the plain DAG, which the caller may go on reading
        assert g.sssp_kept_dag_f64_build(target, max_distance) == (nv, ne, far)
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


def run_case(ctx, n, edges, direction, source, target=None, max_distance=-1.0):
    """edges: (u, v, w) triples over vertex indices."""
    s, d, w = [e[0] for e in edges], [e[1] for e in edges], [float(e[2]) for e in edges]
    g, vid = build(ctx, n, s, d, w, direction)
    try:
        model = weighted_dag(n, s, d, w, direction, source)
        return check_fdag(g, vid, n, model, w, direction, source, target, max_distance)
    finally:
        g.close()


S, A, T, X = 0, 1, 2, 3  # vertex 3 is isolated


def triangle(first, second, direct):
    return [(S, A, first), (A, T, second), (S, T, direct)]


# ---------------- known answers ----------------

def test_kat_heavier_direct_edge_is_not_a_path(ctx):
    dag = run_case(ctx, 4, triangle(0.5, 0.5, 1.5), DIR_BOTH, S, mask(4, T))
    assert lists_of(dag) == {T: [A], A: [S], S: []} and dag[1].tolist() == [1.0, 0.5, 0.0]


def test_kat_exact_tie_spans_two_hop_levels(ctx):
    dag = run_case(ctx, 4, triangle(0.25, 0.25, 0.5), DIR_BOTH, S, mask(4, T))
    lists = lists_of(dag)
    assert sorted(lists[T]) == [S, A] and lists[A] == [S] and lists[S] == [] and len(dag[3]) == 3


def test_kat_near_tie_lists_one_predecessor(ctx):
    """0.1 + 0.2 = 0.30000000000000004 loses to the direct 0.3: no epsilon makes them tie."""
    for direction in (DIR_OUT, DIR_BOTH):
        dag = run_case(ctx, 4, triangle(0.1, 0.2, 0.3), direction, S, mask(4, T))
        assert lists_of(dag) == {T: [S], S: []} and dag[1].tolist() == [0.3, 0.0]
    # and the other way round: a direct edge one ulp above the two-hop sum loses to it
    dag = run_case(ctx, 4, triangle(0.1, 0.2, np.nextafter(0.1 + 0.2, 1.0)), DIR_OUT, S, mask(4, T))
    assert lists_of(dag) == {T: [A], A: [S], S: []} and dag[1].tolist() == [0.1 + 0.2, 0.1, 0.0]


def test_kat_summation_order(ctx):
    """The chain s -0.1- a -0.2- b -0.3- t summed from s (OUT) is 0.6000000000000001, summed from t along the
    reversed edges (IN) it is 0.6: the add goes left to right from the source."""
    chain = [(0, 1, 0.1), (1, 2, 0.2), (2, 3, 0.3)]
    out = run_case(ctx, 4, chain, DIR_OUT, 0)
    inn = run_case(ctx, 4, chain, DIR_IN, 3)
    assert out[1].tolist() == [(0.1 + 0.2) + 0.3, 0.1 + 0.2, 0.1, 0.0] and out[1][0] == 0.6000000000000001
    assert inn[1].tolist() == [(0.3 + 0.2) + 0.1, 0.3 + 0.2, 0.3, 0.0] and inn[1][0] == 0.6
    assert out[0].tolist() == [3, 2, 1, 0] and inn[0].tolist() == [0, 1, 2, 3]


def test_kat_parallel_edges(ctx):
    """u -> v three times, 0.5 / 0.5 / 0.75: the plain DAG lists u once, the edge DAG the two 0.5 ordinals."""
    edges = [(S, A, 0.5), (S, A, 0.75), (S, A, 0.5), (A, T, 0.25)]
    for direction in (DIR_OUT, DIR_BOTH):
        s, d, w = [e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges]
        g, vid = build(ctx, 4, s, d, w, direction)
        dag = check_fdag(g, vid, 4, weighted_dag(4, s, d, w, direction, S), w, direction, S)
        assert lists_of(dag) == {T: [A], A: [S], S: []}
        vertex, dist, off, pred, edge = g.sssp_kept_dag_edges_f64()
        j = vertex.tolist().index(A)
        assert pred[off[j]:off[j + 1]].tolist() == [S, S] and sorted(edge[off[j]:off[j + 1]].tolist()) == [0, 2]
        g.close()


def test_kat_self_loop_isolated_target_unknown_source(ctx):
    edges = triangle(0.5, 0.5, 1.5) + [(A, A, 0.125)]
    dag = run_case(ctx, 4, edges, DIR_BOTH, S, mask(4, X, T))       # X is never reached
    assert lists_of(dag) == {T: [A], A: [S], S: []}
    s, d, w = [e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges]
    g, vid = build(ctx, 4, s, d, w, DIR_BOTH)
    g.sssp_keep_f64(S, DIR_BOTH)
    assert g.sssp_kept_dag_f64_build(mask(4, X)) == (0, 0, -1.0)
    vertex, vdist, off, pred = g.sssp_kept_dag_f64_read(0, 0)
    assert len(vertex) == 0 and off.tolist() == [0] and len(pred) == 0
    g.sssp_keep_f64(12345, DIR_BOTH)                                # not a vertex: every distance absent
    assert g.sssp_kept_row_f64().tolist() == [INF] * 4 and g.sssp_kept_dag_f64_build() == (0, 0, -1.0)
    g.close()


def test_kat_max_distance_at_and_one_ulp_below(ctx):
    total = 0.1 + 0.2
    chain = [(S, A, 0.1), (A, T, 0.2)]
    at = run_case(ctx, 4, chain, DIR_OUT, S, mask(4, T), max_distance=total)
    assert at[0].tolist() == [T, A, S]
    below = run_case(ctx, 4, chain, DIR_OUT, S, mask(4, T), max_distance=np.nextafter(total, 0.0))
    assert len(below[0]) == 0
    every = run_case(ctx, 4, chain, DIR_OUT, S, None, max_distance=np.nextafter(total, 0.0))
    assert sorted(every[0].tolist()) == [S, A]
    zero = run_case(ctx, 4, chain, DIR_OUT, S, None, max_distance=0.0)  # the source alone
    assert zero[0].tolist() == [S]
    nan = run_case(ctx, 4, chain, DIR_OUT, S, None, max_distance=float("nan"))  # no bound
    assert len(nan[0]) == 3


# ---------------- seeded random multigraphs ----------------

def random_weights(kind, m, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 25, m) / 8.0 if kind == "eighths" else rng.uniform(0.01, 3.0, m)


@pytest.mark.parametrize("kind", ["eighths", "uniform"])
@pytest.mark.parametrize("direction", [DIR_OUT, DIR_IN, DIR_BOTH])
def test_random_multigraph(ctx, direction, kind):
    n, m = 2000, 16000
    rng = np.random.default_rng(77)
    s, d = rng.integers(0, n, m), rng.integers(0, n, m)
    s[:200], d[:200] = s[200:400], d[200:400]   # parallel edges
    s[400:500], d[400:500] = d[500:600], s[500:600]  # and reversed twins
    w = random_weights(kind, m, 5)
    g, vid = build(ctx, n, s, d, w, direction, vid=(rng.permutation(n).astype(np.int64) + 3) * 7)
    model = weighted_dag(n, s, d, w.tolist(), direction, 0)
    every = check_fdag(g, vid, n, model, w, direction, 0)
    assert len(every[0]) > n // 2
    if kind == "eighths":
        assert len(every[3]) > len(every[0])   # ties: more DAG entries than vertices
    tg = mask(n, *rng.choice(n, 50, replace=False))
    check_fdag(g, vid, n, model, w, direction, 0, tg, max_distance=float(np.median(model_plane(model[0]))), keep=False)
    g.close()


def test_ranged_read(ctx):
    """Graph.sssp_kept_dag_f64 and sssp_kept_dag_edges_f64 read in ranges of DAG_READ_ENTRIES = 50 entries give,
    array for array, what one read gives.  A hub with 60 tight predecessors, more than a range holds, is read
    alone: 0 -> spoke -> hub over edges of the smallest weight, so no path reaches a spoke or the hub sooner."""
    n, m, hub, fan = 200, 2000, 199, 60
    rng = np.random.default_rng(11)
    s, d = rng.integers(0, n, m), rng.integers(0, n, m)
    w = random_weights("eighths", m, 3)
    spokes = np.arange(1, fan + 1)
    s[:fan], d[:fan] = 0, spokes
    s[fan:2 * fan], d[fan:2 * fan] = spokes, hub
    s[2 * fan:2 * fan + 10], d[2 * fan:2 * fan + 10] = spokes[:10], hub   # parallel: the edge DAG lists them too
    w[:2 * fan + 10] = 0.125
    dist, tight = weighted_dag(n, s, d, w.tolist(), DIR_OUT, 0)
    dag_v, _ = model_dag(model_plane(dist), tight, None, -1.0)
    entries = sum(len(tight[v]) for v in dag_v.tolist())
    assert entries > 50 and len(tight[hub]) >= fan > 50 and hub in dag_v   # ranges, and a vertex read alone
    g, vid = build(ctx, n, s, d, w, DIR_OUT)
    try:
        g.sssp_keep_f64(vid[0], DIR_OUT)
        whole, whole_edges = g.sssp_kept_dag_f64(), g.sssp_kept_dag_edges_f64()
        assert len(whole[3]) == entries and len(whole_edges[4]) >= entries + 10
        g.DAG_READ_ENTRIES = 50
        try:
            ranged, ranged_edges = g.sssp_kept_dag_f64(), g.sssp_kept_dag_edges_f64()
        finally:
            del g.DAG_READ_ENTRIES
        assert len(ranged) == 4 and len(ranged_edges) == 5
        for a, b in zip(ranged + ranged_edges, whole + whole_edges):
            assert a.dtype == b.dtype
            np.testing.assert_array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                          b.view(np.int64) if b.dtype == np.float64 else b)
    finally:
        g.close()


@pytest.fixture(scope="module")
def rmat12(oracle_lib):
    from test_gpu_vdev import rmat_graph
    n, vid, s, t, _ = rmat_graph(oracle_lib, 12)
    source = int(np.bincount(s, minlength=n).argmax())
    return n, vid, s, t, source


@pytest.mark.parametrize("direction", [DIR_OUT, DIR_BOTH])
def test_rmat12(ctx, rmat12, direction):
    n, vid, s, t, source = rmat12
    w = random_weights("uniform", len(s), 12)
    g, _ = build(ctx, n, s, t, w, direction, vid=vid)
    model = weighted_dag(n, s, t, w.tolist(), direction, source)
    every = check_fdag(g, vid, n, model, w, direction, source)
    assert len(every[0]) > n // 4
    g.close()


@pytest.mark.parametrize("direction", [DIR_OUT, DIR_BOTH])
def test_integer_valued_doubles_equal_the_integer_plane(ctx, rmat12, direction):
    """Weights 1..255 as int32 and as the same values in doubles, on one graph: integer-valued doubles below 2^53
    add exactly, so the two planes and the two DAGs agree.  Both kinds of weights live side by side."""
    import janusgraph_amd as jg
    E = jg._lib
    n, vid, s, t, source = rmat12
    wi = np.random.default_rng(12).integers(1, 256, len(s)).astype(np.int32)
    g = ctx.build(vid, vid[s], vid[t], wi, flags=flags_for(direction) | (E.ADJ_WEIGHT_BOTH if direction == DIR_BOTH else 0))
    g.set_weights_f64(wi.astype(np.float64))
    g.sssp_keep(vid[source], direction)
    row_i = g.sssp_kept_row()
    dag_i = g.sssp_kept_dag()
    g.sssp_keep_f64(vid[source], direction)
    row_f = g.sssp_kept_row_f64()
    dag_f = g.sssp_kept_dag_f64()
    want = np.where(row_i == np.iinfo(np.int64).min, INF, row_i.astype(np.float64))
    np.testing.assert_array_equal(bits(row_f), bits(want))
    assert np.isfinite(row_f).sum() > n // 4
    # equal distances may be listed in another order (unspecified inside one distance): compare per vertex
    assert lists_of(dag_i) == lists_of(dag_f)
    np.testing.assert_array_equal(dag_f[1], np.sort(dag_i[1].astype(np.float64))[::-1])
    g.close()


# ---------------- engine edges ----------------

def tuned_delta(value):
    import janusgraph_amd as jg

    class Scope:
        def __enter__(self):
            jg._lib.tune_set("sd_delta", value)

        def __exit__(self, *a):
            jg._lib.tune_set("sd_delta", -1)

    return Scope()


def test_path_with_many_threshold_jumps(ctx):
    """A 3000-row path whose weights swing between 0.3 and 40: with delta 1 every 40.0 edge sends the next row to the
    far pile and the threshold jumps past ~40 empty buckets to it, 334 times; with the automatic delta a few times."""
    n = 3000
    i = np.arange(n - 1)
    w = np.where(i % 9 == 0, 40.0, 0.3 + (i % 5) * 0.17)
    model = weighted_dag(n, i, i + 1, w.tolist(), DIR_OUT, 0)
    g, vid = build(ctx, n, i, i + 1, w, DIR_OUT)
    with tuned_delta(1):
        check_fdag(g, vid, n, model, w, DIR_OUT, 0, mask(n, n - 1), edges=False)
        g.sssp_keep_f64(0, DIR_OUT)
        jumps = g.ctx.stats()["levels"]
    check_fdag(g, vid, n, model, w, DIR_OUT, 0, mask(n, n - 1), edges=False)
    assert jumps >= 334  # (near passes: at least one per jump, one jump per 40.0 edge)
    g.close()


@pytest.mark.parametrize("spread", [True, False])
def test_out_star_needs_a_second_partial_tile(ctx, spread):
    """70 000 leaves under the source: its first near pass walks 70 000 entries, more than one tile of the
    64-workgroup near grid (64 x 256 x 4 = 65 536), so a second, partial tile.  Weights spread over 0.5 .. 700 with
    delta 1 leave ~69 900 rows in the far pile at the first split (more than the 16 x 256 = 4096 rows of one stride
    of the split grid) and split it ~700 times; equal weights put every leaf in one bucket."""
    k = 70000
    n = k + 1
    leaves = np.arange(1, n)
    w = 0.5 + 699.5 * (np.arange(k) / (k - 1)) if spread else np.full(k, 0.75)
    g, vid = build(ctx, n, np.zeros(k, np.int64), leaves, w, DIR_OUT)
    with tuned_delta(1):
        g.sssp_keep_f64(0, DIR_OUT)
        levels = g.ctx.stats()["levels"]
        row = g.sssp_kept_row_f64()
    np.testing.assert_array_equal(bits(row), bits(np.concatenate([[0.0], w])))
    assert levels >= (600 if spread else 1)
    g.sssp_keep_f64(0, DIR_OUT)  # the automatic delta: everything near
    np.testing.assert_array_equal(bits(g.sssp_kept_row_f64()), bits(np.concatenate([[0.0], w])))
    nv, ne, far = g.sssp_kept_dag_f64_build(mask(n, 1, k))
    assert (nv, ne, far) == (3, 2, float(w.max()))
    g.close()


def test_in_star_read_by_the_dag(ctx):
    """Source -> 40 000 middles -> sink, every total exactly 2.0 (k/8 and 2 - k/8): the sink's reverse row has
    40 000 tight entries, walked by ~40 waves of the count and fill passes."""
    k = 40000
    mid = np.arange(1, k + 1)
    sink = k + 1
    n = k + 2
    a = (mid % 7 + 1) / 8.0
    s = np.concatenate([np.zeros(k, np.int64), mid])
    d = np.concatenate([mid, np.full(k, sink)])
    w = np.concatenate([a, 2.0 - a])
    g, vid = build(ctx, n, s, d, w, DIR_OUT)
    model = weighted_dag(n, s, d, w.tolist(), DIR_OUT, 0)
    vertex, vdist, off, pred = check_fdag(g, vid, n, model, w, DIR_OUT, 0, mask(n, sink))
    assert len(vertex) == n and vertex[0] == sink and vdist[0] == 2.0 and len(pred) == 2 * k
    assert len(np.unique(pred[off[0]:off[1]])) == k
    g.close()


def test_one_vertex_no_edges(ctx):
    g, vid = build(ctx, 1, [], [], [], DIR_BOTH, vid=np.asarray([7], np.int64))
    g.sssp_keep_f64(7, DIR_BOTH)
    assert g.sssp_kept_row_f64().tolist() == [0.0]
    assert g.sssp_kept_dag_f64_build() == (1, 0, 0.0)
    vertex, vdist, off, pred = g.sssp_kept_dag_f64_read(0, 1)
    assert vertex.tolist() == [0] and vdist.tolist() == [0.0] and off.tolist() == [0, 0] and len(pred) == 0
    g.close()


# ---------------- errors and state ----------------

def code(fn, *a, **k):
    import janusgraph_amd as jg
    with pytest.raises(jg.JanusGpuError) as e:
        fn(*a, **k)
    return e.value.code


def test_weight_errors(ctx):
    import janusgraph_amd as jg
    E = jg._lib
    s, d, w = [S, A, S], [A, T, T], [0.5, 0.5, 1.5]
    g, vid = build(ctx, 4, s, d, w, DIR_BOTH)
    before = g.info()["device_bytes"]
    g.sssp_keep_f64(S, DIR_BOTH)
    for bad in (0.0, -1.0, float("nan"), float("inf"), -0.0):
        assert code(g.set_weights_f64, [0.5, bad, 1.5]) == E.JG_ERR_ARG, bad
    assert code(g.set_weights_f64, [0.5, 0.5]) == E.JG_ERR_ARG               # a wrong m
    assert code(g.set_weights_f64, [0.5, 0.5, 1.5, 1.0]) == E.JG_ERR_ARG
    assert code(g.set_weights_f64, [1.0, 1e-30, 1.0]) == E.JG_ERR_UNSUPPORTED  # the gate: 1e-30 < 4 * 1.0 * 2^-52
    assert code(g.set_weights_f64, [1e308, 1e308, 1e308]) == E.JG_ERR_UNSUPPORTED  # rows * wmax overflows
    assert code(g.set_weights_f64, [5e-324, 5e-324, 5e-324]) == E.JG_ERR_UNSUPPORTED  # below DBL_MIN
    # every failed call left the graph as it was: the plane, the weights, the byte count
    assert g.sssp_kept_row_f64().tolist() == [0.0, 0.5, 1.0, INF] and g.info()["device_bytes"] == before
    g.set_weights_f64([0.5, 0.5, 0.75])                                       # replaces, and drops the f64 plane
    assert code(g.sssp_kept_row_f64) == E.JG_ERR_STATE and g.info()["device_bytes"] == before
    g.sssp_keep_f64(S, DIR_BOTH)
    assert g.sssp_kept_row_f64().tolist() == [0.0, 0.5, 0.75, INF]
    g.close()
    v4 = np.arange(4, dtype=np.int64)
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    plain = ctx.build(v4, s, d, flags=jg.ADJ_BOTH)
    with_index = ctx.build(v4, s, d, flags=jg.ADJ_BOTH | E.ADJ_EDGE_INDEX)
    assert code(plain.set_weights_f64, w) == E.JG_ERR_UNSUPPORTED            # built without ADJ_EDGE_INDEX
    assert code(with_index.sssp_keep_f64, S, DIR_BOTH) == E.JG_ERR_UNSUPPORTED  # keep before set
    with_index.set_weights_f64(w)
    # the doubles count into device_bytes: 8 bytes per BOTH entry
    assert with_index.info()["device_bytes"] - plain.info()["device_bytes"] == 8 * 6 + 4 * 6
    assert code(with_index.sssp_keep_f64, S, DIR_OUT) == E.JG_ERR_UNSUPPORTED  # that adjacency was not built
    assert code(with_index.sssp_keep_f64, S, 0) == E.JG_ERR_ARG               # a bad direction
    plain.close()
    with_index.close()


def test_two_logical_shards_are_unsupported():
    import janusgraph_amd as jg
    E = jg._lib
    ctx2 = jg.Context((0, 0))
    v4 = np.arange(4, dtype=np.int64)
    s, d = np.asarray([S, A, S], np.int64), np.asarray([A, T, T], np.int64)
    assert code(ctx2.build, v4, s, d, None, jg.ADJ_BOTH | E.ADJ_EDGE_INDEX) == E.JG_ERR_UNSUPPORTED
    g = ctx2.build(v4, s, d, flags=jg.ADJ_BOTH)
    assert g.info()["num_shards"] == 2
    assert code(g.set_weights_f64, [0.5, 0.5, 1.5]) == E.JG_ERR_UNSUPPORTED
    assert code(g.sssp_keep_f64, S, DIR_BOTH) == E.JG_ERR_UNSUPPORTED
    assert code(g.sssp_kept_dag_f64_build) == E.JG_ERR_UNSUPPORTED
    assert code(g.sssp_kept_row_f64) == E.JG_ERR_STATE
    g.close()
    ctx2.close()


def test_the_two_families_do_not_mix(ctx):
    import janusgraph_amd as jg
    E = jg._lib
    v4 = np.arange(4, dtype=np.int64)
    s, d = np.asarray([S, A, S], np.int64), np.asarray([A, T, T], np.int64)
    g = ctx.build(v4, s, d, np.asarray([1, 1, 3], np.int32), flags=jg.ADJ_BOTH | E.ADJ_WEIGHT_BOTH | E.ADJ_EDGE_INDEX)
    g.set_weights_f64([0.5, 0.5, 1.5])
    STATE = E.JG_ERR_STATE
    assert code(g.sssp_kept_row_f64) == STATE and code(g.sssp_kept_dag_f64_build) == STATE  # nothing kept
    assert code(g.sssp_kept_dag_f64_read, 0, 0) == STATE
    g.sssp_keep_f64(S, DIR_BOTH)                                   # an f64 plane: the integer calls refuse it
    assert code(g.sssp_kept_row) == STATE and code(g.sssp_kept_dag_build) == STATE
    assert code(g.sssp_kept_dag_edges_build) == STATE
    assert code(g.sssp_kept_dag_f64_read, 0, 0) == STATE           # a plane, no DAG yet
    assert g.sssp_kept_dag_f64_build() == (3, 2, 1.0)
    assert code(g.sssp_kept_dag_read, 0, 3) == STATE               # an f64 DAG: the integer read refuses it
    assert code(g.sssp_kept_dag_read_edges, 0, 3, 2) == STATE      # not an edge-listing DAG
    assert code(g.sssp_kept_dag_f64_read, 0, 4) == E.JG_ERR_ARG and code(g.sssp_kept_dag_f64_read, -1, 1) == E.JG_ERR_ARG
    assert g.sssp_kept_dag_edges_f64_build() == (3, 2, 1.0)
    assert sorted(g.sssp_kept_dag_read_edges(0, 3, 2).tolist()) == [0, 1]  # the shared ordinal read
    g.sssp_keep(S, DIR_BOTH)                                       # an integer plane: the f64 calls refuse it
    assert code(g.sssp_kept_dag_f64_read, 0, 0) == STATE           # (its DAG went with the f64 plane)
    assert code(g.sssp_kept_row_f64) == STATE and code(g.sssp_kept_dag_f64_build) == STATE
    assert code(g.sssp_kept_dag_edges_f64_build) == STATE
    assert g.sssp_kept_row().tolist() == [0, 1, 2, np.iinfo(np.int64).min]
    assert g.sssp_kept_dag_build() == (3, 2, 2)
    assert code(g.sssp_kept_dag_f64_read, 0, 3) == STATE           # an integer DAG: the f64 read refuses it
    g.sssp_keep_f64(S, DIR_BOTH)
    assert g.sssp_kept_row_f64().tolist() == [0.0, 0.5, 1.0, INF]
    g.sssp_kept_release()                                          # drops either kind; idempotent
    assert code(g.sssp_kept_row_f64) == STATE and code(g.sssp_kept_row) == STATE
    g.sssp_kept_release()
    g.close()


def test_a_kept_bfs_dag_survives_an_f64_keep(ctx):
    import janusgraph_amd as jg
    g, vid = build(ctx, 4, [S, A, S], [A, T, T], [0.25, 0.25, 0.5], DIR_BOTH)
    g.bfs_keep([S], jg.DIR_BOTH)
    hop = g.bfs_kept_dag(0)
    g.sssp_keep_f64(S, DIR_BOTH)
    fdag = g.sssp_kept_dag_f64(mask(4, T))
    assert g.bfs_kept_row(0).tolist() == [0, 1, 1, -1]
    for a, b in zip(g.bfs_kept_dag_read(0, len(hop[0])), hop):
        np.testing.assert_array_equal(a, b)
    g.bfs_keep([A], jg.DIR_BOTH)             # a new BFS keep drops the BFS DAG only
    for a, b in zip(g.sssp_kept_dag_f64_read(0, len(fdag[0])), fdag):
        np.testing.assert_array_equal(a, b)
    assert g.sssp_kept_row_f64().tolist() == [0.0, 0.25, 0.5, INF]
    g.close()


def test_a_second_run_gives_the_same_bytes_and_levels(ctx, rmat12):
    n, vid, s, t, source = rmat12
    w = random_weights("uniform", len(s), 3)
    runs = []
    for _ in range(2):
        g, _ = build(ctx, n, s, t, w, DIR_BOTH, vid=vid)
        g.sssp_keep_f64(vid[source], DIR_BOTH)
        levels = g.ctx.stats()["levels"]
        row = g.sssp_kept_row_f64()
        dag = g.sssp_kept_dag_f64()
        runs.append((levels, row.tobytes()) + tuple(x.tobytes() for x in dag))
        g.close()
    assert runs[0] == runs[1] and runs[0][0] > 0


# ---------------- poison ----------------

@pytest.mark.parametrize("pattern", ["ff", "2a"])
def test_poison(rmat12, monkeypatch, pattern):
    """Set, keep and both DAGs on RMAT-12 with every device allocation filled with a poison byte first: nothing
    any of them reads is left unwritten."""
    import janusgraph_amd as jg
    monkeypatch.setenv("JG_DEV_POISON", pattern)
    n, vid, s, t, source = rmat12
    w = random_weights("eighths", len(s), 9)
    c = jg.Context((0,))
    try:
        g, _ = build(c, n, s, t, w, DIR_BOTH, vid=vid)
        check_fdag(g, vid, n, weighted_dag(n, s, t, w.tolist(), DIR_BOTH, source), w, DIR_BOTH, source)
        g.close()
    finally:
        c.close()


# ---------------- through the computer ----------------

MODERN = [(1, 2, 0.5), (1, 4, 1.0), (1, 3, 0.4), (4, 5, 1.0), (4, 3, 0.4), (6, 3, 0.2)]  # TinkerPop's "modern" weights


def computer_case(ctx, graph, direction, sources=None, targets=None, max_distance=None):
    """Runs the program and returns (its paths, its iteration, the model's paths in the device's predecessor order)."""
    import janusgraph_amd as jg
    b = jg.ShortestPathVertexProgram.build().distanceProperty("weight").edgeDirection(NAMES[direction])
    if sources is not None:
        b = b.source(*sources)
    if targets is not None:
        b = b.target(*targets)
    if max_distance is not None:
        b = b.maxDistance(max_distance)
    memory = jg.GpuGraphComputer(graph, context=ctx).program(b.create(graph)).submit().result().memory()
    vid, src, dst, w = graph.snapshot(weight_property="weight", float_weights=True)
    index = {int(x): i for i, x in enumerate(vid.tolist())}
    si, di = [index[int(x)] for x in src], [index[int(x)] for x in dst]
    g = ctx.build(vid, src, dst, flags=flags_for(direction))  # the order predecessors are listed in

    def order(x):
        return g.neighbors([x], REVERSE[direction])[1].tolist()

    want = model_paths(len(vid), si, di, w.tolist(), direction,
                       [index[x] for x in (vid.tolist() if sources is None else sources)],
                       None if targets is None else [index[x] for x in targets], max_distance, order)
    g.close()
    return (memory.get(jg.ShortestPathVertexProgram.SHORTEST_PATHS), memory.getIteration(),
            [[int(vid[x]) for x in p] for p in want])


@pytest.mark.parametrize("direction", [DIR_OUT, DIR_BOTH])
def test_computer_modern_graph(ctx, direction):
    import janusgraph_amd as jg
    graph = jg.InMemoryGraph()
    v = {k: graph.add_vertex() for k in range(1, 7)}
    for a, b, x in MODERN:
        graph.add_edge(v[a], v[b], "E", weight=x)
    got, iteration, want = computer_case(ctx, graph, direction)
    assert got == want and iteration == 1 + max(len(p) - 1 for p in want)
    marko, lop, josh = v[1].id, v[3].id, v[4].id
    assert [marko, lop] in got and [marko, josh, lop] not in got          # 0.4 beats 1.0 + 0.4
    if direction == DIR_BOTH:
        assert [v[6].id, lop, marko] in got                                # peter - lop - marko: 0.2 + 0.4


@pytest.mark.parametrize("max_distance", [None, 1.25])
@pytest.mark.parametrize("direction", [DIR_OUT, DIR_BOTH])
def test_computer_random_graph(ctx, direction, max_distance):
    import janusgraph_amd as jg
    rng = np.random.default_rng(5)
    graph = jg.InMemoryGraph()
    v = [graph.add_vertex() for _ in range(40)]
    for a, b, k in zip(rng.integers(0, 40, 120), rng.integers(0, 40, 120), rng.integers(1, 9, 120)):
        graph.add_edge(v[int(a)], v[int(b)], "E", weight=int(k) / 8.0 if k != 8 else 1)  # a few ints among the floats
    sources = [v[3].id, v[17].id, v[0].id]
    targets = [x.id for x in v[::3]]
    got, iteration, want = computer_case(ctx, graph, direction, sources, targets, max_distance)
    assert got == want and len(want) >= 3
    assert iteration == 1 + max(len(p) - 1 for p in want)


def test_computer_refusals(ctx):
    import janusgraph_amd as jg

    def graph_with(**bad):
        graph = jg.InMemoryGraph()
        v = [graph.add_vertex() for _ in range(4)]
        graph.add_edge(v[0], v[1], "E", weight=0.5)
        graph.add_edge(v[1], v[2], "E", weight=0.25)
        if bad is not None:
            graph.add_edge(v[2], v[3], "E", **bad)
        return graph, v

    for bad in ({}, {"weight": 0.0}, {"weight": float("inf")}, {"weight": -0.5}, {"weight": float("nan")},
                {"weight": np.float32(0.5)}, {"weight": "0.5"}, {"weight": 2**60}, {"weight": 1e-30}):
        graph, v = graph_with(**bad)
        vp = jg.ShortestPathVertexProgram.build().source(v[0].id).distanceProperty("weight").create(graph)
        with pytest.raises(jg.ProgramNotSupported):
            jg.GpuGraphComputer(graph, context=ctx).program(vp).submit().result()
    graph, v = graph_with(weight=0.75)
    c2 = jg.Context((0, 0))
    try:
        vp = jg.ShortestPathVertexProgram.build().source(v[0].id).distanceProperty("weight").create(graph)
        with pytest.raises(jg.ProgramNotSupported):
            jg.GpuGraphComputer(graph, context=c2).program(vp).submit().result()
    finally:
        c2.close()
    with pytest.raises(ValueError):  # includeEdges + distanceProperty stays refused on both routes
        jg.ShortestPathVertexProgram({"includeEdges": True, "distanceProperty": "weight"})


def test_all_integer_weights_keep_the_integer_route(ctx, monkeypatch):
    import janusgraph_amd as jg
    calls = {"int": 0, "f64": 0}
    keep_i, keep_f = jg._lib.Graph.sssp_keep, jg._lib.Graph.sssp_keep_f64
    monkeypatch.setattr(jg._lib.Graph, "sssp_keep", lambda self, *a: (calls.__setitem__("int", calls["int"] + 1), keep_i(self, *a))[1])
    monkeypatch.setattr(jg._lib.Graph, "sssp_keep_f64", lambda self, *a: (calls.__setitem__("f64", calls["f64"] + 1), keep_f(self, *a))[1])
    for weights, route in (([1, 1, 3], "int"), ([1, 1.0, 3], "f64")):
        graph = jg.InMemoryGraph()
        v = [graph.add_vertex() for _ in range(3)]
        for (a, b), x in zip(((0, 1), (1, 2), (0, 2)), weights):
            graph.add_edge(v[a], v[b], "E", weight=x)
        calls.update(int=0, f64=0)
        vp = jg.ShortestPathVertexProgram.build().source(v[0].id).target(v[2].id).distanceProperty("weight").create(graph)
        memory = jg.GpuGraphComputer(graph, context=ctx).program(vp).submit().result().memory()
        assert memory.get(vp.SHORTEST_PATHS) == [[v[0].id, v[1].id, v[2].id]]
        assert calls == {"int": int(route == "int"), "f64": int(route == "f64")}
