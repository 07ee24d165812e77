"""Edge ordinals in label scopes (jg_builder_keep_scope_ordinals, jg_builder_finish_labels with JG_ADJ_EDGE_INDEX,
jg_graph_scope_positions) and the label-scoped ShortestPath / ConnectedComponent / PeerPressure programs.

The ordinal rule: a scoped graph's edge list is the scope's kept list, ordinal k the k-th kept edge in accumulated
order.  So the reference of every library test is the host-filtered edge list, np.flatnonzero(np.isin(lab, scope)),
given to Context.build; every comparison is exact (integers as integers, doubles by their bits).  The reference of
every computer test is the same program without edgeLabels on an InMemoryGraph holding the scope's edges only.
"""
import copy

import numpy as np
import pytest

import row_edges_stores as rs
from oracle import edgecodec as ec
from test_gpu_builder import row_chunks

pytestmark = pytest.mark.gpu

DIR_OUT, DIR_IN, DIR_BOTH = 1, 2, 3
DIRS = (DIR_OUT, DIR_IN, DIR_BOTH)
TILE = 2048  # kScopeTile


@pytest.fixture(scope="module")
def ctx():
    import janusgraph_amd as jg
    c = jg.Context((0,))
    yield c
    c.close()


def E():
    from janusgraph_amd import _lib
    return _lib


def flags_all(index=True):
    import janusgraph_amd as jg
    return jg.ADJ_IN | jg.ADJ_OUT | jg.ADJ_BOTH | (E().ADJ_EDGE_INDEX if index else 0)


def code(fn, *args):
    import janusgraph_amd as jg
    try:
        fn(*args)
    except jg.JanusGpuError as e:
        return e.code
    return 0


def ids_builder(ctx, vid, src, dst, lab, weight=None, numbered=True, chunks=1):
    b = ctx.builder()
    b.keep_labels()
    if numbered:
        b.keep_scope_ordinals()
    b.add_vertices(vid)
    for part in np.array_split(np.arange(len(src)), chunks):
        b.add_edges(src[part], dst[part], None if weight is None else weight[part], lab[part])
    return b


def sorted_entries(g, direction, rows=None):
    """(row, neighbour, ordinal) of every entry of the `direction` adjacency of `rows` (all by default) as one
    sorted int64 array [3, entries]."""
    rows = np.arange(g.n) if rows is None else np.asarray(rows)
    off, nbr = g.neighbors(rows, direction)
    off2, edge = g.neighbor_edges(rows, direction)
    np.testing.assert_array_equal(off, off2)
    t = np.stack([np.repeat(rows, np.diff(off)), nbr, edge.astype(np.int64)])
    return t[:, np.lexsort(t[::-1])]


def model_entries(vid, src, dst, direction, rows=None):
    """The same from an edge list on the host: ordinal = position in (src, dst); ghost-ended edges have no entry."""
    order = np.argsort(vid)
    def index(x):
        p = np.searchsorted(vid[order], x)
        p[p == len(vid)] = 0
        return np.where(vid[order][p] == x, order[p], -1) if len(vid) else np.full(len(x), -1)
    s, d, o = index(src), index(dst), np.arange(len(src))
    inside = (s >= 0) & (d >= 0)
    s, d, o = s[inside], d[inside], o[inside]
    parts = []
    if direction in (DIR_OUT, DIR_BOTH):
        parts.append(np.stack([s, d, o]))
    if direction in (DIR_IN, DIR_BOTH):
        parts.append(np.stack([d, s, o]))  # BOTH: a self-loop twice on its row
    t = np.concatenate(parts, axis=1)
    if rows is not None:
        t = t[:, np.isin(t[0], rows)]
    return t[:, np.lexsort(t[::-1])]


# ---------------------------------------------------------------- A: the select's columns at the tile edges

def tile_case(ctx, m, scope, directions=DIRS, n=1024, seed=0, rows=None):
    import janusgraph_amd as jg
    rng = np.random.default_rng(seed + m)
    vid = (np.arange(n, dtype=np.int64) + 1) << 8
    src, dst = vid[rng.integers(0, n, m)], vid[rng.integers(0, n, m)]
    lab = rng.integers(0, 4, m).astype(np.int64)  # about half kept, the pattern changing inside every 64-edge run
    want = np.flatnonzero(np.isin(lab, scope))
    kept = len(want)
    b = ids_builder(ctx, vid, src, dst, lab)
    flags = {DIR_OUT: jg.ADJ_OUT, DIR_IN: jg.ADJ_IN, DIR_BOTH: jg.ADJ_BOTH}
    g = b.finish_labels(scope, sum(flags[d] for d in directions) | E().ADJ_EDGE_INDEX)
    b.close()
    stats = ctx.stats()
    assert stats["kernel_launches"] == (0 if m == 0 else 2 if kept else 1)
    assert stats["algorithmic_bytes"] == (16.0 * m + (32.0 + 8.0) * kept if m else 0.0)
    pos = g.scope_positions()
    assert pos.dtype == np.int64
    np.testing.assert_array_equal(pos, want)
    if kept:
        k = min(kept - 1, 70)
        np.testing.assert_array_equal(g.scope_positions(k, 1), want[k:k + 1])
        np.testing.assert_array_equal(g.scope_positions(kept - 1), want[-1:])
    assert len(g.scope_positions(kept, 0)) == 0  # count == 0 at the end of the list
    assert code(g.scope_positions, kept, 1) == E().JG_ERR_ARG
    for d in directions:
        np.testing.assert_array_equal(sorted_entries(g, d, rows), model_entries(vid, src[want], dst[want], d, rows))
    g.set_weights_f64(np.ones(kept))  # exactly the kept count
    assert code(g.set_weights_f64, np.ones(kept + 1)) == E().JG_ERR_ARG
    if kept:
        assert code(g.set_weights_f64, np.ones(kept - 1)) == E().JG_ERR_ARG
    g.close()
    return kept


@pytest.mark.parametrize("tiles,extra", [(0, 0), (0, 1), (1, -1), (1, 0), (1, 1), (3, 5)])
def test_select_columns_at_tile_edges(ctx, tiles, extra):
    m = tiles * TILE + extra
    kept = tile_case(ctx, m, [0, 2])
    assert m < 2 or 0 < kept < m


def test_select_columns_when_a_block_walks_several_tiles(ctx):
    # more tiles than the select's grid of 4096 blocks: a block walks two tiles, the last block's range is short
    # (8.4 M edges over 1024 vertices: the entries of a sample of rows are compared, every position is)
    tile_case(ctx, 4096 * TILE + 1, [0, 2], directions=(DIR_OUT,), rows=[0, 1, 511, 1022, 1023])


@pytest.mark.parametrize("scope,name", [([0, 1, 2, 3], "all"), ([9], "none")])
def test_all_edges_kept_and_none_kept(ctx, scope, name):
    m = 3 * TILE + 5
    assert tile_case(ctx, m, scope) == (m if name == "all" else 0)


# ---------------------------------------------------------------- B: a scope equals the build of the filtered list

LABELS = np.array([-7, 5, (1 << 40) + 3, 1 << 62], np.int64)  # opaque int64 values


@pytest.fixture(scope="module")
def multigraph():
    """About 300 vertices and 3000 edges over 4 labels: self-loops, parallel edges, ghost endpoints."""
    rng = np.random.default_rng(18)
    n, m = 300, 3000
    vid = np.sort(rng.choice(np.arange(1, 1 << 30), n + 20, replace=False)).astype(np.int64) << 8
    rng.shuffle(vid)
    ghosts, vid = vid[n:], vid[:n]
    src, dst = vid[rng.integers(0, n, m)], vid[rng.integers(0, n, m)]
    dst[:60] = src[:60]                       # self-loops
    src[60:160], dst[60:160] = vid[3], vid[4]  # parallel edges, over every label
    g1, g2 = rng.choice(np.arange(160, m), 80, replace=False).reshape(2, 40)
    src[g1] = ghosts[rng.integers(0, 20, 40)]
    dst[g2] = ghosts[rng.integers(0, 20, 40)]
    lab = LABELS[rng.integers(0, 4, m)]
    w = rng.integers(1, 10, m).astype(np.int32)
    wf = rng.integers(1, 17, m) / 8.0  # multiples of 1/8: exact sums, exact ties
    return vid, src, dst, lab, w, wf


def exact(x):
    return x.view(np.int64) if x.dtype == np.float64 else x


def assert_same_arrays(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(exact(np.asarray(x)), exact(np.asarray(y)))


def assert_scope_equals_filtered(ctx, g, vid, src, dst, w, wf, keep, sources):
    """Scoped graph g (ordinals, int weights, no doubles yet) against Context.build of the filtered list."""
    ref = ctx.build(vid, src[keep], dst[keep], w[keep], flags=flags_all())
    np.testing.assert_array_equal(g.scope_positions(), keep)
    rows = np.arange(len(vid))
    for d in DIRS:
        assert_same_arrays(g.neighbors(rows, d), ref.neighbors(rows, d))
        assert_same_arrays(g.neighbor_edges(rows, d), ref.neighbor_edges(rows, d))
    assert g.info()["device_bytes"] == ref.info()["device_bytes"] + 8 * len(keep)  # the position table
    for d in DIRS:
        g.bfs_keep(sources, d)
        ref.bfs_keep(sources, d)
        for k in range(len(sources)):
            assert_same_arrays(g.bfs_kept_dag_edges(k), ref.bfs_kept_dag_edges(k))
    for d in (DIR_OUT, DIR_IN):
        g.sssp_keep(sources[0], d)
        ref.sssp_keep(sources[0], d)
        np.testing.assert_array_equal(g.sssp_kept_row(), ref.sssp_kept_row())
        assert_same_arrays(g.sssp_kept_dag_edges(), ref.sssp_kept_dag_edges())
    g.set_weights_f64(wf[keep])
    ref.set_weights_f64(wf[keep])
    for d in DIRS:
        g.sssp_keep_f64(sources[1], d)
        ref.sssp_keep_f64(sources[1], d)
        np.testing.assert_array_equal(exact(g.sssp_kept_row_f64()), exact(ref.sssp_kept_row_f64()))
        assert_same_arrays(g.sssp_kept_dag_edges_f64(), ref.sssp_kept_dag_edges_f64())
    ref.close()


@pytest.mark.parametrize("scope", [(0,), (1, 3), (0, 1, 2, 3)])
def test_scope_equals_filtered_build(ctx, multigraph, scope):
    vid, src, dst, lab, w, wf = multigraph
    names = LABELS[list(scope)]
    keep = np.flatnonzero(np.isin(lab, names))
    b = ids_builder(ctx, vid, src, dst, lab, w, chunks=3)
    g = b.finish_labels(names, flags_all())
    b.close()
    assert_scope_equals_filtered(ctx, g, vid, src, dst, w, wf, keep, [vid[3], vid[0], vid[7]])
    g.close()


def test_two_scopes_then_finish_from_one_builder(ctx, multigraph):
    vid, src, dst, lab, w, wf = multigraph
    b = ids_builder(ctx, vid, src, dst, lab, w)
    scoped = [(b.finish_labels(LABELS[list(s)], flags_all()), np.flatnonzero(np.isin(lab, LABELS[list(s)])))
              for s in ((2,), (0, 3))]
    whole = b.finish(flags_all())  # every label; the builder survived both scopes
    b.close()
    for g, keep in scoped:
        assert_scope_equals_filtered(ctx, g, vid, src, dst, w, wf, keep, [vid[3], vid[0]])
        g.close()
    ref = ctx.build(vid, src, dst, w, flags=flags_all())
    rows = np.arange(len(vid))
    for d in DIRS:
        assert_same_arrays(whole.neighbor_edges(rows, d), ref.neighbor_edges(rows, d))
    assert code(whole.scope_positions, 0, 0) == E().JG_ERR_UNSUPPORTED  # jg_builder_finish numbers the whole list
    assert whole.info()["device_bytes"] == ref.info()["device_bytes"]
    whole.close()
    ref.close()


def test_opt_in_without_the_flag_changes_nothing(ctx, multigraph):
    vid, src, dst, lab, w, wf = multigraph
    graphs = []
    for numbered in (True, False):
        b = ids_builder(ctx, vid, src, dst, lab, w, numbered=numbered)
        graphs.append(b.finish_labels(LABELS[:2], flags_all(False)))
        stats = ctx.stats()
        keep = int(np.isin(lab, LABELS[:2]).sum())
        assert stats["algorithmic_bytes"] == 16.0 * len(lab) + 40.0 * keep and stats["kernel_launches"] == 2
        b.close()
    a, p = graphs
    assert a.info() == p.info()
    assert code(a.scope_positions, 0, 0) == E().JG_ERR_UNSUPPORTED
    rows = np.arange(len(vid))
    for d in DIRS:
        assert_same_arrays(a.neighbors(rows, d), p.neighbors(rows, d))
    a.close()
    p.close()


# ---------------------------------------------------------------- C: rows builders

def labelled_store(value_of=None, n=200, m=1500, seed=2):
    """A RowStore of n live vertices (and a few ghost rows) with m edges over the four labels.  Returns
    (store object, built arrays, label index of every listed edge, edge number of every listed edge)."""
    rng = np.random.default_rng(seed)
    st = rs.RowStore(5)
    vs = [st.vertex(st.vid(10 + i, int(rng.integers(0, 32))), live=i % 17 != 5) for i in range(n)]
    s, t, L = rng.integers(0, n, m), rng.integers(0, n, m), rng.integers(0, 4, m)
    t[:20] = s[:20]
    s[20:60], t[20:60] = 0, 1
    L[:60] = 0  # MULTI: the multiplicity that allows self-loops and parallel edges
    label_of, number_of = {}, {}
    for e in range(m):
        rel = st.edge(vs[int(s[e])], vs[int(t[e])], int(L[e]), value_of(e, int(L[e]), rng) if value_of else b"")
        label_of[rel], number_of[rel] = int(L[e]), e
    store = st.build()
    rel = st.listed()[2].tolist()
    return st, store, np.array([label_of[r] for r in rel]), np.array([number_of[r] for r in rel])


def rows_builder(ctx, store, relations=True, f64_key=None, numbered=True, bounds=None):
    b = ctx.builder()
    b.set_schema(store[5], store[6], 5)
    b.keep_labels()
    if relations:
        b.keep_relations()
    if numbered:
        b.keep_scope_ordinals()
    if f64_key is not None:
        b.set_weight_key_f64(*rs.key_table(f64_key))
    for ch in row_chunks(store, [0, len(store[0])] if bounds is None else bounds):
        b.add_rows(*ch)
    return b


def test_rows_scope_relations(ctx):
    st, store, label, _ = labelled_store()
    src, dst, rel, _ = st.listed()
    v = st.vertices()
    b = rows_builder(ctx, store, bounds=np.linspace(0, len(store[0]), 4).astype(int))
    for scope in ([0], [3, 1]):
        keep = np.flatnonzero(np.isin(label, scope))
        g = b.finish_labels([rs.LABELS[i] for i in scope], flags_all())
        stats = ctx.stats()
        assert stats["algorithmic_bytes"] == 16.0 * len(rel) + (32.0 + 8.0 + 16.0) * len(keep)
        assert stats["kernel_launches"] == 2
        np.testing.assert_array_equal(g.vertex_ids(), v)
        np.testing.assert_array_equal(g.scope_positions(), keep)
        np.testing.assert_array_equal(g.edge_relations(np.arange(len(keep))), rel[keep])
        assert code(g.edge_relations, [len(keep)]) == E().JG_ERR_ARG
        twin = ctx.build(v, src[keep], dst[keep], flags=flags_all())
        assert g.info()["device_bytes"] == twin.info()["device_bytes"] + 16 * len(keep)  # positions and relations
        sources = [int(src[keep][0]), int(v[0])]
        for d in DIRS:
            np.testing.assert_array_equal(sorted_entries(g, d), sorted_entries(twin, d))
            g.bfs_keep(sources, d)
            twin.bfs_keep(sources, d)
            for k in range(len(sources)):
                got, want = g.bfs_kept_dag_relations(k), twin.bfs_kept_dag_edges(k)
                assert_same_arrays(got[:4], want[:4])
                assert got[4].dtype == np.int64
                np.testing.assert_array_equal(got[4], rel[keep][want[4]])
        g.close()
        twin.close()
    whole = b.finish(flags_all())  # the builder's own table is intact
    np.testing.assert_array_equal(whole.edge_relations(np.arange(len(rel))), rel)
    whole.close()
    b.close()


def test_rows_scope_doubles_only_inside_the_scope(ctx):
    weights = np.random.default_rng(6).integers(1, 33, 1500) / 16.0

    def value_of(e, L, rng):  # the Double key on label 0 only: the other labels' edges decode to NaN
        return rs.weight_value(ec.DOUBLE, float(weights[e]) if L == 0 else None, rng)

    st, store, label, number = labelled_store(value_of)
    src, dst, rel, _ = st.listed()
    v = st.vertices()
    keep = np.flatnonzero(label == 0)
    assert 0 < len(keep) < len(label)
    b = rows_builder(ctx, store, f64_key=ec.DOUBLE)
    g = b.finish_labels([rs.LABELS[0]], flags_all())
    stats = ctx.stats()
    assert stats["algorithmic_bytes"] == 16.0 * len(rel) + (32.0 + 8.0 + 16.0 + 16.0) * len(keep)
    assert stats["kernel_launches"] == 2
    twin = ctx.build(v, src[keep], dst[keep], flags=flags_all())
    twin.set_weights_f64(weights[number[keep]])
    assert g.info()["device_bytes"] == twin.info()["device_bytes"] + 16 * len(keep)
    for source in (int(src[keep][0]), int(src[keep][-1])):
        for d in DIRS:
            g.sssp_keep_f64(source, d)
            twin.sssp_keep_f64(source, d)
            np.testing.assert_array_equal(exact(g.sssp_kept_row_f64()), exact(twin.sssp_kept_row_f64()))
            got, want = g.sssp_kept_dag_relations_f64(), twin.sssp_kept_dag_edges_f64()
            assert_same_arrays(got[:4], want[:4])
            np.testing.assert_array_equal(got[4], rel[keep][want[4]])
    g.close()
    twin.close()
    # a scope that holds an edge without the property: the same refusal as an unscoped finish, and the builder stays
    assert code(b.finish_labels, [rs.LABELS[0], rs.LABELS[1]], flags_all()) == E().JG_ERR_ARG
    g = b.finish_labels([rs.LABELS[0]], flags_all())
    np.testing.assert_array_equal(g.scope_positions(), keep)
    g.close()
    b.close()
    # a second identical builder, finished over every label: the NaNs outside the scope are refused as before
    b = rows_builder(ctx, store, f64_key=ec.DOUBLE)
    assert code(b.finish, flags_all()) == E().JG_ERR_ARG
    b.close()


# ---------------------------------------------------------------- D: errors

def test_errors(ctx, multigraph):
    import janusgraph_amd as jg
    vid, src, dst, lab, w, wf = multigraph
    scope = LABELS[:2]
    b = ids_builder(ctx, vid, src, dst, lab, numbered=False)
    assert code(b.keep_scope_ordinals) == E().JG_ERR_STATE                   # the opt-in after a chunk
    assert code(b.finish_labels, scope, flags_all()) == E().JG_ERR_UNSUPPORTED  # EDGE_INDEX without the opt-in
    g = b.finish_labels(scope, flags_all(False))
    assert code(g.scope_positions) == E().JG_ERR_UNSUPPORTED
    g.close()
    assert code(b.keep_scope_ordinals) == E().JG_ERR_STATE                   # ... and on a sealed builder
    b.close()
    b = ctx.builder()
    b.keep_scope_ordinals()  # without keep_labels: refused at finish_labels
    b.add_vertices(vid)
    b.add_edges(src, dst)
    assert code(b.finish_labels, scope, flags_all()) == E().JG_ERR_STATE
    assert code(b.finish_labels, scope, flags_all(False)) == E().JG_ERR_STATE
    b.close()
    b = ctx.builder()
    b.keep_scope_ordinals()  # either order
    b.keep_labels()
    b.add_vertices(vid)
    b.add_edges(src, dst, label=lab)
    g = b.finish_labels(scope, flags_all())
    kept = int(np.isin(lab, scope).sum())
    assert len(g.scope_positions()) == kept
    assert len(g.scope_positions(kept)) == 0 and len(g.scope_positions(0, 0)) == 0
    for first, count in ((0, kept + 1), (kept, 1), (kept + 1, 0), (-1, 1), (0, -1)):
        assert code(g.scope_positions, first, count) == E().JG_ERR_ARG, (first, count)
    g.close()
    b.close()
    plain = ctx.build(vid, src, dst, flags=flags_all())
    assert code(plain.scope_positions, 0, 0) == E().JG_ERR_UNSUPPORTED  # a plain graph holds no table
    plain.close()
    ctx2 = jg.Context((0, 0))  # two logical shards
    try:
        b = ids_builder(ctx2, vid, src, dst, lab)
        assert code(b.finish_labels, scope, flags_all()) == E().JG_ERR_UNSUPPORTED
        g = b.finish_labels(scope, flags_all(False))
        assert g.info()["num_shards"] == 2 and code(g.scope_positions, 0, 0) == E().JG_ERR_UNSUPPORTED
        g.close()
        b.close()
    finally:
        ctx2.close()


# ---------------------------------------------------------------- E: the computer

def gods():
    import janusgraph_amd as jg
    graph = jg.InMemoryGraph()
    jg.load_graph_of_the_gods(graph)
    return graph


def modern():
    """TinkerPop-modern-shaped: "knows" carries Double weights (two exactly tied routes marko -> peter), "created"
    has no weight property."""
    import janusgraph_amd as jg
    graph = jg.InMemoryGraph()
    v = {name: graph.add_vertex("person" if name not in ("lop", "ripple") else "software", name=name)
         for name in ("marko", "vadas", "lop", "josh", "ripple", "peter")}
    A = graph.add_edge
    A(v["marko"], v["vadas"], "knows", weight=0.5)
    A(v["marko"], v["lop"], "created")
    A(v["marko"], v["josh"], "knows", weight=1.0)
    A(v["josh"], v["ripple"], "created")
    A(v["josh"], v["peter"], "knows", weight=0.75)
    A(v["josh"], v["lop"], "created")
    A(v["vadas"], v["peter"], "knows", weight=1.25)
    A(v["peter"], v["lop"], "created")
    A(v["peter"], v["marko"], "knows", weight=4.0)
    A(v["marko"], v["josh"], "knows", weight=1.0)  # a parallel edge
    return graph


def filtered(graph, labels):
    """The same vertices and ids with the scope's edges only, in their relative order; and their positions."""
    pos = [i for i, e in enumerate(graph.edges) if e.label in labels]
    f = copy.deepcopy(graph)
    f.edges = [f.edges[i] for i in pos]
    return f, pos


def run(ctx, graph, vp, map_reduces=(), persist=None):
    import janusgraph_amd as jg
    c = jg.GpuGraphComputer(graph, context=ctx).program(vp)
    for mr in map_reduces:
        c.mapReduce(mr)
    if persist is not None:
        c.persist(persist)
    return c.submit().result()


def path_builder(labels=None, **conf):
    import janusgraph_amd as jg
    b = jg.ShortestPathVertexProgram.build()
    for k, v in conf.items():
        b = getattr(b, k)(*v) if isinstance(v, tuple) else getattr(b, k)(v)
    return b.edgeLabels(*labels) if labels is not None else b


def plain_paths(graph, paths, edge_index=None):
    """Paths with every Edge replaced by ("edge", its index in graph.edges) (through edge_index, if given)."""
    number = {id(e): i for i, e in enumerate(graph.edges)}
    out = []
    for p in paths:
        row = []
        for x in p:
            if isinstance(x, int):
                row.append(x)
            else:
                i = number[id(x)]
                row.append(("edge", i if edge_index is None else edge_index[i]))
        out.append(row)
    return out


def assert_paths_scoped(ctx, graph, labels, **conf):
    import janusgraph_amd as jg
    key = jg.ShortestPathVertexProgram.SHORTEST_PATHS
    small, pos = filtered(graph, labels)
    got = run(ctx, graph, path_builder(labels, **conf).create()).memory()
    want = run(ctx, small, path_builder(None, **conf).create()).memory()
    # in order; the filtered graph's j-th edge is the full graph's pos[j]-th
    assert plain_paths(graph, got.get(key)) == plain_paths(small, want.get(key), pos)
    assert got.getIteration() == want.getIteration()
    return got.get(key)


ONE_WAY_SOURCES = ("hercules", "jupiter", "pluto", "cerberus", "neptune", "saturn", "tartarus")
GOD_SCOPES = [("battled",), ("brother", "father"), ("no such label",)]


@pytest.mark.parametrize("labels", GOD_SCOPES)
@pytest.mark.parametrize("direction", ["in", "out", "both"])
@pytest.mark.parametrize("include_edges", [False, True])
def test_computer_hop_paths(ctx, labels, direction, include_edges):
    graph = gods()
    ids = {v.properties["name"]: vid for vid, v in graph.vertices.items()}
    # every vertex as a source along "both"; one-way traversals take at most 8 sources at a time, scoped or not
    conf = {} if direction == "both" else {"source": tuple(ids[x] for x in ONE_WAY_SOURCES)}
    sources = list(graph.vertices) if direction == "both" else list(conf["source"])
    paths = assert_paths_scoped(ctx, graph, labels, edgeDirection=direction, includeEdges=include_edges, **conf)
    assert len(paths) >= len(sources)  # every source reaches itself
    if labels == ("no such label",):  # the edgeless graph over all vertices: a source that is a target yields [s]
        assert sorted(map(tuple, paths)) == sorted((v,) for v in sources)
    unscoped = run(ctx, graph, path_builder(None, edgeDirection=direction, **conf).create()).memory()
    assert len(unscoped.get(jg_key())) > len(paths)  # the scope matters


def jg_key():
    import janusgraph_amd as jg
    return jg.ShortestPathVertexProgram.SHORTEST_PATHS


@pytest.mark.parametrize("include_edges", [False, True])
def test_computer_hop_paths_max_distance_and_endpoints(ctx, include_edges):
    graph = gods()
    ids = {v.properties["name"]: vid for vid, v in graph.vertices.items()}
    assert_paths_scoped(ctx, graph, ("brother", "father"), maxDistance=1, includeEdges=include_edges)
    paths = assert_paths_scoped(ctx, graph, ("brother", "father"), source=(ids["hercules"], ids["pluto"]),
                                target=(ids["saturn"], ids["neptune"], ids["hercules"]), edgeDirection="out",
                                includeEdges=include_edges)
    assert [p[0] for p in paths].count(ids["hercules"]) == 3  # itself, saturn and neptune through jupiter
    assert_paths_scoped(ctx, graph, ("brother", "father"), source=(ids["hercules"],), maxDistance=2,
                        edgeDirection="out", includeEdges=include_edges)


@pytest.mark.parametrize("direction", ["in", "out", "both"])
def test_computer_integer_distance_property(ctx, direction):
    import janusgraph_amd as jg
    graph = gods()
    # "time" is on the "battled" edges only: scoped to them the integer route runs, unscoped it is refused
    assert_paths_scoped(ctx, graph, ("battled",), distanceProperty="time", edgeDirection=direction)
    assert_paths_scoped(ctx, graph, ("battled",), distanceProperty="time", edgeDirection=direction, maxDistance=2)
    with pytest.raises(jg.ProgramNotSupported):
        run(ctx, graph, path_builder(None, distanceProperty="time", edgeDirection=direction).create())
    with pytest.raises(jg.ProgramNotSupported):  # a scope with an edge that lacks the property
        run(ctx, graph, path_builder(("battled", "pet"), distanceProperty="time").create())
    graph.edges[9].properties["time"] = 0  # a weight < 1 inside the scope / outside it
    with pytest.raises(jg.ProgramNotSupported):
        run(ctx, graph, path_builder(("battled",), distanceProperty="time").create())
    graph.edges[9].properties["time"] = 1
    graph.edges[15].properties["time"] = 0  # "pet"
    assert_paths_scoped(ctx, graph, ("battled",), distanceProperty="time")


@pytest.mark.parametrize("direction", ["in", "out", "both"])
def test_computer_double_distance_property(ctx, direction):
    import janusgraph_amd as jg
    graph = modern()
    ids = {v.properties["name"]: vid for vid, v in graph.vertices.items()}
    paths = assert_paths_scoped(ctx, graph, ("knows",), distanceProperty="weight", edgeDirection=direction)
    assert_paths_scoped(ctx, graph, ("knows",), distanceProperty="weight", edgeDirection=direction, maxDistance=1.75)
    assert_paths_scoped(ctx, graph, ("knows",), distanceProperty="weight", edgeDirection=direction, maxDistance=1.5)
    if direction == "out":  # the tie 0.5 + 1.25 == 1.0 + 0.75, the second over either parallel edge's vertices
        tied = [p for p in paths if p[0] == ids["marko"] and p[-1] == ids["peter"]]
        assert {tuple(p) for p in tied} == {(ids["marko"], ids["vadas"], ids["peter"]),
                                            (ids["marko"], ids["josh"], ids["peter"])}
    with pytest.raises(jg.ProgramNotSupported):  # "created" lacks the property
        run(ctx, graph, path_builder(None, distanceProperty="weight", edgeDirection=direction).create())
    with pytest.raises(jg.ProgramNotSupported):
        run(ctx, graph, path_builder(("knows", "created"), distanceProperty="weight").create())
    # the checks look at the scope only: a bad value outside it is legal, inside it refused
    graph.edges[1].properties["weight"] = float("nan")
    graph.edges[3].properties["weight"] = "heavy"
    assert_paths_scoped(ctx, graph, ("knows",), distanceProperty="weight", edgeDirection=direction)
    for bad in (float("inf"), 0.0, -1.0, np.float32(0.5)):
        graph.edges[4].properties["weight"] = bad
        with pytest.raises(jg.ProgramNotSupported):
            run(ctx, graph, path_builder(("knows",), distanceProperty="weight").create())


def test_computer_include_edges_with_distance_property_stays_refused():
    with pytest.raises(ValueError):
        path_builder(("knows",), distanceProperty="weight", includeEdges=True).create()


@pytest.mark.parametrize("labels", GOD_SCOPES + [("lives", "pet")])
def test_computer_connected_components(ctx, labels):
    import janusgraph_amd as jg
    graph = gods()
    small, _ = filtered(graph, labels)
    CC = jg.ConnectedComponentVertexProgram
    got = run(ctx, graph, CC.build().edgeLabels(*labels).create(), persist=jg.Persist.VERTEX_PROPERTIES)
    want = run(ctx, small, CC.build().create(), persist=jg.Persist.VERTEX_PROPERTIES)
    comp = {vid: got.graph().vertices[vid].properties[CC.COMPONENT] for vid in graph.vertices}
    assert comp == {vid: want.graph().vertices[vid].properties[CC.COMPONENT] for vid in small.vertices}
    assert got.memory().getIteration() == want.memory().getIteration()
    unscoped = run(ctx, gods(), CC.build().create(), persist=jg.Persist.VERTEX_PROPERTIES)
    assert comp != {vid: v.properties[CC.COMPONENT] for vid, v in unscoped.graph().vertices.items()}

    def census(g, vp):  # the census route: nothing persisted, only the cluster map-reduces
        mrs = [jg.ClusterCountMapReduce.build().clusterProperty(CC.COMPONENT).create(),
               jg.ClusterPopulationMapReduce.build().clusterProperty(CC.COMPONENT).create()]
        m = run(ctx, g, vp, mrs, jg.Persist.NOTHING).memory()
        return m.get("clusterCount"), m.get("clusterPopulation"), m.getIteration()

    count, population, it = census(gods(), CC.build().edgeLabels(*labels).create())
    assert (count, population, it) == census(small, CC.build().create())
    assert count == len(set(comp.values())) and sum(population.values()) == len(graph.vertices)


@pytest.mark.parametrize("labels", GOD_SCOPES)
@pytest.mark.parametrize("edges", ["outE", "bothE"])
@pytest.mark.parametrize("distribute", [False, True])
def test_computer_peer_pressure(ctx, labels, edges, distribute):
    import janusgraph_amd as jg
    graph = gods()
    small, _ = filtered(graph, labels)
    PP = jg.PeerPressureVertexProgram

    def clusters(g, builder):
        r = run(ctx, g, builder.edges(edges).distributeVote(distribute).create())
        return {vid: r.graph().value(vid, PP.CLUSTER) for vid in g.vertices}, r.memory().getIteration()

    got = clusters(graph, PP.build().edgeLabels(*labels))
    assert got == clusters(small, PP.build())
    if labels == ("brother", "father") and not distribute:
        # unit votes over the scope's edges merge clusters (a distributed vote of hercules, a third along each
        # "battled" edge, never outweighs the receiver's own 1)
        assert len(set(got[0].values())) < len(graph.vertices)
    if labels == ("no such label",):
        assert got[0] == {vid: vid for vid in graph.vertices}


def test_computer_on_two_logical_shards(ctx):
    """Sharded graphs: the plain hop route, CC and the combiner run scoped (finish_labels shards); includeEdges, both
    weighted routes and peer pressure raise ProgramNotSupported, as they do unscoped."""
    import janusgraph_amd as jg
    graph, labels = gods(), ("brother", "father")
    small, _ = filtered(graph, labels)
    ids = {v.properties["name"]: vid for vid, v in graph.vertices.items()}
    source = (ids["hercules"], ids["pluto"])
    CC = jg.ConnectedComponentVertexProgram
    ctx2 = jg.Context((0, 0))
    try:
        got = run(ctx2, graph, path_builder(labels, source=source).create()).memory()
        want = run(ctx, small, path_builder(None, source=source).create()).memory()  # one shard, the scope's edges only
        assert got.get(jg_key()) == want.get(jg_key()) and got.getIteration() == want.getIteration()
        assert len(got.get(jg_key())) > len(source)

        def components(c, g, vp):
            r = run(c, g, vp, persist=jg.Persist.VERTEX_PROPERTIES)
            return {vid: v.properties[CC.COMPONENT] for vid, v in r.graph().vertices.items()}, r.memory().getIteration()

        assert components(ctx2, gods(), CC.build().edgeLabels(*labels).create()) == \
            components(ctx, small, CC.build().create())

        def degrees(c, g, scope):
            vp = jg.CombinerVertexProgram(2, "d", "sum", "inE", 1, True, labels=scope)
            r = run(c, g, vp)
            return {vid: r.graph().value(vid, "d") for vid in g.vertices}

        assert degrees(ctx2, graph, ("battled", "father")) == degrees(ctx, filtered(graph, ("battled", "father"))[0], None)

        refused = [path_builder(labels, source=source, includeEdges=True),
                   path_builder(("battled",), source=source, distanceProperty="time"),
                   jg.PeerPressureVertexProgram.build().edgeLabels(*labels)]
        for b in refused:
            with pytest.raises(jg.ProgramNotSupported):
                run(ctx2, graph, b.create())
        with pytest.raises(jg.ProgramNotSupported):
            run(ctx2, modern(), path_builder(("knows",), distanceProperty="weight").create())
    finally:
        ctx2.close()
