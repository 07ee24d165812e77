"""Edge ordinals, relation ids and fp64 weights of graphs built from edgestore rows (jg_builder_keep_relations,
jg_builder_set_weight_key_f64, jg_graph_edge_relations, jg_*_kept_dag_read_relations).

Every store comes from tests/row_edges_stores.py with its edge list known by construction;
tests/test_row_edges_host.py pins those lists against the oracle on the CPU.  Every comparison here is exact:
integers as integers, doubles through .view(np.int64).  The ids twin of a rows graph is Context.build over the
same edge list with ADJ_EDGE_INDEX, its ordinals mapped through the construction's relation list.
"""
import numpy as np
import pytest

import row_edges_stores as rs
import test_edgestore_paths_host as host
from oracle import edgecodec as ec
from test_gpu_builder import row_chunks

pytestmark = pytest.mark.gpu

DIR_OUT, DIR_IN, DIR_BOTH = 1, 2, 3
DIRS = (DIR_OUT, DIR_IN, DIR_BOTH)


@pytest.fixture(scope="module")
def ctx():
    import janusgraph_amd as jg
    c = jg.Context((0,))
    yield c
    c.close()


def flags_all(index=True):
    import janusgraph_amd as jg
    return jg.ADJ_IN | jg.ADJ_OUT | jg.ADJ_BOTH | (jg._lib.ADJ_EDGE_INDEX if index else 0)


def code(fn, *args):
    import janusgraph_amd as jg
    try:
        fn(*args)
    except jg.JanusGpuError as e:
        return e.code
    return 0


def rows_builder(ctx, store, bounds=None, relations=True, int_key=None, f64_key=None, labels=False):
    """A builder fed the store's rows in chunks of whole rows [bounds[i], bounds[i + 1])."""
    b = ctx.builder()
    b.set_schema(store[5], store[6], 5)
    if relations:
        b.keep_relations()
    if labels:
        b.keep_labels()
    if int_key is not None:
        b.set_weight_key(*rs.key_table(int_key))
    if f64_key is not None:
        b.set_weight_key_f64(*rs.key_table(f64_key))
    for ch in row_chunks(store, [0, len(store[0])] if bounds is None else bounds):
        b.add_rows(*ch)
    return b


def rows_graph(ctx, store, flags=None, **kw):
    b = rows_builder(ctx, store, **kw)
    try:
        return b.finish(flags_all() if flags is None else flags)
    finally:
        b.close()


def thirds(store):
    return np.linspace(0, len(store[0]), 4).astype(int)


def expected_triples(v, src, dst, rel, direction):
    """(row vid, neighbour vid, relation id) of every entry of the `direction` adjacency, sorted."""
    inside = np.isin(src, v) & np.isin(dst, v)
    s, t, r = src[inside].tolist(), dst[inside].tolist(), rel[inside].tolist()
    out = []
    if direction in (DIR_OUT, DIR_BOTH):
        out += list(zip(s, t, r))
    if direction in (DIR_IN, DIR_BOTH):
        out += list(zip(t, s, r))  # BOTH: a self-loop twice on its row
    return sorted(out)


def gpu_triples(g, direction):
    vid = g.vertex_ids()
    rows = np.arange(g.n)
    off, nbr = g.neighbors(rows, direction)
    off2, edge = g.neighbor_edges(rows, direction)
    np.testing.assert_array_equal(off, off2)
    rel = g.edge_relations(edge)
    return sorted(zip(np.repeat(vid, np.diff(off)).tolist(), vid[nbr].tolist(), rel.tolist()))


def assert_exact(g, st):
    """Ordinals and relations of graph g against the construction of store st."""
    src, dst, rel, _ = st.listed()
    np.testing.assert_array_equal(g.vertex_ids(), st.vertices())
    for d in DIRS:
        assert gpu_triples(g, d) == expected_triples(st.vertices(), src, dst, rel, d), d
    # the whole list, ghost-ended edges included, in its order
    np.testing.assert_array_equal(g.edge_relations(np.arange(len(rel))), rel)


# ---------------------------------------------------------------- A: ordinals and relations

@pytest.fixture(scope="module")
def random_store():
    st = rs.store_random()
    return st, st.build()


@pytest.mark.parametrize("nchunks", [1, 3])
def test_ordinals_and_relations(ctx, random_store, nchunks):
    st, store = random_store
    bounds = thirds(store) if nchunks == 3 else None
    src, dst, rel, _ = st.listed()
    v = st.vertices()
    g = rows_graph(ctx, store, bounds=bounds)
    assert_exact(g, st)
    plain = rows_graph(ctx, store, flags=flags_all(False), bounds=bounds, relations=False)
    inside = int((np.isin(src, v) & np.isin(dst, v)).sum())
    # a uint32 ordinal per adjacency entry (OUT, IN, and twice on BOTH), 8 bytes per listed edge
    assert g.info()["device_bytes"] == plain.info()["device_bytes"] + 4 * 4 * inside + 8 * len(rel)
    # the same builder finished without the flag: the plain graph
    dropped = rows_graph(ctx, store, flags=flags_all(False), bounds=bounds)
    assert dropped.info()["device_bytes"] == plain.info()["device_bytes"]
    rows = np.arange(plain.n)
    for d in DIRS:
        for a, b in zip(dropped.neighbors(rows, d), plain.neighbors(rows, d)):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(g.neighbors(rows, d), plain.neighbors(rows, d)):
            np.testing.assert_array_equal(a, b)
    import janusgraph_amd as jg
    assert code(dropped.edge_relations, [0]) == jg._lib.JG_ERR_UNSUPPORTED
    for x in (g, plain, dropped):
        x.close()


# ---------------------------------------------------------------- B: tile edges of the decoder

def test_decoder_tile_edges(ctx):
    from janusgraph_amd import _lib
    st, hub = rs.store_tiles()
    store = st.build()
    h = st.order().index(hub)
    nrows = len(store[0])
    lowered = 1000
    cut = host.one_shot_chunks(store[1], store[3], lowered, 1 << 30)  # the chunker's rule under a lowered limit
    assert h in cut and h + 1 in cut  # the hub is a chunk of its own
    _lib.tune_set("edgestore_chunk_entries", lowered)
    try:
        for bounds in (None, [0, h + 1, nrows], cut):
            g = rows_graph(ctx, store, bounds=bounds)
            assert_exact(g, st)
            g.close()
    finally:
        _lib.tune_set("edgestore_chunk_entries", host.CHUNKER_DEFAULTS[0])


# ---------------------------------------------------------------- C: includeEdges from rows

def twin_of(ctx, st, weight=None):
    src, dst, rel, _ = st.listed()
    return ctx.build(st.vertices(), src, dst, weight, flags=flags_all())


def per_vertex(dag, names):
    """{DAG vertex: sorted [(pred, name of its edge)]}"""
    vertex, value, off, pred, edge = dag
    named = np.asarray(names)[edge] if names is not None else edge
    return {int(v): sorted(zip(pred[off[j]:off[j + 1]].tolist(), named[off[j]:off[j + 1]].tolist()))
            for j, v in enumerate(vertex.tolist())}


def assert_same_dag(rows_dag, twin_dag, rel):
    def exact(x):  # doubles compare by their bits
        return x.view(np.int64) if x.dtype == np.float64 else x

    for k in range(3):  # vertex, depth / distance, offsets
        np.testing.assert_array_equal(exact(rows_dag[k]), exact(twin_dag[k]))
    assert rows_dag[4].dtype == np.int64
    assert per_vertex(rows_dag, None) == per_vertex(twin_dag, rel)


def live_sources(st, k=3):
    src, dst, rel, _ = st.listed()
    v = st.vertices()
    deg = {}
    for a in src[np.isin(dst, v)].tolist():
        deg[a] = deg.get(a, 0) + 1
    return [a for a, _ in sorted(deg.items(), key=lambda x: (-x[1], x[0]))[:k]]


def test_bfs_dag_relations(ctx, random_store):
    st, store = random_store
    rel = st.listed()[2]
    g, twin = rows_graph(ctx, store), twin_of(ctx, st)
    sources = live_sources(st)
    for d in DIRS:
        g.bfs_keep(sources, d)
        twin.bfs_keep(sources, d)
        for s in range(len(sources)):
            assert_same_dag(g.bfs_kept_dag_relations(s), twin.bfs_kept_dag_edges(s), rel)
    g.close()
    twin.close()


def test_diamond_edge_paths(ctx):
    from janusgraph_amd.computer import DevicePathDag
    st, (s, a, b, t), rel = rs.diamond()
    store = st.build()
    g, twin = rows_graph(ctx, store), twin_of(ctx, st)
    vid = g.vertex_ids().tolist()
    for d in DIRS:
        g.bfs_keep([s, a, t], d)
        twin.bfs_keep([s, a, t], d)
        for k in range(3):
            assert_same_dag(g.bfs_kept_dag_relations(k), twin.bfs_kept_dag_edges(k), st.listed()[2])
    g.bfs_keep([s], DIR_OUT)
    dag = g.bfs_kept_dag_relations(0)
    paths, deepest = DevicePathDag(g.n).edge_paths(dag, vid.index(s))
    named = sorted(tuple(vid[x] if i % 2 == 0 else x for i, x in enumerate(p)) for p in paths)
    assert deepest == 2
    assert named == sorted([(s,), (s, rel["sa"], a), (s, rel["sb"], b), (s, rel["sa"], a, rel["at1"], t),
                            (s, rel["sa"], a, rel["at2"], t), (s, rel["sb"], b, rel["bt"], t)])
    g.close()
    twin.close()


def test_sssp_dag_relations_integer_row_weights(ctx):
    import janusgraph_amd as jg
    st = rs.store_random(seed=7, value_of=lambda e, rng: rs.weight_value(ec.INT, 1 + e % 9, rng))
    store = st.build()
    rel = st.listed()[2]
    w = np.array([1 + st.edge_no[r] % 9 for r in rel.tolist()], np.int32)
    flags = jg.ADJ_IN | jg.ADJ_OUT | jg._lib.ADJ_EDGE_INDEX
    g = rows_graph(ctx, store, flags=flags, bounds=thirds(store), int_key=ec.INT)
    twin = ctx.build(st.vertices(), st.listed()[0], st.listed()[1], w, flags=flags)
    for source in live_sources(st):
        for d in (DIR_OUT, DIR_IN):
            g.sssp_keep(source, d)
            twin.sssp_keep(source, d)
            np.testing.assert_array_equal(g.sssp_kept_row(), twin.sssp_kept_row())
            assert_same_dag(g.sssp_kept_dag_relations(), twin.sssp_kept_dag_edges(), rel)
    g.close()
    twin.close()


# ---------------------------------------------------------------- D: doubles from rows

@pytest.mark.parametrize("nchunks", [1, 3])
def test_star_doubles_bit_for_bit(ctx, nchunks):
    st, hub, w = rs.store_star()
    store = st.build()
    g = rows_graph(ctx, store, bounds=thirds(store) if nchunks == 3 else None, f64_key=ec.DOUBLE)
    g.sssp_keep_f64(hub, DIR_OUT)
    row = g.sssp_kept_row_f64()
    vid = g.vertex_ids().tolist()
    want = np.array([0.0 if u == hub else w[u] for u in vid], np.float64)
    np.testing.assert_array_equal(row.view(np.int64), want.view(np.int64))
    g.close()


def f64_pair(ctx, wtype, weight_of, bounds=True, seed=11):
    """(store, rows graph decoding `wtype` weights, ids twin given float(weight) through set_weights_f64)."""
    st = rs.store_random(seed=seed, value_of=lambda e, rng: rs.weight_value(wtype, weight_of(e), rng))
    store = st.build()
    rel = st.listed()[2]
    w = np.array([float(weight_of(st.edge_no[r])) for r in rel.tolist()], np.float64)
    g = rows_graph(ctx, store, bounds=thirds(store) if bounds else None, f64_key=wtype)
    twin = twin_of(ctx, st)
    twin.set_weights_f64(w)
    return st, g, twin


def assert_same_planes(ctx, st, g, twin, dag=False):
    rel = st.listed()[2]
    for source in live_sources(st):
        for d in DIRS:
            g.sssp_keep_f64(source, d)
            levels = ctx.stats()["levels"]
            twin.sssp_keep_f64(source, d)
            assert ctx.stats()["levels"] == levels
            np.testing.assert_array_equal(g.sssp_kept_row_f64().view(np.int64), twin.sssp_kept_row_f64().view(np.int64))
            if dag:
                assert_same_dag(g.sssp_kept_dag_relations_f64(), twin.sssp_kept_dag_edges_f64(), rel)


def test_random_doubles_equal_the_ids_twin(ctx):
    ws = np.random.default_rng(4).uniform(0.5, 2.0, 3000)
    st, g, twin = f64_pair(ctx, ec.DOUBLE, lambda e: float(ws[e]))
    assert_same_planes(ctx, st, g, twin, dag=True)
    # a later set_weights_f64 on the rows graph replaces the decoded weights (m = the list length)
    m = len(st.listed()[2])
    g.set_weights_f64(np.full(m, 1.0))
    twin.set_weights_f64(np.full(m, 1.0))
    source = live_sources(st)[0]
    g.sssp_keep_f64(source, DIR_BOTH)
    twin.sssp_keep_f64(source, DIR_BOTH)
    np.testing.assert_array_equal(g.sssp_kept_row_f64().view(np.int64), twin.sssp_kept_row_f64().view(np.int64))
    g.close()
    twin.close()


@pytest.mark.parametrize("wtype", [ec.INT, ec.LONG])
def test_integer_keys_as_f64_weights(ctx, wtype):
    st, g, twin = f64_pair(ctx, wtype, lambda e: 1 + (e * 7919) % 1000)
    assert_same_planes(ctx, st, g, twin)
    g.close()
    twin.close()


def chain_finish(ctx, wtype, weights, values=None, flags=None):
    """The status of finishing a chain store whose edges carry `weights` as `wtype` (values: the raw value bytes
    instead); the builder is closed either way."""
    if values is None:
        values = [rs.weight_value(wtype, w, pad=i % 10) for i, w in enumerate(weights)]
    st, vs = rs.store_chain(values)
    b = rows_builder(ctx, st.build(), f64_key=wtype)
    got = []

    def finish():
        got.append(b.finish(flags_all() if flags is None else flags))

    status = code(finish)
    for g in got:
        g.close()
    b.close()
    return status


def test_long_beyond_2_53_is_refused(ctx):
    import janusgraph_amd as jg
    E = jg._lib
    big = 1 << 53
    assert chain_finish(ctx, ec.LONG, [big, big, big]) == 0
    assert chain_finish(ctx, ec.LONG, [big, big + 1, big]) == E.JG_ERR_UNSUPPORTED
    assert chain_finish(ctx, ec.LONG, [big, -(big + 1), big]) == E.JG_ERR_UNSUPPORTED
    assert chain_finish(ctx, ec.INT, [5, big + 1, 5]) == E.JG_ERR_UNSUPPORTED


def test_f64_key_types_refused_at_the_set_call(ctx):
    import janusgraph_amd as jg
    E = jg._lib
    wid, ids, types = rs.key_table(ec.DOUBLE)
    for wtype in (ec.FLOAT, ec.STRING, ec.DATE, 0, 99):  # a Float key, other types, unknown types
        b = ctx.builder()
        assert code(b.set_weight_key_f64, wid, ids, types[:2] + [wtype]) == E.JG_ERR_UNSUPPORTED, wtype
        b.close()
    b = ctx.builder()
    assert code(b.set_weight_key_f64, wid, ids[:2], types[:2]) == E.JG_ERR_UNSUPPORTED  # a key not in the table
    assert code(b.set_weight_key_f64, wid, [], []) == E.JG_ERR_UNSUPPORTED
    b.set_weight_key_f64(wid, ids, types)  # the refusals left the builder usable
    b.close()


def test_f64_refusals_at_finish(ctx):
    import janusgraph_amd as jg
    E = jg._lib
    D = ec.DOUBLE
    assert chain_finish(ctx, D, [1.0, 1.5, 0.75]) == 0
    assert chain_finish(ctx, D, [1.0, None, 0.75]) == E.JG_ERR_ARG    # an edge without the property
    assert chain_finish(ctx, D, [1.0, "null", 0.75]) == E.JG_ERR_ARG  # a null value
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert chain_finish(ctx, D, [1.0, bad, 0.75]) == E.JG_ERR_ARG, bad
    assert chain_finish(ctx, D, [1e-300, 1e300, 1.0]) == E.JG_ERR_UNSUPPORTED  # an absorbing range
    whole = [rs.weight_value(D, w, pad=3) for w in (1.0, 1.5, 0.75)]
    for cut in (1, 7, 8):  # the value cut short at the end of its entry (8: the flag byte is the last)
        values = [whole[0], whole[1][:-cut], whole[2]]
        assert chain_finish(ctx, D, None, values=values) == E.JG_ERR_ARG, cut
    assert chain_finish(ctx, D, [1.0, 1.5, 0.75], flags=flags_all(False)) == E.JG_ERR_ARG  # without EDGE_INDEX


# ---------------------------------------------------------------- E: state and refusals

def test_state_and_refusals(ctx, random_store):
    import janusgraph_amd as jg
    E = jg._lib
    st, store = random_store
    vid = (np.arange(4, dtype=np.int64) + 1) * 10
    b = rows_builder(ctx, store, relations=False)
    assert code(b.keep_relations) == E.JG_ERR_STATE  # after a chunk
    assert code(b.set_weight_key_f64, *rs.key_table(ec.DOUBLE)) == E.JG_ERR_STATE
    assert code(b.finish, flags_all()) == E.JG_ERR_UNSUPPORTED  # no opt-in: the flag stays refused
    b.close()
    b = ctx.builder()
    b.keep_relations()
    assert code(b.set_query_limit, 100, jg.DIR_OUT) == E.JG_ERR_STATE
    b.set_query_limit(0, jg.DIR_OUT)  # no limit: allowed
    assert code(b.add_vertices, vid) == E.JG_ERR_ARG  # ids chunks on a relation-keeping builder
    assert code(b.add_edges, vid[:2], vid[1:3]) == E.JG_ERR_ARG
    b.keep_labels()
    assert code(b.add_edges, vid[:2], vid[1:3], None, [1, 2]) == E.JG_ERR_ARG
    b.close()
    b = ctx.builder()
    b.set_query_limit(100, jg.DIR_OUT)
    assert code(b.keep_relations) == E.JG_ERR_STATE
    b.close()
    for first, second in (("set_weight_key", "set_weight_key_f64"), ("set_weight_key_f64", "set_weight_key")):
        b = ctx.builder()
        getattr(b, first)(*rs.key_table(ec.INT))
        assert code(getattr(b, second), *rs.key_table(ec.INT)) == E.JG_ERR_STATE
        b.close()
    # keep_labels with keep_relations: finish_labels keeps refusing the flag
    b = rows_builder(ctx, store, labels=True)
    assert code(b.finish_labels, [rs.LABELS[0]], flags_all()) == E.JG_ERR_UNSUPPORTED
    g = b.finish(flags_all())
    assert_exact(g, st)
    g.close()
    b.close()
    ctx2 = jg.Context((0, 0))  # two logical shards
    try:
        b = rows_builder(ctx2, store)
        assert code(b.finish, flags_all()) == E.JG_ERR_UNSUPPORTED
        g = b.finish(flags_all(False))
        assert g.info()["num_shards"] == 2 and code(g.edge_relations, [0]) == E.JG_ERR_UNSUPPORTED
        g.close()
        b.close()
    finally:
        ctx2.close()
    src, dst, rel, _ = st.listed()
    twin = twin_of(ctx, st)
    assert code(twin.edge_relations, [0]) == E.JG_ERR_UNSUPPORTED  # an ids graph holds no relation ids
    twin.bfs_keep([int(src[0])], DIR_OUT)
    twin.bfs_kept_dag_edges_build(0)
    assert code(twin.bfs_kept_dag_read_relations, 0, 1) == E.JG_ERR_UNSUPPORTED
    twin.close()
    g = rows_graph(ctx, store)
    m = len(rel)
    assert len(g.edge_relations([])) == 0
    assert g.edge_relations([m - 1]).tolist() == [int(rel[-1])]
    assert code(g.edge_relations, [m]) == E.JG_ERR_ARG
    assert code(g.edge_relations, [0, 1, m, 2]) == E.JG_ERR_ARG
    assert code(g.edge_relations, [0xFFFFFFFF]) == E.JG_ERR_ARG
    source = live_sources(st)[0]
    assert code(g.bfs_kept_dag_read_relations, 0, 1) == E.JG_ERR_STATE  # none held
    g.bfs_keep([source], DIR_OUT)
    nv, ne, _ = g.bfs_kept_dag_build(0)  # a plain DAG
    assert code(g.bfs_kept_dag_read_relations, 0, 1, 1) == E.JG_ERR_STATE
    nv, ne, _ = g.bfs_kept_dag_edges_build(0)
    assert len(g.bfs_kept_dag_read_relations(0, nv, ne)) == ne
    assert code(g.bfs_kept_dag_read_relations, 0, g.n + 1, 1) == E.JG_ERR_ARG
    assert code(g.bfs_kept_dag_read_relations, nv, 1, 1) == E.JG_ERR_ARG
    assert code(g.sssp_kept_dag_read_relations, 0, 1, 1) == E.JG_ERR_STATE  # no weighted DAG held
    g.close()
