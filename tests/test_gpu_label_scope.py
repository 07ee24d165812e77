"""Label-scoped graphs from one snapshot (jg_builder_keep_labels / jg_builder_add_labeled_edges /
jg_builder_finish_labels): the typed message scopes of Fulgora (VertexProgramScanJob.java:126-134,
BasicVertexCentricQueryBuilder.java:482-587).

The expected values always come from filtering on the host and then using what exists: Context.build /
build_edgestore (or a plain builder) of the pre-filtered input, and the CPU oracle on the filtered edge
list.  Integer outputs are compared exactly, PageRank within 1e-9 relative per vertex of oracle.pagerank.
"""
import numpy as np
import pytest

from janusgraph_amd.idmanager import IDManager
from oracle import edgecodec as ec
from oracle import pymirror as pm

pytestmark = pytest.mark.gpu

INFO_KEYS = ("num_vertices", "num_edges", "ghost_edges", "self_loops", "truncated_vertices", "max_in_degree",
             "max_out_degree", "num_shards", "flags")
DIRS = (1, 2, 3)  # DIR_OUT, DIR_IN, DIR_BOTH


def scope_info(g):
    i = g.info()
    return {k: i[k] for k in INFO_KEYS}


def sorted_rows(g, direction):
    off, nbr = g.neighbors(np.arange(g.n, dtype=np.int64), direction)
    return off, np.concatenate([np.sort(nbr[off[i]:off[i + 1]]) for i in range(g.n)] + [np.zeros(0, np.int64)])


def dense(vid, src, dst, weight=None):
    """Dense (caller-order) endpoints of the edges with both endpoints in vid, and their weights."""
    index = {int(v): i for i, v in enumerate(vid)}
    ds = np.array([index.get(int(a), -1) for a in src], np.int64)
    dd = np.array([index.get(int(b), -1) for b in dst], np.int64)
    ok = (ds >= 0) & (dd >= 0)
    w = None if weight is None else np.asarray(weight, np.int32)[ok]
    return ds[ok].astype(np.int32), dd[ok].astype(np.int32), w


def assert_same_graph(o, g, ref, vid, ds, dd, w=None, sources=(), seed=None, full=True):
    """g (scoped) against ref (the host-filtered build) and the oracle on the filtered dense edges."""
    n = len(vid)
    assert np.array_equal(g.vertex_ids(), vid) and np.array_equal(ref.vertex_ids(), vid)
    assert scope_info(g) == scope_info(ref)
    assert g.info()["num_edges"] == len(ds)
    rank, ecount = g.pagerank(0.85, n, 10)
    rank_ref, ecount_ref = ref.pagerank(0.85, n, 10)
    want, want_e = o.pagerank(n, ds, dd, 0.85, n, 10)
    assert np.max(np.abs(rank - want) / np.abs(want)) <= 1e-9
    assert np.max(np.abs(rank - rank_ref) / np.abs(want)) <= 1e-9
    np.testing.assert_array_equal(ecount, want_e)
    np.testing.assert_array_equal(ecount, ecount_ref)
    comp, it = g.connected_components()
    comp_ref, it_ref = ref.connected_components()
    want_c, want_it = o.connected_components(n, ds, dd, vid)
    np.testing.assert_array_equal(comp, want_c)
    np.testing.assert_array_equal(comp, comp_ref)
    assert it == it_ref == want_it
    if not full:
        return
    for d in DIRS:
        np.testing.assert_array_equal(g.degrees(d), ref.degrees(d))
        off, nbr = sorted_rows(g, d)
        off_ref, nbr_ref = sorted_rows(ref, d)
        np.testing.assert_array_equal(off, off_ref)
        np.testing.assert_array_equal(nbr, nbr_ref)
    np.testing.assert_array_equal(g.degrees(1), np.bincount(ds, minlength=n))
    np.testing.assert_array_equal(g.degrees(2), np.bincount(dd, minlength=n))
    for d in (3, 1):
        depth = g.bfs(vid[list(sources)], d)
        np.testing.assert_array_equal(depth, ref.bfs(vid[list(sources)], d))
        for k, s in enumerate(sources):
            np.testing.assert_array_equal(depth[k], o.bfs(n, ds, dd, s, d))
    init = np.random.default_rng(17).integers(-(1 << 31), 1 << 31, n)
    for d in DIRS:
        for combiner in (0, 1, 2):
            x, rec = g.combine_steps(d, combiner, 2, init, True)
            x_ref, rec_ref = ref.combine_steps(d, combiner, 2, init, True)
            np.testing.assert_array_equal(x, x_ref)
            np.testing.assert_array_equal(rec, rec_ref)
            want_x, want_rec = o.combine_steps(n, ds, dd, d, combiner, 2, init, True)
            np.testing.assert_array_equal(x, want_x)
            np.testing.assert_array_equal(rec, want_rec)
    if seed is not None:
        dist = g.shortest_distance(int(vid[seed]), 4)
        np.testing.assert_array_equal(dist, ref.shortest_distance(int(vid[seed]), 4))
        np.testing.assert_array_equal(dist, o.shortest_distance(n, ds, dd, seed, 4, w))


# ---- 1. ids mode ----
LABELS = np.array([-7, 5, (1 << 40) + 3, 1 << 62], np.int64)  # opaque int64 values
UNKNOWN = 12345


def labeled_ids(n=300, m=5003, seed=3):
    rng = np.random.default_rng(seed)
    vid = (rng.permutation(4 * n)[:n].astype(np.int64) + 1) << 8
    s = rng.integers(0, n, m)
    t = rng.integers(0, n, m)
    t[: m // 50] = s[: m // 50]  # self-loops
    s[m // 50: m // 25] = s[0]   # a hub with multi-edges
    t[m // 50: m // 25] = t[1]
    src, dst = vid[s], vid[t]
    ghost = rng.random(m) < 0.05  # edges to ids the scan never returned
    dst[ghost] = ((1 << 35) + rng.integers(0, 1000, int(ghost.sum()))) << 8
    src[m - 7:] = (1 << 36) << 8  # and from one
    lab = LABELS[rng.integers(0, 4, m)]
    w = rng.integers(1, 256, m).astype(np.int32)
    return vid, src, dst, w, lab


@pytest.fixture(scope="module")
def ids_case():
    import janusgraph_amd as jg
    vid, src, dst, w, lab = labeled_ids()
    ctx = jg.Context((0,))
    b = ctx.builder()
    b.keep_labels()
    for part in np.array_split(np.arange(len(vid)), 2):
        b.add_vertices(vid[part])
    for part in np.array_split(np.arange(len(src)), 3):
        b.add_edges(src[part], dst[part], w[part], label=lab[part])
    yield ctx, b, (vid, src, dst, w, lab)
    b.close()
    ctx.close()


@pytest.mark.parametrize("scope", [(0,), (1, 3), (0, 1, 2, 3), (0, 0), None], ids=["L0", "L1L3", "all", "dup", "unknown"])
def test_ids_scope_equals_host_filtered_build(oracle_lib, ids_case, scope):
    import janusgraph_amd as jg
    ctx, b, (vid, src, dst, w, lab) = ids_case
    labels = [UNKNOWN] if scope is None else [int(LABELS[i]) for i in scope]
    mask = np.isin(lab, labels)
    assert (mask.sum() == 0) == (scope is None)
    g = b.finish_labels(labels)
    st = ctx.stats()
    kept = int(mask.sum())
    assert st["build_ms"] > 0 and st["kernel_launches"] == (2 if kept else 1) and st["kernel_ms_total"] > 0
    assert st["algorithmic_bytes"] == 16.0 * len(src) + 2 * 20.0 * kept
    ref = ctx.build(vid, src[mask], dst[mask], weight=w[mask])
    ds, dd, dw = dense(vid, src[mask], dst[mask], w[mask])
    assert g.info()["ghost_edges"] == kept - len(ds)
    seed = int(dd[0]) if len(dd) else 0
    assert_same_graph(oracle_lib, g, ref, vid, ds, dd, dw, sources=(0, 7, seed), seed=seed)
    g.close()
    ref.close()


def test_ids_scopes_share_the_vertex_set(ids_case):
    ctx, b, (vid, src, dst, w, lab) = ids_case
    graphs = [b.finish_labels([int(x)]) for x in LABELS] + [b.finish_labels(LABELS), b.finish_labels([UNKNOWN])]
    for g in graphs:
        assert np.array_equal(g.vertex_ids(), vid)
        g.close()


# ---- 2. tile edges ----
@pytest.mark.parametrize("tiles,extra", [(0, 0), (0, 1), (1, -1), (1, 0), (1, 1), (64, 17)])
def test_tile_boundaries(tiles, extra):
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    T = _lib.SCOPE_TILE
    m = tiles * T + extra
    n = 64
    rng = np.random.default_rng(m)
    vid = (np.arange(n, dtype=np.int64) + 1) << 8
    s, t = rng.integers(0, n, m), rng.integers(0, n, m)
    lab = rng.integers(0, 3, m).astype(np.int64)  # 0 and 2 are kept, 1 is dropped
    lab[:T] = 2       # a fully kept tile (or the whole list when it is shorter)
    lab[T:2 * T] = 1  # a fully dropped tile
    w = rng.integers(1, 100, m).astype(np.int32)
    ctx = jg.Context((0,))
    for weighted in (False, True):
        b = ctx.builder()
        b.keep_labels()
        b.add_vertices(vid)
        b.add_edges(vid[s], vid[t], w if weighted else None, label=lab)
        g = b.finish_labels([0, 2], jg.ADJ_OUT | jg.ADJ_IN)
        b.close()
        mask = lab != 1
        assert g.info()["num_edges"] == int(mask.sum())
        off, nbr = g.neighbors(np.arange(n, dtype=np.int64), jg.DIR_OUT)
        got = sorted(zip(np.repeat(np.arange(n), np.diff(off)).tolist(), nbr.tolist()))
        assert got == sorted(zip(s[mask].tolist(), t[mask].tolist()))
        if weighted and m:
            ref = ctx.build(vid, vid[s[mask]], vid[t[mask]], weight=w[mask], flags=jg.ADJ_OUT | jg.ADJ_IN)
            seed = int(vid[t[mask][0]]) if mask.any() else int(vid[0])
            np.testing.assert_array_equal(g.shortest_distance(seed, 3), ref.shortest_distance(seed, 3))
            ref.close()
        g.close()
    ctx.close()


# ---- 3. rows mode ----
EDGE_LABELS = [ec.schema_id(c, "user_edge") for c in (11, 12, 13, 14)]
EDGE_MULTS = [ec.MULTI, ec.SIMPLE, ec.ONE2MANY, ec.MANY2ONE]
DIST_KEY = ec.schema_id(9, "user_key")  # the Integer weight key of the weighted store
VEXISTS = ec.schema_id(1, "system_key")


def labeled_store(n=300, m=2000, seed=0, ghosts=0.08, partition_bits=5, partitioned=4, weighted=False):
    """An edgestore in JanusGraph's layout (as tests/test_edgestore.py writes it): four edge labels of
    different multiplicities, ghost rows, vertex-cut representatives, system and invisible edges, schema
    rows; with `weighted` every edge carries an Integer property.  Returns the store arrays."""
    from oracle.oracle import canonical_vertex_id
    rng = np.random.default_rng(seed)
    idm = IDManager(partition_bits)
    vids, seen = [], set()
    while len(vids) < n:
        v = (((int(rng.integers(1, 1 << 30)) << partition_bits) + int(rng.integers(0, 1 << partition_bits))) << 3)
        if v not in seen:
            seen.add(v)
            vids.append(v)
    reps = {}
    for i in range(n - partitioned, n):
        count = int(rng.integers(1, 1 << 30))
        canon = canonical_vertex_id((count << (partition_bits + 3)) | 2, partition_bits)
        others = [x for x in ((((count << partition_bits) + p) << 3) | 2 for p in range(1 << partition_bits)) if x != canon]
        vids[i] = canon
        reps[i] = [canon] + [others[int(k)] for k in rng.choice(len(others), 2, replace=False)]
    ghost = rng.random(n) < ghosts
    ghost[n - partitioned:] = False
    name_key = ec.schema_id(5, "user_key")
    sys_edge = ec.schema_id(2, "system_edge")
    s, t = rng.integers(0, n, m), rng.integers(0, n, m)
    t[: m // 50] = s[: m // 50]
    s[m // 50: m // 25] = s[0]
    t[m // 50: m // 25] = t[0]
    lab = rng.choice(4, m, p=[0.4, 0.3, 0.2, 0.1])
    rows = {}

    def row_of(i):
        return reps[i][int(rng.integers(0, 3))] if i in reps else vids[i]

    rel = 1000
    for i in range(n):
        for rv in reps.get(i, [vids[i]]):
            rows.setdefault(rv, [])
        if not ghost[i]:
            rows[vids[i]].append(ec.encode_property(VEXISTS, rel, b"\x01"))
            rel += 1
        rows[vids[i]].append(ec.encode_property(name_key, rel, b"name%d" % i))
        rel += 1
        if rng.integers(0, 10) == 0:
            rows[vids[i]].append(ec.encode_edge(sys_edge, ec.OUT, vids[int(rng.integers(0, n))], rel))
            rel += 1
        if rng.integers(0, 10) == 0:
            rows[vids[i]].append(ec.encode_edge(EDGE_LABELS[0], ec.OUT, vids[int(rng.integers(0, n))], rel,
                                                invisible=True))
            rel += 1
    for e in range(m):
        a, b, L = int(s[e]), int(t[e]), int(lab[e])
        ra, rb = row_of(a), row_of(b)
        value = ec.write_properties([(DIST_KEY, ec.INT, int(rng.integers(1, 10)))]) if weighted else b""
        rows[ra].append(ec.encode_edge(EDGE_LABELS[L], ec.OUT, rb, rel, EDGE_MULTS[L], value=value))
        rows[rb].append(ec.encode_edge(EDGE_LABELS[L], ec.IN, ra, rel, EDGE_MULTS[L], value=value))
        rel += 1
    keys = [idm.get_key(v) for v in rows]
    ents = list(rows.values())
    for c in (3, 7, 9):  # schema rows (odd keys), never decoded
        keys.append(ec.schema_id(c, "user_edge"))
        ents.append([(b"\xff\xff\xff", 1)])
    order = sorted(range(len(keys)), key=lambda r: keys[r])
    data, off, vpos, roff = bytearray(), [0], [], [0]
    for r in order:
        for b, vp in sorted(ents[r], key=lambda ev: ev[0][: ev[1]]):
            data += b
            off.append(len(data))
            vpos.append(vp)
        roff.append(len(vpos))
    return (np.array([keys[r] for r in order], np.uint64), np.array(roff, np.int64), bytes(data),
            np.array(off, np.int64), np.array(vpos, np.int32), np.array(EDGE_LABELS[1:], np.int64),
            np.array(EDGE_MULTS[1:], np.int8))


def strip_entries(store, keep):
    """The store without the entries whose keep flag is False (rows stay, possibly shorter)."""
    keys, roff, data, off, vpos, tids, tmult = store
    buf = np.frombuffer(data, np.uint8)
    idx = np.flatnonzero(keep)
    lens = np.diff(off)[idx]
    new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    new_data = b"".join(bytes(buf[off[e]:off[e + 1]]) for e in idx)
    new_roff = np.concatenate([[0], np.cumsum(keep)])[roff].astype(np.int64)
    return keys, new_roff, new_data, new_off, vpos[idx], tids, tmult


def row_chunks(store, nchunks):
    keys, roff, data, off, vpos, _, _ = store
    bounds = np.linspace(0, len(keys), nchunks + 1).astype(int)
    for r0, r1 in zip(bounds[:-1], bounds[1:]):
        e0, e1 = int(roff[r0]), int(roff[r1])
        b0, b1 = int(off[e0]), int(off[e1])
        yield keys[r0:r1], roff[r0:r1 + 1] - e0, data[b0:b1], off[e0:e1 + 1] - b0, vpos[e0:e1]


@pytest.fixture(scope="module")
def rows_case(oracle_lib):
    store = labeled_store()
    keys, roff, data, off, vpos, tids, tmult = store
    etype, _, _, _ = oracle_lib.decode_edges(data, off, vpos, tids, tmult)  # the label of every entry
    return store, etype


@pytest.mark.parametrize("nchunks", [1, 3])
def test_rows_scope_equals_host_stripped_store(oracle_lib, rows_case, nchunks):
    import janusgraph_amd as jg
    store, etype = rows_case
    keys, roff, data, off, vpos, tids, tmult = store
    ctx = jg.Context((0,))
    b = ctx.builder()
    b.keep_labels()
    b.set_schema(tids, tmult, 5)
    for ch in row_chunks(store, nchunks):
        b.add_rows(*ch)
    vid = None
    for scope in ([EDGE_LABELS[0]], [EDGE_LABELS[3], EDGE_LABELS[1]], EDGE_LABELS):
        others = [x for x in EDGE_LABELS if x not in scope]
        stripped = strip_entries(store, ~np.isin(etype, others))
        ref, ref_vid = ctx.build_edgestore(*stripped)
        ov, os_, ot = oracle_lib.edgestore_snapshot(*stripped)
        g = b.finish_labels(scope)
        if vid is None:
            vid = g.vertex_ids()
        assert np.array_equal(ref_vid, vid) and np.array_equal(ov, vid)
        ds, dd, _ = dense(ov, os_, ot)
        assert_same_graph(oracle_lib, g, ref, vid, ds, dd, full=False)
        if len(scope) == 4:  # every label: the same graph as finish() on the same builder, called last
            last = b.finish()
            assert_same_graph(oracle_lib, last, g, vid, ds, dd, full=False)
            np.testing.assert_array_equal(last.pagerank(0.85, len(vid), 10)[0], g.pagerank(0.85, len(vid), 10)[0])
            last.close()
        g.close()
        ref.close()
    b.close()
    ctx.close()


def test_rows_scope_with_device_decoded_weights(oracle_lib):
    import janusgraph_amd as jg
    store = labeled_store(seed=5, weighted=True)
    keys, roff, data, off, vpos, tids, tmult = store
    etype, _, _, _ = oracle_lib.decode_edges(data, off, vpos, tids, tmult)
    scope = [EDGE_LABELS[0], EDGE_LABELS[2]]
    stripped = strip_entries(store, ~np.isin(etype, [x for x in EDGE_LABELS if x not in scope]))
    ctx = jg.Context((0,))
    graphs = []
    for st, labeled in ((store, True), (stripped, False)):
        b = ctx.builder()
        if labeled:
            b.keep_labels()
        b.set_schema(tids, tmult, 5)
        b.set_weight_key(ec.inline_id(DIST_KEY), [ec.inline_id(DIST_KEY)], [ec.INT])
        for ch in row_chunks(st, 2):
            b.add_rows(*ch)
        graphs.append(b.finish_labels(scope, jg.ADJ_IN | jg.ADJ_OUT) if labeled else b.finish(jg.ADJ_IN | jg.ADJ_OUT))
        b.close()
    g, ref = graphs
    vid = g.vertex_ids()
    assert np.array_equal(vid, ref.vertex_ids())
    assert scope_info(g) == scope_info(ref) and g.info()["num_edges"] > 0
    ov, os_, ot = oracle_lib.edgestore_snapshot(*stripped)
    assert np.array_equal(ov, vid)
    _, dd, _ = dense(ov, os_, ot)
    reached = 0
    for seed in (int(vid[dd[0]]), int(vid[dd[len(dd) // 2]]), int(vid[0])):
        dist = g.shortest_distance(seed, 5)
        np.testing.assert_array_equal(dist, ref.shortest_distance(seed, 5))
        reached += int((dist != jg.DIST_ABSENT).sum())
    assert reached > 3
    g.close()
    ref.close()
    ctx.close()


# ---- 4. two logical shards ----
def test_two_logical_shards_equal_one(oracle_lib):
    import janusgraph_amd as jg
    vid, src, dst, w, lab = labeled_ids(seed=9)
    scope = [int(LABELS[1]), int(LABELS[2])]
    out = []
    for devices in ((0,), (0, 0)):
        ctx = jg.Context(devices)
        b = ctx.builder()
        b.keep_labels()
        b.add_vertices(vid)
        b.add_edges(src, dst, w, label=lab)
        g = b.finish_labels(scope)
        b.close()
        assert g.info()["num_shards"] == len(devices)
        out.append((g.pagerank(0.85, len(vid), 10)[0], g.bfs(vid[[0, 5, 11]], jg.DIR_BOTH), g.bfs(vid[[0, 5, 11]], jg.DIR_OUT),
                    g.info()["num_edges"]))
        g.close()
        ctx.close()
    mask = np.isin(lab, scope)
    ds, dd, _ = dense(vid, src[mask], dst[mask])
    want, _ = oracle_lib.pagerank(len(vid), ds, dd, 0.85, len(vid), 10)
    for rank, both, outd, m in out:
        assert m == len(ds)
        assert np.max(np.abs(rank - want) / np.abs(want)) <= 1e-9
        np.testing.assert_array_equal(both, out[0][1])
        np.testing.assert_array_equal(outd, out[0][2])
    np.testing.assert_array_equal(out[0][1][1], oracle_lib.bfs(len(vid), ds, dd, 5, oracle_lib.DIR_BOTH))


# ---- 5. state and argument errors ----
def test_state_and_argument_errors():
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    ctx = jg.Context((0,))
    v = np.array([256, 512, 768], np.int64)

    def code(call, *args, **kw):
        with pytest.raises(jg.JanusGpuError) as e:
            call(*args, **kw)
        return e.value.code

    b = ctx.builder()  # keep_labels after a chunk
    b.add_vertices(v)
    assert code(b.keep_labels) == _lib.JG_ERR_STATE
    assert code(b.add_edges, v[:1], v[1:2], label=[1]) == _lib.JG_ERR_STATE  # a labelled add without keep_labels
    assert code(b.finish_labels, [1]) == _lib.JG_ERR_STATE                   # finish_labels without keep_labels
    b.close()
    b = ctx.builder()  # keep_labels after a positive query limit, and the reverse order
    b.set_query_limit(100, jg.DIR_IN)
    assert code(b.keep_labels) == _lib.JG_ERR_STATE
    b.close()
    b = ctx.builder()
    b.set_query_limit(0, jg.DIR_IN)  # no limit: not exclusive
    b.keep_labels()
    assert code(b.set_query_limit, 100, jg.DIR_IN) == _lib.JG_ERR_STATE
    b.close()
    b = ctx.builder()
    b.keep_labels()
    b.add_vertices(v)
    assert code(b.add_edges, v[:1], v[1:2]) == _lib.JG_ERR_ARG  # plain add_edges after keep_labels
    b.add_edges(v[:2], v[1:], label=[4, 5])
    assert code(b.finish_labels, []) == _lib.JG_ERR_ARG         # nlabels = 0
    assert code(b.finish_labels, np.arange(_lib.MAX_SCOPE_LABELS + 1)) == _lib.JG_ERR_ARG  # more labels than the cap
    big = np.concatenate([np.arange(_lib.MAX_SCOPE_LABELS), np.arange(_lib.MAX_SCOPE_LABELS)])  # distinct: at the cap
    g = b.finish_labels(big)
    assert g.info()["num_edges"] == 2
    g.close()
    assert code(b.add_vertices, v) == _lib.JG_ERR_STATE         # add_* after the first finish_labels
    assert code(b.add_edges, v[:1], v[1:2], label=[4]) == _lib.JG_ERR_STATE
    assert code(b.add_edges, v[:1], v[1:2]) == _lib.JG_ERR_STATE
    assert code(b.add_rows, np.zeros(0, np.uint64), [0], b"", [0], []) == _lib.JG_ERR_STATE
    assert code(b.keep_labels) == _lib.JG_ERR_STATE
    g = b.finish_labels([5])
    assert g.info()["num_edges"] == 1
    g.close()
    g = b.finish(jg.ADJ_IN)
    assert g.info()["num_edges"] == 2
    g.close()
    assert code(b.finish_labels, [4]) == _lib.JG_ERR_STATE      # finish_labels after finish
    b.close()
    b = ctx.builder()  # an empty label-keeping builder still gives a valid empty graph
    b.keep_labels()
    g = b.finish_labels([1])
    assert g.info()["num_vertices"] == 0 and g.info()["num_edges"] == 0
    assert ctx.stats()["kernel_launches"] == 0
    g.close()
    b.close()
    ctx.close()


# ---- 6. lifetime ----
def test_scoped_graphs_survive_their_builder(oracle_lib):
    import janusgraph_amd as jg
    vid, src, dst, w, lab = labeled_ids(n=100, m=900, seed=4)
    ctx = jg.Context((0,))
    b = ctx.builder()
    b.keep_labels()
    b.add_vertices(vid)
    b.add_edges(src, dst, w, label=lab)
    scopes = ([int(LABELS[0])], [int(LABELS[2]), int(LABELS[3])])
    graphs = [b.finish_labels(s) for s in scopes]
    b.close()
    for g, s in zip(graphs, scopes):
        mask = np.isin(lab, s)
        ds, dd, _ = dense(vid, src[mask], dst[mask])
        comp, _ = g.connected_components()
        np.testing.assert_array_equal(comp, oracle_lib.connected_components(len(vid), ds, dd, vid)[0])
        want, _ = oracle_lib.pagerank(len(vid), ds, dd, 0.85, len(vid), 10)
        assert np.max(np.abs(g.pagerank(0.85, len(vid), 10)[0] - want) / np.abs(want)) <= 1e-9
        g.close()
    ctx.close()


# ---- 7. computer level, GraphOfTheGods ----
def mirror_degrees(graph, labels, length):
    vid, src, dst, _ = graph.snapshot()
    keep = [e.label in labels for e in graph.edges]
    edges = [(int(a), int(b)) for a, b, k in zip(src, dst, keep) if k]
    props, it = pm.Engine(pm.MiniGraph(vid.tolist(), edges)).run(pm.DegreeCounterProgram(length, key="d"))
    return {v: props[v]["d"] for v in vid.tolist()}, it


@pytest.mark.parametrize("labels,length", [(("battled",), 1), (("brother",), 2), (("nosuch",), 1),
                                           (("battled", "pet"), 1)])
def test_computer_typed_scope_on_graph_of_the_gods(labels, length):
    import janusgraph_amd as jg
    graph = jg.InMemoryGraph()
    v = jg.load_graph_of_the_gods(graph)
    prog = jg.CombinerVertexProgram(length, "d", "sum", "inE", 1, True, labels=labels)
    result = jg.GpuGraphComputer(graph).resultMode(jg.ResultMode.LOCALTX).program(prog).submit().result()
    assert result.memory().getIteration() == length
    got = {x.id: result.graph().value(x.id, "d") for x in v.values()}
    want, it = mirror_degrees(graph, labels, length)
    assert it == length and got == want
    if labels == ("battled",):
        assert got == {x.id: (3 if name == "hercules" else 0) for name, x in v.items()}
    if labels == ("nosuch",):
        assert set(got.values()) == {0}
