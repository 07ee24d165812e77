"""The edgestore decoder (jg_decode.hip) edge for edge, at its staging and row limits.

Every snapshot case builds a store that reaches one data-dependent path of the decoder (asserted first,
with the predicates of tests/test_edgestore_paths_host.py, which also pins these stores and the oracle on
the CPU) and then reads the whole adjacency back through jg_graph_neighbors: assert_snapshot_exact
compares V in order, the counts and every vertex's OUT, IN and BOTH lists as sorted multisets with the
oracle's restatement (oracle.edgestore_snapshot).  An edge attributed to the neighbouring row, a row kept
or dropped wrongly, an entry decoded from the wrong bytes all change some list.  Integer work throughout:
every comparison is exact.
"""
import numpy as np
import pytest

import test_edgestore_paths_host as host
from test_edgestore import _dense, make_edgestore
from test_gpu_builder import row_chunks
from test_gpu_slice_cap import capped_reference, gpu_graph

pytestmark = pytest.mark.gpu

_REF = {}


def oracle_snapshot(oracle_lib, store, partition_bits):
    """The oracle's (V, dense src, dense dst, ghost edges) of a store, computed once per store."""
    key = (id(store[2]), partition_bits)
    if key not in _REF:
        keys, roff, data, off, vpos, tids, tmult = store
        ov, os_, od = oracle_lib.edgestore_snapshot(keys, roff, data, off, vpos, tids, tmult,
                                                    partition_bits=partition_bits)
        ds, dd = _dense(ov, os_, od)  # drops the edges with an endpoint outside V
        _REF[key] = (store, ov, ds.astype(np.int64), dd.astype(np.int64), len(os_) - len(ds))
    return _REF[key][1:]


def assert_adjacency(g, direction, rows, cols, err=""):
    """g's `direction` lists of every vertex == the (row, neighbour) pairs, as sorted multisets."""
    n = g.n
    off, nbr = g.neighbors(np.arange(n, dtype=np.int64), direction)
    assert len(nbr) == len(rows), f"{err}: {len(nbr)} entries, want {len(rows)}"
    got_rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    g_order, w_order = np.lexsort((nbr, got_rows)), np.lexsort((cols, rows))
    np.testing.assert_array_equal(got_rows[g_order], rows[w_order], err_msg=f"{err}: rows")
    np.testing.assert_array_equal(nbr[g_order], cols[w_order], err_msg=f"{err}: neighbours")


def assert_snapshot_exact(g, store, oracle_lib, partition_bits=5):
    import janusgraph_amd as jg
    ov, ds, dd, ghost_edges = oracle_snapshot(oracle_lib, store, partition_bits)
    np.testing.assert_array_equal(g.vertex_ids(), ov)
    info = g.info()
    assert info["num_vertices"] == len(ov)
    assert info["num_edges"] == len(ds)
    assert info["ghost_edges"] == ghost_edges
    assert_adjacency(g, jg.DIR_OUT, ds, dd, "OUT")
    assert_adjacency(g, jg.DIR_IN, dd, ds, "IN")
    assert_adjacency(g, jg.DIR_BOTH, np.concatenate([ds, dd]), np.concatenate([dd, ds]), "BOTH")  # a self-loop twice


def build_chunks(ctx, store, chunks, partition_bits=5):
    import janusgraph_amd as jg
    b = ctx.builder()
    try:
        b.set_schema(store[5], store[6], partition_bits)
        for ch in chunks:
            b.add_rows(*ch)
        return b.finish(jg.ADJ_IN | jg.ADJ_OUT | jg.ADJ_BOTH)
    finally:
        b.close()


def thirds(store):
    return np.linspace(0, len(store[0]), 4).astype(int)


def check_every_build(oracle_lib, store, partition_bits=5):
    """jg_graph_build_edgestore, and the builder in 1 and 3 chunks of whole rows: each equals the oracle."""
    import janusgraph_amd as jg
    ctx = jg.Context((0,))
    try:
        g, _ = ctx.build_edgestore(*store, partition_bits=partition_bits)
        assert_snapshot_exact(g, store, oracle_lib, partition_bits)
        g.close()
        for bounds in ([0, len(store[0])], thirds(store)):
            g = build_chunks(ctx, store, row_chunks(store, bounds), partition_bits)
            assert_snapshot_exact(g, store, oracle_lib, partition_bits)
            g.close()
    finally:
        ctx.close()


def check_refused(store, partition_bits=5):
    import janusgraph_amd as jg
    ctx = jg.Context((0,))
    try:
        with pytest.raises(jg.JanusGpuError):
            ctx.build_edgestore(*store, partition_bits=partition_bits)
        with pytest.raises(jg.JanusGpuError):
            build_chunks(ctx, store, row_chunks(store, [0, len(store[0])]), partition_bits)
    finally:
        ctx.close()


# ---------------------------------------------------------------- A: the row window

def test_row_window_and_search(oracle_lib):
    """Block iterations 0 and 1 span 1025 rows (binary search on global memory), iteration 2 exactly 1024
    (a full window), the last one 1028 rows with r1 = nrows.  The ghosts' OUT entries and the vertex-cut
    representative's lie in the search iterations: a wrong keep flag or row id there changes the lists."""
    store = host.store_row_window().build()
    host.check_row_window_paths(store)
    per_chunk = [host.snapshot_paths(ch[1], ch[3]) for ch in row_chunks(store, thirds(store))]
    assert any(p[1] == "search" for paths in per_chunk for p in paths)  # in three chunks too
    check_every_build(oracle_lib, store)


# ---------------------------------------------------------------- B: rows against block iterations

def test_row_and_iteration_alignment(oracle_lib):
    """A hub row over four block iterations, rows starting and ending exactly on iteration boundaries,
    empty rows first, on a boundary and last."""
    st, hub = host.store_alignment()
    store = st.build()
    host.check_alignment_paths(st, hub, store)
    check_every_build(oracle_lib, store)


@pytest.mark.parametrize("nentries", [0, 1, host.CHUNK - 1, host.CHUNK, host.CHUNK + 1])
def test_entry_counts_around_one_iteration(oracle_lib, nentries):
    """E = 1, 1023, 1024, 1025; and three empty rows with no entry at all."""
    store = host.store_tiny(nentries, 3).build()
    assert len(store[4]) == nentries and len(store[0]) > 0
    check_every_build(oracle_lib, store)


# ---------------------------------------------------------------- C: the stage limit

def test_stage_limit(oracle_lib):
    """Iterations of exactly 4096 words (staged) and 4097 (global memory), starts at off % 4 = 0, 1, 2, 3,
    staged and global iterations side by side in one build.  The last iteration's dword loads run into
    the byte array's padding: run under JG_DEV_POISON=ff and 2a as well (README)."""
    store = host.store_stage_limit().build()
    host.check_stage_paths(store)
    check_every_build(oracle_lib, store)


# ---------------------------------------------------------------- D: narrow and wide

@pytest.mark.parametrize("longest", [host.WIDE_LEN - 1, host.WIDE_LEN])
@pytest.mark.parametrize("nentries", [2047, 2048, 2049])
def test_narrow_and_wide_staging(oracle_lib, nentries, longest):
    """A longest entry of 255 bytes stages narrow (one value position is 255), of 256 wide; 2047 to 2049
    entries around the tile of the length scan; and the same chunk with entry_off[0] = 5."""
    import janusgraph_amd as jg
    store = host.store_width(nentries, longest).build()
    host.check_width(store, nentries, longest)
    check_every_build(oracle_lib, store)
    whole = row_chunks(store, [0, len(store[0])])[0]
    based = host.with_entry_base(whole)
    assert based[3][0] == 5 and host.chunk_width(based[3]) == host.chunk_width(store[3])
    ctx = jg.Context((0,))
    try:
        g = build_chunks(ctx, store, [based])
        assert_snapshot_exact(g, store, oracle_lib)
        g.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- E: slot reuse

def test_chunk_slots_are_reused(oracle_lib):
    """One builder, chunks large narrow, small wide, empty, tiny narrow, large wide: chunks 0, 2 and 4
    share a slot whose device buffers only grow.  Equal to the one-chunk build and the oracle."""
    import janusgraph_amd as jg
    st, bounds = host.store_slot_reuse()
    store = st.build()
    chunks = host.check_slot_reuse(store, bounds)
    ctx = jg.Context((0,))
    try:
        g = build_chunks(ctx, store, chunks)
        assert_snapshot_exact(g, store, oracle_lib)
        g1 = build_chunks(ctx, store, row_chunks(store, [0, len(store[0])]))
        assert_snapshot_exact(g1, store, oracle_lib)
        for direction in (jg.DIR_OUT, jg.DIR_IN, jg.DIR_BOTH):
            np.testing.assert_array_equal(g.degrees(direction), g1.degrees(direction))
        g.close()
        g1.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- F: under the cap

def check_capped(oracle_lib, store, limit, nchunks, min_truncated):
    """truncated_vertices, PageRank's edgeCount (the capped OUT degrees) and the IN lists read back
    through neighbors(DIR_IN) (the IN adjacency is built from the capped IN entries), all exact."""
    import janusgraph_amd as jg
    ov, out_list, in_list, trunc = capped_reference(oracle_lib, store, limit)
    assert trunc >= min_truncated
    ctx, g = gpu_graph(store, limit, jg.ADJ_IN, jg.DIR_IN, nchunks=nchunks)
    try:
        np.testing.assert_array_equal(g.vertex_ids(), ov)
        assert g.info()["truncated_vertices"] == trunc
        _, edge_count = g.pagerank(0.85, 1, 2)
        np.testing.assert_array_equal(edge_count, np.bincount(out_list[0], minlength=len(ov)).astype(np.float64))
        assert_adjacency(g, jg.DIR_IN, in_list[1].astype(np.int64), in_list[0].astype(np.int64), f"IN, limit {limit}")
    finally:
        g.close()
        ctx.close()
    return out_list, in_list


@pytest.mark.parametrize("limit", [1, 3])
def test_row_window_under_the_cap(oracle_lib, limit):
    """The store of the row-window case: at limit 1 every one-entry ghost-free row with an edge reaches
    the limit (the representative in a search iteration among them)."""
    store = host.store_row_window().build()
    host.check_row_window_paths(store)
    for nchunks in (1, 3):
        check_capped(oracle_lib, store, limit, nchunks, 2)


def test_hub_under_the_cap(oracle_lib):
    """The hub's slice is cut in its second block iteration; a row holding exactly `limit` slice entries
    counts as truncated with nothing cut, one with limit + 1 loses its last."""
    limit = 300
    st, hub = host.store_alignment(limit)
    store = st.build()
    host.check_alignment_paths(st, hub, store)
    first = 3 * host.CHUNK - host.HUB_START - 1  # slice entries of the hub in its first iteration
    assert first < limit < first + host.CHUNK
    for nchunks in (1, 3):
        out_list, in_list = check_capped(oracle_lib, store, limit, nchunks, 3)
    ov = oracle_snapshot(oracle_lib, store, 5)[0]
    index = {int(v): i for i, v in enumerate(ov)}
    exact, over = index[st.vid(40)], index[st.vid(41)]
    assert np.sum(out_list[0] == exact) == limit                                       # nothing cut
    assert np.sum(out_list[0] == over) + np.sum(in_list[1] == over) == limit           # one of limit + 1 cut
    assert np.sum(out_list[0] == index[hub]) == limit and np.sum(in_list[1] == index[hub]) == 0


# ---------------------------------------------------------------- G: partition bits

@pytest.mark.parametrize("pbits,cut", [(1, True), (16, True), (0, False)])
def test_partition_bits(oracle_lib, pbits, cut):
    store = host.store_partition_bits(pbits, cut).build()
    check_every_build(oracle_lib, store, pbits)


def test_no_partition_bits_refuse_a_cut_vertex():
    st = host.store_partition_bits(0, False)
    st.vertex(st.vid(77, 0, 2))
    check_refused(st.build(), 0)


# ---------------------------------------------------------------- H: refusals on these paths

def test_malformed_entry_in_a_search_iteration():
    """On a kept row (the vertex-cut representative) it is refused; on a ghost row and on a schema row it
    is never decoded."""
    st = host.store_row_window("rep")
    store = st.build()
    paths = host.check_row_window_paths(store)
    assert paths[st.tagged()["bad"] // host.CHUNK][1] == "search"
    check_refused(store)


def test_malformed_entry_on_ignored_rows_of_a_search_iteration(oracle_lib):
    """The ghost row's malformed entry is its second: its first is what the ghost rule decodes (a malformed
    first entry is refused on any vertex row, as VertexJobConverter.isGhostVertex parses it)."""
    st = host.store_row_window("ghost+schema")
    store = st.build()
    paths = host.check_row_window_paths(store)
    assert paths[st.tagged()["bad"] // host.CHUNK][1] == "search" and paths[0][1] == "search"  # the schema row: entry 1
    check_every_build(oracle_lib, store)


def test_malformed_entry_in_a_global_iteration(oracle_lib):
    """Refused on a live row; never decoded on a ghost row (behind its first entry) and on a schema row,
    both inside the iteration that reads global memory."""
    st = host.store_stage_limit("live")
    store = st.build()
    paths = host.check_stage_paths(store)
    assert paths[st.tagged()["bad"] // host.CHUNK][0] == "global"
    check_refused(store)
    st = host.store_stage_limit("ghost+schema")
    store = st.build()
    paths = host.check_stage_paths(store)
    tags = st.tagged()
    assert paths[tags["bad"] // host.CHUNK][0] == "global" and paths[tags["bad in schema"] // host.CHUNK][0] == "global"
    assert store[0][np.searchsorted(store[1], tags["bad in schema"], side="right") - 1] == host.STAGE_SCHEMA_KEY
    check_every_build(oracle_lib, store)


# ---------------------------------------------------------------- the one-shot chunker

@pytest.mark.parametrize("max_entries,max_bytes", host.CHUNKER_LIMITS)
def test_one_shot_chunker_rebases(oracle_lib, max_entries, max_bytes):
    """jg_graph_build_edgestore under lowered chunk limits (jg_tune_set edgestore_chunk_entries /
    edgestore_chunk_bytes): many chunks with nonzero entry and byte bases, the hub row a chunk of its own
    above the limit.  Equal to the default build and the oracle."""
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    store = host.store_stage_limit(hub=True).build()
    host.check_stage_paths(store)
    host.check_chunker(store, max_entries, max_bytes)
    ctx = jg.Context((0,))
    try:
        g0, vid0 = ctx.build_edgestore(*store)
        assert_snapshot_exact(g0, store, oracle_lib)
        _lib.tune_set("edgestore_chunk_entries", max_entries)
        _lib.tune_set("edgestore_chunk_bytes", max_bytes)
        g, vid = ctx.build_edgestore(*store)
        np.testing.assert_array_equal(vid, vid0)
        assert_snapshot_exact(g, store, oracle_lib)
        for direction in (jg.DIR_OUT, jg.DIR_IN, jg.DIR_BOTH):
            np.testing.assert_array_equal(g.degrees(direction), g0.degrees(direction))
        g.close()
        g0.close()
    finally:
        _lib.tune_set("edgestore_chunk_entries", host.CHUNKER_DEFAULTS[0])
        _lib.tune_set("edgestore_chunk_bytes", host.CHUNKER_DEFAULTS[1])
        ctx.close()


def test_chunker_knobs_have_a_minimum_of_one(oracle_lib):
    """At 1 entry / 1 byte every row is a chunk of its own: equal to the oracle and to the default build."""
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    store, _, _ = make_edgestore(n=40, m=150, seed=3)
    ctx = jg.Context((0,))
    try:
        for key in ("edgestore_chunk_entries", "edgestore_chunk_bytes"):
            with pytest.raises(jg.JanusGpuError):
                _lib.tune_set(key, 0)
            _lib.tune_set(key, 1)
        g, vid = ctx.build_edgestore(*store)
        assert_snapshot_exact(g, store, oracle_lib)
        _lib.tune_set("edgestore_chunk_entries", host.CHUNKER_DEFAULTS[0])
        _lib.tune_set("edgestore_chunk_bytes", host.CHUNKER_DEFAULTS[1])
        g0, vid0 = ctx.build_edgestore(*store)
        np.testing.assert_array_equal(vid, vid0)
        assert_snapshot_exact(g0, store, oracle_lib)
    finally:
        _lib.tune_set("edgestore_chunk_entries", host.CHUNKER_DEFAULTS[0])
        _lib.tune_set("edgestore_chunk_bytes", host.CHUNKER_DEFAULTS[1])
        ctx.close()  # closes its graphs first


# ---------------------------------------------------------------- jg_decode_edges

def gpu_decode(batch):
    import janusgraph_amd as jg
    data, off, vpos, want = batch
    ctx = jg.Context((0,))
    try:
        return np.stack([np.asarray(x, np.int64) for x in ctx.decode_edges(data, off, vpos, host.TIDS, host.TMULT)],
                        axis=1)
    finally:
        ctx.close()


def test_decode_edges_mixed_stage_paths(oracle_lib):
    """Blocks above 16 KB (global memory) between blocks below it, every block start alignment, n no
    multiple of 256: equal to the tuples by construction and to the oracle."""
    batch = host.decode_mixed_batch()
    data, off, vpos, want = batch
    assert host.decode_paths(off) == host.DECODE_MIXED_PATHS and len(vpos) % host.DECODE_BLOCK
    assert {int(off[b]) % 4 for b in range(0, len(vpos), host.DECODE_BLOCK)} == {0, 1, 2, 3}
    got = gpu_decode(batch)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, np.stack(oracle_lib.decode_edges(data, off, vpos, host.TIDS, host.TMULT), axis=1))


def test_decode_edges_known_answers_at_the_varint_edges(oracle_lib):
    batch = host.decode_kat_batch()
    data, off, vpos, want = batch
    assert {0, 1, 127, 128, 1 << 56, 1 << 62, (1 << 63) - 1} <= set(host.varint_edge_values())
    got = gpu_decode(batch)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, np.stack(oracle_lib.decode_edges(data, off, vpos, host.TIDS, host.TMULT), axis=1))


def test_decode_edges_malformed_entries_stay_inside_their_bytes():
    """A varint that runs off its entry is reported (dir = other = rel = -1), never completed from the
    neighbouring entry's bytes, in staged and global blocks alike.  The type of a malformed entry is not
    compared (the oracle does not define it).  The array's end: test_decode_edges_malformed_last_entry."""
    batch = host.decode_malformed_batch()
    data, off, vpos, want = batch
    assert host.decode_paths(off) == host.DECODE_MALFORMED_PATHS
    got = gpu_decode(batch)
    np.testing.assert_array_equal(got[:, 1:], want[:, 1:])
    ok = want[:, 1] >= 0
    np.testing.assert_array_equal(got[ok, 0], want[ok, 0])


@pytest.mark.parametrize("kind,path", host.MALFORMED_LAST)
def test_decode_edges_malformed_last_entry(kind, path):
    """Each malformed entry as the very last of the array, its block staged and read from global memory:
    behind a varint without a stop byte lies only the device array's padding (JG_DEV_POISON=ff makes every
    byte of it a stop byte)."""
    batch = host.decode_malformed_last_batch(kind, path)
    data, off, vpos, want = batch
    assert host.decode_paths(off) == ["staged", path] and want[-1, 1] == host.MALFORMED and len(data) == off[-1]
    got = gpu_decode(batch)
    np.testing.assert_array_equal(got[:, 1:], want[:, 1:])
    np.testing.assert_array_equal(got[:-1, 0], want[:-1, 0])
