"""The CSR build (csrc/jg_build.hip: id table, stable select, prim::radix_sort, csr_from_sorted_kernel), every row of
every built adjacency read back through jg_graph_neighbors / jg_graph_neighbor_edges and checked entry for entry
against the caller's edge list, at the sizes where the build's tiles change.

check_rows is the whole check, numpy only (tests/test_build_edges_host.py proves it can fail).  With ordinals
(JG_ADJ_EDGE_INDEX): off is monotone and ends at the kept edges (twice that for BOTH); every entry (owner,
neighbour, ordinal) is the caller's edge `ordinal` seen from `owner`; the multiset of ordinals is exactly the
non-ghost edges (twice each on BOTH, a self-loop's two entries in its one row, any other edge's in its two end
rows); the entries of one (owner, neighbour) pair are contiguous (the sort is by column); inside such a run the
ordinals ascend (the select emits in edge order and the sort is stable), a BOTH self-loop's two equal ordinals
adjacent.  Without ordinals (no flag, or several logical shards, where the flag is refused) the sorted (owner,
neighbour) pairs of all rows equal numpy's, as whole arrays, and the runs are contiguous all the same.

Sizes: kSelTile = 2048 edges per select block, kRadixTile = 4096 keys per sort block, the sort's copy-back after an
odd number of 8-bit passes, the relabel sort over n keys, the 1024-slot id table wrapping at its mask, and the
two-level scan of 2049 select block counts.  Vertex ids are sparse and shuffled: caller order, numeric order and
degree order all differ.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ADJ_OUT, ADJ_IN, ADJ_BOTH, ADJ_EDGE_INDEX = 1, 2, 4, 16
DIR_OUT, DIR_IN, DIR_BOTH = 1, 2, 3
ALL = ADJ_IN | ADJ_OUT | ADJ_BOTH
DIRECTIONS = ((ADJ_OUT, DIR_OUT), (ADJ_IN, DIR_IN), (ADJ_BOTH, DIR_BOTH))


# ---------------- the checker (numpy only) ----------------

def expected_pairs(n, si, di, direction):
    """Sorted owner * n + neighbour of every entry the direction's adjacency holds; si / di < 0: a ghost endpoint."""
    si, di = np.asarray(si, np.int64), np.asarray(di, np.int64)
    real = (si >= 0) & (di >= 0)
    s, d = si[real], di[real]
    rows = np.concatenate([s] * (direction != DIR_IN) + [d] * (direction != DIR_OUT))
    cols = np.concatenate([d] * (direction != DIR_IN) + [s] * (direction != DIR_OUT))
    return np.sort(rows * n + cols)


def numpy_rows(n, si, di, direction):
    """A correct read-back made on the host: (off, nbr, edge) with every row ordered by neighbour, then ordinal."""
    si, di = np.asarray(si, np.int64), np.asarray(di, np.int64)
    real = np.flatnonzero((si >= 0) & (di >= 0))
    owner = np.concatenate([si[real]] * (direction != DIR_IN) + [di[real]] * (direction != DIR_OUT))
    nbr = np.concatenate([di[real]] * (direction != DIR_IN) + [si[real]] * (direction != DIR_OUT))
    edge = np.tile(real, 2 if direction == DIR_BOTH else 1)
    order = np.lexsort((edge, nbr, owner))
    off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(np.int64)
    return off, nbr[order], edge[order].astype(np.uint32)


def check_rows(n, si, di, direction, off, nbr, edge=None):
    """All n rows of one adjacency against the caller's edges (vertex indices, < 0 a ghost endpoint); edge: the
    entries' ordinals, or None for a graph without them.  Raises AssertionError."""
    si, di = np.asarray(si, np.int64), np.asarray(di, np.int64)
    off, nbr = np.asarray(off, np.int64), np.asarray(nbr, np.int64)
    real = np.flatnonzero((si >= 0) & (di >= 0))
    both = direction == DIR_BOTH
    assert len(off) == n + 1 and off[0] == 0 and (np.diff(off) >= 0).all(), "off is not monotone from 0"
    assert off[-1] == len(real) * (2 if both else 1) == len(nbr), f"{off[-1]} / {len(nbr)} entries for {len(real)} kept edges"
    assert ((nbr >= 0) & (nbr < n)).all(), "a neighbour outside [0, n)"
    owner = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    key = owner * n + nbr
    np.testing.assert_array_equal(np.sort(key), expected_pairs(n, si, di, direction), err_msg="(owner, neighbour) pairs")
    first = np.ones(len(key), bool)  # the first entry of a run of equal (owner, neighbour)
    first[1:] = key[1:] != key[:-1]
    assert first.sum() == len(np.unique(key)), "the entries of one (owner, neighbour) pair are not contiguous"
    if edge is None:
        return
    e = np.asarray(edge).astype(np.int64)
    assert len(e) == len(nbr) and ((e >= 0) & (e < len(si))).all(), "an ordinal outside the caller's edge list"
    out_entry = (si[e] == owner) & (di[e] == nbr)  # the row's vertex is the edge's source
    in_entry = (di[e] == owner) & (si[e] == nbr)
    ok = {DIR_OUT: out_entry, DIR_IN: in_entry, DIR_BOTH: out_entry | in_entry}[direction]
    assert ok.all(), f"entry {np.flatnonzero(~ok)[:5]} is not its ordinal's edge seen from its owner"
    np.testing.assert_array_equal(np.sort(e), np.sort(np.tile(real, 2 if both else 1)), err_msg="multiset of ordinals")
    if both:  # an edge's two entries sit in its two end rows (a self-loop's: both in its one row)
        o = np.lexsort((owner, e))
        ends, es = owner[o].reshape(-1, 2), e[o][::2]
        assert (ends[:, 0] == np.minimum(si[es], di[es])).all() and (ends[:, 1] == np.maximum(si[es], di[es])).all(), \
            "an edge has both its entries in one end's row"
    same_run = ~first[1:]
    loop = both & (owner == nbr)
    strict = same_run & ~loop[1:]
    assert (e[1:][strict] > e[:-1][strict]).all(), "ordinals inside a run do not ascend"
    if both:  # a self-loop's run: adjacent pairs of equal ordinals, the pairs ascending
        le, lown = e[loop], owner[loop]
        a, b, own = le[0::2], le[1::2], lown[0::2]
        assert len(le) % 2 == 0 and (a == b).all(), "a self-loop's two entries are not adjacent"
        same = own[1:] == own[:-1]
        assert (a[1:][same] > a[:-1][same]).all(), "self-loop ordinals do not ascend"


# ---------------- graphs ----------------

class EdgeList:
    """Vertex ids (sparse, shuffled, some negative) and edges as vertex indices, -1 for a ghost endpoint."""

    def __init__(self, n, si, di, seed=0):
        rng = np.random.default_rng(1000 + seed)
        self.n = n
        self.vid = (rng.permutation(8 * n + 8)[:n].astype(np.int64) - 3 * n) * 977 + 5
        self.ghost = int(self.vid.max()) + 4242 if n else 4242
        self.si, self.di = np.asarray(si, np.int64), np.asarray(di, np.int64)
        self.m = len(self.si)
        self.real = np.flatnonzero((self.si >= 0) & (self.di >= 0))

    def ids(self, idx):
        return np.where(idx >= 0, self.vid[np.maximum(idx, 0)], self.ghost) if self.n else np.full(len(idx), self.ghost)

    def build(self, ctx, flags, weight=None):
        return ctx.build(self.vid, self.ids(self.si), self.ids(self.di), weight=weight, flags=flags)


def tile_graph(n, m, seed=0):
    """m random edges over n vertices seeded for the select and radix tiles: self-loops (one vertex twice), a run of
    one pair whose ordinals lie on both sides of positions 2047 / 2048 (one select block's tail and the next one's
    head emit the same key) and of 4095 / 4096, once more early and reversed, and ghost endpoints at positions 0,
    2047, 2048 and m - 1, which the ordinals count."""
    rng = np.random.default_rng(seed * 100003 + m)
    si, di = rng.integers(0, n, m), rng.integers(0, n, m)

    def put(pos, a, b):
        if 0 <= pos < m:
            si[pos], di[pos] = a, b

    a, b, c = int(rng.integers(0, n)), int(rng.integers(0, n)), int(rng.integers(0, n))
    for pos in (3, 5, 2046 - 8, m - 3):
        put(pos, c, c)
    for pos in (10, 2045, 2046, 2049, 2050, 2051, 4094, 4095, 4096, 4097, m - 2):
        put(pos, a, b)
    put(11, b, a)
    put(0, -1, di[0] if m else 0)
    put(2047, si[2047] if m > 2047 else 0, -1)
    put(2048, -1, -1)
    put(m - 1, si[m - 1] if m else 0, -1)
    return EdgeList(n, si, di, seed)


def random_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    si, di = rng.integers(0, n, m), rng.integers(0, n, m)
    for pos in range(0, m, 37):  # self-loops and ghosts as they fall
        di[pos] = si[pos]
    for pos in range(5, m, 101):
        si[pos] = -1
    return EdgeList(n, si, di, seed)


def star_graph(n, m, seed=3):
    """hub -> every other vertex, round and round: one row owns every OUT entry across all tiles."""
    hub = n // 3
    others = np.delete(np.arange(n), hub)
    di = others[np.random.default_rng(seed).permutation(m) % (n - 1)]
    return EdgeList(n, np.full(m, hub), di, seed), hub


def bipartite_graph(n, m, seed=4):
    """Sources (every seventh vertex) have no in-edge and the targets no out-edge: empty rows before, between and
    after the non-empty ones in either directed CSR, whatever order the relabel gives the rows."""
    rng = np.random.default_rng(seed)
    sources = np.arange(0, n, 7)
    targets = np.setdiff1d(np.arange(n - 50), sources)[::3]  # the last 50 vertices: no in-edge either
    return EdgeList(n, rng.choice(sources, m), rng.choice(targets, m), seed)


def pair_graph(n, m, seed=5):
    """Every edge between the same two vertices: one (row, column) key m times."""
    return EdgeList(n, np.full(m, n - 2), np.full(m, 17), seed)


# ---------------- running a case ----------------

@pytest.fixture(scope="module")
def ctx():
    import janusgraph_amd as jg
    c = jg.Context((0,))
    yield c
    c.close()


def check_graph(g, el, flags):
    """info, vertex_ids and every built direction's rows."""
    info = g.info()
    assert (info["num_vertices"], info["num_edges"], info["ghost_edges"]) == (el.n, len(el.real), el.m - len(el.real))
    assert info["self_loops"] == int((el.si[el.real] == el.di[el.real]).sum())
    np.testing.assert_array_equal(g.vertex_ids(), el.vid)
    rows = np.arange(el.n, dtype=np.int64)
    for adj, direction in DIRECTIONS:
        if not flags & adj:
            continue
        off, nbr = g.neighbors(rows, direction)
        edge = None
        if flags & ADJ_EDGE_INDEX:
            eoff, edge = g.neighbor_edges(rows, direction)
            np.testing.assert_array_equal(off, eoff)
        check_rows(el.n, el.si, el.di, direction, off, nbr, edge)


def build_and_check(ctx, el, flags, weight=None):
    g = el.build(ctx, flags, weight)
    try:
        check_graph(g, el, flags)
    except BaseException:
        g.close()
        raise
    return g


# 1. edge count at the select tile and the radix tile (BOTH doubles the entries: its radix edge is at m = 2048)
@pytest.mark.parametrize("m", [0, 1, 2047, 2048, 2049, 4095, 4096, 4097, 8193])
def test_edge_count_at_the_tiles(ctx, m):
    el = tile_graph(300, m)  # 9 + 9 key bits: three passes, the copy-back runs
    build_and_check(ctx, el, ALL | ADJ_EDGE_INDEX).close()


# 2. vertex count: the relabel sort across its tile and its count-table edge; 16: one pass, 17: two
@pytest.mark.parametrize("n", [1, 2, 16, 17, 4095, 4096, 4097, 32769])
def test_vertex_count_at_the_tiles(ctx, n):
    el = random_graph(n, 3 * n, n)
    build_and_check(ctx, el, ALL | ADJ_EDGE_INDEX).close()


# 3. degree shapes
def test_star(ctx):
    el, hub = star_graph(5000, 4097 + 4096)
    g = build_and_check(ctx, el, ALL | ADJ_EDGE_INDEX)
    off, edge = g.neighbor_edges([hub], DIR_OUT)
    assert off[-1] == el.m  # the one row owns every entry
    g.close()


def test_bipartite_rows_with_gaps(ctx):
    el = bipartite_graph(5000, 4097 + 4096)
    g = build_and_check(ctx, el, ALL | ADJ_EDGE_INDEX)
    deg = g.degrees(DIR_IN)
    assert deg[0] == 0 and deg[-1] == 0 and (deg > 0).sum() > 100 and (deg == 0).sum() > 3000
    g.close()


def test_one_key_8193_times(ctx):
    el = pair_graph(5000, 4097 + 4096)
    g = build_and_check(ctx, el, ALL | ADJ_EDGE_INDEX)
    for direction, row in ((DIR_OUT, el.n - 2), (DIR_IN, 17)):
        _, edge = g.neighbor_edges([row], direction)
        np.testing.assert_array_equal(edge, np.arange(el.m))  # the ordinals come back 0..8192 in order
    g.close()


# 4. keys-only and weighted sorts
@pytest.mark.parametrize("m", [2049, 4097])
def test_keys_only(ctx, m):
    build_and_check(ctx, tile_graph(300, m), ALL).close()  # no payload in the downsweep


def check_weights_by_distance(oracle_lib, g, el, w, seeds):
    """weight[e] = e + 1 is unique, so a weight that travelled with the wrong entry changes some minimum."""
    s, d, wr = el.si[el.real], el.di[el.real], w[el.real]
    for seed in seeds:
        np.testing.assert_array_equal(g.shortest_distance(el.vid[seed], 1), oracle_lib.shortest_distance(el.n, s, d, int(seed), 1, wr),
                                      err_msg=f"seed {seed}")


@pytest.mark.parametrize("m", [2049, 4097])
def test_weighted(ctx, oracle_lib, m):
    el = tile_graph(300, m)
    w = (np.arange(el.m) + 1).astype(np.int32)
    g = build_and_check(ctx, el, ALL, weight=w)  # the payload carries the weights; the ordinals are dropped
    busiest = int(np.bincount(el.si[el.real], minlength=el.n).argmax())
    check_weights_by_distance(oracle_lib, g, el, w, [busiest] + np.random.default_rng(m).integers(0, el.n, 4).tolist())
    g.close()


def test_weighted_star(ctx, oracle_lib):
    el, hub = star_graph(5000, 4097 + 4096)
    w = (np.arange(el.m) + 1).astype(np.int32)
    g = build_and_check(ctx, el, ALL, weight=w)
    check_weights_by_distance(oracle_lib, g, el, w, [hub] + np.random.default_rng(9).integers(0, el.n, 3).tolist())
    g.close()


# 5. logical shards: the halo layout's compact column ids map back to the same neighbours
@pytest.mark.parametrize("halo", [1, 0])
@pytest.mark.parametrize("shards", [2, 3])
def test_logical_shards(shards, halo):
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    n = 301  # not a multiple of the shard count
    graphs = [tile_graph(n, 2049), tile_graph(n, 4097), star_graph(n, 4097 + 4096)[0]]
    _lib.tune_set("halo", halo)
    c = jg.Context((0,) * shards)
    try:
        for el in graphs:
            g = build_and_check(c, el, ALL)
            assert g.info()["num_shards"] == shards
            g.close()
    finally:
        c.close()
        _lib.tune_set("halo", 1)


# 6. the id table: a probe chain that wraps past the mask, misses that walk all of it
def id_hash(x):
    """csrc/jg_build.hip id_hash: splitmix64's finaliser, on uint64 arrays (numpy wraps modulo 2^64)."""
    x = np.asarray(x).astype(np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def ids_in_slots(rng, count, lo, hi, mask=1023, taken=()):
    """`count` distinct random int64 ids whose table slot (id_hash & mask) lies in [lo, hi]."""
    found, seen = [], set(taken)
    while len(found) < count:
        cand = rng.integers(-(1 << 62), 1 << 62, 1 << 16)
        slot = (id_hash(cand) & np.uint64(mask)).astype(np.int64)
        for v in cand[(slot >= lo) & (slot <= hi)].tolist():
            if v not in seen and len(found) < count:
                seen.add(v)
                found.append(v)
    return np.asarray(found, np.int64)


def test_id_hash_known_answer():
    """splitmix64 from seed 0: the first output is the finaliser of the golden-ratio increment."""
    assert int(id_hash(np.asarray([0x9e3779b97f4a7c15], np.uint64))[0]) == 0xe220a8397b1dcdaf


def test_id_table_chain_wraps_at_the_mask(ctx):
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    rng = np.random.default_rng(6)
    chain = ids_in_slots(rng, 200, 1023, 1023)  # 200 ids for one slot: the chain runs 1023, 0, 1, ..., 198
    special = np.asarray([np.iinfo(np.int64).max, np.iinfo(np.int64).min + 1, -1, -2, -(1 << 40), 0], np.int64)
    vid = rng.permutation(np.concatenate([chain, special]))
    n = len(vid)
    assert n * 7 <= 1024 * 5  # still the 1024-slot table
    ghosts = np.concatenate([ids_in_slots(rng, 25, 1023, 1023, taken=vid.tolist()),
                             ids_in_slots(rng, 25, 0, 150, taken=vid.tolist())])  # each miss walks to the chain's end
    m = 1500
    si, di = rng.integers(0, n, m), rng.integers(0, n, m)
    src, dst = vid[si], vid[di]
    gpos = rng.choice(m, 50, replace=False)
    src[gpos[:25]], dst[gpos[25:]] = ghosts[:25], ghosts[25:]
    si[gpos[:25]], di[gpos[25:]] = -1, -1
    flags = ALL | ADJ_EDGE_INDEX
    g = ctx.build(vid, src, dst, flags=flags)
    el = EdgeList(n, si, di)
    el.vid = vid
    assert g.info()["ghost_edges"] == 50
    check_graph(g, el, flags)
    g.close()
    for bad in (np.concatenate([vid, [np.iinfo(np.int64).min]]), np.concatenate([vid, vid[:1]])):
        with pytest.raises(jg.JanusGpuError) as e:
            ctx.build(bad, src, dst, flags=flags)
        assert e.value.code == _lib.JG_ERR_ARG


# 7. select_keys scans 2049 block counts on two levels; the sort runs 1025 tiles
def test_two_level_block_count_scan(ctx):
    n, m = 1 << 16, 2048 * 2048 + 1
    rng = np.random.default_rng(7)
    si, di = rng.integers(0, n, m), rng.integers(0, n, m)
    si[::4099] = -1  # ghosts across the blocks
    di[5::4001] = si[5::4001]
    el = EdgeList(n, si, di, 7)
    build_and_check(ctx, el, ADJ_IN | ADJ_EDGE_INDEX).close()
