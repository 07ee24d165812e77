"""Every program against the CPU oracle with device allocations poisoned (JG_DEV_POISON, csrc/jg_common.h).

Nothing zeroes a block that DevBuf hands out, so correctness rests on every buffer being written before a
kernel reads it.  A test process normally cannot see a violation: fresh pages read as zero, and a recycled
block usually holds valid data of the same graph.  With JG_DEV_POISON=<hex byte> every block, fresh or
recycled, is filled with that byte first.  Two patterns, because each hides what the other shows:
  ff  doubles are NaN, int32/int64 are -1 (below every label, rank and depth: min-folds show it), bit words are
      all ones; but it equals the library's own "unreached" fill, so it cannot show a missing -1 fill;
  2a  int32 is 0x2A2A2A2A (~7e8: above every label and depth here, unlike the fills 0x00, 0x7F and 0xFF the
      library uses: a missing -1 / 0x7F fill and max-folds show it), bit words are partly set; as a double it
      is ~1e-103 and invisible, which is why ff is needed too.
Each test sets the variable, creates its own Context (the switch is read at context creation), builds, runs
one program and compares with the oracle (oracle/) or the host restatements of the path-DAG and census
tests; never with a second GPU run.  Integers exactly, PageRank per vertex within PR_RTOL.

The sequence tests run the programs one after another on one graph (scratch a graph keeps between programs is
poisoned only at its first allocation; the order revisits each program after others used the shared
buffers), then on a smaller and a larger graph in the same context, which hands each the other's blocks.
"""
import os

import numpy as np
import pytest

from test_cc_census_host import expected_census
from test_gpu_path_dag import host_dag
from test_gpu_vdev import PR_RTOL, rmat_graph

pytestmark = pytest.mark.gpu

PATTERNS = ("ff", "2a")
DEPTH_INF = 2**31 - 1
PLEN = 40  # the path hanging off the hub


@pytest.fixture(params=PATTERNS)
def poison(request, monkeypatch):
    monkeypatch.setenv("JG_DEV_POISON", request.param)
    return request.param


class Case:
    """The base graph: RMAT (shuffled sparse ids) + an isolated vertex, a two-vertex component and a PLEN-vertex
    path hanging off the hub.  Oracle results are computed once per argument set and handed out read-only."""

    def __init__(self, o, scale):
        self.o = o
        n0, vid0, s0, t0, _ = rmat_graph(o, scale)
        extra = 3 + PLEN
        self.n0, self.n = n0, n0 + extra
        self.vid = np.concatenate([vid0, (np.arange(extra, dtype=np.int64) + n0 + 1) << 8 | 7])
        self.hub = int(np.bincount(s0, minlength=n0).argmax())
        self.isolated, self.pair = n0, (n0 + 1, n0 + 2)
        p0 = n0 + 3
        self.path_end = self.n - 1
        ps = np.concatenate([[n0 + 1, self.hub], np.arange(p0, self.n - 1)])
        pd = np.concatenate([[n0 + 2, p0], np.arange(p0 + 1, self.n)])
        self.s = np.concatenate([s0, ps]).astype(np.int64)
        self.t = np.concatenate([t0, pd]).astype(np.int64)
        m = len(self.s)
        self.w = (np.arange(m) % 7 + 1).astype(np.int32)
        self.w_neg = np.random.default_rng(scale).integers(-2, 9, m).astype(np.int32)
        self.w_nonneg = np.random.default_rng(scale + 1).integers(0, 40, m).astype(np.int32)
        deg = np.bincount(self.s, minlength=self.n) + np.bincount(self.t, minlength=self.n)
        self.connected = np.flatnonzero(deg[:n0] > 0)
        self.memo = {}

    def _memo(self, key, fn):
        if key not in self.memo:
            r = fn()
            for a in (r if isinstance(r, tuple) else (r,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self.memo[key] = r
        return self.memo[key]

    def sources(self, k, seed=11):
        """k distinct sources: vertices of the giant part, then the isolated vertex, the pair and the path's end."""
        special = [self.isolated, self.pair[1], self.path_end, self.hub][:max(0, min(4, k - 1))]
        rest = [v for v in np.random.default_rng(seed).permutation(self.connected).tolist() if v not in special]
        return np.array(rest[:k - len(special)] + special, np.int64)

    def build(self, ctx, weight=None, flags=7):
        return ctx.build(self.vid, self.vid[self.s], self.vid[self.t], weight=weight, flags=flags)

    def bfs(self, src, direction=3, max_depth=-1):
        return self._memo(("bfs", int(src), direction, max_depth),
                          lambda: self.o.bfs(self.n, self.s, self.t, int(src), direction, max_depth))

    def pagerank(self, vertex_count, k):
        return self._memo(("pr", vertex_count, k), lambda: self.o.pagerank(self.n, self.s, self.t, 0.85, vertex_count, k))

    def cc(self):
        return self._memo("cc", lambda: self.o.connected_components(self.n, self.s, self.t, self.vid))

    def sd(self, seed, depth, weight=None):
        w = None if weight is None else getattr(self, weight)
        return self._memo(("sd", int(seed), depth, weight),
                          lambda: self.o.shortest_distance(self.n, self.s, self.t, int(seed), depth, w))

    def combine(self, direction, combiner, steps, wrap):
        return self._memo(("comb", direction, combiner, steps, wrap),
                          lambda: self.o.combine_steps(self.n, self.s, self.t, direction, combiner, steps, self.init(), wrap))

    def init(self):
        return self._memo("init", lambda: np.random.default_rng(17).integers(-(1 << 39), 1 << 39, self.n))

    def csr_both(self):
        return self._memo("csr", lambda: self.o.csr_unordered(self.n, self.s, self.t, both=True))


_cases = {}


def case_of(o, scale=12):
    if scale not in _cases:
        _cases[scale] = Case(o, scale)
    return _cases[scale]


@pytest.fixture
def base(oracle_lib):
    return case_of(oracle_lib)


class Session:
    """A context made after the switch is set, closed (with its graphs) at the end; tuning knobs set through
    it go back to their defaults."""
    DEFAULTS = {"cc_uf": 1, "cc_uf_sharded": 1, "sd_dist32": 1, "sd_delta": -1, "halo": 1}

    def __init__(self, shards=1, **knobs):
        self.shards, self.knobs = shards, knobs

    def __enter__(self):
        import janusgraph_amd as jg
        from janusgraph_amd import _lib
        for k, v in self.knobs.items():
            _lib.tune_set(k, v)
        self.ctx = jg.Context((0,) * self.shards)
        return self.ctx

    def __exit__(self, *exc):
        from janusgraph_amd import _lib
        try:
            self.ctx.close()
        finally:
            for k in self.knobs:
                _lib.tune_set(k, self.DEFAULTS[k])
        return False


def assert_pr(rank, want):
    rel = np.abs(rank - want) / np.maximum(np.abs(want), 1e-300)
    assert not np.isnan(rank).any() and rel.max() <= PR_RTOL, f"max rel err {np.nanmax(rel)}, NaN {np.isnan(rank).sum()}"


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


# ---- the switch itself ----
def test_switch_is_live(monkeypatch):
    """jg_tune_set("dev_poison_probe", bytes) reads a first and a recycled block back and fails unless every
    byte holds the pattern; with the switch off (unset, empty or unparsable) it refuses."""
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    for value, on in (("ff", True), ("2a", True), ("", False), ("zz", False), ("100", False), (None, False), ("0", True)):
        if value is None:
            monkeypatch.delenv("JG_DEV_POISON", raising=False)
        else:
            monkeypatch.setenv("JG_DEV_POISON", value)
        c = jg.Context((0,))
        try:
            for nbytes in (1, 4099, (1 << 20) + 3):
                if on:
                    _lib.tune_set("dev_poison_probe", nbytes)
                else:
                    with pytest.raises(jg.JanusGpuError) as e:
                        _lib.tune_set("dev_poison_probe", nbytes)
                    assert e.value.code == _lib.JG_ERR_STATE and "is off" in str(e.value)
        finally:
            c.close()


def test_patterns_give_the_same_ranks_bitwise(oracle_lib, monkeypatch):
    base = case_of(oracle_lib)
    ranks = {}
    for p in PATTERNS:
        monkeypatch.setenv("JG_DEV_POISON", p)
        with Session() as c:
            ranks[p], _ = base.build(c, flags=2).pagerank(0.85, base.n, 12)
    assert_pr(ranks["ff"], base.pagerank(base.n, 12)[0])
    np.testing.assert_array_equal(bits(ranks["ff"]), bits(ranks["2a"]))


# ---- builds ----
@pytest.mark.parametrize("weighted", [False, True])
def test_build_counts_and_ids(base, poison, weighted):
    with Session() as c:
        g = base.build(c, weight=base.w if weighted else None)
        info = g.info()
        assert (info["num_vertices"], info["num_edges"], info["ghost_edges"], info["num_shards"]) == (base.n, len(base.s), 0, 1)
        assert info["self_loops"] == int((base.s == base.t).sum())
        assert info["max_in_degree"] == np.bincount(base.t, minlength=base.n).max()
        assert info["max_out_degree"] == np.bincount(base.s, minlength=base.n).max()
        np.testing.assert_array_equal(g.vertex_ids(), base.vid)
        np.testing.assert_array_equal(g.vertex_ids(1000, 77), base.vid[1000:1077])


@pytest.mark.parametrize("direction", [1, 2, 3], ids=["OUT", "IN", "BOTH"])
def test_neighbors(base, poison, direction):
    n = base.n
    rows = np.concatenate([base.s] * (direction != 2) + [base.t] * (direction != 1))
    cols = np.concatenate([base.t] * (direction != 2) + [base.s] * (direction != 1))
    with Session() as c:
        g = base.build(c)
        off, nbr = g.neighbors(np.arange(n, dtype=np.int64), direction)
        np.testing.assert_array_equal(np.diff(off), np.bincount(rows, minlength=n))
        got = np.repeat(np.arange(n, dtype=np.int64), np.diff(off)) * n + nbr
        np.testing.assert_array_equal(np.sort(got), np.sort(rows * n + cols))
        some = np.array([base.hub, base.isolated, base.path_end, 5], np.int64)  # a few rows, not in order
        off, nbr = g.neighbors(some, direction)
        for j, r in enumerate(some):
            np.testing.assert_array_equal(np.sort(nbr[off[j]:off[j + 1]]), np.sort(cols[rows == r]))


def test_build_rmat_degrees(oracle_lib, poison):
    import janusgraph_amd as jg
    s, t = oracle_lib.rmat_edges(12, 16, 5)
    with Session() as c:
        g = c.build_rmat(12, 16, 5, flags=jg.ADJ_IN | jg.ADJ_OUT)
        assert g.info()["num_edges"] == len(s)
        np.testing.assert_array_equal(g.degrees(jg.DIR_IN), np.bincount(t, minlength=1 << 12))
        np.testing.assert_array_equal(g.degrees(jg.DIR_OUT), np.bincount(s, minlength=1 << 12))


def test_row_builder_with_weight_key(oracle_lib, poison):
    """set_schema, set_weight_key, add_rows in two chunks (test_gpu_weights.build): the weights decoded on the
    device, shortest distance against the oracle on the host-parsed weights."""
    from test_gpu_weights import build, weighted_store
    store, hw = weighted_store(n=300, m=2500, seed=5)
    keys, roff, data, off, vpos, tids, tmult = store
    ov, os_, ot, ent = oracle_lib.edgestore_snapshot(keys, roff, data, off, vpos, tids, tmult, return_entries=True)
    index = {int(v): i for i, v in enumerate(ov)}
    ds = np.array([index[int(a)] for a in os_], np.int32)
    dd = np.array([index[int(b)] for b in ot], np.int32)
    ctx, g = build(store)
    try:
        np.testing.assert_array_equal(g.vertex_ids(), ov)
        assert g.info()["num_edges"] == len(ds)
        for s in (0, 7, 99):
            np.testing.assert_array_equal(g.shortest_distance(int(ov[s]), 6),
                                          oracle_lib.shortest_distance(len(ov), ds, dd, s, 6, hw[ent].astype(np.int32)))
    finally:
        ctx.close()


def test_row_builder_under_a_query_limit(oracle_lib, poison):
    import janusgraph_amd as jg
    from test_edgestore import make_edgestore
    from test_gpu_slice_cap import capped_reference, gpu_graph, pagerank_ref
    limit = 8
    store, _, _ = make_edgestore(n=700, m=6000, seed=limit)
    ov, out_list, in_list, trunc = capped_reference(oracle_lib, store, limit)
    ctx, g = gpu_graph(store, limit, jg.ADJ_IN, jg.DIR_IN, nchunks=2)
    try:
        np.testing.assert_array_equal(g.vertex_ids(), ov)
        assert g.info()["truncated_vertices"] == trunc > 0
        rank, ec = g.pagerank(0.85, 1, 10)
        want, want_ec = pagerank_ref(oracle_lib, len(ov), out_list, in_list)
        np.testing.assert_array_equal(ec, want_ec)
        np.testing.assert_allclose(rank, want, rtol=PR_RTOL, atol=0)  # +inf where a sender's edgeCount is 0
    finally:
        ctx.close()


def test_row_builder_label_scopes(oracle_lib, poison):
    """keep_labels, add_rows in two chunks, two finish_labels scopes: each against the oracle's snapshot of the
    host-stripped store."""
    import janusgraph_amd as jg
    from test_gpu_label_scope import EDGE_LABELS, dense, labeled_store, row_chunks, strip_entries
    store = labeled_store()
    keys, roff, data, off, vpos, tids, tmult = store
    etype, _, _, _ = oracle_lib.decode_edges(data, off, vpos, tids, tmult)
    with Session() as c:
        b = c.builder()
        b.keep_labels()
        b.set_schema(tids, tmult, 5)
        for ch in row_chunks(store, 2):
            b.add_rows(*ch)
        for scope in ([EDGE_LABELS[0]], [EDGE_LABELS[3], EDGE_LABELS[1]]):
            others = [x for x in EDGE_LABELS if x not in scope]
            ov, os_, ot = oracle_lib.edgestore_snapshot(*strip_entries(store, ~np.isin(etype, others)))
            ds, dd, _ = dense(ov, os_, ot)
            n = len(ov)
            g = b.finish_labels(scope)
            np.testing.assert_array_equal(g.vertex_ids(), ov)
            assert g.info()["num_edges"] == len(ds)
            rank, ecount = g.pagerank(0.85, n, 10)
            want, want_e = oracle_lib.pagerank(n, ds, dd, 0.85, n, 10)
            assert_pr(rank, want)
            np.testing.assert_array_equal(ecount, want_e)
            comp, it = g.connected_components()
            want_c, want_it = oracle_lib.connected_components(n, ds, dd, ov)
            np.testing.assert_array_equal(comp, want_c)
            assert it == want_it
            np.testing.assert_array_equal(g.degrees(jg.DIR_OUT), np.bincount(ds, minlength=n))
            g.close()
        b.close()


# ---- PageRank ----
@pytest.mark.parametrize("k", [0, 1, 2, 12])
def test_pagerank(base, poison, k):
    vc = base.n + 5  # the user's vertexCount, not |V|
    want, want_e = base.pagerank(vc, k)
    with Session() as c:
        rank, ecount = base.build(c, flags=2).pagerank(0.85, vc, k)
    if k == 0:  # no property is written
        assert np.isnan(want).all() and np.isnan(rank).all()
        return
    assert_pr(rank, want)
    np.testing.assert_array_equal(ecount, want_e)


def test_pagerank_stepwise_equals_one_call(base, poison):
    want, want_e = base.pagerank(base.n, 12)  # K = 12: supersteps 0 and 1, then 11 power steps
    with Session() as c:
        g = base.build(c, flags=2)
        g.pagerank_begin(0.85, base.n)
        g.pagerank_step(3)
        g.pagerank_step(8)
        rank, ecount = g.pagerank_end()
        one, _ = g.pagerank(0.85, base.n, 12)
    assert_pr(rank, want)
    assert_pr(one, want)
    np.testing.assert_array_equal(ecount, want_e)
    np.testing.assert_array_equal(bits(rank), bits(one))


# ---- shortest distance ----
@pytest.mark.parametrize("depth", [0, 1, 4])
def test_shortest_distance_unit(base, poison, depth):
    with Session() as c:
        g = base.build(c, flags=3)
        for seed in (base.hub, int(base.t[0]), base.isolated):
            np.testing.assert_array_equal(g.shortest_distance(base.vid[seed], depth), base.sd(seed, depth))


def test_shortest_distance_negative_weights(base, poison):
    with Session() as c:
        g = base.build(c, weight=base.w_neg, flags=3)
        for seed in (base.hub, int(base.t[0])):
            np.testing.assert_array_equal(g.shortest_distance(base.vid[seed], 5), base.sd(seed, 5, "w_neg"))


@pytest.mark.parametrize("dist32", [0, 2])
def test_shortest_distance_delta_stepping(base, poison, dist32):
    """Unbounded, no negative weight: the delta-stepping path, with 64-bit and with forced 32-bit distances."""
    with Session(sd_dist32=dist32) as c:
        g = base.build(c, weight=base.w_nonneg, flags=3)
        for seed in (int(base.t[0]), base.path_end):
            got = g.shortest_distance(base.vid[seed], DEPTH_INF)
            np.testing.assert_array_equal(got, base.sd(seed, DEPTH_INF, "w_nonneg"))


# ---- BFS ----
def check_rows(case, got, srcs, direction=3, max_depth=-1):
    assert len(got) == len(srcs)
    for k, sv in enumerate(srcs):
        np.testing.assert_array_equal(got[k], case.bfs(sv, direction, max_depth), err_msg=f"source {k} ({sv})")


@pytest.mark.parametrize("direction", [3, 1, 2], ids=["BOTH", "OUT", "IN"])
def test_bfs_one_source(base, poison, direction):
    with Session() as c:
        g = base.build(c)
        for sv in (base.hub, base.path_end, base.isolated, int(base.s[7])):
            check_rows(base, g.bfs([base.vid[sv]], direction), [sv], direction)


@pytest.mark.parametrize("direction", [1, 2], ids=["OUT", "IN"])
def test_bfs_both_after_a_directed_one_from_an_isolated_vertex(base, poison, direction):
    """Found by reading the depth buffer's bookkeeping (Shard::bfs_depth_tail_clean): a BOTH traversal skips
    the init of the rows without an entry, which keep -1 between traversals.  A directed traversal from an
    isolated vertex left that vertex's 0 among them and still called them clean, so the next BOTH traversal
    handed depth 0 back for the isolated vertex."""
    with Session() as c:
        g = base.build(c)
        check_rows(base, g.bfs([base.vid[base.hub]], 3), [base.hub])  # the suffix is filled and clean
        check_rows(base, g.bfs([base.vid[base.isolated]], direction), [base.isolated], direction)
        check_rows(base, g.bfs([base.vid[base.hub]], 3), [base.hub])
        check_rows(base, g.bfs([base.vid[base.path_end]], 3, 2), [base.path_end], 3, 2)


@pytest.mark.parametrize("nsrc", [2, 8, 130])
def test_bfs_sources(base, poison, nsrc):
    """2 and 8 sources: the narrow engine; 130: three batches of the 64-source engine."""
    srcs = base.sources(nsrc)
    with Session() as c:
        g = base.build(c, flags=4)
        check_rows(base, g.bfs(base.vid[srcs], 3), srcs)


def test_bfs_64_sources_pull_after_top_down(oracle_lib, poison):
    """Scale 14: the frontier grows past the top-down threshold, so pull levels follow the top-down ones."""
    big = case_of(oracle_lib, 14)
    srcs = big.sources(64)
    with Session() as c:
        g = big.build(c, flags=4)
        check_rows(big, g.bfs(big.vid[srcs], 3), srcs)


@pytest.mark.parametrize("nsrc", [1, 8, 64])
def test_bfs_bounded(base, poison, nsrc):
    srcs = base.sources(nsrc, seed=3)
    with Session() as c:
        g = base.build(c, flags=4)
        check_rows(base, g.bfs(base.vid[srcs], 3, 2), srcs, 3, 2)


def test_bfs_rows(base, poison):
    srcs = base.sources(9, seed=4)
    want = [k % 3 != 1 for k in range(len(srcs))]
    with Session() as c:
        g = base.build(c, flags=4)
        rows = g.bfs_rows(base.vid[srcs], 3, want=want)
    for k, sv in enumerate(srcs):
        if want[k]:
            np.testing.assert_array_equal(rows[k], base.bfs(sv), err_msg=f"source {k}")
        else:
            assert rows[k] is None


@pytest.mark.parametrize("nsrc", [1, 64])
def test_bfs_unwanted_then_wanted(base, poison, nsrc):
    first, second = base.sources(nsrc, seed=5), base.sources(nsrc, seed=6)
    with Session() as c:
        g = base.build(c, flags=4)
        assert g.bfs(base.vid[first], 3, want=False) is None
        check_rows(base, g.bfs(base.vid[second], 3), second)


@pytest.mark.parametrize("nsrc", [1, 7, 64])
def test_bfs_keep_and_kept_rows(base, poison, nsrc):
    srcs = base.sources(nsrc, seed=7)
    with Session() as c:
        g = base.build(c, flags=4)
        g.bfs_keep(base.vid[srcs], 3)
        for k, sv in enumerate(srcs):
            np.testing.assert_array_equal(g.bfs_kept_row(k), base.bfs(sv), err_msg=f"row {k}")
        g.bfs_kept_release()


def check_dag(case, g, row, source, target):
    """The DAG of kept row `row` against test_gpu_path_dag.host_dag (the oracle's CSR walked back on the host):
    vertex set, depths, order by depth, and every predecessor set; read back in two vertex ranges."""
    n = case.n
    ptr, adj = case.csr_both()
    depth = case.bfs(source)
    want_v, want_pairs, want_deepest = host_dag(n, ptr, adj, depth, target)
    nv, ne, deepest = g.bfs_kept_dag_build(row, target)
    assert (nv, deepest, ne) == (len(want_v), want_deepest, len(want_pairs))
    half = nv // 2
    a, b = g.bfs_kept_dag_read(0, half), g.bfs_kept_dag_read(half, nv - half)
    vertex, vdepth = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    off, pred = np.concatenate([a[2], b[2][1:]]), np.concatenate([a[3], b[3]])
    assert a[2][-1] == b[2][0] and off[0] == 0 and off[-1] == ne == len(pred)
    np.testing.assert_array_equal(np.sort(vertex), want_v)
    np.testing.assert_array_equal(vdepth, depth[vertex])
    assert np.all(np.diff(vdepth) <= 0) and vertex[-1] == source and np.all(np.diff(off) >= 0)
    got_pairs = np.repeat(vertex.astype(np.int64), np.diff(off)) * n + pred
    np.testing.assert_array_equal(np.sort(got_pairs), want_pairs)


@pytest.mark.parametrize("masked", [False, True], ids=["all", "sparse_mask"])
def test_bfs_kept_dag(base, poison, masked):
    srcs = np.array([base.hub, int(base.s[7]), base.path_end], np.int64)
    target = None
    if masked:
        target = np.random.default_rng(8).random(base.n) < 0.01
        target[[base.path_end, base.isolated]] = True
    with Session() as c:
        g = base.build(c, flags=4)
        g.bfs_keep(base.vid[srcs], 3)
        for row in (0, 2):
            check_dag(base, g, row, int(srcs[row]), target)


# ---- connected components ----
@pytest.mark.parametrize("uf", [1, 0], ids=["union_find", "propagation"])
def test_connected_components(base, poison, uf):
    want, want_it = base.cc()
    with Session(cc_uf=uf) as c:
        comp, it = base.build(c, flags=4).connected_components()
    np.testing.assert_array_equal(comp, want)
    assert it == want_it


@pytest.mark.parametrize("uf", [1, 0], ids=["union_find", "propagation"])
def test_connected_components_path_past_the_cap(oracle_lib, poison, uf):
    """150 vertices in a path, the minimum label at one end: the 99-superstep cap binds."""
    n = 150
    vid = np.arange(1000, 1000 + n, dtype=np.int64)  # four digits each: String order = numeric order
    s, t = np.arange(n - 1), np.arange(1, n)
    want, want_it = oracle_lib.connected_components(n, s, t, vid)
    assert len(np.unique(want)) > 1  # the cap bound: the far end never heard of the minimum
    with Session(cc_uf=uf) as c:
        comp, it = c.build(vid, vid[s], vid[t], flags=4).connected_components()
    np.testing.assert_array_equal(comp, want)
    assert it == want_it


@pytest.mark.parametrize("n", [1, 333])
@pytest.mark.parametrize("uf", [1, 0], ids=["union_find", "propagation"])
def test_connected_components_without_an_edge(oracle_lib, poison, uf, n):
    """Found by the existing suite under ff (test_gpu_cc_census.test_edge_graphs hung): with no edge at all the
    union-find wrote no parent entry, and its giant-root pick still walked up from row 0 through whatever the
    block held.  A fresh block reads 0 (row 0 its own root), so no test saw it."""
    none = np.zeros(0, np.int64)
    vid = np.random.default_rng(n).choice(np.arange(1, 50 * n + 100, dtype=np.int64), size=n, replace=False)
    want, want_it = oracle_lib.connected_components(n, none, none, vid)
    assert want_it == 0
    nc, largest, wv, wp = expected_census(want, 1)
    with Session(cc_uf=uf) as c:
        g = c.build(vid, none, none, flags=4)
        comp, it = g.connected_components()
        np.testing.assert_array_equal(comp, want)
        assert it == want_it
        it, gc, glargest, gv, gp = g.cc_census(1)
        assert (it, gc, glargest) == (want_it, nc, largest) == (0, n, 1)
        np.testing.assert_array_equal(gv, wv)
        np.testing.assert_array_equal(gp, wp)


@pytest.mark.parametrize("min_population", [1, 2])
def test_cc_census(base, poison, min_population):
    labels, want_it = base.cc()
    nc, largest, wv, wp = expected_census(labels, min_population)
    with Session() as c:
        g = base.build(c, flags=4)
        it, gc, gl, glargest, _ = g.cc_census_build(min_population)
        assert (it, gc, gl, glargest) == (want_it, nc, len(wv), largest)
        half = gl // 2
        (v0, p0), (v1, p1) = g.cc_census_read(0, half), g.cc_census_read(half, gl - half)
        g.cc_census_release()
    np.testing.assert_array_equal(np.concatenate([v0, v1]), wv)
    np.testing.assert_array_equal(np.concatenate([p0, p1]), wp)


# ---- combiners ----
@pytest.mark.parametrize("direction", [1, 2, 3], ids=["OUT", "IN", "BOTH"])
@pytest.mark.parametrize("combiner", [0, 1, 2], ids=["SUM", "MIN", "MAX"])
def test_combiners(base, poison, combiner, direction):
    with Session() as c:
        g = base.build(c)
        for wrap in (True, False):
            for steps in (1, 3):
                want, wrec = base.combine(direction, combiner, steps, wrap)
                x, rec = g.combine_steps(direction, combiner, steps, base.init(), wrap)
                np.testing.assert_array_equal(rec, wrec, err_msg=f"wrap {wrap} steps {steps}")
                np.testing.assert_array_equal(x, want, err_msg=f"wrap {wrap} steps {steps}")


# ---- sharded ----
LAYOUTS = [(2, 1), (3, 1), (3, 0)]  # (logical shards, halo)


def sharded_pagerank(case, g):
    assert_pr(g.pagerank(0.85, case.n, 12)[0], case.pagerank(case.n, 12)[0])


def sharded_cc(case, g):
    comp, it = g.connected_components()
    np.testing.assert_array_equal(comp, case.cc()[0])
    assert it == case.cc()[1]


def sharded_bfs1(case, g):
    for sv in (case.hub, case.path_end, case.isolated):
        check_rows(case, g.bfs([case.vid[sv]], 3), [sv])


def sharded_bfs64(case, g):
    srcs = case.sources(64)
    check_rows(case, g.bfs(case.vid[srcs], 3), srcs)


def sharded_sd(case, g):
    for seed in (case.hub, int(case.t[0])):
        np.testing.assert_array_equal(g.shortest_distance(case.vid[seed], 5), case.sd(seed, 5, "w"))


def sharded_sum(case, g):
    for direction in (1, 2, 3):
        want, wrec = case.combine(direction, 0, 3, True)
        x, rec = g.combine_steps(direction, 0, 3, case.init(), True)
        np.testing.assert_array_equal(rec, wrec, err_msg=f"direction {direction}")
        np.testing.assert_array_equal(x, want, err_msg=f"direction {direction}")


SHARDED = {"pagerank": (sharded_pagerank, {}), "cc_union_find": (sharded_cc, {}),
           "cc_propagation": (sharded_cc, {"cc_uf_sharded": 0}), "bfs_1": (sharded_bfs1, {}),
           "bfs_64": (sharded_bfs64, {}), "sd_weighted": (sharded_sd, {}), "sum": (sharded_sum, {})}


@pytest.mark.parametrize("program", list(SHARDED))
@pytest.mark.parametrize("shards,halo", LAYOUTS)
def test_sharded(base, poison, shards, halo, program):
    fn, knobs = SHARDED[program]
    with Session(shards, halo=halo, **knobs) as c:
        g = base.build(c, weight=base.w if program == "sd_weighted" else None)
        assert g.info()["num_shards"] == shards
        if program == "sd_weighted" and not halo:  # sharded shortest distance runs over the halo plan only
            import janusgraph_amd as jg
            with pytest.raises(jg.JanusGpuError) as e:
                fn(base, g)
            assert e.value.code == jg._lib.JG_ERR_UNSUPPORTED
            return
        fn(base, g)


def test_two_ranks_over_host_transport(tmp_path, poison):
    """Rank mode (two processes, the host transport) under the pattern: test_multirank_transport's worker,
    which checks PageRank, CC, both BFS engines, degrees and weighted shortest distance against the oracle.
    The spawned ranks inherit the variable."""
    import multiprocessing as mp
    from test_multirank_transport import _free_port, _worker
    world = 2
    ctx = mp.get_context("spawn")
    errfile = str(tmp_path / "err.txt")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, 1, errfile)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    for p in procs:
        if p.is_alive():
            p.kill()
    err = open(errfile).read() if os.path.exists(errfile) else ""
    assert all(p.exitcode == 0 for p in procs), f"exit codes {[p.exitcode for p in procs]}\n{err}"


# ---- program sequences on one graph ----
def run_sequence(case, g, shards, first_only=False):
    """The fixed sequence; every step against the oracle.  first_only: the first five steps."""
    from janusgraph_amd import _lib
    one = shards == 1
    src64, other64, src8 = case.sources(64), case.sources(64, seed=23), case.sources(8, seed=29)
    kept = case.sources(5, seed=31)
    seed = int(case.t[0])

    def cc():
        comp, it = g.connected_components()
        np.testing.assert_array_equal(comp, case.cc()[0])
        assert it == case.cc()[1]

    def pagerank():
        assert_pr(g.pagerank(0.85, case.n, 12)[0], case.pagerank(case.n, 12)[0])

    cc()
    check_rows(case, g.bfs(case.vid[src64], 3), src64)
    pagerank()
    check_rows(case, g.bfs([case.vid[case.path_end]], 3), [case.path_end])
    np.testing.assert_array_equal(g.shortest_distance(case.vid[seed], 5), case.sd(seed, 5, "w"))
    if first_only:
        return
    want, wrec = case.combine(2, 0, 3, True)
    x, rec = g.combine_steps(2, 0, 3, case.init(), True)
    np.testing.assert_array_equal(rec, wrec)
    np.testing.assert_array_equal(x, want)
    if one:  # the census and the DAG run on one shard
        labels, want_it = case.cc()
        nc, largest, wv, wp = expected_census(labels, 1)
        it, gc, largest_got, gv, gp = g.cc_census(1)
        assert (it, gc, largest_got) == (want_it, nc, largest)
        np.testing.assert_array_equal(gv, wv)
        np.testing.assert_array_equal(gp, wp)
    g.bfs_keep(case.vid[kept], 3)
    if one:
        check_dag(case, g, 1, int(kept[1]), None)
    _lib.tune_set("cc_uf_sharded" if not one else "cc_uf", 0)
    try:
        cc()
    finally:
        _lib.tune_set("cc_uf_sharded" if not one else "cc_uf", 1)
    check_rows(case, g.bfs(case.vid[src8], 3), src8)
    pagerank()
    check_rows(case, g.bfs(case.vid[other64], 3), other64)
    cc()
    for k, sv in enumerate(kept):
        np.testing.assert_array_equal(g.bfs_kept_row(k), case.bfs(sv), err_msg=f"kept row {k}")


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("pattern", [None, "ff", "2a"], ids=["off", "ff", "2a"])
def test_program_sequence(oracle_lib, monkeypatch, pattern, shards):
    if pattern is None:
        monkeypatch.delenv("JG_DEV_POISON", raising=False)
    else:
        monkeypatch.setenv("JG_DEV_POISON", pattern)
    with Session(shards) as c:
        case = case_of(oracle_lib, 12)
        g = case.build(c, weight=case.w)
        run_sequence(case, g, shards)
        g.close()
        for scale in (10, 13):  # a smaller, then a larger graph in the same context: each gets the other's blocks
            case = case_of(oracle_lib, scale)
            g = case.build(c, weight=case.w)
            run_sequence(case, g, shards, first_only=True)
            g.close()
