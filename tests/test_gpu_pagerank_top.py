"""jg_pagerank_top / jg_pagerank_top_read / jg_pagerank_top_release: the k highest-ranked vertices of a
PageRank session, selected on the device (janusgraph_amd/csrc/jg_top.hip).

What is expected is always test_pagerank_top_host.expected_top applied to what pagerank_end() returns for the
same session on the same graph (the existing entry point, which the suite checks against the oracle; the RMAT
cases here anchor it once more).  The listed ranks and edge counts must equal those arrays bit for bit at the
listed indices, the vids must be vertex_ids()[index], and the whole sequence is compared in order.  Vertex ids
are sparse and shuffled, so vid != caller index != device row.
"""
import os
import socket
import sys

import numpy as np
import pytest

from test_pagerank_top_host import expected_top

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_RTOL = 1e-9  # the suite's PageRank tolerance (test_gpu_parity.py)


@pytest.fixture(scope="module")
def ctx():
    import janusgraph_amd as jg
    c = jg.Context((0,))
    yield c
    c.close()


def code(fn, *a):
    import janusgraph_amd as jg
    with pytest.raises(jg.JanusGpuError) as e:
        fn(*a)
    return e.value.code


def sparse_ids(n, seed):
    """n distinct positive ids, sparse and shuffled (as test_gpu_cc_census.sparse_ids)."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.arange(1, 50 * n + 100, dtype=np.int64), size=n, replace=False)


def build(ctx, n, s, t, seed=1, flags=None):
    import janusgraph_amd as jg
    vid = sparse_ids(n, seed)
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    return ctx.build(vid, vid[s], vid[t], flags=jg.ADJ_IN if flags is None else flags)


def path_edges(n):
    """0 -> 1 -> ... -> n - 1 (n == 1: a self-loop, so that the edge list is not empty)."""
    if n == 1:
        return np.zeros(1, np.int64), np.zeros(1, np.int64)
    v = np.arange(n - 1, dtype=np.int64)
    return v, v + 1


def star_edges(n, hub):
    leaves = np.delete(np.arange(n, dtype=np.int64), hub)
    return leaves, np.full(n - 1, hub, np.int64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_top(g, k, basis=None):
    """top(k) of g's session against expected_top of its pagerank_end(); returns (indices, rank, select_ms)."""
    rank, ec = g.pagerank_end() if basis is None else basis
    want = expected_top(rank, k)
    listed, ms = g.pagerank_top_build(k)
    vid, idx, r, e = g.pagerank_top_read(0, listed)
    assert listed == min(k, g.n) == len(want)
    np.testing.assert_array_equal(idx, want)               # the whole sequence, in order
    np.testing.assert_array_equal(bits(r), bits(rank[want]))   # the stored bit patterns
    np.testing.assert_array_equal(bits(e), bits(ec[want]))
    np.testing.assert_array_equal(vid, g.vertex_ids()[want])
    assert ms >= 0
    return idx, rank, ms


# ---- one tie class: the whole tie-cut path at block, wave and tile edges ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 2049, 70001])
def test_one_tie_class(ctx, n):
    g = build(ctx, n, *path_edges(n), seed=n)
    try:
        g.pagerank_begin(0.85, n)   # no step: every rank is 1/N
        basis = g.pagerank_end()
        assert (bits(basis[0]) == bits(np.array([1.0 / n]))[0]).all()
        for k in (1, 2, n - 1, n, n + 5):
            if k < 1:
                continue
            idx, _, _ = check_top(g, k, basis)
            np.testing.assert_array_equal(idx, np.arange(min(k, n)))
    finally:
        g.close()


# ---- star: one hub above n - 1 equal ranks, the cut inside the big class for every k > 1 ----
def test_star(ctx):
    n, hub = 70001, 12345
    g = build(ctx, n, *star_edges(n, hub), seed=7)
    try:
        g.pagerank_begin(0.85, n)
        g.pagerank_step(2)          # K = 3
        basis = g.pagerank_end()
        assert len(np.unique(basis[0])) == 2 and basis[0].argmax() == hub
        for k in (1, 2, 1000, n):
            idx, _, _ = check_top(g, k, basis)
            assert idx[0] == hub
            np.testing.assert_array_equal(idx[1:], np.delete(np.arange(n), hub)[:min(k, n) - 1])
    finally:
        g.close()


# ---- tie classes with the cut exactly between them ----
def test_cut_between_tie_classes(ctx):
    """Two stars of different sizes (2 hubs), a class of 100 vertices fed by one source of out-degree 1 each,
    and everything else at the teleport rank: upper classes of 2 and 102 vertices."""
    n = 3000
    rng = np.random.default_rng(11)
    perm = rng.permutation(n)
    hub_a, hub_b = perm[0], perm[1]
    la, lb = perm[2:302], perm[302:502]        # leaves: 300 and 200
    fed, src = perm[502:602], perm[602:702]    # 100 fed vertices, their sources
    s = np.concatenate([la, lb, src])
    t = np.concatenate([np.full(300, hub_a), np.full(200, hub_b), fed])
    g = build(ctx, n, s, t, seed=13)
    try:
        g.pagerank_begin(0.85, n)
        g.pagerank_step(2)
        basis = g.pagerank_end()
        rank = basis[0]
        assert rank[hub_a] > rank[hub_b] > rank[fed[0]] > rank[src[0]]
        assert (rank == rank[fed[0]]).sum() == 100 and (rank == rank[src[0]]).sum() == n - 102
        for k in (1, 2, 3, 101, 102, 103):
            idx, _, _ = check_top(g, k, basis)
            if k >= 102:
                np.testing.assert_array_equal(idx[2:102], np.sort(fed))
    finally:
        g.close()


# ---- all-distinct ranks: no tie pass, the select ends early ----
def test_all_distinct(ctx):
    """A random digraph of 16 in-edges per vertex on average (a path's ranks converge to one value along
    the path, so they tie; these do not)."""
    n = 2049
    rng = np.random.default_rng(5)
    s, t = rng.integers(0, n, 16 * n), rng.integers(0, n, 16 * n)
    g = build(ctx, n, s, t, seed=17)
    try:
        g.pagerank_begin(0.85, n)
        g.pagerank_step(9)
        basis = g.pagerank_end()
        assert len(np.unique(basis[0])) == n
        for k in (1, 2, 100, 2047, 2048, 2049):
            check_top(g, k, basis)
    finally:
        g.close()


# ---- RMAT: natural tie classes and hubs; the basis itself anchored to the oracle ----
@pytest.fixture(scope="module")
def rmat(oracle_lib):
    out = {}
    for scale in (12, 16):
        s, t = oracle_lib.rmat_edges(scale, 16, 40 + scale)
        ref, _ = oracle_lib.pagerank(1 << scale, s.astype(np.int32), t.astype(np.int32), 0.85, 1 << scale, 10)
        out[scale] = (s, t, ref)
    return out


@pytest.mark.parametrize("scale", [12, 16])
def test_rmat(ctx, rmat, scale):
    n = 1 << scale
    s, t, ref = rmat[scale]
    g = build(ctx, n, s, t, seed=scale)
    try:
        g.pagerank_begin(0.85, n)
        g.pagerank_step(9)          # K = 10
        basis = g.pagerank_end()
        rel = np.abs(basis[0] - ref) / np.abs(ref)
        assert rel.max() <= PR_RTOL, f"PageRank parity {rel.max()}"
        for k in (1, 10, 1000, 1 << 12, n):
            _, _, ms = check_top(g, k, basis)
            st = ctx.stats()
            print(f"rmat-{scale} k {k}: select_ms {ms:.3f} launches {st['kernel_launches']} "
                  f"bytes {st['algorithmic_bytes']:.0f}")
            assert st["compute_ms"] == pytest.approx(ms) and st["kernel_launches"] > 0
            assert st["algorithmic_bytes"] > 0
    finally:
        g.close()


# ---- the sign flip, the zeros, NaN ----
def test_negative_ranks(ctx, rmat):
    n = 1 << 12
    s, t, _ = rmat[12]
    g = build(ctx, n, s, t, seed=3)
    try:
        g.pagerank_begin(0.85, -7)
        g.pagerank_step(4)
        basis = g.pagerank_end()
        assert (basis[0] < 0).all()
        for k in (1, 10, 3000, n):
            idx, rank, _ = check_top(g, k, basis)
            assert idx[0] == rank.argmax()
        idx, rank, _ = check_top(g, n, basis)
        assert rank[idx[-1]] == rank.min()   # the most negative comes last
    finally:
        g.close()


def test_zero_ranks(ctx, rmat):
    n = 1 << 12
    s, t, _ = rmat[12]
    g = build(ctx, n, s, t, seed=4)
    try:
        g.pagerank_begin(1.0, n)    # teleport 0: a vertex without in-edges ranks 0.0
        g.pagerank_step(4)
        basis = g.pagerank_end()
        zeros = int((basis[0] == 0).sum())
        assert 0 < zeros < n
        for k in (1, n - zeros, n - zeros + 1, n - 1, n):
            check_top(g, k, basis)
    finally:
        g.close()


def test_nan_damping(ctx, rmat):
    n = 1 << 12
    s, t, _ = rmat[12]
    g = build(ctx, n, s, t, seed=5)
    try:
        g.pagerank_begin(float("nan"), n)
        g.pagerank_step(2)
        basis = g.pagerank_end()
        for k in (1, 7, n - 1, n):
            idx, rank, _ = check_top(g, k, basis)   # the call returns
            if np.isnan(rank).all():
                np.testing.assert_array_equal(idx, np.arange(min(k, n)))
        assert np.isnan(basis[0]).any()
    finally:
        g.close()


# ---- the session goes on; the list is the graph's own ----
def test_session_and_lifetime(ctx, rmat):
    import janusgraph_amd as jg
    n = 1 << 12
    s, t, _ = rmat[12]
    g = build(ctx, n, s, t, seed=6, flags=jg.ADJ_IN | jg.ADJ_BOTH)
    try:
        g.pagerank_begin(0.85, n)
        g.pagerank_step(2)
        listed, _ = g.pagerank_top_build(50)          # before any pagerank_end
        first = g.pagerank_top_read(0, listed)
        rank2, _ = g.pagerank_end()
        np.testing.assert_array_equal(first[1], expected_top(rank2, 50))
        np.testing.assert_array_equal(bits(first[2]), bits(rank2[first[1]]))
        g.pagerank_step(3)                            # the session was not disturbed: steps follow
        idx5, rank5, _ = check_top(g, 50)             # ... and the second list replaces the first
        assert not np.array_equal(bits(rank5), bits(rank2))
        ref, _ = g.pagerank(0.85, n, 6)               # begin + 5 steps in one call: the same ranks
        np.testing.assert_array_equal(bits(ref), bits(rank5))
        # a jg_pagerank counts as a session, and one of 0 iterations leaves it as it was
        check_top(g, 20)
        g.pagerank(0.85, n, 0)
        check_top(g, 20, basis=g.pagerank_end())
        # the held list survives a new begin, a connected_components and a bfs, unchanged on read
        g.pagerank_begin(0.5, n)
        g.pagerank_step(1)
        held = check_top(g, 300)
        before = g.pagerank_top_read(0, 300)
        g.pagerank_begin(0.85, 3)
        g.pagerank_step(2)
        g.connected_components()
        g.bfs([g.vertex_ids()[0]], jg.DIR_BOTH)
        after = g.pagerank_top_read(0, 300)
        for a, b in zip(before, after):
            np.testing.assert_array_equal(bits(a) if a.dtype == np.float64 else a,
                                          bits(b) if b.dtype == np.float64 else b)
        np.testing.assert_array_equal(after[1], held[0])
        # ranged reads concatenate to the full read; an empty range at the end is accepted
        parts = [g.pagerank_top_read(f, c) for f, c in ((0, 1), (1, 99), (100, 0), (100, 200), (300, 0))]
        for j in range(4):
            np.testing.assert_array_equal(np.concatenate([p[j] for p in parts]), after[j])
    finally:
        g.close()


def test_errors(ctx, rmat):
    from janusgraph_amd import _lib
    n = 1 << 12
    s, t, _ = rmat[12]
    g = build(ctx, n, s, t, seed=8)
    try:
        assert code(g.pagerank_top_build, 5) == _lib.JG_ERR_STATE      # no session
        assert code(g.pagerank_top_read, 0, 0) == _lib.JG_ERR_STATE    # nothing held
        g.pagerank_top_release()                                        # nothing held: JG_OK
        g.pagerank_begin(0.85, n)
        assert code(g.pagerank_top_build, 0) == _lib.JG_ERR_ARG
        assert code(g.pagerank_top_build, -1) == _lib.JG_ERR_ARG
        listed, _ = g.pagerank_top_build(5)
        assert listed == 5
        assert code(g.pagerank_top_read, 0, 6) == _lib.JG_ERR_ARG       # past the end
        assert code(g.pagerank_top_read, 6, 0) == _lib.JG_ERR_ARG
        assert code(g.pagerank_top_read, -1, 1) == _lib.JG_ERR_ARG
        assert code(g.pagerank_top_read, 2, -1) == _lib.JG_ERR_ARG
        assert len(g.pagerank_top_read(5, 0)[0]) == 0
        assert code(g.pagerank_top_build, 0) == _lib.JG_ERR_ARG         # a failed top after a good one ...
        assert code(g.pagerank_top_read, 0, 1) == _lib.JG_ERR_STATE    # ... leaves nothing held
        g.pagerank_top_build(5)
        g.pagerank_top_release()
        assert code(g.pagerank_top_read, 0, 1) == _lib.JG_ERR_STATE    # a read after a release
        g.pagerank_top_release()                                        # a double release
    finally:
        g.close()


# ---- rank mode: unsupported ----
def _rank_worker(rank, world, port, errfile):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        sys.path.insert(0, ROOT)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import janusgraph_amd as jg
        from janusgraph_amd import _lib
        from janusgraph_amd.transport import GlooTransport
        n = 600
        vid = (np.arange(n, dtype=np.int64) + 1) << 8
        v = np.arange(n - 1)
        c = jg.Context((0,), rank=rank, nranks=world, transport=GlooTransport(dist, world))
        g = c.build(vid, vid[v], vid[v + 1], flags=jg.ADJ_IN)
        g.pagerank_begin(0.85, n)
        for fn, a in ((g.pagerank_top_build, (5,)), (g.pagerank_top, (5,))):
            try:
                fn(*a)
                raise AssertionError("jg_pagerank_top ran in rank mode")
            except jg.JanusGpuError as e:
                assert e.code == _lib.JG_ERR_UNSUPPORTED, e.code
        try:
            g.pagerank_top_read(0, 0)
            raise AssertionError("a list is held after an unsupported call")
        except jg.JanusGpuError as e:
            assert e.code == _lib.JG_ERR_STATE, e.code
        g.pagerank_end(want=False)
        g.close()
        c.close()
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        import traceback
        with open(errfile, "a") as f:
            f.write(f"rank {rank}:\n" + traceback.format_exc())
        raise


def test_rank_mode_is_unsupported(tmp_path):
    import multiprocessing as mp
    mpc = mp.get_context("spawn")
    errfile = str(tmp_path / "err.txt")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [mpc.Process(target=_rank_worker, args=(r, 2, port, errfile)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    for p in procs:
        if p.is_alive():
            p.kill()
    err = open(errfile).read() if os.path.exists(errfile) else ""
    assert all(p.exitcode == 0 for p in procs), f"exit codes {[p.exitcode for p in procs]}\n{err}"


# ---- logical shards: each shard selects, the records are merged on the host ----
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_logical_shards(rmat, devices):
    import janusgraph_amd as jg
    c = jg.Context(devices)
    try:
        n, hub = 70001, 12345
        g = build(c, n, *star_edges(n, hub), seed=7)
        try:
            assert g.info()["num_shards"] == len(devices)
            g.pagerank_begin(0.85, n)
            g.pagerank_step(2)
            basis = g.pagerank_end()
            for k in (1, 2, 1000, n // len(devices) + 10, n):   # the last two exceed a shard's rows
                check_top(g, k, basis)
        finally:
            g.close()
        n = 1 << 12
        s, t, ref = rmat[12]
        g = build(c, n, s, t, seed=12)
        try:
            g.pagerank_begin(0.85, n)
            g.pagerank_step(9)
            basis = g.pagerank_end()
            rel = np.abs(basis[0] - ref) / np.abs(ref)
            assert rel.max() <= PR_RTOL
            for k in (1, 10, 1000, 1500, 3000, n, n + 5):
                check_top(g, k, basis)
            g.pagerank_begin(0.85, n)    # one tie class across the shards
            basis = g.pagerank_end()
            for k in (1, 100, n - 1):
                idx, _, _ = check_top(g, k, basis)
                np.testing.assert_array_equal(idx, np.arange(k))
        finally:
            g.close()
    finally:
        c.close()


# ---- façade ----
def test_computer_top_route(ctx, monkeypatch):
    import janusgraph_amd as jg
    graph = jg.InMemoryGraph()
    jg.load_graph_of_the_gods(graph)
    n = len(graph.snapshot()[0])

    def submit(extra, persist=jg.Persist.NOTHING, iterations=10):
        c = jg.GpuGraphComputer(graph, context=ctx).persist(persist).result(jg.ResultGraph.NEW)
        c.program(jg.PageRankVertexProgram.build().iterations(iterations).vertexCount(n).create())
        c.mapReduce(jg.PageRankTopMapReduce.build().limit(3).create())
        c.mapReduce(jg.PageRankTopMapReduce.build().memoryKey("all").limit(n + 4).create())
        for mr in extra:
            c.mapReduce(mr)
        mem = c.submit().result().memory()
        return c, mem

    gc, gmem = submit([jg.PageRankMapReduce.build().create()])          # generic route
    assert not gc._map_reduced
    pc, pmem = submit([], persist=jg.Persist.VERTEX_PROPERTIES)          # persisting: generic too
    assert not pc._map_reduced
    # the device route hands back no per-vertex array
    def refuse(self, *a, **k):
        raise AssertionError("the top route must not hand the ranks back")
    monkeypatch.setattr(jg.Graph, "pagerank", refuse)
    monkeypatch.setattr(jg.Graph, "pagerank_end", refuse)
    dc, dmem = submit([])
    monkeypatch.undo()
    assert dc._map_reduced
    for mem in (gmem, pmem):
        assert dmem.get("pageRankTop") == mem.get("pageRankTop") and len(dmem.get("pageRankTop")) == 3
        assert dmem.get("all") == mem.get("all") and len(dmem.get("all")) == n
    assert dmem.getIteration() == gmem.getIteration() == 10
    ranks = dict(gmem.get("pageRank"))
    assert dmem.get("all") == sorted(ranks.items(), key=lambda kv: -kv[1])   # stable: snapshot order in ties
    zc, zmem = submit([], iterations=0)                                  # today's early return
    assert zmem.get("pageRankTop") == [] and zmem.get("all") == []
