"""The merge kernel's segmented fold (csrc/jg_pull.h pull_merge_kernel) on hand-made graphs that put
every row of two or more entries through it (band0_deg = 2, 8 sub-slices, no second band).

The big graph (4096 vertices) has
  * one row of 3000 in-edges: ~375 entries in every sub-slice, so with the short rows in front of it
    its sub-rows straddle task boundaries (carries, and carry runs across tasks),
  * 600 rows of in-degree 2-8: their sub-rows are mostly single entries, so lanes hold 8 heads, heads
    sit at lane positions 0 and 7, and a task has far more than 64 heads (over a 64-slot staging
    window, inside a 512-slot one),
  * 50 rows of in-degree 30-60,
  * 1500 rows of in-degree 2 and 3 as padding.  A sub-slice's last task holds its entry count modulo
    512; the eight counts are sums of ~2500 random sub-row lengths, so that they are all multiples of
    8 is as good as impossible.
The tiny graph (256 vertices, three rows of in-degree 2: six entries in all) guarantees the other
partial task: every non-empty sub-slice is one task of fewer than 8 entries.  Both graphs are small
enough for the LDS image kernels (the whole vector is staged); a 16-vertex copy of the tiny graph is
below one line group per sub-slice and runs the kernels without an LDS image.

Integer sums are compared exactly: a segment credited to the wrong slot cannot hide in a tolerance.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PR_RTOL = 1e-9  # north_star: per-vertex relative error <= 1e-9 (fp64)
N = 4096
KNOBS = (("band0_deg", 2), ("band0_sub", 8), ("band1_deg", 0))
DEFAULTS = (("band0_deg", 96), ("band0_bit", 0), ("band1_deg", -1), ("merge_stage0", -1), ("merge_stage1", -1))


def big_edges():
    rng = np.random.default_rng(20)
    deg = np.zeros(N, np.int64)
    rows = rng.permutation(N)
    deg[rows[0]] = 3000
    deg[rows[1:601]] = rng.integers(2, 9, 600)
    deg[rows[601:651]] = rng.integers(30, 61, 50)
    deg[rows[651:2151]] = rng.integers(2, 4, 1500)
    dst = np.repeat(np.arange(N), deg)
    src = rng.integers(0, N, len(dst))
    p = rng.permutation(len(dst))
    return src[p].astype(np.int32), dst[p].astype(np.int32)


def tiny_edges(n):
    dst = np.array([3, 3, 7, 7, 12, 12], np.int32)
    src = np.array([1, n - 1, 0, 5, n - 2, 9], np.int32)
    return src, dst


@pytest.fixture(scope="module")
def graphs():
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    made = []
    ctx = None
    try:
        for k, v in KNOBS:
            _lib.tune_set(k, v)
        ctx = jg.Context((0,))
        out = {}
        for name, n, (s, t) in (("big", N, big_edges()), ("tiny", 256, tiny_edges(256)), ("tiny16", 16, tiny_edges(16))):
            vid = (np.arange(n, dtype=np.int64) + 1) << 8
            g = ctx.build(vid, vid[s], vid[t], flags=jg.ADJ_IN | jg.ADJ_OUT | jg.ADJ_BOTH)
            made.append(g)
            out[name] = (g, n, vid, s, t)
        yield out
    finally:
        for g in made:
            g.close()
        if ctx is not None:
            ctx.close()
        for k, v in DEFAULTS:
            _lib.tune_set(k, v)


@pytest.fixture
def stage():
    """Sets merge_stage0 for one test and puts the automatic window back."""
    from janusgraph_amd import _lib
    try:
        yield lambda v: _lib.tune_set("merge_stage0", v)
    finally:
        _lib.tune_set("merge_stage0", -1)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("name", ["big", "tiny", "tiny16"])
@pytest.mark.parametrize("combiner", [0, 1, 2])  # COMBINE_SUM, _MIN, _MAX
def test_combiner_supersteps_exact(graphs, oracle_lib, stage, name, combiner):
    g, n, vid, s, t = graphs[name]
    init = np.random.default_rng(combiner).integers(-(1 << 39), 1 << 39, n)
    for direction in (2, 1):  # DIR_IN, DIR_OUT
        for steps in (1, 3):
            want, wrec = oracle_lib.combine_steps(n, s, t, direction, combiner, steps, init, False)
            for window in (-1, 64, 512, 0):
                stage(window)
                x, rec = g.combine_steps(direction, combiner, steps, init, False)
                np.testing.assert_array_equal(rec, wrec, err_msg=f"dir {direction} steps {steps} stage {window}")
                np.testing.assert_array_equal(x, want, err_msg=f"dir {direction} steps {steps} stage {window}")


@pytest.mark.parametrize("name", ["big", "tiny", "tiny16"])
def test_pagerank_oracle_and_stage_windows_bitwise(graphs, oracle_lib, stage, name):
    """Within PR_RTOL of the oracle; the staged and the direct body (and two runs of one setting) give
    the same ranks bit for bit: they do the same arithmetic and differ only in how they store."""
    g, n, vid, s, t = graphs[name]
    want, _ = oracle_lib.pagerank(n, s, t, 0.85, n, 12)
    ranks = {}
    for window in (-1, 0, 64, 512):
        stage(window)
        ranks[window], _ = g.pagerank(0.85, n, 12)
    again, _ = g.pagerank(0.85, n, 12)
    rel = np.abs(ranks[-1] - want) / np.maximum(np.abs(want), 1e-300)
    assert rel.max() <= PR_RTOL, f"max rel err {rel.max()}"
    np.testing.assert_array_equal(bits(again), bits(ranks[512]), err_msg="run to run")
    for window in (0, 64, 512):
        np.testing.assert_array_equal(bits(ranks[window]), bits(ranks[-1]), err_msg=f"stage {window} vs automatic")


def test_bfs_64_sources(graphs, oracle_lib):
    """The 64-source BFS folds 64-bit ORs through the same kernel and passes it the task bitmap."""
    import janusgraph_amd as jg
    g, n, vid, s, t = graphs["big"]
    deg = np.bincount(s, minlength=n) + np.bincount(t, minlength=n)
    srcs = np.random.default_rng(5).choice(np.flatnonzero(deg > 0), 64, replace=False)
    depth = g.bfs(vid[srcs], jg.DIR_BOTH)
    for k in range(64):
        np.testing.assert_array_equal(depth[k], oracle_lib.bfs(n, s, t, int(srcs[k]), oracle_lib.DIR_BOTH), err_msg=f"source {k}")


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("bit", [5, 8])
def test_temporal_schedule_at_a_small_shape(oracle_lib, bit, shards):
    """The merge kernel's temporal schedule (merge_temporal = 2 forces it; by default only vectors past 64 MB
    take it, RMAT-24 and larger): every block of an XCD sweeps the XCD's sub-slices in rounds and restages
    its LDS image each round.  32 and 256 sub-slices give 4 and 32 rounds per XCD (at 8 sub-slices there is
    one round, the static schedule); 3 logical shards take the multi-segment kernel.  The knob is read at
    launch, so one graph runs both schedules: combiners and the 64-source BFS exactly, PageRank within
    PR_RTOL of the oracle.  The ranks of the two schedules are equal bit for bit: a task belongs to a
    sub-slice and writes its own partials, and the schedule only chooses which block (and round) takes it
    (jg_pull.h pull_merge_kernel: h, g and G are all the schedule changes; task_of only permutes tasks)."""
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    s, t = big_edges()
    vid = (np.arange(N, dtype=np.int64) + 1) << 8
    init = np.random.default_rng(bit).integers(-(1 << 39), 1 << 39, N)
    deg = np.bincount(s, minlength=N) + np.bincount(t, minlength=N)
    srcs = np.random.default_rng(5).choice(np.flatnonzero(deg > 0), 64, replace=False)
    want_pr, _ = oracle_lib.pagerank(N, s, t, 0.85, N, 12)
    ctx = None
    try:
        for k, v in (("band0_deg", 2), ("band0_bit", bit), ("band1_deg", 0)):
            _lib.tune_set(k, v)
        ctx = jg.Context((0,) * shards)
        g = ctx.build(vid, vid[s], vid[t], flags=jg.ADJ_IN | jg.ADJ_OUT | jg.ADJ_BOTH)
        assert g.info()["num_shards"] == shards
        ranks = {}
        for temporal in (0, 2):
            _lib.tune_set("merge_temporal", temporal)
            for combiner in (0, 1, 2):
                for direction in (2, 1):
                    want, wrec = oracle_lib.combine_steps(N, s, t, direction, combiner, 3, init, False)
                    x, rec = g.combine_steps(direction, combiner, 3, init, False)
                    np.testing.assert_array_equal(rec, wrec, err_msg=f"temporal {temporal} combiner {combiner} dir {direction}")
                    np.testing.assert_array_equal(x, want, err_msg=f"temporal {temporal} combiner {combiner} dir {direction}")
            depth = g.bfs(vid[srcs], jg.DIR_BOTH)
            for k in range(64):
                np.testing.assert_array_equal(depth[k], oracle_lib.bfs(N, s, t, int(srcs[k]), oracle_lib.DIR_BOTH),
                                              err_msg=f"temporal {temporal} source {k}")
            ranks[temporal], _ = g.pagerank(0.85, N, 12)
            rel = np.abs(ranks[temporal] - want_pr) / np.maximum(np.abs(want_pr), 1e-300)
            assert rel.max() <= PR_RTOL, f"temporal {temporal}: max rel err {rel.max()}"
        np.testing.assert_array_equal(bits(ranks[2]), bits(ranks[0]), err_msg="temporal vs static schedule")
    finally:
        if ctx is not None:
            ctx.close()
        _lib.tune_set("merge_temporal", 1)
        for k, v in DEFAULTS:
            _lib.tune_set(k, v)
