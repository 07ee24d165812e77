"""The merge kernel's gather half (csrc/jg_pull.h pull_merge_kernel, SliceGather): the full-task and the
partial-task body, the clamped hot index, cold gathers through 32-bit byte offsets and through 64-bit
addresses, on the hand-made 4096-vertex graph of test_gpu_merge_fold.py (band0_deg = 2, no second
band: every row of two or more entries goes through the kernel).

By default a graph this small is staged whole in LDS (every slot hot) or not at all.  The knob
merge_hot caps the hot prefix of the vector, so that one task reads hot and cold entries side by side:
with 8 sub-slices of 512 elements, 128 leaves 16 elements (1/32) of every sub-slice hot and 1024 leaves
128 (1/4); 0 selects the kernels without an image.  Hot or cold only changes where a value is read
from, so the ranks of every setting are equal bit for bit, and integer results are compared exactly.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PR_RTOL = 1e-9  # north_star: per-vertex relative error <= 1e-9 (fp64)
N = 4096
DEFAULTS = (("band0_deg", 96), ("band0_bit", 0), ("band1_deg", -1), ("merge_hot", -1), ("merge_off32", 1),
            ("merge_temporal", 1))
CASES = [(c, d, k) for c in (0, 1, 2) for d in (2, 1) for k in (1, 3)]  # combiner, DIR_IN / DIR_OUT, steps


def big_edges():
    """test_gpu_merge_fold.py's big graph: one row of 3000 in-edges, 600 rows of 2-8, 50 of 30-60, 1500 of 2-3."""
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


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def restore():
    from janusgraph_amd import _lib
    for k, v in DEFAULTS:
        _lib.tune_set(k, v)


@pytest.fixture(scope="module")
def big(oracle_lib):
    """The big graph's edges and its oracle results, computed once and shared (read-only)."""
    s, t = big_edges()
    vid = (np.arange(N, dtype=np.int64) + 1) << 8
    init = np.random.default_rng(3).integers(-(1 << 39), 1 << 39, N)
    deg = np.bincount(s, minlength=N) + np.bincount(t, minlength=N)
    srcs = np.random.default_rng(5).choice(np.flatnonzero(deg > 0), 64, replace=False)
    ref = {"s": s, "t": t, "vid": vid, "init": init, "srcs": srcs,
           "combine": {c: oracle_lib.combine_steps(N, s, t, c[1], c[0], c[2], init, False) for c in CASES},
           "rank": oracle_lib.pagerank(N, s, t, 0.85, N, 12)[0],
           "depth": [oracle_lib.bfs(N, s, t, int(v), oracle_lib.DIR_BOTH) for v in srcs]}
    for a in [ref["rank"], *ref["depth"]] + [x for pair in ref["combine"].values() for x in pair]:
        a.setflags(write=False)
    return ref


def build(ctx, ref):
    import janusgraph_amd as jg
    return ctx.build(ref["vid"], ref["vid"][ref["s"]], ref["vid"][ref["t"]], flags=jg.ADJ_IN | jg.ADJ_OUT | jg.ADJ_BOTH)


def check_all(g, ref, tag):
    """Combiner supersteps and the 64-source BFS exactly, PageRank within PR_RTOL; returns the ranks."""
    import janusgraph_amd as jg
    for case in CASES:
        combiner, direction, steps = case
        want, wrec = ref["combine"][case]
        x, rec = g.combine_steps(direction, combiner, steps, ref["init"], False)
        np.testing.assert_array_equal(rec, wrec, err_msg=f"{tag} combiner {combiner} dir {direction} steps {steps}")
        np.testing.assert_array_equal(x, want, err_msg=f"{tag} combiner {combiner} dir {direction} steps {steps}")
    depth = g.bfs(ref["vid"][ref["srcs"]], jg.DIR_BOTH)
    for k in range(64):
        np.testing.assert_array_equal(depth[k], ref["depth"][k], err_msg=f"{tag} source {k}")
    rank, _ = g.pagerank(0.85, N, 12)
    rel = np.abs(rank - ref["rank"]) / np.maximum(np.abs(ref["rank"]), 1e-300)
    assert rel.max() <= PR_RTOL, f"{tag}: max rel err {rel.max()}"
    return rank


@pytest.fixture(scope="module")
def graph8(big):
    """The big graph in 8 sub-slices on one shard."""
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    ctx = g = None
    try:
        for k, v in (("band0_deg", 2), ("band0_sub", 8), ("band1_deg", 0)):
            _lib.tune_set(k, v)
        ctx = jg.Context((0,))
        g = build(ctx, big)
        yield g
    finally:
        if g is not None:
            g.close()
        if ctx is not None:
            ctx.close()
        restore()


def test_mixed_slots(graph8, big):
    """All hot, no image, 1/32 hot and 1/4 hot of every sub-slice."""
    from janusgraph_amd import _lib
    ranks = {}
    try:
        for hot in (-1, 0, 128, 1024):
            _lib.tune_set("merge_hot", hot)
            ranks[hot] = check_all(graph8, big, f"merge_hot {hot}")
    finally:
        _lib.tune_set("merge_hot", -1)
    for hot in (0, 128, 1024):
        np.testing.assert_array_equal(bits(ranks[hot]), bits(ranks[-1]), err_msg=f"merge_hot {hot} vs automatic")


def test_offsets_32_and_64_bit(graph8, big):
    """The vector is far below 4 GiB, so the launches above gathered through 32-bit byte offsets;
    merge_off32 = 0 forces the 64-bit addresses that larger vectors take.  Same checks, same ranks."""
    from janusgraph_amd import _lib
    ranks = {}
    try:
        for off32 in (1, 0):
            _lib.tune_set("merge_off32", off32)
            for hot in (-1, 0, 128):
                _lib.tune_set("merge_hot", hot)
                ranks[off32, hot] = check_all(graph8, big, f"merge_off32 {off32} merge_hot {hot}")
    finally:
        _lib.tune_set("merge_off32", 1)
        _lib.tune_set("merge_hot", -1)
    for key, r in ranks.items():
        np.testing.assert_array_equal(bits(r), bits(ranks[1, -1]), err_msg=f"(merge_off32, merge_hot) = {key}")


@pytest.mark.parametrize("shards", [1, 3])
def test_sub_slice_and_shard_variants(big, shards):
    """32 sub-slices (a line group is 512 elements; merge_hot = 512 keeps one group per segment hot), the
    static and the temporal schedule, one shard and three logical shards (the multi-segment kernel,
    whose hot index stays a compare and a select)."""
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    ctx = g = None
    ranks = {}
    try:
        for k, v in (("band0_deg", 2), ("band0_bit", 5), ("band1_deg", 0)):
            _lib.tune_set(k, v)
        ctx = jg.Context((0,) * shards)
        g = build(ctx, big)
        assert g.info()["num_shards"] == shards
        for temporal in (0, 2):
            _lib.tune_set("merge_temporal", temporal)
            for hot in (512, -1):
                _lib.tune_set("merge_hot", hot)
                ranks[temporal, hot] = check_all(g, big, f"shards {shards} temporal {temporal} merge_hot {hot}")
    finally:
        if g is not None:
            g.close()
        if ctx is not None:
            ctx.close()
        restore()
    for key, r in ranks.items():
        np.testing.assert_array_equal(bits(r), bits(ranks[0, 512]), err_msg=f"(merge_temporal, merge_hot) = {key}")


def last_task_edges(entries):
    """1024 vertices; rows 0..127 have in-degree 8 (1024 entries), row 0 one fewer or one more for 1023 or
    1025, and rows 200..299 in-degree 1 (below the band).  Sources are distinct within a row and never the
    row itself, so no edge is a duplicate or a loop and the band holds exactly `entries` entries."""
    n = 1024
    deg = np.zeros(n, np.int64)
    deg[:128] = 8
    deg[0] += entries - 1024
    deg[200:300] = 1
    rng = np.random.default_rng(entries)
    src = np.concatenate([(r + 1 + rng.choice(n - 1, d, replace=False)) % n for r, d in enumerate(deg) if d])
    dst = np.repeat(np.arange(n), deg)
    assert int(deg[deg >= 2].sum()) == entries and (src != dst).all()
    p = rng.permutation(len(dst))
    return n, src[p].astype(np.int32), dst[p].astype(np.int32)


@pytest.mark.parametrize("entries", [1023, 1024, 1025])
def test_full_and_partial_last_task(oracle_lib, entries):
    """One sub-slice holds every band entry, so its length is chosen exactly: 1023 entries end in a task
    one entry short, 1024 are two full tasks and no partial one, 1025 end in a task of one entry."""
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    n, s, t = last_task_edges(entries)
    vid = (np.arange(n, dtype=np.int64) + 1) << 8
    init = np.random.default_rng(entries).integers(-(1 << 39), 1 << 39, n)
    want_pr, _ = oracle_lib.pagerank(n, s, t, 0.85, n, 12)
    ctx = g = None
    ranks = {}
    try:
        for k, v in (("band0_deg", 2), ("band0_sub", 1), ("band1_deg", 0)):
            _lib.tune_set(k, v)
        ctx = jg.Context((0,))
        g = ctx.build(vid, vid[s], vid[t], flags=jg.ADJ_IN | jg.ADJ_OUT | jg.ADJ_BOTH)
        assert g.info()["num_edges"] == len(s)
        for hot in (-1, 0):
            _lib.tune_set("merge_hot", hot)
            for steps in (1, 3):
                want, wrec = oracle_lib.combine_steps(n, s, t, 2, 0, steps, init, False)  # DIR_IN, COMBINE_SUM
                x, rec = g.combine_steps(2, 0, steps, init, False)
                np.testing.assert_array_equal(rec, wrec, err_msg=f"merge_hot {hot} steps {steps}")
                np.testing.assert_array_equal(x, want, err_msg=f"merge_hot {hot} steps {steps}")
            ranks[hot], _ = g.pagerank(0.85, n, 12)
            rel = np.abs(ranks[hot] - want_pr) / np.maximum(np.abs(want_pr), 1e-300)
            assert rel.max() <= PR_RTOL, f"merge_hot {hot}: max rel err {rel.max()}"
    finally:
        if g is not None:
            g.close()
        if ctx is not None:
            ctx.close()
        restore()
    np.testing.assert_array_equal(bits(ranks[0]), bits(ranks[-1]), err_msg="no image vs automatic")
