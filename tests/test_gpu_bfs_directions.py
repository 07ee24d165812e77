"""The level control of the two direction-optimising BFS engines (csrc/jg_traverse.hip: bfs_decide,
bfs_level_kernel, bfs_td_claim_kernel under dobfs_single; sbfs_decide and the sbfs_pre / mid / post / copy
kernels under dobfs_sharded) under every direction sequence, exactly against the oracle.  The RMAT graphs
of the other files all tell one story (two top-down levels, two or three bottom-up ones, a top-down tail,
one batch); the graphs here are made so that the thresholds, and the four settings of them below, give
the others.

D, the dumbbell (n = 3179 = 49 * 64 + 43): a blob of 1024 vertices and 8192 distinct random edges, a
directed path of 70 vertices from the blob's last vertex into a blob of 2048 vertices and 16384 edges, and
37 isolated vertices; 3142 = 49 * 64 + 6 vertices have an edge, so both `rows` and `bu_rows` end inside a
64-row word.  No self-loop, duplicate or reciprocal pair (a BOTH degree is in-degree + out-degree), random
orientation inside the blobs, shuffled sparse vertex ids.  From either blob at the default thresholds the
directions are T2 B2 T72 B2 T1: two bottom-up runs of two levels (the first level after a switch probes
depth == level, the second the bitmap of the other parity, which the older run wrote last), 79 levels
(batches of 10, 4, 8, 16, 32 and 64: the 4-slot ring wraps about 20 times).

P, the probe ladder (BOTH only): for every pull-row length d in PROBE_DS and both places, a row at depth
>= 2 whose only neighbour in the previous layer sorts first, or last, among its d columns; the other d - 1
are its children.  This assumes what the build does with a BOTH-only graph: vertices are relabelled by
BOTH degree, descending (ties by hottest neighbour, then id), and a row's columns ascend in that order.
The parent's degree differs from every child's (leaves hung on parents and children separate them: a
"first" parent has degree 10, a "last" parent 2, every child 5), so no tie decides its place.  With every
level bottom-up such a row is scanned to its end without a hit on each level before its parent's.

MODES sets (alpha, beta): the defaults; every level bottom-up; alternating B T B T ...; and (1, 1), a
single bottom-up level at the peak.  `directions` restates the rule (bfs_decide, sbfs_decide) from the
oracle's depths; the value tests take the level count, the edge sum and the bounded runs' max_depth from
it, and the two dump tests (JG_DEBUG_BFS=1, read once per process: a child process per engine) assert the
direction of every level the engines really ran, and for the single-shard engine the next frontier's
vertex and edge counts: if the thresholds or the rule move, those tests fail instead of the value tests
going blind.  The unmarked tests check the generators and the restatement with numpy alone.

Every comparison is exact and against the oracle (oracle.bfs, connected_components, shortest_distance).
"""
import contextlib
import functools
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADJ_OUT, ADJ_IN, ADJ_BOTH = 1, 2, 4
DIR_OUT, DIR_IN, DIR_BOTH = 1, 2, 3

# the knobs this file moves, with the library's defaults (every test puts them back)
DEFAULTS = {"dobfs_alpha": 30, "bfs_alpha": 14, "bfs_beta": 24, "bfs_td_split": 2, "bfs_td_split_min": 65536,
            "bfs_batch0": 10, "bfs_tail_grid": 64, "halo": 1}
MODES = {"default": (30, 24), "bottom_up": (10**6, 10**6), "alternate": (10**6, 1), "ones": (1, 1)}
PROBE_DS = (1, 2, 4, 5, 6, 8, 9, 10, 13)  # the first column alone, then batches of kBuBatch = 4 with a clamped tail
BLOB_A, PATH, BLOB_B, ISOLATED = 1024, 70, 2048, 37
SHARD_COUNTS = (2, 3, 8)  # logical shards on one device, over the halo plan


# ---------------- generators (numpy alone) ----------------
def blob_edges(rng, n, m):
    """m distinct unordered pairs of [0, n), each with a random orientation."""
    a, b = rng.integers(0, n, 3 * m), rng.integers(0, n, 3 * m)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    _, first = np.unique(np.where(lo < hi, lo * n + hi, -1), return_index=True)
    pick = np.sort(first[1:])[:m]  # (first[0]: the self-loops' code)
    assert len(pick) == m
    flip = rng.random(m) < 0.5
    return np.where(flip, hi[pick], lo[pick]), np.where(flip, lo[pick], hi[pick])


def finish(name, rng, n, src, dst, sources):
    """Shuffles the vertices, gives them sparse ids and shuffles the edges."""
    perm = rng.permutation(n)
    vid = (rng.choice(1 << 20, n, replace=False).astype(np.int64) + 1) << 8
    e = rng.permutation(len(src))
    s = np.ascontiguousarray(perm[np.asarray(src)][e], np.int32)
    t = np.ascontiguousarray(perm[np.asarray(dst)][e], np.int32)
    for a in (vid, s, t):
        a.setflags(write=False)
    return types.SimpleNamespace(name=name, n=n, vid=vid, s=s, t=t, perm=perm,
                                 sources={k: int(perm[v]) for k, v in sources.items()})


@functools.lru_cache(maxsize=None)
def dumbbell():
    rng = np.random.default_rng(3)  # (a seed and sources that keep test_dumbbell_* true)
    sa, ta = blob_edges(rng, BLOB_A, 8192)
    sb, tb = blob_edges(rng, BLOB_B, 16384)
    b0 = BLOB_A + PATH
    chain = np.arange(BLOB_A - 1, b0 + 1)  # the blob's last vertex, the path, the second blob's first
    src = np.concatenate([sa, chain[:-1], sb + b0])
    dst = np.concatenate([ta, chain[1:], tb + b0])
    n = BLOB_A + PATH + BLOB_B + ISOLATED
    return finish("D", rng, n, src, dst, {"a": 5, "b": b0 + 4, "iso": n - 3})


@functools.lru_cache(maxsize=None)
def probe_ladder():
    """Edges point away from the root (source "a"); source "b" is a leaf under the deepest row."""
    rng = np.random.default_rng(11)
    src, dst = [], []

    def child(parent, count=1):
        first = len(dst) + 1  # a tree: every vertex but the root is the target of one edge
        src.extend([parent] * count)
        dst.extend(range(first, first + count))
        return first

    spine = [0, child(0)]
    spine.append(child(spine[1]))
    rows, leaf = {}, None
    for k, (d, place) in enumerate((d, place) for d in PROBE_DS for place in ("first", "last")):
        parent = child(spine[k % 3])
        if place == "first":
            child(parent, 8)  # degree 10: above every child's 5
        row = child(parent)
        rows[(d, place)] = row
        for _ in range(d - 1):
            leaf = child(child(row), 4)  # a child of degree 5: the row and 4 leaves
    n = len(dst) + 1 + 5  # and five isolated vertices
    g = finish("P", rng, n, src, dst, {"a": 0, "b": leaf, "iso": n - 2})
    g.rows = {k: int(g.perm[v]) for k, v in rows.items()}
    return g


GRAPHS = {"D": dumbbell, "P": probe_ladder}


def np_bfs(g, source, direction):
    """Depths by numpy (the generators' tests; the GPU tests take the oracle's)."""
    key, other = {DIR_OUT: (g.s, g.t), DIR_IN: (g.t, g.s),
                  DIR_BOTH: (np.concatenate([g.s, g.t]), np.concatenate([g.t, g.s]))}[direction]
    depth = np.full(g.n, -1, np.int32)
    depth[source] = 0
    level = 0
    while True:
        cand = other[depth[key] == level]
        cand = cand[depth[cand] < 0]
        if len(cand) == 0:
            return depth
        level += 1
        depth[cand] = level


def degrees(g, which):
    """The degree of the adjacency the frontier counts come from."""
    out, inn = np.bincount(g.s, minlength=g.n), np.bincount(g.t, minlength=g.n)
    return {"out": out, "in": inn, "both": out + inn}[which]


# ---------------- the direction rule, restated ----------------
def directions(depth, deg, rows, alpha, beta, max_depth=-1, push=True, pull=True):
    """(dirs, levels, edges, nexts): the direction of every level run ("T" / "B"), the level count, the
    degree sum of every frontier, and (vertices, degree sum) of the frontier each level leaves behind."""
    mu, edges, bottom_up, dirs, nexts, level = int(deg.sum()), 0, False, [], [], 0
    while True:
        at = depth == level
        nf, mf = int(at.sum()), int(deg[at].sum())
        mu -= mf
        edges += mf
        if dirs:
            nexts.append((nf, mf))
        if nf == 0 or (max_depth >= 0 and level >= max_depth):
            return dirs, level, edges, nexts
        if not bottom_up and pull and (not push or mf > mu / alpha):
            bottom_up = True
        elif bottom_up and push and nf < rows / beta:
            bottom_up = False
        dirs.append("B" if bottom_up else "T")
        level += 1


def runs(dirs):
    out = []
    for d in dirs:
        if out and out[-1][0] == d:
            out[-1][1] += 1
        else:
            out.append([d, 1])
    return [(d, k) for d, k in out]


def binding_depths(dirs):
    """max_depth values at which the last level run is bottom-up (and the one stopped would have been,
    where the sequence has such a place): the first and the last of them; and the same for top-down."""
    out = []
    for x in "BT":
        at = [L for L in range(1, len(dirs) + 1) if dirs[L - 1] == x]
        both = [L for L in at if L < len(dirs) and dirs[L] == x]
        if at:
            out += [(both or at)[0], (both or at)[-1]]
    return sorted(set(out))


# ---------------- the generators' premises (no GPU) ----------------
def test_directions_by_hand():
    # a path 0 - 1 - 2 - 3 - 4 from its end: frontiers of one vertex, degree sums 1 2 2 2 1, mu 7 5 3 1 0
    depth, deg = np.arange(5), np.array([1, 2, 2, 2, 1])
    assert directions(depth, deg, 5, 1, 24)[:3] == (list("TTTBB"), 5, 8)  # 2 > 1 / 1, then 1 < 5 / 24 is false ...
    assert directions(depth, deg, 5, 1, 4)[0] == list("TTTBT")            # ... but 1 < 5 / 4 is true
    assert directions(depth, deg, 5, 1, 24)[3] == [(1, 2), (1, 2), (1, 2), (1, 1), (0, 0)]
    assert directions(depth, deg, 5, 2, 24)[0] == list("TTBBB")  # 2 > 3 / 2 a level sooner
    assert directions(depth, deg, 5, 30, 24)[0] == list("BBBBB")  # 1 > 7 / 30 at once
    assert directions(depth, deg, 5, 1, 4, push=False)[0] == list("BBBBB")
    assert directions(depth, deg, 5, 10**6, 1, pull=False)[0] == list("TTTTT")
    assert directions(depth, deg, 5, 10**6, 1)[0] == list("BTBTB")
    assert directions(depth, deg, 5, 1, 24, max_depth=2)[:3] == (list("TT"), 2, 5)
    assert directions(depth, deg, 5, 1, 24, max_depth=2)[3] == [(1, 2), (1, 2)]
    assert directions(depth, deg, 5, 1, 24, max_depth=4)[:3] == (list("TTTB"), 4, 8)
    assert directions(depth, deg, 5, 1, 24, max_depth=0)[:3] == ([], 0, 1)
    assert runs(list("TTBBT")) == [("T", 2), ("B", 2), ("T", 1)]
    assert binding_depths(list("TTBBT")) == [1, 3] and binding_depths(list("BBB")) == [1, 2]
    assert binding_depths(list("BTBT")) == [1, 2, 3, 4] and binding_depths(list("TTBBTTTBBT")) == [1, 3, 6, 8]


def test_dumbbell_generator():
    g = dumbbell()
    assert g.n == 3179 == 49 * 64 + 43 and len(g.s) == 8192 + 71 + 16384
    assert g.s.dtype == np.int32 and min(g.s.min(), g.t.min()) >= 0 and max(g.s.max(), g.t.max()) < g.n
    assert (g.s != g.t).all()
    lo, hi = np.minimum(g.s, g.t).astype(np.int64), np.maximum(g.s, g.t).astype(np.int64)
    assert len(np.unique(lo * g.n + hi)) == len(g.s)  # no duplicate and no reciprocal pair
    out, inn = degrees(g, "out"), degrees(g, "in")
    assert int(((out + inn) > 0).sum()) == 3142 == 49 * 64 + 6
    assert ((inn > 0) & (out == 0)).any() and ((out > 0) & (inn == 0)).any()  # empty pull rows before the suffix
    assert len(np.unique(g.vid)) == g.n and (np.diff(g.vid) < 0).any() and g.vid.min() > 0
    # random orientation inside the blobs: neither end of an edge is always the smaller vertex
    assert 0.4 < (g.s < g.t).mean() < 0.6
    for k in ("a", "b"):
        assert out[g.sources[k]] + inn[g.sources[k]] > 0
    assert out[g.sources["iso"]] + inn[g.sources["iso"]] == 0


@pytest.mark.parametrize("source", ["a", "b"])
def test_dumbbell_sequences(source):
    g = dumbbell()
    depth, deg = np_bfs(g, g.sources[source], DIR_BOTH), degrees(g, "both")
    assert int((depth >= 0).sum()) == 3142

    def seq(mode):
        return directions(depth, deg, g.n, *MODES[mode])

    dirs, levels, edges, _ = seq("default")
    assert runs(dirs) == [("T", 2), ("B", 2), ("T", 72), ("B", 2), ("T", 1)]
    assert levels == len(dirs) == 79 and edges == 2 * len(g.s)  # past 10 + 4 + 8 + 16 + 32: the sixth batch
    assert seq("bottom_up")[0] == ["B"] * 79
    assert seq("alternate")[0] == list("BT" * 40)[:79]
    ones = seq("ones")[0]
    assert "B" in ones and "T" in ones
    for mode in MODES:  # the bounded runs bind on both kinds of level wherever the sequence has both
        d = seq(mode)[0]
        assert {d[L - 1] for L in binding_depths(d)} == set(d)
    assert binding_depths(dirs) == [1, 3, 75, 77]  # the second bottom-up run is in the sixth batch


def test_dumbbell_directed_sequences():
    """The directed traversals also leave top-down: over OUT from the first blob, over IN from the second."""
    g = dumbbell()
    for direction, source, which in ((DIR_OUT, "a", "out"), (DIR_IN, "b", "in")):
        depth = np_bfs(g, g.sources[source], direction)
        dirs = directions(depth, degrees(g, which), g.n, *MODES["default"])[0]
        assert len(dirs) >= 79 and len(runs(dirs)) >= 4, runs(dirs)


def test_probe_ladder_generator():
    g = probe_ladder()
    assert g.n <= 4000 and len(np.unique(g.vid)) == g.n
    deg, depth = degrees(g, "both"), np_bfs(g, g.sources["a"], DIR_BOTH)
    assert int((depth >= 0).sum()) == g.n - 5 and depth[g.sources["b"]] == depth.max()
    nbrs = {v: [] for v in range(g.n)}
    for a, b in zip(g.s.tolist(), g.t.tolist()):
        nbrs[a].append(b)
        nbrs[b].append(a)
    seen = set()
    for (d, place), v in g.rows.items():
        assert deg[v] == d == len(set(nbrs[v])) and depth[v] >= 2  # scanned to its end on the levels before
        up = [u for u in nbrs[v] if depth[u] == depth[v] - 1]
        rest = [u for u in nbrs[v] if depth[u] != depth[v] - 1]
        assert len(up) == 1 and all(depth[u] == depth[v] + 1 for u in rest)
        if place == "first":
            assert all(deg[up[0]] > deg[u] for u in rest)
        else:
            assert all(deg[up[0]] < deg[u] for u in rest)
        seen.add((d, place))
    assert seen == {(d, place) for d in PROBE_DS for place in ("first", "last")}
    assert {int(depth[v]) for v in g.rows.values()} == {2, 3, 4}


# ---------------- GPU ----------------
_REF = {}  # oracle results, computed once per graph and traversal


def ref(key, fn):
    if key not in _REF:
        out = fn()
        for a in out if isinstance(out, tuple) else (out,):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


@contextlib.contextmanager
def knobs(**kw):
    from janusgraph_amd import _lib
    try:
        for k, v in kw.items():
            _lib.tune_set(k, v)
        yield
    finally:
        for k in kw:
            _lib.tune_set(k, DEFAULTS[k])


@contextlib.contextmanager
def built(g, flags, shards=1):
    import janusgraph_amd as jg
    ctx = h = None
    try:
        with knobs(halo=1):
            ctx = jg.Context((0,) * shards)
            h = ctx.build(g.vid, g.vid[g.s], g.vid[g.t], flags=flags)
        assert h.info()["num_shards"] == shards
        yield ctx, h
    finally:
        if h is not None:
            h.close()
        if ctx is not None:
            ctx.close()


# the builds of one shard: flags, and per traversal (direction, source, the frontier counts' degree, push, pull)
BUILDS = {
    "both": (ADJ_BOTH, [(DIR_BOTH, "a", "both", True, True), (DIR_BOTH, "b", "both", True, True),
                        (DIR_BOTH, "iso", "both", True, True)]),
    "inout": (ADJ_IN | ADJ_OUT, [(DIR_OUT, "a", "out", True, True), (DIR_IN, "b", "in", True, True),
                                 (DIR_OUT, "b", "out", True, True), (DIR_IN, "a", "in", True, True)]),
    "push_only": (ADJ_OUT, [(DIR_OUT, "a", "out", True, False)]),
    "pull_only": (ADJ_IN, [(DIR_OUT, "a", "in", False, True)]),  # bottom-up from level 0
}


def single_runs(g, build, mode, oracle=None):
    """(direction, source vertex, max_depth, restatement) of every traversal of one build and mode: each
    unbounded, and the BOTH ones from a blob bounded where max_depth binds (binding_depths)."""
    alpha, beta = MODES[mode]
    out = []
    for direction, source, which, push, pull in BUILDS[build][1]:
        v = g.sources[source]
        depth = (ref((g.name, "bfs", direction, v), lambda: oracle.bfs(g.n, g.s, g.t, v, direction))
                 if oracle else ref((g.name, "np_bfs", direction, v), lambda: np_bfs(g, v, direction)))
        free = directions(depth, degrees(g, which), g.n, alpha, beta, -1, push, pull)
        out.append((direction, v, -1, free))
        if build == "both" and source != "iso":
            for md in binding_depths(free[0]):
                out.append((direction, v, md, directions(depth, degrees(g, which), g.n, alpha, beta, md, push, pull)))
    return out


def check_traversal(oracle, ctx, h, g, direction, v, max_depth, want):
    """Depths against the oracle's; levels and edges against the restatement's."""
    _, levels, edges, _ = want
    depth = ref((g.name, "bfs", direction, v, max_depth), lambda: oracle.bfs(g.n, g.s, g.t, v, direction, max_depth))
    msg = f"{g.name} direction {direction} source {v} max_depth {max_depth}"
    np.testing.assert_array_equal(h.bfs([g.vid[v]], direction, max_depth)[0], depth, err_msg=msg)
    st = ctx.stats()
    assert st["levels"] == levels, msg
    assert st["edges_traversed"] == (edges / 2 if direction == DIR_BOTH else edges), msg


@gpu
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_single_shard_values(oracle_lib, graph, build, mode, split):
    g = GRAPHS[graph]()
    alpha, beta = MODES[mode]
    with built(g, BUILDS[build][0]) as (ctx, h):
        with knobs(dobfs_alpha=alpha, bfs_beta=beta, bfs_td_split=split, bfs_td_split_min=1):
            for direction, v, max_depth, want in single_runs(g, build, mode, oracle_lib):
                check_traversal(oracle_lib, ctx, h, g, direction, v, max_depth, want)


@gpu
@pytest.mark.parametrize("mode", ["default", "alternate"])
def test_single_shard_tail_grid_and_batches_of_one(oracle_lib, mode):
    """bfs_batch0 1 (batches of 1, 4, 8, ...: the bottom-up runs fall into other batches) and bfs_tail_grid 1
    after two traversals of one level: every level from 1 on runs on one workgroup, both directions."""
    g = dumbbell()
    alpha, beta = MODES[mode]
    with built(g, ADJ_BOTH) as (ctx, h):
        with knobs(dobfs_alpha=alpha, bfs_beta=beta, bfs_batch0=1, bfs_tail_grid=1):
            runs_ = single_runs(g, "both", mode, oracle_lib)
            iso = [r for r in runs_ if r[1] == g.sources["iso"]]
            for r in iso + iso + [r for r in runs_ if r[2] < 0]:
                check_traversal(oracle_lib, ctx, h, g, *r)


@gpu
@pytest.mark.parametrize("shards", (1,) + SHARD_COUNTS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_connected_components(oracle_lib, graph, mode, shards):
    """The root-eccentricity pass of CC runs on the same engines (bfs_alpha is its threshold)."""
    g = GRAPHS[graph]()
    want, want_it = ref((g.name, "cc"), lambda: oracle_lib.connected_components(g.n, g.s, g.t, g.vid))
    alpha, beta = MODES[mode]
    with built(g, ADJ_IN | ADJ_OUT | ADJ_BOTH, shards) as (ctx, h):
        with knobs(bfs_alpha=alpha, bfs_beta=beta):
            comp, it = h.connected_components()
    np.testing.assert_array_equal(comp, want)
    assert it == want_it


@gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_unit_shortest_distance_bounded(oracle_lib, mode):
    """Unit-weight ShortestDistance is a traversal over IN (pull: OUT); max_depth stops it inside the path
    and, from the other side, inside the first blob."""
    g = dumbbell()
    alpha, beta = MODES[mode]
    with built(g, ADJ_IN | ADJ_OUT) as (ctx, h):
        with knobs(dobfs_alpha=alpha, bfs_beta=beta):
            for source, max_depth in (("b", 40), ("b", 3), ("a", 2), ("b", 200)):
                v = g.sources[source]
                want = ref((g.name, "sd", v, max_depth), lambda: oracle_lib.shortest_distance(g.n, g.s, g.t, v, max_depth))
                np.testing.assert_array_equal(h.shortest_distance(g.vid[v], max_depth), want,
                                              err_msg=f"source {source} max_depth {max_depth}")


def sharded_runs(g, mode, oracle=None):
    """As single_runs for the sharded engine (BOTH): from both blobs, bounded, and from the empty suffix."""
    return single_runs(g, "both", mode, oracle)


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shards", SHARD_COUNTS)
def test_sharded_values(oracle_lib, shards, mode):
    g = dumbbell()
    alpha, beta = MODES[mode]
    with built(g, ADJ_IN | ADJ_OUT | ADJ_BOTH, shards) as (ctx, h):
        with knobs(dobfs_alpha=alpha, bfs_beta=beta):
            for direction, v, max_depth, want in sharded_runs(g, mode, oracle_lib):
                check_traversal(oracle_lib, ctx, h, g, direction, v, max_depth, want)


@gpu
@pytest.mark.parametrize("shards", SHARD_COUNTS)
def test_sharded_back_to_back(oracle_lib, shards):
    """Two traversals on one graph, the first alternating, the second at the defaults (then all bottom-up and
    alternating again from the other blob): stale stamps, send-list words or frontier bitmaps would show."""
    g = dumbbell()
    with built(g, ADJ_IN | ADJ_OUT | ADJ_BOTH, shards) as (ctx, h):
        for mode, source in (("alternate", "a"), ("default", "b"), ("bottom_up", "a"), ("alternate", "b"), ("ones", "a")):
            alpha, beta = MODES[mode]
            with knobs(dobfs_alpha=alpha, bfs_beta=beta):
                for direction, v, max_depth, want in sharded_runs(g, mode, oracle_lib):
                    if v == g.sources[source] and max_depth < 0:
                        check_traversal(oracle_lib, ctx, h, g, direction, v, max_depth, want)


# ---------------- the directions really taken ----------------
def dump_child(engine):
    """Runs in a child process with JG_DEBUG_BFS=1: the traversals of the value tests on D, a marker line
    before each."""
    g = dumbbell()

    def mark(*words):
        sys.stderr.write("[case] " + " ".join(str(w) for w in words) + "\n")
        sys.stderr.flush()

    if engine == "single":
        for build in BUILDS:
            with built(g, BUILDS[build][0]) as (ctx, h):
                for mode, (alpha, beta) in MODES.items():
                    for split in (0, 1):
                        with knobs(dobfs_alpha=alpha, bfs_beta=beta, bfs_td_split=split, bfs_td_split_min=1):
                            for k, (direction, v, max_depth, _) in enumerate(single_runs(g, build, mode)):
                                mark(build, mode, split, k)
                                h.bfs([g.vid[v]], direction, max_depth, want=False)
    else:
        for shards in SHARD_COUNTS:
            with built(g, ADJ_IN | ADJ_OUT | ADJ_BOTH, shards) as (ctx, h):
                for mode, (alpha, beta) in MODES.items():
                    with knobs(dobfs_alpha=alpha, bfs_beta=beta):
                        for k, (direction, v, max_depth, _) in enumerate(sharded_runs(g, mode)):
                            mark(shards, mode, 0, k)
                            h.bfs([g.vid[v]], direction, max_depth, want=False)


def dump_of(engine):
    """{case: [(level, "T" / "B", done, vertices, edges)]} of the child's per-level lines."""
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), engine],
                       env={**os.environ, "JG_DEBUG_BFS": "1"}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    tag = {"single": "bfs", "sharded": "sbfs"}[engine]
    other = {"single": "sbfs", "sharded": "bfs"}[engine]
    cases, lines = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("[case] "):
            lines = cases.setdefault(tuple(line.split()[1:]), [])
        assert not line.startswith(f"[jg {other}] "), line  # the other engine took the traversal
        m = re.match(rf"\[jg {tag}\] level (\d+) (top-down|bottom-up) done (\d) (?:shard-0 )?next frontier (\d+) vertices "
                     r"(\d+) (?:edges|entries)$", line)
        if m:
            lines.append((int(m.group(1)), "B" if m.group(2) == "bottom-up" else "T", int(m.group(3)),
                          int(m.group(4)), int(m.group(5))))
    return cases


def check_dump(lines, want, counts, msg):
    dirs, levels, _, nexts = want
    assert [x[0] for x in lines] == list(range(len(lines))), msg  # every level enqueued, once
    ran = [x for x in lines if not x[2]]
    assert ran == lines[:len(ran)] and len(lines) > len(ran), msg  # then the level that stops, and no-ops
    assert [x[1] for x in ran] == dirs, f"{msg}: ran {runs([x[1] for x in ran])}, restated {runs(dirs)}"
    assert len(ran) == levels, msg
    if counts:
        assert [x[3:] for x in ran] == nexts[:len(ran)], msg


@gpu
def test_single_shard_directions_taken(oracle_lib):
    g = dumbbell()
    cases = dump_of("single")
    checked = 0
    for build in BUILDS:
        for mode in MODES:
            for split in (0, 1):
                for k, (direction, v, max_depth, want) in enumerate(single_runs(g, build, mode, oracle_lib)):
                    check_dump(cases[(build, mode, str(split), str(k))], want, True,
                               f"{build} {mode} split {split} direction {direction} source {v} max_depth {max_depth}")
                    checked += 1
    assert checked == len(cases) >= 4 * 2 * (3 + 4 + 1 + 1)
    # what the graph is for: at the defaults both blobs give two bottom-up runs of two levels, 79 levels in all
    for k in (0, 1 + len(binding_depths(single_runs(g, "both", "default", oracle_lib)[0][3][0]))):
        ran = [x[1] for x in cases[("both", "default", "0", str(k))] if not x[2]]
        assert runs(ran) == [("T", 2), ("B", 2), ("T", 72), ("B", 2), ("T", 1)]
    pull_only = [x[1] for x in cases[("pull_only", "default", "0", "0")] if not x[2]]
    assert pull_only and set(pull_only) == {"B"}


@gpu
def test_sharded_directions_taken(oracle_lib):
    g = dumbbell()
    cases = dump_of("sharded")
    checked = 0
    for shards in SHARD_COUNTS:
        for mode in MODES:
            for k, (direction, v, max_depth, want) in enumerate(sharded_runs(g, mode, oracle_lib)):
                check_dump(cases[(str(shards), mode, "0", str(k))], want, False,
                           f"{shards} shards {mode} source {v} max_depth {max_depth}")
                checked += 1
    assert checked == len(cases) >= 3 * 4 * 3


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    dump_child(sys.argv[1])
