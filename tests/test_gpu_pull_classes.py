"""The pull engine's lane classes, hub chunks and degree runs (csrc/jg_pull.h: pull_rows_class,
fold_strided, fold_short, pull_block's chunk path, pull_hub_finalize_kernel; csrc/jg_build.hip:
build_pull_plan) on hand-made graphs, exactly against the oracle.  The merge half of the engine has
test_gpu_merge_fold.py and test_gpu_merge_gather.py; this file is the other half.

Every graph has 16384 vertices and about 100k edges.

L, the ladder.  One row per in-degree around every threshold of the engine (LADDER: the class
thresholds 256/128/64/32/16/8/1, fold_short's 8, the band floors 96 and 8, fold_strided's batches of 4 L,
the hub degree 8192, the hub chunk 4096 and its 1024-entry batches) and, per lane class, one row more
than a 256-thread block takes (EXTRA), at random vertices with uniform sources, multi-edges and four
self-loops.  Built as the IN adjacency alone and, transposed, as the OUT adjacency alone (the OUT plan is
then the degree-sorted one), with pull_split 0 (every class runs) and 1 (rows of degree >= 8 go to the
bands; the light rows are addressed by degree run).

U, unsorted adjacencies.  20 actors of in-degree 2000, 1999, ..., 1981 (rows 0..19 of an IN|OUT|BOTH
graph, which is sorted by in-degree) whose out-degrees are ACTOR_OUT in row order; all other edges'
ends are fillers of in-degree <= 20.  The OUT plan is cut from that unsorted order: bands [0,3) and
[3,4), a hub inside the split and three past it, rows of 8191 and 4096 entries folded by one lane, empty
rows in the middle of the 1-lane class, no degree runs.  U0 rotates ACTOR_OUT so that row 0 is empty:
no split rows with the split on.

R, degree runs.  IN alone, default knobs: one row of degree 100, ten of degree 20, then light rows of
the degrees in the parameter (300 rows of the highest degree, 5 of each one between, 257 of the lowest;
a single degree has 300), then 50 rows without in-edges that are sources, then isolated vertices.
Every second light vertex has no out-edge (the relabel orders those last inside a degree).

One test per family reads the plan dump (JG_DEBUG_PLAN=1, read once per process: a child process) and
asserts that the graph lands in the classes, chunks, bands and runs claimed above, from the
thresholds written down here: if the engine's move, those tests fail instead of the value tests going
blind.  The unmarked tests check the generators with numpy alone.

Integer programs are compared exactly, with initial values from +-2^39 (a duplicated or dropped term
cannot cancel); PageRank to the project's bound, PR_RTOL.
"""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu

PR_RTOL = 1e-9  # north_star: per-vertex relative error <= 1e-9 (fp64)
N = 16384
VID = (np.arange(N, dtype=np.int64) + 1) << 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the engine's constants as this file's graphs assume them (the plan tests compare with the dump)
CLASS_THR = (256, 128, 64, 32, 16, 8, 1)  # lane classes 1..7: 64 >> (c - 1) lanes per row
HUB_DEGREE, HUB_CHUNK, BLOCK, RUN_MAX = 8192, 4096, 256, 7
BAND_FLOORS = (96, 8)  # the default bands of an 8-byte vector on one shard

LADDER = (list(range(10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257,
                             511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 9215, 9216, 9217, 12288, 12289])
EXTRA = ((257, 7), (129, 8), (65, 16), (33, 32), (17, 64), (9, 128), (5, 256))  # (rows, degree)
ACTORS = 20
ACTOR_OUT = [9000, 100, 96, 8, 7, 8193, 0, 8, 9, 1, 4096, 12289, 3, 0, 8192, 300, 2, 8191, 0, 5]
RUN_SETS = [(7,), (1,), (3, 1), (7, 1), (6, 5, 2), (7, 6, 5, 4, 3, 2, 1)]
RUN_IDS = ["".join(map(str, p)) for p in RUN_SETS]


# ---------------- generators (numpy alone) ----------------
def ladder_degrees():
    return np.array(LADDER + [d for rows, d in EXTRA for _ in range(rows)], np.int64)


def shuffled(rng, src, dst):
    p = rng.permutation(len(src))
    return np.ascontiguousarray(src[p], np.int32), np.ascontiguousarray(dst[p], np.int32)


def ladder_edges():
    """(src, dst) with the ladder on the in-degrees."""
    rng = np.random.default_rng(31)
    degs = ladder_degrees()
    deg = np.zeros(N, np.int64)
    special = rng.permutation(N)[:len(degs)]
    deg[special] = degs
    dst = np.repeat(np.arange(N), deg)
    src = rng.integers(0, N, len(dst))
    first = np.cumsum(deg) - deg
    for d in (1, 9, 64, 8192):  # a self-loop in a short row, a strided one, a 64-lane one and a hub
        v = special[list(degs).index(d)]
        src[first[v]] = v
    return shuffled(rng, src, dst)


def actor_out_degrees(variant):
    rot = {"U": 0, "U0": ACTOR_OUT.index(0)}[variant]
    return ACTOR_OUT[rot:] + ACTOR_OUT[:rot]


def actor_edges(variant):
    """(src, dst, actors): actor k has in-degree 2000 - k and out-degree actor_out_degrees()[k]."""
    rng = np.random.default_rng(41)
    perm = rng.permutation(N)
    actors, fillers = perm[:ACTORS], perm[ACTORS:]
    src, dst = [], []
    for k, od in enumerate(actor_out_degrees(variant)):
        a = np.int64(actors[k])
        fr = rng.choice(fillers, 2000 - k, replace=False)
        to = rng.choice(fillers, od, replace=False)
        src += [fr, np.full(od, a)]
        dst += [np.full(2000 - k, a), to]
    s, t = shuffled(rng, np.concatenate(src), np.concatenate(dst))
    return s, t, actors


def run_counts(present):
    ds = sorted(present, reverse=True)
    counts = {d: 5 for d in ds}
    if len(ds) > 1:
        counts[ds[-1]] = 257
    counts[ds[0]] = 300
    return counts


def run_edges(present):
    """(src, dst, light, dead): `light` the light rows' vertices, `dead` those of them without out-edges."""
    rng = np.random.default_rng(sum(1 << d for d in present))
    counts = run_counts(present)
    light_deg = np.concatenate([np.full(c, d) for d, c in counts.items()])
    perm = rng.permutation(N)
    heavy, light = perm[:11], perm[11:11 + len(light_deg)]
    sources50 = perm[11 + len(light_deg):11 + len(light_deg) + 50]
    dead = np.zeros(len(light), bool)
    for d in counts:  # every second row of each degree
        dead[np.flatnonzero(light_deg == d)[::2]] = True
    deg = np.zeros(N, np.int64)
    deg[heavy] = [100] + [20] * 10
    deg[light] = light_deg
    pool = np.concatenate([heavy, light[~dead], sources50])
    dst = np.repeat(np.arange(N), deg)
    src = np.concatenate([pool, rng.choice(pool, len(dst) - len(pool))])  # every pool vertex sends
    src = src[rng.permutation(len(src))]
    s, t = shuffled(rng, src, dst)
    return s, t, light, light[dead]


# ---------------- the generators' premises (no GPU) ----------------
def in_range(*arrays):
    return all(a.dtype == np.int32 and a.min() >= 0 and a.max() < N for a in arrays)


def test_ladder_generator():
    s, t = ladder_edges()
    assert in_range(s, t) and len(s) <= 150000
    indeg = np.bincount(t, minlength=N)
    want = np.zeros(N, np.int64)
    want[:len(ladder_degrees())] = ladder_degrees()
    np.testing.assert_array_equal(np.sort(indeg), np.sort(want))
    assert len(ladder_degrees()) == len(LADDER) + 515
    assert (s == t).sum() >= 4  # self-loops
    pairs = s.astype(np.int64) * N + t
    assert len(np.unique(pairs)) < len(pairs)  # multi-edges


@pytest.mark.parametrize("variant", ["U", "U0"])
def test_actor_generator(variant):
    s, t, actors = actor_edges(variant)
    assert in_range(s, t) and len(s) == 90310
    indeg, outdeg = np.bincount(t, minlength=N), np.bincount(s, minlength=N)
    np.testing.assert_array_equal(indeg[actors], 2000 - np.arange(ACTORS))
    np.testing.assert_array_equal(outdeg[actors], actor_out_degrees(variant))
    filler = np.ones(N, bool)
    filler[actors] = False
    assert indeg[filler].max() <= ACTORS < indeg[actors].min()
    # every edge joins an actor and a filler, and an actor's edges of one direction have distinct fillers
    assert len(np.unique(s.astype(np.int64) * N + t)) == len(s)
    assert (filler[s] ^ filler[t]).all()
    assert actor_out_degrees("U0")[0] == 0 and sorted(actor_out_degrees("U0")) == sorted(ACTOR_OUT)


@pytest.mark.parametrize("present", RUN_SETS, ids=RUN_IDS)
def test_run_generator(present):
    s, t, light, dead = run_edges(present)
    assert in_range(s, t)
    indeg, outdeg = np.bincount(t, minlength=N), np.bincount(s, minlength=N)
    counts = run_counts(present)
    assert sorted(counts) == sorted(present) and (len(present) == 1 or counts[min(present)] == 257)
    got = np.bincount(indeg)
    assert got[100] == 1 and got[20] == 10
    for d in range(1, 20):
        assert got[d] == counts.get(d, 0), d
    assert sorted(indeg[light]) == sorted(d for d, c in counts.items() for _ in range(c))
    assert ((indeg == 0) & (outdeg > 0)).sum() == 50
    live = np.setdiff1d(light, dead)
    assert (outdeg[dead] == 0).all() and (outdeg[live] > 0).all()
    for d in present:  # both kinds inside every degree: the tie-break has something to reorder
        assert abs(int((indeg[dead] == d).sum()) - int((indeg[live] == d).sum())) <= 1


# ---------------- GPU ----------------
_REF = {}  # oracle results, computed once per graph and program


def ref(key, fn):
    if key not in _REF:
        out = fn()
        for a in out if isinstance(out, tuple) else (out,):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


@contextlib.contextmanager
def built(s, t, flags, shards=1, knobs=()):
    """A graph built (and used) under `knobs`; they go back to their defaults afterwards."""
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    defaults = {"pull_split": 1, "cc_uf": 1}
    ctx = g = None
    try:
        for k, v in knobs:
            _lib.tune_set(k, v)
        ctx = jg.Context((0,) * shards)
        g = ctx.build(VID, VID[s], VID[t], flags=flags)
        assert g.info()["num_shards"] == shards
        yield g
    finally:
        if g is not None:
            g.close()
        if ctx is not None:
            ctx.close()
        for k, _ in knobs:
            _lib.tune_set(k, defaults[k])


def init_values(combiner):
    return np.random.default_rng(100 + combiner).integers(-(1 << 39), 1 << 39, N)


def check_combiners(g, oracle, name, s, t, directions):
    for direction in directions:
        for combiner in (0, 1, 2):  # COMBINE_SUM, _MIN, _MAX
            init = init_values(combiner)
            for steps in (1, 3):
                want, wrec = ref((name, "combine", direction, combiner, steps),
                                 lambda: oracle.combine_steps(N, s, t, direction, combiner, steps, init, False))
                x, rec = g.combine_steps(direction, combiner, steps, init, False)
                msg = f"{name} dir {direction} combiner {combiner} steps {steps}"
                np.testing.assert_array_equal(rec, wrec, err_msg=msg)
                np.testing.assert_array_equal(x, want, err_msg=msg)


def check_pagerank(g, oracle, name, s, t):
    want, _ = ref((name, "pagerank"), lambda: oracle.pagerank(N, s, t, 0.85, N, 12))
    rank, _ = g.pagerank(0.85, N, 12)
    rel = np.abs(rank - want) / np.maximum(np.abs(want), 1e-300)
    assert rel.max() <= PR_RTOL, f"{name}: max rel err {rel.max()} at vertex {rel.argmax()}"


def ladder(adj):
    s, t = ladder_edges()
    return (s, t) if adj == "in" else (t, s)


@gpu
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("adj", ["in", "out"])
def test_ladder_combiners(oracle_lib, adj, split):
    import janusgraph_amd as jg
    s, t = ladder(adj)
    flags, direction = (jg.ADJ_IN, jg.DIR_IN) if adj == "in" else (jg.ADJ_OUT, jg.DIR_OUT)
    with built(s, t, flags, knobs=(("pull_split", split),)) as g:
        check_combiners(g, oracle_lib, "L" + adj, s, t, (direction,))


@gpu
@pytest.mark.parametrize("split", [0, 1])
def test_ladder_pagerank(oracle_lib, split):
    import janusgraph_amd as jg
    s, t = ladder("in")
    with built(s, t, jg.ADJ_IN, knobs=(("pull_split", split),)) as g:
        check_pagerank(g, oracle_lib, "Lin", s, t)


@gpu
def test_ladder_three_shards(oracle_lib):
    """Rows are striped over the shards: each gets every third row of the ladder and class tables of its own."""
    import janusgraph_amd as jg
    s, t = ladder("in")
    with built(s, t, jg.ADJ_IN, shards=3, knobs=(("pull_split", 1),)) as g:
        check_combiners(g, oracle_lib, "Lin", s, t, (jg.DIR_IN,))
        check_pagerank(g, oracle_lib, "Lin", s, t)


ALL = 1 | 2 | 4  # ADJ_OUT | ADJ_IN | ADJ_BOTH


@gpu
@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("variant", ["U", "U0"])
def test_unsorted_combiners(oracle_lib, variant, shards):
    """OUT and BOTH are cut from the IN order; on 3 shards OUT's vector is refreshed by the dense allgather."""
    import janusgraph_amd as jg
    s, t, _ = actor_edges(variant)
    with built(s, t, ALL, shards=shards) as g:
        check_combiners(g, oracle_lib, variant, s, t, (jg.DIR_OUT, jg.DIR_IN, jg.DIR_BOTH))


@gpu
@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("variant", ["U", "U0"])
def test_unsorted_pagerank(oracle_lib, variant, shards):
    s, t, _ = actor_edges(variant)
    with built(s, t, ALL, shards=shards) as g:
        check_pagerank(g, oracle_lib, variant, s, t)


@gpu
@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("uf", [1, 0])
@pytest.mark.parametrize("variant", ["U", "U0"])
def test_unsorted_connected_components(oracle_lib, variant, uf, shards):
    """cc_uf = 0: label propagation through the pull engine on the BOTH plan."""
    s, t, _ = actor_edges(variant)
    want, _ = ref((variant, "cc"), lambda: oracle_lib.connected_components(N, s, t, VID))
    with built(s, t, ALL, shards=shards, knobs=(("cc_uf", uf),)) as g:
        comp, _ = g.connected_components()
        np.testing.assert_array_equal(comp, want)


@gpu
@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("variant", ["U", "U0"])
def test_unsorted_bfs_64_sources(oracle_lib, variant, shards):
    import janusgraph_amd as jg
    s, t, actors = actor_edges(variant)
    deg = np.bincount(s, minlength=N) + np.bincount(t, minlength=N)
    deg[actors] = 0
    srcs = np.concatenate([actors[:4], np.random.default_rng(5).choice(np.flatnonzero(deg > 0), 60, replace=False)])
    want = ref((variant, "bfs"), lambda: np.stack([oracle_lib.bfs(N, s, t, int(v), oracle_lib.DIR_BOTH) for v in srcs]))
    with built(s, t, ALL, shards=shards) as g:
        depth = g.bfs(VID[srcs], jg.DIR_BOTH)
        for k in range(64):
            np.testing.assert_array_equal(depth[k], want[k], err_msg=f"source {k}")


@gpu
@pytest.mark.parametrize("present", RUN_SETS, ids=RUN_IDS)
def test_degree_runs(oracle_lib, present):
    import janusgraph_amd as jg
    s, t, _, _ = run_edges(present)
    name = "R" + "".join(map(str, present))
    with built(s, t, jg.ADJ_IN) as g:
        check_combiners(g, oracle_lib, name, s, t, (jg.DIR_IN,))
        check_pagerank(g, oracle_lib, name, s, t)


# ---------------- the plans behind the value tests ----------------
def plan_child(family):
    """Runs in a child process with JG_DEBUG_PLAN=1: builds the family's graphs, a marker line before each."""
    import janusgraph_amd as jg

    def case(name, s, t, flags, shards=1, knobs=()):
        sys.stderr.write(f"[case] {name}\n")
        sys.stderr.flush()
        with built(s, t, flags, shards=shards, knobs=knobs) as g:
            if flags & jg.ADJ_OUT:
                g.combine_steps(jg.DIR_OUT, 0, 1, None, False)

    if family == "L":
        for split in (0, 1):
            case(f"in{split}", *ladder("in"), jg.ADJ_IN, knobs=(("pull_split", split),))
            case(f"out{split}", *ladder("out"), jg.ADJ_OUT, knobs=(("pull_split", split),))
    elif family == "U":
        for variant in ("U", "U0"):
            s, t, _ = actor_edges(variant)
            case(variant, s, t, ALL)
            case(variant + "x3", s, t, ALL, shards=3)
    else:
        for present in RUN_SETS:
            s, t, _, _ = run_edges(present)
            case("".join(map(str, present)), s, t, jg.ADJ_IN)


def plans_of(family):
    """{case: [plan]} of the child's dump; a plan is a dict of the header's numbers with "adj", "class" and
    "light" ({c: (first row, end row, blocks)}), "bands" ([(first row, end row)]), "runs" and "run_begin"."""
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), family],
                       env={**os.environ, "JG_DEBUG_PLAN": "1"}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    cases, plan = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("[case] "):
            plans = cases.setdefault(line.split()[1], [])
        m = re.match(r"\[jg plan\] shard (\d+) adj (\w+) (.*)", line)
        if m:
            words = m.group(3).split()
            plan = {"shard": int(m.group(1)), "adj": m.group(2), "class": {}, "light": {}, "bands": [], "runs": None}
            plan.update({k: int(v) for k, v in zip(words[::2], words[1::2])})
            plans.append(plan)
        m = re.match(r"\[jg plan\]   (class|light) (\d) lanes +\d+ rows \[(\d+),(\d+)\) = \d+ nnz \d+ blocks (\d+)", line)
        if m:
            plan[m.group(1)][int(m.group(2))] = tuple(int(m.group(i)) for i in (3, 4, 5))
        m = re.match(r"\[jg plan\]   band \d+ bits \d+ rows \[(\d+),(\d+)\)", line)
        if m:
            plan["bands"].append((int(m.group(1)), int(m.group(2))))
        m = re.match(r"\[jg plan\]   runs (\d)(?: run_begin((?: \d+)+))?", line)
        if m:
            plan["runs"] = int(m.group(1))
            plan["run_begin"] = [None] + [int(x) for x in (m.group(2) or "").split()]
    return cases


def class_table(degrees, first_row=0):
    """The class table of degree-sorted rows [first_row, rows): {c: (first row, end row, blocks)}."""
    d = np.sort(np.asarray(degrees))[::-1]
    table, begin = {}, first_row
    for c in range(1, 9):
        end = max(begin, int((d >= CLASS_THR[c - 1]).sum())) if c < 8 else len(d)
        per_block = BLOCK // (64 >> (c - 1)) if c < 8 else BLOCK
        table[c] = (begin, end, -(-(end - begin) // per_block))
        begin = end
    return table


def chunks_of(degrees):
    return sum(-(-int(d) // HUB_CHUNK) for d in degrees if d >= HUB_DEGREE)


@gpu
def test_ladder_plans():
    cases = plans_of("L")
    deg = np.zeros(N, np.int64)
    deg[:len(ladder_degrees())] = ladder_degrees()
    hubs = int((deg >= HUB_DEGREE).sum())
    assert (hubs, chunks_of(deg)) == (7, 21)
    full = class_table(deg)
    # 21 rows of 256 and more (a last block of one row), then 12, 23, 36, 68, 132 and 264, all over one block
    assert [full[c][1] - full[c][0] for c in range(1, 8)] == [21, 12, 23, 36, 68, 132, 264]
    assert all(full[c][2] >= 2 for c in range(1, 8))
    heavy = int((deg >= BAND_FLOORS[1]).sum())
    for name, adj in (("in", "IN"), ("out", "OUT")):
        for split in (0, 1):
            (p,) = cases[f"{name}{split}"]
            assert (p["adj"], p["rows"], p["nnz"]) == (adj, N, int(deg.sum()))
            assert (p["hubs"], p["chunks"], p["max_hub_row"]) == (hubs, chunks_of(deg), hubs - 1)
            assert p["class"] == full
            if split == 0:
                assert p["split_rows"] == 0 and p["bands"] == [] and p["light"] == full
            else:  # every class but the 1-lane one is in the bands; its rows are addressed by degree run
                assert p["bands"] == [(0, int((deg >= BAND_FLOORS[0]).sum())), (int((deg >= BAND_FLOORS[0]).sum()), heavy)]
                assert p["split_rows"] == heavy > p["max_hub_row"]
                assert p["light"] == class_table(deg, heavy)
                assert [p["light"][c][1] - p["light"][c][0] for c in range(1, 8)] == [0] * 6 + [264]
            # the 1-lane rows are runs of 258 rows of degree 7 and one of each degree below
            assert p["runs"] == 1 and p["run_begin"][1:] == [heavy + 258 + 6 - d for d in range(1, 7)] + [heavy]


@gpu
def test_unsorted_plans():
    cases = plans_of("U")
    for variant in ("U", "U0"):
        s, t, actors = actor_edges(variant)
        outdeg = np.bincount(s, minlength=N)
        plans = {p["adj"]: p for p in cases[variant]}
        assert sorted(plans) == ["BOTH", "IN", "OUT"] and len(cases[variant]) == 3
        p = plans["OUT"]
        assert (p["rows"], p["nnz"], p["hubs"], p["chunks"]) == (N, len(s), 4, 12)
        assert p["runs"] == 0
        last = p["class"][7][1]  # the empty suffix starts after the last row with an entry
        assert p["class"][8] == (last, N, -(-(N - last) // BLOCK)) and last > N - int((outdeg == 0).sum())
        assert p["max_hub_row"] == max(k for k, d in enumerate(actor_out_degrees(variant)) if d >= HUB_DEGREE)
        if variant == "U":
            assert p["bands"] == [(0, 3), (3, 4)] and p["split_rows"] == 4
            assert p["max_hub_row"] == 14 >= p["split_rows"]
            # classes are cut at the first row below each threshold: row 1 (100 entries) ends classes 1 and
            # 2, row 3 (8 entries) classes 3 to 5, row 4 (7 entries) class 6; the 1-lane class takes the rest
            assert [p["class"][c][:2] for c in range(1, 8)] == [(0, 1), (1, 1), (1, 3), (3, 3), (3, 3), (3, 4), (4, last)]
            assert [p["light"][c][:2] for c in range(1, 8)] == [(4, 4)] * 6 + [(4, last)]
        else:
            assert p["bands"] == [] and p["split_rows"] == 0
            assert [p["class"][c][:2] for c in range(1, 8)] == [(0, 0)] * 6 + [(0, last)]
            assert p["light"] == p["class"]
        # IN is the sorted one: the actors are its first band
        assert plans["IN"]["bands"][0] == (0, ACTORS) and plans["IN"]["hubs"] == 0
        # 3 shards: OUT's plan is built by the first combine over it, one per shard
        out3 = [q for q in cases[variant + "x3"] if q["adj"] == "OUT"]
        assert sorted(q["shard"] for q in out3) == [0, 1, 2]
        assert sum(q["hubs"] for q in out3) == 4 and sum(q["chunks"] for q in out3) == 12
        assert sum(q["nnz"] for q in out3) == len(s) and all(q["runs"] == 0 for q in out3)


@gpu
def test_degree_run_plans():
    cases = plans_of("R")
    for present in RUN_SETS:
        (p,) = cases["".join(map(str, present))]
        counts = run_counts(present)
        light = sum(counts.values())
        assert p["adj"] == "IN" and p["bands"] == [(0, 1), (1, 11)] and p["split_rows"] == 11 and p["hubs"] == 0
        assert p["light"][7][:2] == (11, 11 + light) and p["light"][8][:2] == (11 + light, N)
        assert p["runs"] == 1
        want, row = [None] * (RUN_MAX + 1), 11
        for d in range(RUN_MAX, 0, -1):
            if d in counts:
                want[d], row = row, row + counts[d]
        nxt = row  # an absent degree: an empty run at the start of the next smaller present one
        for d in range(1, RUN_MAX + 1):
            if want[d] is None:
                want[d] = nxt
            nxt = want[d]
        assert p["run_begin"] == want, present
        # runs start inside a block of 256 rows and cross block ends
        assert counts[max(present)] > BLOCK and (len(present) == 1 or (want[min(present)] - 11) % BLOCK != 0)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    plan_child(sys.argv[1])
