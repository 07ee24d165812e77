"""jg_peer_pressure on the device: PeerPressureVertexProgram against the host restatement of its semantics
(tests/test_peer_pressure_host.py: exact sums, smallest id among tied clusters).  No expectation comes from
the library.  Ids are sparse and shuffled, so caller order, id order and degree order all differ."""
import os

import numpy as np
import pytest

from test_peer_pressure_host import (GENERAL_SEEDS, OSCILLATOR, OSCILLATOR_KAT, expected_peer_pressure,
                                     fixed_point_gap, general_graph)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIRS = {"outE": 1, "bothE": 3}
# entry counts (degree + 1) at which jg_peer.hip changes the row's class: lane groups of 4, 16 and 64, then the
# sort path; and the sort path's longest run summed by one lane (kPeerLaneRun)
CLASS_DEGREES = (3, 15, 63)
LANE_RUN = 32
HUB_DEGREE, HUB_CHUNK = 8192, 4096  # kHubDegree, kHubChunk (jg_internal.h)


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
    """n distinct positive ids, sparse and shuffled: numeric order != caller order."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.arange(1, 50 * n + 100, dtype=np.int64), size=n, replace=False)


def check(ctx, vid, s, t, direction="outE", distribute=False, cap=30, exact=True, need_unambiguous=False):
    """Runs the program on the device and the restatement on the host; compares labels and iterations when
    `exact`, and checks the fixed point of any run that halts before the cap.  Returns (labels, iterations)."""
    import janusgraph_amd as jg
    vid = np.asarray(vid, np.int64)
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    want, want_it, amb = expected_peer_pressure(vid, s, t, direction, distribute, cap)
    if need_unambiguous:
        assert amb == 0, f"the input is not ambiguity-free: {amb}"
    g = ctx.build(vid, vid[s], vid[t], flags=jg.ADJ_IN if direction == "outE" else jg.ADJ_BOTH)
    try:
        got, it = g.peer_pressure(DIRS[direction], distribute, cap)
        again, it2 = g.peer_pressure(DIRS[direction], distribute, cap)
        stats = ctx.stats()
    finally:
        g.close()
    assert got.tobytes() == again.tobytes() and it == it2  # the same bytes on every run
    assert set(got.tolist()) <= set(vid.tolist())
    votes = it - 1 - (1 if distribute else 0)
    assert stats["supersteps"] == it and stats["levels"] == votes
    if votes < cap:
        gap = fixed_point_gap(vid, s, t, direction, distribute, got)
        assert gap <= 1e-9, gap
    if exact:
        assert it == want_it
        np.testing.assert_array_equal(got, want)
    return got, it


# ---- known answers ----
def test_kats(ctx):
    got, it = check(ctx, [7, 3], [0, 1], [1, 0])
    assert got.tolist() == [3, 3] and it == 3
    vid, s, t = OSCILLATOR
    for cap, (want, want_it) in OSCILLATOR_KAT.items():
        got, it = check(ctx, vid, s, t, cap=cap)
        assert (got.tolist(), it) == (want, want_it), cap
    got, it = check(ctx, vid, s, t, distribute=True, cap=4)
    assert got.tolist() == [7, 3] and it == 6


@pytest.mark.parametrize("name", ["gods", "cc_kat", "random_small", "random_medium", "spvp_diamond"])
def test_golden(ctx, name):
    z = np.load(os.path.join(GOLD, f"{name}.npz"))
    vid = z["vid"].astype(np.int64)
    index = {int(v): i for i, v in enumerate(vid.tolist())}
    pairs = [(index[int(a)], index[int(b)]) for a, b in zip(z["src"], z["dst"])
             if int(a) in index and int(b) in index]  # an edge to a vertex outside vid is a ghost edge
    s = np.asarray([p[0] for p in pairs], np.int64)
    t = np.asarray([p[1] for p in pairs], np.int64)
    for direction in DIRS:
        check(ctx, vid, s, t, direction)


# ---- random graphs ----
def skewed(rng, n, m):
    """m endpoints in [0, n), a few of them drawn very often: rows of every class up to a few hundred entries."""
    return np.minimum((n * rng.random(m) ** 3).astype(np.int64), n - 1)


@pytest.mark.parametrize("direction", ["outE", "bothE"])
@pytest.mark.parametrize("seed", [3, 4])
def test_random_unit(ctx, direction, seed):
    rng = np.random.default_rng(seed)
    n, m = 2500, 20000
    perm = rng.permutation(n)
    s, t = perm[rng.integers(0, n, m)], perm[skewed(rng, n, m)]
    check(ctx, sparse_ids(n, seed), s, t, direction)


def pow2_graph(rng, n, skew):
    """Every out-degree drawn from {0, 1, 2, 4, 8, 16}: with distribute every sum is exact in any order."""
    deg = rng.choice([0, 1, 2, 4, 8, 16], n)
    s = np.repeat(np.arange(n), deg)
    t = skewed(rng, n, len(s)) if skew else rng.integers(0, n, len(s))
    perm = rng.permutation(n)
    return perm[s], perm[t]


@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("seed", [5, 6])
def test_distribute_power_of_two_degrees(ctx, seed, skew):
    rng = np.random.default_rng(seed)
    n = 1500
    s, t = pow2_graph(rng, n, skew)
    check(ctx, sparse_ids(n, seed), s, t, "outE", True, need_unambiguous=True)


def test_distribute_power_of_two_both(ctx):
    # bothE divides by the BOTH row length: a ring over every vertex (2 entries each) and a second ring over
    # the first half (4 entries there)
    n = 1024
    v = np.arange(n)
    s = np.concatenate([v, v[: n // 2]])
    t = np.concatenate([(v + 1) % n, (v[: n // 2] + 3) % (n // 2)])
    rng = np.random.default_rng(8)
    perm = rng.permutation(n)
    check(ctx, sparse_ids(n, 8), perm[s], perm[t], "bothE", True, need_unambiguous=True)


@pytest.mark.parametrize("seed,direction,want_it", GENERAL_SEEDS)
def test_distribute_general_degrees(ctx, seed, direction, want_it):
    vid, s, t = general_graph(seed)
    _, it = check(ctx, vid, s, t, direction, True, need_unambiguous=True)
    assert it == want_it


@pytest.mark.parametrize("direction", ["outE", "bothE"])
def test_distribute_fixed_point_on_any_input(ctx, direction):
    # not ambiguity-free: only the fixed point (of a run that halts) and the run-to-run identity are checked
    vid, s, t = general_graph(7)
    check(ctx, vid, s, t, direction, True, exact=False)


# ---- shapes where the kernels can go wrong ----
def in_star(d, extra=0, hub_votes=False):
    """(vid, s, t, hub): d distinct sources -> the hub, `extra` vertices without in-edges from the sources; the
    smallest id is a source in the middle of caller order.  hub_votes (needs extra > 0): one edge hub -> the
    last vertex, so that with distribute the hub has a finite strength (1/1, as every source)."""
    n = d + 1 + extra
    vid = np.sort(sparse_ids(n, 100 + d))[::-1].copy()  # descending: the smallest id is last ...
    hub = n // 3
    src = np.asarray([i for i in range(d + 1) if i != hub], np.int64)
    mid = int(src[len(src) // 2])
    vid[[mid, n - 1]] = vid[[n - 1, mid]]  # ... and now sits in the middle, on a source
    s, t = src, np.full(d, hub, np.int64)
    if hub_votes:
        s, t = np.append(s, hub), np.append(t, n - 1)
    return vid, s, t, hub


@pytest.mark.parametrize("d", sorted({c + k for c in CLASS_DEGREES for k in (-1, 0, 1, 2)} | {1}))
@pytest.mark.parametrize("distribute", [False, True])
def test_in_star_at_class_boundaries(ctx, d, distribute):
    vid, s, t, hub = in_star(d, extra=3, hub_votes=distribute)
    got, _ = check(ctx, vid, s, t, "outE", distribute, need_unambiguous=True)
    assert got[hub] == vid.min()  # d + 1 clusters of one vote each: the smallest id wins
    check(ctx, vid, s, t, "bothE", distribute, need_unambiguous=True)


# kHubDegree - 1 / 0 / + 1; the last is 2 * kHubChunk + 1 as well
@pytest.mark.parametrize("d", [HUB_DEGREE - 1, HUB_DEGREE, 2 * HUB_CHUNK + 1])
def test_in_star_at_hub_boundaries(ctx, d):
    vid, s, t, hub = in_star(d)
    got, _ = check(ctx, vid, s, t)
    assert got[hub] == vid.min()


def test_in_star_of_40000_distinct_labels(ctx):
    vid, s, t, hub = in_star(40000, extra=5)
    got, it = check(ctx, vid, s, t)
    assert got[hub] == vid.min() and it == 3
    vid, s, t, hub = in_star(40000, extra=5, hub_votes=True)  # every strength is 1/1
    got, _ = check(ctx, vid, s, t, distribute=True, need_unambiguous=True)
    assert got[hub] == vid.min()


@pytest.mark.parametrize("k,k2", [(4097, 4096), (4096, 4096), (4096, 4097)])
def test_two_team_hub(ctx, k, k2):
    """Leaders A and B (the two smallest ids) feed k and k2 sources, which all feed the hub: in the second
    superstep the hub counts k votes for A against k2 for B, spread over the whole sorted row."""
    n = k + k2 + 3
    vid = np.sort(sparse_ids(n, 9))
    a, b, hub = 0, 1, 2
    team_a = np.arange(3, 3 + k)
    team_b = np.arange(3 + k, n)
    rng = np.random.default_rng(k + k2)
    s = np.concatenate([np.full(k, a), np.full(k2, b), team_a, team_b])
    t = np.concatenate([team_a, team_b, np.full(k + k2, hub)])
    perm = rng.permutation(n)  # caller order != id order
    order = np.argsort(perm)
    got, _ = check(ctx, vid[order], perm[s], perm[t])
    assert got[perm[hub]] == (vid[a] if k >= k2 else vid[b])


@pytest.mark.parametrize("run", [LANE_RUN - 1, LANE_RUN, LANE_RUN + 1, LANE_RUN + 2, 65, 100])
def test_distributed_runs_in_the_sort_path(ctx, run):
    """With distribute, a hub whose sorted row holds runs of `run` and `run` - 1 equal labels (each entry of
    strength 1/128) beside singletons: the longer run must win, summed by a lane or by the wave.  Every vertex
    that votes has out-degree 128 (padded with edges to a sink), so every sum is exact."""
    deg = 128
    teams = (run, run - 1)
    n_src = sum(teams) + 40
    lead = [0, 1]
    hub, sink = 2, 3
    first = 4
    n = first + n_src
    s, t = [hub] * deg, [sink] * deg  # the hub votes too: a finite strength
    at = first
    for leader, size in zip(lead, teams):
        members = list(range(at, at + size))
        at += size
        s += [leader] * deg
        t += members + [sink] * (deg - size)
        for m_ in members:
            s += [m_] * deg
            t += [hub] + [sink] * (deg - 1)
    for m_ in range(at, n):  # singletons
        s += [m_] * deg
        t += [hub] + [sink] * (deg - 1)
    vid = np.sort(sparse_ids(n, run))
    # the leaders have the smallest ids (a source's tie between its own vote and its leader's goes to the
    # leader); the shorter team's leader has the smaller one, so only the sums can make the longer team win
    vid[[0, 1]] = vid[[1, 0]]
    rng = np.random.default_rng(run)
    perm = rng.permutation(n)
    order = np.argsort(perm)
    got, _ = check(ctx, vid[order], perm[np.asarray(s)], perm[np.asarray(t)], "outE", True, need_unambiguous=True)
    assert got[perm[hub]] == vid[0]


def test_multi_edges_self_loops_and_edgeless(ctx):
    # 4 parallel edges 1 -> 0 are four votes against 4 single ones (with distribute 4 x 1/4: a tie, exact)
    vid = np.asarray([50, 40, 1, 2, 3, 4, 99], np.int64)
    s = [1] * 4 + [2, 3, 4, 5]
    t = [0] * 8
    got, _ = check(ctx, vid, s, t, cap=1)
    assert got[0] == 40 and got[6] == 99
    check(ctx, vid, s, t)
    check(ctx, vid, s, t, distribute=True, need_unambiguous=True)
    # self-loops: twice in the BOTH row, once in the IN row
    vid = np.asarray([9, 5, 7, 1], np.int64)
    s, t = [0, 0, 1, 2, 2, 3], [0, 1, 0, 2, 0, 3]
    for direction in DIRS:
        check(ctx, vid, s, t, direction)
        check(ctx, vid, s, t, direction, True, need_unambiguous=True)
    # n = 1, and no edge at all
    none = np.zeros(0, np.int64)
    got, it = check(ctx, [42], none, none)
    assert got.tolist() == [42] and it == 2
    got, it = check(ctx, [42], [0], [0], "bothE", True)
    assert got.tolist() == [42] and it == 3
    got, it = check(ctx, sparse_ids(300, 2), none, none, "bothE")
    assert it == 2
    got, it = check(ctx, sparse_ids(300, 2), none, none, cap=0)
    assert it == 1


@pytest.mark.parametrize("rows", [63, 64, 65, 255, 256, 257])
def test_wave_and_block_boundaries(ctx, rows):
    """Exactly `rows` rows with entries, every one of in-degree 2 (a double ring), so that the last lane group
    of a wave / block is the partial one; 7 edgeless vertices besides."""
    v = np.arange(rows)
    s = np.concatenate([v, v])
    t = np.concatenate([(v + 1) % rows, (v + 5) % rows])
    rng = np.random.default_rng(rows)
    perm = rng.permutation(rows + 7)
    for distribute in (False, True):
        check(ctx, sparse_ids(rows + 7, rows), perm[s], perm[t], "outE", distribute, need_unambiguous=True)


# ---- API behaviour ----
def test_status_stats_and_lifetime():
    import janusgraph_amd as jg
    E = jg._lib
    ctx = jg.Context((0,))
    rng = np.random.default_rng(12)
    n, m = 600, 3000
    vid = sparse_ids(n, 12)
    s, t = rng.integers(0, n, m), rng.integers(0, n, m)
    want, want_it, _ = expected_peer_pressure(vid, s, t, "outE", False, 30)
    g = ctx.build(vid, vid[s], vid[t], flags=jg.ADJ_IN | jg.ADJ_BOTH)
    assert code(g.peer_pressure, jg.DIR_IN) == E.JG_ERR_UNSUPPORTED
    assert code(g.peer_pressure, jg.DIR_OUT, False, -1) == E.JG_ERR_ARG
    assert code(g.peer_pressure, 7) == E.JG_ERR_ARG
    # other programs' held results on the same graph are not disturbed
    it_cc, nc, nl, largest, _ = g.cc_census_build(1)
    census = g.cc_census_read(0, nl)
    g.bfs_keep(vid[:3], jg.DIR_BOTH, -1)
    kept = g.bfs_kept_row(1).copy()
    g.pagerank_begin(0.85, n)
    g.pagerank_step(3)
    none, it = g.peer_pressure(want_clusters=False)  # cluster_vid_out NULL
    assert none is None and it == want_it
    got, it = g.peer_pressure()
    np.testing.assert_array_equal(got, want)
    assert it == want_it
    st = ctx.stats()
    votes = want_it - 1
    nnz = m
    assert st["supersteps"] == want_it and st["levels"] == votes
    assert st["edges_traversed"] == votes * nnz
    assert st["kernel_launches"] >= votes and 0 < st["kernel_ms_total"] <= st["compute_ms"]
    assert st["algorithmic_bytes"] >= votes * 8 * nnz
    again = g.cc_census_read(0, nl)
    np.testing.assert_array_equal(census[0], again[0])
    np.testing.assert_array_equal(census[1], again[1])
    np.testing.assert_array_equal(g.bfs_kept_row(1), kept)
    g.pagerank_step(2)
    rank, _ = g.pagerank_end()
    g.close()
    g = ctx.build(vid, vid[s], vid[t], flags=jg.ADJ_IN)  # the same session with nothing in between
    g.pagerank_begin(0.85, n)
    g.pagerank_step(5)
    ref, _ = g.pagerank_end()
    assert rank.tobytes() == ref.tobytes()
    g.close()
    # missing adjacency
    g = ctx.build(vid, vid[s], vid[t], flags=jg.ADJ_OUT | jg.ADJ_BOTH)
    assert code(g.peer_pressure, jg.DIR_OUT) == E.JG_ERR_UNSUPPORTED
    g.peer_pressure(jg.DIR_BOTH)
    g.close()
    g = ctx.build(vid, vid[s], vid[t], flags=jg.ADJ_IN)
    assert code(g.peer_pressure, jg.DIR_BOTH) == E.JG_ERR_UNSUPPORTED
    g.close()
    ctx.close()
    # two logical shards
    ctx2 = jg.Context((0, 0))
    g = ctx2.build(vid, vid[s], vid[t], flags=jg.ADJ_IN | jg.ADJ_BOTH)
    assert code(g.peer_pressure) == E.JG_ERR_UNSUPPORTED
    assert code(g.peer_pressure, jg.DIR_BOTH, True) == E.JG_ERR_UNSUPPORTED
    g.close()
    ctx2.close()


def random_in_memory_graph(n, m, seed):
    import janusgraph_amd as jg
    rng = np.random.default_rng(seed)
    g = jg.InMemoryGraph()
    vs = [g.add_vertex() for _ in range(n)]
    for a, b in zip(rng.integers(0, n - 20, m).tolist(), rng.integers(0, n - 20, m).tolist()):
        g.add_edge(vs[a], vs[b], "knows")
    return g


@pytest.mark.parametrize("edges", ["outE", "bothE"])
def test_computer_route(ctx, edges):
    import janusgraph_amd as jg
    graph = random_in_memory_graph(400, 1500, 41)
    vid, src, dst, _ = graph.snapshot()
    index = {int(v): i for i, v in enumerate(vid.tolist())}
    s = np.asarray([index[int(x)] for x in src], np.int64)
    t = np.asarray([index[int(x)] for x in dst], np.int64)
    want, want_it, _ = expected_peer_pressure(vid, s, t, edges, False, 30)
    vp = jg.PeerPressureVertexProgram.build().edges(edges).create(graph)
    c = jg.GpuGraphComputer(graph, context=ctx).program(vp)
    c.mapReduce(jg.ClusterCountMapReduce.build().create())         # the default cluster property
    c.mapReduce(jg.ClusterPopulationMapReduce.build().create())
    result = c.submit().result()
    mem = result.memory()
    assert mem.getIteration() == want_it
    for v, w in zip(vid.tolist(), want.tolist()):
        got = result.graph().value(v, vp.CLUSTER)
        assert type(got) is int and got == w  # the Long id, not a String
    ids, pops = np.unique(want, return_counts=True)
    assert mem.get("clusterCount") == len(ids)
    assert mem.get("clusterPopulation") == {int(i): int(p) for i, p in zip(ids, pops)}


def test_computer_refuses_a_sharded_context():
    import janusgraph_amd as jg
    graph = random_in_memory_graph(200, 500, 42)
    ctx2 = jg.Context((0, 0))
    try:
        c = jg.GpuGraphComputer(graph, context=ctx2).program(jg.PeerPressureVertexProgram.build().create())
        with pytest.raises(jg.ProgramNotSupported):
            c.submit().result()
    finally:
        ctx2.close()
