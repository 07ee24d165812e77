"""jg_bfs_kept_dag / jg_bfs_kept_dag_read: the shortest-path predecessor DAG of a kept depth row, built on the
device (janusgraph_amd/csrc/jg_pathdag.hip).

What is expected comes from the host: the kept row itself is checked against oracle.bfs_csr, the DAG's
vertex set and each vertex's predecessor SET from the oracle's CSR (oracle.csr_unordered) by a plain
walk-back over the levels, and every predecessor LIST, order included, against what
PathDag(g.neighbors, n).predecessors builds from jg_graph_neighbors (the route the computer took before).
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def entries_of(ptr, rows):
    """(owner position in rows, entry index) of every CSR entry of the given rows, row by row."""
    rows = np.asarray(rows, np.int64)
    lens = ptr[rows + 1] - ptr[rows]
    owner = np.repeat(np.arange(len(rows)), lens)
    start = np.repeat(np.cumsum(lens) - lens, lens)
    return owner, np.arange(int(lens.sum())) - start + np.repeat(ptr[rows], lens)


def host_dag(n, ptr, adj, depth, target):
    """(DAG vertices, sorted distinct (vertex, predecessor) pairs as v * n + u, deepest) by a level walk-back."""
    on = depth >= 0
    if target is not None:
        on &= np.asarray(target, bool)
    if not on.any():
        return np.zeros(0, np.int64), np.zeros(0, np.int64), -1
    on = on.copy()
    deepest = int(depth[on].max())
    pairs = []
    for d in range(deepest, 0, -1):
        cur = np.flatnonzero(on & (depth == d))
        owner, idx = entries_of(ptr, cur)
        u = adj[idx].astype(np.int64)
        keep = depth[u] == d - 1
        on[u[keep]] = True
        pairs.append(np.unique(cur[owner[keep]] * n + u[keep]))
    return np.flatnonzero(on), np.sort(np.concatenate(pairs)) if pairs else np.zeros(0, np.int64), deepest


def check_dag(g, o, n, ptr, adj, row, source, target=None, max_depth=-1):
    """Builds and reads the DAG of kept row `row` (its source: `source`) and checks all of it.  Returns
    (vertex, depth, off, pred)."""
    from janusgraph_amd.computer import PathDag
    depth = g.bfs_kept_row(row)
    np.testing.assert_array_equal(depth, o.bfs_csr(n, ptr, adj, int(source), max_depth))
    want_v, want_pairs, want_deepest = host_dag(n, ptr, adj, depth, target)
    nv, ne, deepest = g.bfs_kept_dag_build(row, target)
    stats = g.ctx.stats()
    vertex, vdepth, off, pred = g.bfs_kept_dag_read(0, nv)
    print(f"dag: nv {nv} ne {ne} deepest {deepest} compute_ms {stats['compute_ms']:.3f} "
          f"launches {stats['kernel_launches']} edges {stats['edges_traversed']:.0f}")
    assert (nv, deepest) == (len(want_v), want_deepest)
    assert len(vertex) == nv and len(off) == nv + 1 and off[0] == 0 and off[-1] == ne == len(pred)
    if nv == 0:
        assert ne == 0 and deepest == -1
        return vertex, vdepth, off, pred
    np.testing.assert_array_equal(np.sort(vertex), want_v)           # the vertex set, each once
    np.testing.assert_array_equal(vdepth, depth[vertex])
    assert np.all(np.diff(vdepth) <= 0) and vertex[-1] == source and vdepth[0] == deepest
    assert np.all(np.diff(off) >= 0) and off[-1] - off[-2] == 0      # the source: an empty range
    got_pairs = np.repeat(vertex.astype(np.int64), np.diff(off)) * n + pred
    np.testing.assert_array_equal(np.sort(got_pairs), want_pairs)    # distinct predecessors, as sets
    # every list with its order: the host walk-back over jg_graph_neighbors
    hp, htargets, hdeepest = PathDag(g.neighbors, n).predecessors(depth, target)
    assert hdeepest == deepest and set(hp) == set(vertex[vdepth >= 1].tolist())
    for j, v in enumerate(vertex.tolist()):
        if vdepth[j] >= 1:
            assert pred[off[j]:off[j + 1]].tolist() == hp[v].tolist(), v
    on_path = vertex[vdepth >= 1]
    assert stats["edges_traversed"] == float((ptr[on_path + 1] - ptr[on_path]).sum())
    assert stats["levels"] == deepest and stats["kernel_launches"] >= 1
    # the same call again: the same order
    assert g.bfs_kept_dag_build(row, target) == (nv, ne, deepest)
    again = g.bfs_kept_dag_read(0, nv)
    for a, b in zip(again, (vertex, vdepth, off, pred)):
        np.testing.assert_array_equal(a, b)
    return vertex, vdepth, off, pred


@pytest.fixture(scope="module")
def ctx():
    import janusgraph_amd as jg
    c = jg.Context((0,))
    yield c
    c.close()


def small_graph(ctx, o, n, edges, flags=None):
    import janusgraph_amd as jg
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    vid = np.arange(n, dtype=np.int64)
    g = ctx.build(vid, e[:, 0], e[:, 1], flags=jg.ADJ_BOTH if flags is None else flags)
    ptr, adj = o.csr_unordered(n, e[:, 0], e[:, 1], both=True)
    return g, ptr, adj


def mask(n, *on):
    t = np.zeros(n, bool)
    t[list(on)] = True
    return t


DIAMOND = [(1, 2), (2, 4), (1, 3), (3, 4)]  # vertex 0 is isolated
# triangle 0-1-2 with 0-1 doubled and a self-loop on the middle vertex 1; 3 hangs off 1 (doubled) and 2
TRIANGLE = [(0, 1), (0, 1), (1, 1), (1, 2), (0, 2), (1, 3), (3, 1), (2, 3)]


@pytest.mark.parametrize("name,n,edges,source,target,want", [
    ("diamond", 5, DIAMOND, 1, mask(5, 4), (4, 4, 2)),
    ("triangle", 4, TRIANGLE, 0, None, (4, 4, 2)),
    ("target_is_source", 5, DIAMOND, 1, mask(5, 1), (1, 0, 0)),
    ("isolated_source", 5, DIAMOND, 0, None, (1, 0, 0)),
    ("unreachable_and_reachable", 5, DIAMOND, 1, mask(5, 0, 2), (2, 1, 1)),
    ("all_zero_mask", 5, DIAMOND, 1, mask(5), (0, 0, -1)),
    ("target_none", 5, DIAMOND, 1, None, (4, 4, 2)),
])
def test_kats(ctx, oracle_lib, name, n, edges, source, target, want):
    g, ptr, adj = small_graph(ctx, oracle_lib, n, edges)
    g.bfs_keep([source])
    vertex, vdepth, off, pred = check_dag(g, oracle_lib, n, ptr, adj, 0, source, target)
    assert (len(vertex), len(pred), int(vdepth[0]) if len(vertex) else -1) == want
    if name == "triangle":  # duplicates removed, the self-loop ignored
        lists = {int(v): pred[off[j]:off[j + 1]].tolist() for j, v in enumerate(vertex)}
        assert lists[1] == [0] and lists[2] == [0] and sorted(lists[3]) == [1, 2] and lists[0] == []
    g.close()


def test_hub_row_spans_many_waves(ctx, oracle_lib):
    """Source 0 - 5000 middle vertices - sink, every edge doubled: the sink's 10000-entry row is walked by
    ~157 waves' worth of lanes and still emitted in row order, duplicates dropped."""
    k = 5000
    mid = np.arange(1, k + 1)
    one = np.concatenate([np.stack([np.zeros(k, np.int64), mid], 1), np.stack([mid, np.full(k, k + 1)], 1)])
    edges = np.concatenate([one, one])
    n = k + 2
    g, ptr, adj = small_graph(ctx, oracle_lib, n, edges)
    g.bfs_keep([0])
    vertex, vdepth, off, pred = check_dag(g, oracle_lib, n, ptr, adj, 0, 0, mask(n, k + 1))
    assert len(vertex) == k + 2 and len(pred) == 2 * k and vertex[0] == k + 1
    sink = pred[off[0]:off[1]]
    assert len(sink) == k and len(np.unique(sink)) == k
    g.close()


def test_many_levels(ctx, oracle_lib):
    """A 3000-vertex path with a chord every 7 vertices, the far end the only target: thousands of levels of
    one or two rows each.  The time limit is one a pass over every row per level would also meet at this
    size (tools/path_dag_bench.py times the work bound at 2^20 vertices)."""
    n = 3000
    i = np.arange(n - 1)
    chords = np.arange(0, n - 2, 7)
    edges = np.concatenate([np.stack([i, i + 1], 1), np.stack([chords, chords + 2], 1)])
    g, ptr, adj = small_graph(ctx, oracle_lib, n, edges)
    g.bfs_keep([0])
    t0 = time.perf_counter()
    nv, ne, deepest = g.bfs_kept_dag_build(0, mask(n, n - 1))
    wall = time.perf_counter() - t0
    print(f"many levels: deepest {deepest} nv {nv} ne {ne} wall {wall * 1e3:.1f} ms")
    assert wall < 2.0
    vertex, vdepth, off, pred = check_dag(g, oracle_lib, n, ptr, adj, 0, 0, mask(n, n - 1))
    assert int(vdepth[0]) == deepest > 2000
    g.close()


@pytest.fixture(scope="module")
def rmat14(ctx, oracle_lib):
    import janusgraph_amd as jg
    from test_gpu_configs import EF, host_edges, pick_sources, seed_of
    scale = 14
    n = 1 << scale
    s, d = host_edges(oracle_lib, scale)
    ptr, adj = oracle_lib.csr_unordered(n, s, d, both=True)
    g = ctx.build_rmat(scale, EF, seed_of(scale), flags=jg.ADJ_BOTH)
    yield g, n, ptr, adj, pick_sources(ptr, 64, scale)
    g.close()


@pytest.mark.parametrize("nsrc,rows", [(1, (0,)), (3, (0, 2)), (64, (0, 63))])
def test_width_rmat14(oracle_lib, rmat14, nsrc, rows):
    """target=None on RMAT-14 from each producer of kept planes: the single-source driver, the narrow
    engine and the bit-parallel batch."""
    g, n, ptr, adj, srcs = rmat14
    g.bfs_keep(srcs[:nsrc])
    for r in rows:
        vertex, vdepth, off, pred = check_dag(g, oracle_lib, n, ptr, adj, r, srcs[r])
        assert len(vertex) > n // 2


def test_rmat16_random_targets_and_bounded_keep(ctx, oracle_lib):
    import janusgraph_amd as jg
    from test_gpu_configs import EF, host_edges, pick_sources, seed_of
    scale = 16
    n = 1 << scale
    s, d = host_edges(oracle_lib, scale)
    ptr, adj = oracle_lib.csr_unordered(n, s, d, both=True)
    g = ctx.build_rmat(scale, EF, seed_of(scale), flags=jg.ADJ_BOTH)
    src = pick_sources(ptr, 1, scale)
    g.bfs_keep(src)
    depth = g.bfs_kept_row(0)
    t = mask(n, *np.random.default_rng(16).choice(np.flatnonzero(depth >= 1), 200, replace=False))
    vertex, _, _, _ = check_dag(g, oracle_lib, n, ptr, adj, 0, src[0], t)
    assert 200 < len(vertex) < n // 2
    g.bfs_keep(src, max_depth=2)
    check_dag(g, oracle_lib, n, ptr, adj, 0, src[0], t, max_depth=2)
    g.close()


def test_directed_keep_reads_the_reverse_rows(ctx, oracle_lib):
    """A DIR_OUT traversal's predecessors are IN neighbours: an edge u -> v puts u in v's list, never v in u's."""
    import janusgraph_amd as jg
    o = oracle_lib
    n = 1 << 10
    s, d = o.rmat_edges(10, 8, 11)
    vid = np.arange(n, dtype=np.int64)
    g = ctx.build(vid, s, d, flags=jg.ADJ_OUT | jg.ADJ_IN)
    optr, oadj = o.csr_unordered(n, s, d)
    iptr, iadj = o.csr_unordered(n, d, s)
    src = int(np.flatnonzero(np.diff(optr) > 3)[0])
    g.bfs_keep([src], jg.DIR_OUT)
    depth = g.bfs_kept_row(0)
    np.testing.assert_array_equal(depth, o.bfs_csr(n, optr, oadj, src))
    want_v, want_pairs, want_deepest = host_dag(n, iptr, iadj, depth, None)
    vertex, vdepth, off, pred = g.bfs_kept_dag(0)
    assert int(vdepth[0]) == want_deepest >= 2
    np.testing.assert_array_equal(np.sort(vertex), want_v)
    np.testing.assert_array_equal(np.sort(np.repeat(vertex.astype(np.int64), np.diff(off)) * n + pred), want_pairs)
    ioff, inbr = g.neighbors(vertex, jg.DIR_IN)
    for j in range(len(vertex)):  # the order: the IN row's, first occurrences
        nb = inbr[ioff[j]:ioff[j + 1]]
        nb = nb[depth[nb] == vdepth[j] - 1]
        _, first = np.unique(nb, return_index=True)
        assert pred[off[j]:off[j + 1]].tolist() == nb[np.sort(first)].tolist()
    g.close()


def test_ranged_read(oracle_lib, rmat14):
    g, n, ptr, adj, srcs = rmat14
    g.bfs_keep(srcs[:1])
    nv, ne, _ = g.bfs_kept_dag_build(0)
    vertex, vdepth, off, pred = g.bfs_kept_dag_read(0, nv)
    cuts = [0, nv // 3, nv // 3 + 1, nv]
    parts = [g.bfs_kept_dag_read(a, b - a) for a, b in zip(cuts, cuts[1:])]
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), vertex)
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), vdepth)
    np.testing.assert_array_equal(np.concatenate([p[3] for p in parts]), pred)
    for (a, b), p in zip(zip(cuts, cuts[1:]), parts):  # absolute offsets
        np.testing.assert_array_equal(p[2], off[a:b + 1])
    empty = g.bfs_kept_dag_read(nv, 0)
    assert len(empty[0]) == 0 and empty[2].tolist() == [ne] and len(empty[3]) == 0
    g.DAG_READ_ENTRIES = 1000  # Graph.bfs_kept_dag's own ranges (a large DAG's): dozens of reads here
    try:
        for a, b in zip(g.bfs_kept_dag(0), (vertex, vdepth, off, pred)):
            np.testing.assert_array_equal(a, b)
    finally:
        del g.DAG_READ_ENTRIES
    g.bfs_kept_release()


def test_lifetime(ctx, oracle_lib):
    import janusgraph_amd as jg
    g, _, _ = small_graph(ctx, oracle_lib, 5, DIAMOND)

    def no_dag():
        with pytest.raises(jg.JanusGpuError) as e:
            g.bfs_kept_dag_read(0, 0)
        assert e.value.code == jg._lib.JG_ERR_STATE

    no_dag()                      # never built
    g.bfs_keep([1])
    no_dag()
    assert g.bfs_kept_dag_build(0) == (4, 4, 2)
    g.bfs_kept_dag_read(0, 4)
    g.bfs_kept_release()
    no_dag()                      # dropped by the release
    g.bfs_keep([1])
    g.bfs_kept_dag_build(0)
    g.bfs_keep([2])
    no_dag()                      # dropped by a new keep
    g.close()


def test_errors(oracle_lib):
    import janusgraph_amd as jg
    E = jg._lib

    def code(fn, *a):
        with pytest.raises(jg.JanusGpuError) as e:
            fn(*a)
        return e.value.code

    ctx = jg.Context((0,))
    g, _, _ = small_graph(ctx, oracle_lib, 5, DIAMOND)
    assert code(g.bfs_kept_dag_build, 0) == E.JG_ERR_ARG          # nothing kept
    g.bfs_keep([1, 2])
    assert code(g.bfs_kept_dag_build, 2) == E.JG_ERR_ARG
    assert code(g.bfs_kept_dag_build, -1) == E.JG_ERR_ARG
    nv, _, _ = g.bfs_kept_dag_build(1)
    assert code(g.bfs_kept_dag_read, 0, nv + 1) == E.JG_ERR_ARG
    assert code(g.bfs_kept_dag_read, nv, 1) == E.JG_ERR_ARG
    assert code(g.bfs_kept_dag_read, -1, 1) == E.JG_ERR_ARG
    g.close()
    # a DIR_OUT traversal of an OUT-only graph: its predecessors are IN rows, which were not built
    e = np.asarray(DIAMOND, np.int64)
    g = ctx.build(np.arange(5, dtype=np.int64), e[:, 0], e[:, 1], flags=jg.ADJ_OUT)
    g.bfs_keep([1], jg.DIR_OUT)
    assert code(g.bfs_kept_dag_build, 0) == E.JG_ERR_UNSUPPORTED
    g.close()
    ctx.close()
    ctx2 = jg.Context((0, 0))  # two logical shards
    g, _, _ = small_graph(ctx2, oracle_lib, 5, DIAMOND)
    g.bfs_keep([1])
    assert code(g.bfs_kept_dag_build, 0) == E.JG_ERR_UNSUPPORTED
    assert code(g.bfs_kept_dag_read, 0, 0) == E.JG_ERR_STATE
    g.close()
    ctx2.close()                  # still destroys cleanly


def host_route_paths(ctx, graph, sources, targets, max_distance=None):
    """memory[SHORTEST_PATHS] the way the computer built it before: jg_bfs_rows + PathDag over jg_graph_neighbors."""
    import janusgraph_amd as jg
    from janusgraph_amd.computer import PathDag
    vid, src, dst, _ = graph.snapshot()
    index = {int(v): i for i, v in enumerate(vid.tolist())}
    target = np.zeros(len(vid), bool)
    target[[index[t] for t in targets]] = True
    g = ctx.build(vid, src, dst, flags=jg.ADJ_BOTH)
    dag = PathDag(g.neighbors, len(vid))
    batch = [index[s] for s in sources]
    paths, level = [], 0
    for s, depth in zip(batch, g.bfs_rows(vid[batch], jg.DIR_BOTH, -1 if max_distance is None else max_distance)):
        got, deepest = dag.paths(depth, s, target)
        level = max(level, deepest)
        paths.extend([int(vid[x]) for x in p] for p in got)
    g.close()
    return paths, level + 1


def test_computer_takes_the_device_route(ctx, oracle_lib):
    import janusgraph_amd as jg
    key = jg.ShortestPathVertexProgram.SHORTEST_PATHS
    dia = jg.InMemoryGraph()
    v = [dia.add_vertex() for _ in range(4)]
    for a, b in ((0, 1), (0, 2), (1, 3), (2, 3)):
        dia.add_edge(v[a], v[b], "E")
    rm = jg.InMemoryGraph()
    rv = [rm.add_vertex() for _ in range(1 << 10)]
    s, d = oracle_lib.rmat_edges(10, 8, 10)
    for a, b in zip(s.tolist(), d.tolist()):
        rm.add_edge(rv[a], rv[b], "E")
    cases = [(dia, [v[0].id], [v[3].id], None),
             (rm, [x.id for x in rv[3:400:90]], [x.id for x in rv[::9]], None),
             (rm, [x.id for x in rv[3:400:90]], [x.id for x in rv[::9]], 2)]
    for graph, sources, targets, max_distance in cases:
        b = jg.ShortestPathVertexProgram.build().source(*sources).target(*targets)
        if max_distance is not None:
            b = b.maxDistance(max_distance)
        memory = jg.GpuGraphComputer(graph, context=ctx).program(b.create(graph)).submit().result().memory()
        want, iteration = host_route_paths(ctx, graph, sources, targets, max_distance)
        assert memory.get(key) == want and len(want) >= 2  # equal lists, not merely set-equal
        assert memory.getIteration() == iteration
