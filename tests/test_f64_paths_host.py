"""Double edge weights for ShortestPathVertexProgram (jg_graph_set_weights_f64 / jg_sssp_keep_f64 /
jg_sssp_kept_dag_f64): what needs no GPU.

The host model of tests/test_weighted_paths_host.py (heapq Dijkstra, then the tight edges with an exact ==) is
type-agnostic; here it is fed Python floats and pinned against brute-force enumeration of every simple path,
summed left to right from the source, on seeded multigraphs whose weights tie often (k/4, k/8: exact in binary),
round (k/10) or hardly ever tie (uniform).  tests/test_gpu_f64_paths.py checks the device against this model bit for bit.
"""
import os
import re

import numpy as np
import pytest

from test_weighted_paths_host import DIR_BOTH, DIR_IN, DIR_OUT, brute_force, model_paths, weighted_dag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = ("jg_graph_set_weights_f64", "jg_sssp_keep_f64", "jg_sssp_kept_row_f64", "jg_sssp_kept_dag_f64",
                    "jg_sssp_kept_dag_edges_f64", "jg_sssp_kept_dag_read_f64")


def float_multigraph(seed, kind):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 8))
    m = int(rng.integers(1, 15))
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n, m)          # self-loops as they fall
    for i in range(min(int(rng.integers(0, m + 1)), 3)):  # some parallel edges, same or reversed endpoints
        j = int(rng.integers(0, m))
        src[i], dst[i] = (src[j], dst[j]) if rng.integers(0, 2) else (dst[j], src[j])
    if kind == "quarters":
        w = rng.integers(1, 3, m) / 4.0      # 0.25 or 0.5: ties on most graphs
    elif kind == "eighths":
        w = rng.integers(1, 9, m) / 8.0      # 0.125 .. 1.0: every sum exact, ties everywhere
    elif kind == "tenths":
        w = rng.integers(1, 9, m) / 10.0     # sums round: ties depend on the order of the adds
    else:
        w = rng.uniform(0.01, 3.0, m)
    return n, src.astype(np.int64), dst.astype(np.int64), w.astype(np.float64)


def check_model(seed, kind):
    """The model against brute force on one seeded graph; returns how many (source, target) pairs had several
    last hops of equal summed weight."""
    n, src, dst, w = float_multigraph(seed, kind)
    tied = 0
    for direction in (DIR_OUT, DIR_IN, DIR_BOTH):
        for source in range(n):
            dist, pred = weighted_dag(n, src, dst, w, direction, source)
            want = brute_force(n, src, dst, w, direction, source)
            # == on floats: the model's distance is the smallest left-to-right sum, bit for bit
            assert {v: float(d) for v, d in enumerate(dist) if d is not None} == {v: float(d) for v, (d, _) in want.items()}
            for v in range(n):
                last_hops = {p[-2] for p in want[v][1] if len(p) > 1} if v in want else set()
                assert pred[v] == last_hops, (direction, source, v)
                tied += len(last_hops) > 1
            paths = model_paths(n, src, dst, w, direction, [source])
            assert sorted(map(tuple, paths)) == sorted(p for _, ps in want.values() for p in ps)
            reached = sorted(float(d) for d in dist if d is not None)
            bound = reached[len(reached) // 2]
            cut = model_paths(n, src, dst, w, direction, [source], max_distance=bound)
            assert cut == [p for p in paths if dist[p[-1]] <= bound]
    return tied


@pytest.mark.parametrize("kind", ["quarters", "eighths", "tenths", "uniform"])
@pytest.mark.parametrize("seed", range(12))
def test_float_model_against_brute_force(seed, kind):
    check_model(seed, kind)


def test_exact_ties_occur():
    """The k/4 graphs exercise exact ties (several last hops of equal summed weight), not only unique paths."""
    assert sum(check_model(seed, "quarters") for seed in range(12)) >= 1


def test_kat_arithmetic():
    """The facts the device KATs rest on: binary64, round to nearest even, no epsilon."""
    assert 0.1 + 0.2 != 0.3 and 0.1 + 0.2 == 0.30000000000000004 and 0.1 + 0.2 > 0.3
    assert 0.25 + 0.25 == 0.5
    assert (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)
    assert (0.0 + 0.1 + 0.2) + 0.3 == 0.6000000000000001 and (0.0 + 0.3 + 0.2) + 0.1 == 0.6
    # non-negative doubles order as their bit patterns read as signed integers
    x = np.sort(np.abs(np.random.default_rng(3).standard_normal(1000)) * 10.0 ** np.random.default_rng(4).integers(-300, 300, 1000))
    assert np.all(np.diff(x.view(np.int64)) >= 0) and np.array([0.0, np.inf]).view(np.int64).tolist() == [0, 0x7FF0 << 48]
    # the model on the two KATs: a tie across hop levels, and a near-tie that is none
    s, a, t = 0, 1, 2
    _, pred = weighted_dag(3, [s, a, s], [a, t, t], [0.25, 0.25, 0.5], DIR_OUT, s)
    assert pred[t] == {a, s}
    dist, pred = weighted_dag(3, [s, a, s], [a, t, t], [0.1, 0.2, 0.3], DIR_OUT, s)
    assert pred[t] == {s} and dist[t] == 0.3


def test_max_distance_keeps_a_fraction():
    import janusgraph_amd as jg
    P = jg.ShortestPathVertexProgram
    vp = P.build().source(1).maxDistance(0.75).distanceProperty("weight").create()
    assert vp.max_distance == 0.75 and isinstance(vp.max_distance, float)
    assert P(vp.store_state()).max_distance == 0.75
    vp = P.build().source(1).maxDistance(3).create()
    assert vp.max_distance == 3 and isinstance(vp.max_distance, int)
    assert isinstance(P.build().maxDistance(3.0).create().max_distance, int)
    from janusgraph_amd.computer import _int_bound
    assert [_int_bound(x) for x in (None, 3, 2.75, float("inf"), float("nan"))] == [-1, 3, 2, -1, -1]


def test_float_snapshot_and_the_default_one():
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    graph = jg.InMemoryGraph()
    v = [graph.add_vertex() for _ in range(3)]
    graph.add_edge(v[0], v[1], "E", weight=0.5)
    graph.add_edge(v[1], v[2], "E", weight=2)
    graph.add_edge(v[0], v[2], "E")
    vid, src, dst, w = graph.snapshot(weight_property="weight", float_weights=True)
    assert w.dtype == np.float64 and w[:2].tolist() == [0.5, 2.0] and np.isnan(w[2]) and len(vid) == 3
    assert graph.snapshot(float_weights=True)[3] is None
    # the default call: int32, truncated, WEIGHT_ABSENT
    vid2, src2, dst2, w2 = graph.snapshot(weight_property="weight")
    assert w2.dtype == np.int32 and w2.tolist() == [0, 2, int(_lib.WEIGHT_ABSENT)]
    for a, b in ((vid, vid2), (src, src2), (dst, dst2)):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(TypeError):
        graph.snapshot("weight", True)  # keyword-only


def test_header_and_bindings_declare_the_f64_entry_points():
    from janusgraph_amd import _lib
    header = open(os.path.join(ROOT, "include", "janusgpu.h")).read()
    assert re.search(r"#define\s+JG_ABI_VERSION\s+3\b", header)
    assert re.search(r"#define\s+JG_DISTF_ABSENT\b", header)
    for f in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", header), f
        assert f in _lib.EXPORTS, f
    assert re.search(r"jg_sssp_kept_dag_f64\(jg_graph\* g, const uint8_t\* target, double max_distance", header)
    for m in ("set_weights_f64", "sssp_keep_f64", "sssp_kept_row_f64", "sssp_kept_dag_f64_build", "sssp_kept_dag_f64_read",
              "sssp_kept_dag_f64", "sssp_kept_dag_edges_f64"):
        assert callable(getattr(_lib.Graph, m)), m
