"""The order of jg_pagerank_top stated in numpy (expected_top), PageRankTopMapReduce's final result, and the
three entry points' symbols: everything about the PageRank top list that needs no GPU.

The order: rank descending by numeric value, ties by index ascending; -0.0 orders as +0.0, NaN orders below
every number and ties with other NaNs.
"""
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "janusgpu.h")
TOP_FUNCTIONS = ["jg_pagerank_top", "jg_pagerank_top_read", "jg_pagerank_top_release"]


def expected_top(rank, k):
    """Indices of the min(k, n) first entries of `rank` under the order above."""
    rank = np.asarray(rank, np.float64)
    nan = np.isnan(rank)
    folded = np.where(nan, 0.0, rank) + 0.0   # -0.0 + 0.0 == +0.0
    order = np.lexsort((np.arange(len(rank)), -folded, nan))  # last key first: NaN last, rank desc, index asc
    return order[:max(min(int(k), len(rank)), 0)].astype(np.int64)


def brute_top(rank, k):
    def key(i):
        r = float(rank[i])
        if math.isnan(r):
            return (1, 0.0, i)
        return (0, -r if r != 0 else 0.0, i)
    return sorted(range(len(rank)), key=key)[:k]


VECTORS = [
    [0.5, 0.25, 0.5, 0.125, 0.5, 0.25],                                   # duplicates
    [0.0, -0.0, 0.0, -0.0, 1.0, -1.0],                                    # both zeros: one tie class
    [-1.0, -2.0, -0.5, -2.0, 3.0, -1e300, 1e-300, -1e-300],               # negatives, tiny magnitudes
    [np.inf, -np.inf, 1.0, np.inf, -np.inf, 0.0],                         # infinities
    [np.nan, 1.0, np.nan, -np.inf, 0.0, -0.0, np.nan, np.inf],            # NaN below -inf, NaNs tie by index
    [np.nan, np.nan, np.nan],
    [5e-324, 0.0, -5e-324, 2.2250738585072014e-308],                      # subnormals
    [],
    [7.0],
]


def test_expected_top_matches_a_brute_force_sort():
    for v in VECTORS:
        a = np.array(v, np.float64)
        for k in (1, 2, 3, len(a), len(a) + 5):
            assert list(expected_top(a, k)) == brute_top(a, k), (v, k)
    # a NaN with the sign bit set is still a NaN
    a = np.array([1.0, 0.0, 2.0, 0.0], np.float64)
    a.view(np.uint64)[1] = 0xFFF8000000000001
    assert list(expected_top(a, 4)) == [2, 0, 3, 1]
    rng = np.random.default_rng(3)
    a = rng.choice(np.array([0.0, -0.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 1e-9]), 500)
    for k in (1, 17, 499, 500, 900):
        assert list(expected_top(a, k)) == brute_top(a, k)


def test_expected_top_one_tie_class_lists_the_smallest_indices():
    a = np.full(1000, 1.0 / 1000)
    np.testing.assert_array_equal(expected_top(a, 37), np.arange(37))


def test_map_reduce_final_result():
    from janusgraph_amd import PageRankTopMapReduce, PageRankVertexProgram
    emitted = [(70, 0.25), (10, 0.5), (30, 0.25), (20, float("nan")), (50, 0.5), (60, -0.0), (40, 0.0)]
    mr = PageRankTopMapReduce.build().limit(4).create()
    assert mr.memory_key == "pageRankTop" and mr.k == 4
    assert mr.generate_final_result(list(emitted)) == [(10, 0.5), (50, 0.5), (70, 0.25), (30, 0.25)]  # emission order
    whole = PageRankTopMapReduce(100).generate_final_result(list(emitted))   # k > len: everything, NaN last
    assert [v for v, _ in whole] == [10, 50, 70, 30, 60, 40, 20]
    assert PageRankTopMapReduce(1).generate_final_result(list(emitted)) == [(10, 0.5)]
    assert PageRankTopMapReduce(3).generate_final_result([]) == []
    mr = PageRankTopMapReduce.build().memoryKey("best").limit(2).create()
    assert mr.memory_key == "best" and mr.k == 2
    got = []
    mr.map(5, {PageRankVertexProgram.PAGE_RANK: 0.75}, lambda k, v: got.append((k, v)))
    mr.map(6, {}, lambda k, v: got.append((k, v)))
    assert got == [(5, 0.75)]


def test_header_declares_and_library_exports_the_entry_points():
    import janusgraph_amd._lib as L
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(jg_\w+)\s*\(", text, flags=re.M))
    lib = L.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for f in TOP_FUNCTIONS:
        assert f in declared and f in L.EXPORTS and f in exported, f
        assert getattr(lib, f).argtypes is not None, f
    assert "#define JG_ABI_VERSION 3" in open(HEADER).read()
