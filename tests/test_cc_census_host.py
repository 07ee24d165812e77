"""The component census's host side (no GPU): the three C-ABI names on every side, the two cluster map-reduces
mirrored from TinkerPop, and the helper the GPU tests use to order an expected census."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS_SYMBOLS = ("jg_cc_census", "jg_cc_census_read", "jg_cc_census_release")


def expected_census(labels, min_population=1):
    """(num_components, largest, vids, populations) of per-vertex component labels (vertex ids): the listed
    components have population >= min_population and are ordered by population descending, ties by the
    label's decimal String ascending (String.compareTo, as the program orders labels)."""
    labels = np.asarray(labels, np.int64)
    if len(labels) == 0:
        return 0, 0, np.zeros(0, np.int64), np.zeros(0, np.int64)
    ids, pops = np.unique(labels, return_counts=True)
    order = sorted(range(len(ids)), key=lambda j: (-int(pops[j]), str(int(ids[j]))))
    ids, pops = ids[order], pops[order].astype(np.int64)
    keep = pops >= min_population
    return len(order), int(pops[0]), ids[keep], pops[keep]


def test_expected_order_helper_kat():
    # ids 9, 10, 100: as Strings "10" < "100" < "9", as numbers 9 < 10 < 100
    labels = [9, 9, 10, 10, 100, 100, 7, 7, 7, 5]
    nc, largest, vids, pops = expected_census(labels)
    assert (nc, largest) == (5, 3)
    assert vids.tolist() == [7, 10, 100, 9, 5] and pops.tolist() == [3, 2, 2, 2, 1]
    nc, largest, vids, pops = expected_census(labels, 2)
    assert (nc, largest) == (5, 3) and vids.tolist() == [7, 10, 100, 9] and pops.tolist() == [3, 2, 2, 2]
    nc, largest, vids, pops = expected_census(labels, 4)
    assert (nc, largest, len(vids), len(pops)) == (5, 3, 0, 0)
    assert expected_census([])[:2] == (0, 0)


def test_symbols_in_exports_and_header():
    from janusgraph_amd import _lib
    header = open(os.path.join(ROOT, "include", "janusgpu.h")).read()
    for f in CENSUS_SYMBOLS:
        assert f in _lib.EXPORTS, f
        assert re.search(r"\bint " + f + r"\(jg_graph\* g", header), f
    assert re.search(r"#define JG_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3


def test_cluster_count_map_reduce():
    import janusgraph_amd as jg
    mr = jg.ClusterCountMapReduce.build().create()
    assert mr.memory_key == jg.ClusterCountMapReduce.DEFAULT_MEMORY_KEY == "clusterCount"
    assert mr.cluster_property == "gremlin.peerPressureVertexProgram.cluster"
    emitted = []
    for vid, props in [(1, {mr.cluster_property: "1"}), (2, {mr.cluster_property: "1"}), (3, {}),
                       (4, {mr.cluster_property: "4"}), (5, {"other": "9"})]:
        mr.map(vid, props, lambda k, v: emitted.append((k, v)))
    assert emitted == [(None, "1"), (None, "1"), (None, "4")]
    got = mr.generate_final_result(emitted)
    assert got == 2 and isinstance(got, int)
    assert mr.generate_final_result([]) == 0


def test_cluster_population_map_reduce():
    import janusgraph_amd as jg
    mr = jg.ClusterPopulationMapReduce.build().create()
    assert mr.memory_key == jg.ClusterPopulationMapReduce.DEFAULT_MEMORY_KEY == "clusterPopulation"
    emitted = []
    for vid, props in [(1, {mr.cluster_property: "10"}), (2, {mr.cluster_property: "9"}),
                       (3, {mr.cluster_property: "10"}), (4, {}), (5, {mr.cluster_property: "10"})]:
        mr.map(vid, props, lambda k, v: emitted.append((k, v)))
    assert emitted == [("10", 1), ("9", 1), ("10", 1), ("10", 1)]
    assert mr.generate_final_result(emitted) == {"10": 3, "9": 1}
    # a hand-made list, as the generic map-reduce loop hands it over
    assert mr.generate_final_result([("a", 1), ("b", 1), ("a", 1)]) == {"a": 2, "b": 1}
    assert mr.generate_final_result([]) == {}


def test_builders_and_memory_keys():
    import janusgraph_amd as jg
    key = jg.ConnectedComponentVertexProgram.COMPONENT
    for cls in (jg.ClusterCountMapReduce, jg.ClusterPopulationMapReduce):
        mr = cls.build().memoryKey("mine").clusterProperty(key).create()
        assert isinstance(mr, cls) and mr.memory_key == "mine" and mr.cluster_property == key
        assert cls.build().create().memory_key == cls.DEFAULT_MEMORY_KEY
        assert cls().memory_key == cls.DEFAULT_MEMORY_KEY
    assert "ClusterCountMapReduce" in jg.__all__ and "ClusterPopulationMapReduce" in jg.__all__


def test_census_route_choice():
    """The computer takes the census route only for ConnectedComponentVertexProgram + the two cluster
    map-reduces over its property + Persist.NOTHING (the one-shard condition is checked on the built graph)."""
    import janusgraph_amd as jg
    key = jg.ConnectedComponentVertexProgram.COMPONENT
    vp = jg.ConnectedComponentVertexProgram.build().create()

    def computer(persist, *mrs):
        c = jg.GpuGraphComputer(jg.InMemoryGraph()).persist(persist)
        for m in mrs:
            c.mapReduce(m)
        return c

    count = jg.ClusterCountMapReduce.build().clusterProperty(key).create()
    pop = jg.ClusterPopulationMapReduce.build().clusterProperty(key).create()
    assert computer(jg.Persist.NOTHING, count, pop)._census_route(vp)
    assert computer(jg.Persist.NOTHING, pop)._census_route(vp)
    assert not computer(jg.Persist.NOTHING)._census_route(vp)
    assert not computer(jg.Persist.VERTEX_PROPERTIES, count, pop)._census_route(vp)
    assert not computer(jg.Persist.NOTHING, count, jg.PageRankMapReduce())._census_route(vp)
    assert not computer(jg.Persist.NOTHING, jg.ClusterCountMapReduce.build().create())._census_route(vp)  # other key
    renamed = jg.ConnectedComponentVertexProgram.build().property("c").create()
    assert not computer(jg.Persist.NOTHING, count)._census_route(renamed)
    assert computer(jg.Persist.NOTHING, jg.ClusterCountMapReduce.build().clusterProperty("c").create())._census_route(renamed)
