"""Label-scoped path, component and cluster programs, host side: the `edgeLabels` key of
ShortestPathVertexProgram, ConnectedComponentVertexProgram and PeerPressureVertexProgram, and the two entry
points behind numbered scopes (jg_builder_keep_scope_ordinals, jg_graph_scope_positions).  Nothing here needs a
GPU; tests/test_gpu_scope_edges.py runs the scopes.
"""
import os
import re

import pytest

from janusgraph_amd import programs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAMS = (P.ShortestPathVertexProgram, P.ConnectedComponentVertexProgram, P.PeerPressureVertexProgram)
NEW_ENTRY_POINTS = ("jg_builder_keep_scope_ordinals", "jg_graph_scope_positions")


@pytest.mark.parametrize("cls", PROGRAMS)
def test_programs_accept_edge_labels(cls):
    assert cls({}).edge_labels is None  # the default: every edge
    assert cls({"edgeLabels": None}).edge_labels is None
    assert cls({"edgeLabels": ("knows",)}).edge_labels == ("knows",)
    assert cls({"edgeLabels": ["brother", "father"]}).edge_labels == ("brother", "father")
    assert cls({"edgeLabels": "knows"}).edge_labels == ("knows",)  # one name, as CombinerVertexProgram.labels


@pytest.mark.parametrize("cls", PROGRAMS)
def test_builders_round_trip_edge_labels(cls):
    vp = cls.build().edgeLabels("brother", "father").create()
    assert vp.edge_labels == ("brother", "father")
    state = vp.store_state()
    assert state["edgeLabels"] == ("brother", "father")
    assert state[P.VertexProgram.VERTEX_PROGRAM] == cls.__name__
    again = cls(state)
    assert again.edge_labels == ("brother", "father")
    assert again.store_state() == state
    assert "edgeLabels" not in cls.build().create().store_state()


@pytest.mark.parametrize("cls", PROGRAMS)
@pytest.mark.parametrize("bad", [(), ("",), ("knows", ""), (1,), ("knows", None), (b"knows",), 7])
def test_bad_edge_labels_are_rejected(cls, bad):
    with pytest.raises(ValueError):
        cls({"edgeLabels": bad})
    if isinstance(bad, tuple):
        with pytest.raises(ValueError):
            cls.build().edgeLabels(*bad)


def test_edge_labels_keep_the_other_keys():
    vp = (P.ShortestPathVertexProgram.build().source(256).edgeLabels("knows").edgeDirection("out").maxDistance(3)
          .includeEdges(True).create())
    assert (vp.sources, vp.edge_labels, vp.edge_direction, vp.max_distance, vp.include_edges) == \
        ([256], ("knows",), "out", 3, True)
    with pytest.raises(ValueError):  # includeEdges with a distanceProperty stays refused, scoped or not
        P.ShortestPathVertexProgram({"includeEdges": True, "distanceProperty": "w", "edgeLabels": ("knows",)})
    pp = P.PeerPressureVertexProgram.build().edges("bothE").edgeLabels("knows").create()
    assert (pp.edges, pp.edge_labels) == ("bothE", ("knows",))


def test_bindings_declare_the_entry_points():
    from janusgraph_amd import _lib
    src = open(os.path.join(ROOT, "janusgraph_amd", "_lib.py")).read()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.EXPORTS, name
        assert re.search(r'"%s":\s*\(\[' % name, src), name  # declared with its argtypes
    assert callable(_lib.Builder.keep_scope_ordinals) and callable(_lib.Graph.scope_positions)


def test_header_names_the_entry_points():
    header = open(os.path.join(ROOT, "include", "janusgpu.h")).read()
    assert re.search(r"\bint jg_builder_keep_scope_ordinals\(jg_builder\* b\);", header)
    assert re.search(r"\bint jg_graph_scope_positions\(const jg_graph\* g, int64_t first, int64_t count, "
                     r"int64_t\* pos_out\);", header)
    assert "#define JG_ABI_VERSION 3" in header
    note = header[header.index("Still 3"):header.index("#define JG_ABI_VERSION")]
    for name in NEW_ENTRY_POINTS:
        assert name in note, name
