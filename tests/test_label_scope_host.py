"""Label-scoped graphs (jg_builder_keep_labels / jg_builder_add_labeled_edges / jg_builder_finish_labels):
what can be checked without a GPU.  The device side is tests/test_gpu_label_scope.py."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "janusgpu.h")
CSRC = os.path.join(ROOT, "janusgraph_amd", "csrc")
NEW = ("jg_builder_keep_labels", "jg_builder_add_labeled_edges", "jg_builder_finish_labels")


def test_header_declares_the_entry_points_and_the_abi_stays_3():
    import janusgraph_amd._lib as L
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for f in NEW:
        assert re.search(r"^int " + f + r"\(jg_builder\* b", text, flags=re.M), f
        assert f in L.EXPORTS
    lib = L.load()
    assert lib.jg_abi_version() == 3 and L.ABI_VERSION == 3
    assert re.search(r"#define JG_ABI_VERSION 3\b", text)
    for f in NEW:
        assert hasattr(lib, f)
    cap = int(re.search(r"#define JG_MAX_SCOPE_LABELS (\d+)", text).group(1))
    assert cap == L.MAX_SCOPE_LABELS
    assert cap == int(re.search(r"kScopeMaxLabels = (\d+);", open(os.path.join(CSRC, "jg_labelset.h")).read()).group(1))


def test_exported_tile_size_is_the_kernels():
    import janusgraph_amd._lib as L
    internal = open(os.path.join(CSRC, "jg_internal.h")).read()
    ept = int(re.search(r"constexpr int kScopeEpt = (\d+);", internal).group(1))
    block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(CSRC, "jg_common.h")).read()).group(1))
    assert re.search(r"kScopeTile = \(int64_t\)kScopeEpt \* kBlock;", internal)
    assert L.SCOPE_TILE == ept * block


def test_null_builder_is_a_status_without_a_gpu():
    import janusgraph_amd._lib as L
    lib = L.load()
    assert lib.jg_builder_keep_labels(None) == L.JG_ERR_ARG
    assert lib.jg_builder_add_labeled_edges(None, None, None, None, None, 0) == L.JG_ERR_ARG
    assert lib.jg_builder_finish_labels(None, None, 0, 7, None) == L.JG_ERR_ARG


def test_edge_label_ids_follow_the_snapshot_order():
    import janusgraph_amd as jg
    g = jg.InMemoryGraph()
    v = jg.load_graph_of_the_gods(g)
    lab, ids = g.edge_label_ids()
    _, src, dst, _ = g.snapshot()
    assert lab.dtype == np.int64 and len(lab) == len(src) == len(g.edges)
    # ids by first appearance, deterministic
    assert ids == {"father": 0, "lives": 1, "brother": 2, "mother": 3, "battled": 4, "pet": 5}
    lab2, ids2 = g.edge_label_ids()
    assert np.array_equal(lab, lab2) and ids == ids2
    for i, e in enumerate(g.edges):
        assert (src[i], dst[i], lab[i]) == (e.out_id, e.in_id, ids[e.label])
    battled = lab == ids["battled"]
    assert set(src[battled].tolist()) == {v["hercules"].id} and battled.sum() == 3
    empty = jg.InMemoryGraph().edge_label_ids()
    assert len(empty[0]) == 0 and empty[0].dtype == np.int64 and empty[1] == {}


def test_combiner_labels_option():
    import janusgraph_amd as jg
    with pytest.raises(ValueError):
        jg.CombinerVertexProgram(labels=())
    assert jg.CombinerVertexProgram().labels is None and jg.DegreeCounter(2).labels is None
    p = jg.CombinerVertexProgram(1, "d", "sum", "inE", 1, True, labels=("battled", "pet"))
    assert p.labels == ("battled", "pet") and p.length == 1 and p.property_key == "d"
    assert jg.CombinerVertexProgram(labels=["lives"]).labels == ("lives",)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were checked")


def test_add_edges_rejects_a_label_length_mismatch_before_any_library_call(monkeypatch):
    import janusgraph_amd._lib as L
    b = L.Builder.__new__(L.Builder)  # no context, no handle: only the argument checks can run
    b._h = None
    monkeypatch.setattr(L, "_lib", _NoLibrary())
    src, dst = np.array([1, 2, 3]), np.array([2, 3, 1])
    with pytest.raises(ValueError, match="label"):
        b.add_edges(src, dst, label=[1, 2])
    with pytest.raises(ValueError, match="label"):
        b.add_edges(src, dst, weight=[1, 1, 1], label=np.zeros((3, 1), np.int64))
    with pytest.raises(ValueError, match="weight"):
        b.add_edges(src, dst, weight=[1], label=[1, 2, 3])


def test_label_set_preparation_under_asan_ubsan(tmp_path):
    """The host code of a scope (sort, dedup, cap: csrc/jg_labelset.h) in a stand-alone program of its own,
    compiled with AddressSanitizer + UBSan and run on the CPU."""
    exe = str(tmp_path / "label_set")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "san", "label_set_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    out = p.stdout + p.stderr
    assert p.returncode == 0 and " 0 bad" in out, out
    assert "AddressSanitizer" not in out and "runtime error" not in out, out
