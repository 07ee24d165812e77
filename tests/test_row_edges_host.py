"""Edge ordinals, relation ids and fp64 weights of graphs built from edgestore rows: the CPU side.

The header declares the entry points; the encoders the fixtures use (tests/row_edges_stores.py) are pinned to
known answers; and every store the GPU tests (tests/test_gpu_row_edges.py) build is checked here against the
oracle's restatement of the scan (oracle.edgestore_snapshot with its entry indices, oracle.decode_edges for the
relation ids): the edge list known by construction, edge for edge and in order, is what the oracle lists, so the
GPU tests compare against a reference that is itself verified without a GPU.
"""
import os
import re

import numpy as np
import pytest

import row_edges_stores as rs
from oracle import edgecodec as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["jg_builder_keep_relations", "jg_builder_set_weight_key_f64", "jg_graph_edge_relations",
                "jg_bfs_kept_dag_read_relations", "jg_sssp_kept_dag_read_relations"]


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "janusgpu.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    assert re.search(r"^#define JG_ABI_VERSION 3$", text, re.M)
    from janusgraph_amd import _lib
    assert _lib.ABI_VERSION == 3 and all(name in _lib.EXPORTS for name in ENTRY_POINTS)


def test_library_exports_the_entry_points():
    from janusgraph_amd import _lib
    lib = _lib.load()
    assert lib.jg_abi_version() == 3
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None


def test_encoders_known_answers():
    assert rs.enc_double(1.0) == bytes.fromhex("3ff0000000000000")
    assert rs.enc_long(0) == bytes.fromhex("8000000000000000")
    assert rs.enc_long(-1) == bytes.fromhex("7fffffffffffffff")
    assert rs.enc_long((1 << 63) - 1) == b"\xff" * 8 and rs.enc_long(-(1 << 63)) == bytes(8)
    # the property as the value holds it: inline key id, flag byte 0, the 8 bytes
    wid = ec.write_positive(ec.inline_id(rs.W_KEY))
    assert rs.weight_value(ec.DOUBLE, 1.0) == wid + b"\x00" + bytes.fromhex("3ff0000000000000")
    assert rs.weight_value(ec.LONG, -1) == wid + b"\x00" + bytes.fromhex("7fffffffffffffff")
    assert rs.weight_value(ec.DOUBLE, "null") == wid + b"\xff"
    assert rs.weight_value(ec.INT, -3) == wid + b"\x00" + ec.write_signed(-3)


def assert_list_is_the_oracles(oracle_lib, st, store):
    """The construction's edge list against the oracle's: (src, dst), entry index and relation id of every listed
    edge, in order; V in row order."""
    keys, roff, data, off, vpos, tids, tmult = store
    ov, os_, ot, ent = oracle_lib.edgestore_snapshot(keys, roff, data, off, vpos, tids, tmult, return_entries=True)
    src, dst, rel, entry = st.listed()
    np.testing.assert_array_equal(ov, st.vertices())
    np.testing.assert_array_equal(ent, entry)
    np.testing.assert_array_equal(os_, src)
    np.testing.assert_array_equal(ot, dst)
    orel = oracle_lib.decode_edges(np.frombuffer(data, np.uint8), off, vpos, tids, tmult)[3]
    np.testing.assert_array_equal(np.asarray(orel)[ent], rel)
    assert len(set(rel.tolist())) == len(rel)  # every edge has a relation id of its own
    return ov, src, dst, rel


def test_random_store_against_the_oracle(oracle_lib):
    st = rs.store_random()
    store = st.build()
    v, src, dst, rel = assert_list_is_the_oracles(oracle_lib, st, store)
    assert len(st.rows) >= 400 and len(st.ends) == 3000
    inside = np.isin(dst, v)
    assert 0 < int((~inside).sum()) < len(rel) and np.isin(src, v).all()  # ghost-ended edges are listed
    assert int((src == dst).sum()) >= 40  # self-loops
    pairs = {}
    for a, b in zip(src.tolist(), dst.tolist()):
        pairs[(a, b)] = pairs.get((a, b), 0) + 1
    assert max(pairs.values()) >= 50  # parallel edges
    mults = {int(m) for m in oracle_lib.decode_edges(np.frombuffer(store[2], np.uint8), store[3], store[4],
                                                     store[5], store[6])[0][st.listed()[3]]}
    assert mults == set(rs.LABELS)
    assert any(v_ & 7 == 2 for v_ in v.tolist())  # a vertex-cut vertex


def test_tile_store_against_the_oracle(oracle_lib):
    st, hub = rs.store_tiles()
    store = st.build()
    keys, roff = store[0], store[1]
    assert_list_is_the_oracles(oracle_lib, st, store)
    h = st.order().index(hub)
    assert roff[h] == 2 * rs.CHUNK and rs.CHUNK in roff.tolist()  # rows start and end on iteration boundaries
    src, dst, rel, entry = st.listed()
    out = entry[src == hub]
    assert len(out) == 2 * rs.CHUNK + 3 + 1  # the hub's OUT entries (and its self-loop)
    assert {int(e) // rs.CHUNK for e in out.tolist()} == {2, 3, 4}  # three block iterations
    assert roff[h + 1] < 5 * rs.CHUNK and h + 1 < len(keys)


def test_diamond_store_against_the_oracle(oracle_lib):
    st, (s, a, b, t), rel = rs.diamond()
    store = st.build()
    v, src, dst, r = assert_list_is_the_oracles(oracle_lib, st, store)
    got = {int(x): (int(p), int(q)) for p, q, x in zip(src, dst, r)}
    assert got == {rel["sa"]: (s, a), rel["sb"]: (s, b), rel["at1"]: (a, t), rel["at2"]: (a, t), rel["bt"]: (b, t)}


def test_star_store_alignment(oracle_lib):
    st, hub, w = rs.store_star()
    store = st.build()
    assert_list_is_the_oracles(oracle_lib, st, store)
    src, dst, rel, entry = st.listed()
    assert len(rel) == 1500 and (src == hub).all() and len(set(dst.tolist())) == 1500
    at = rs.weight_offsets(store, entry)
    assert set((at % 8).tolist()) == set(range(8))  # the weight's first byte at every residue mod 8
    assert int(at.max()) + 8 == len(store[2])       # a weight whose last byte is the last byte of the store
    bits = np.array([int.from_bytes(store[2][a:a + 8], "big") for a in at.tolist()], np.uint64).view(np.float64)
    np.testing.assert_array_equal(bits.view(np.int64), np.array([w[d] for d in dst.tolist()]).view(np.int64))
    assert bits.min() >= 0.5 and bits.max() < 2.0


@pytest.mark.parametrize("wtype", [ec.INT, ec.LONG, ec.DOUBLE])
def test_weighted_random_stores_against_the_oracle(oracle_lib, wtype):
    st = rs.store_random(seed=7, value_of=lambda e, rng: rs.weight_value(wtype, 1 + e % 9, rng))
    assert_list_is_the_oracles(oracle_lib, st, st.build())
