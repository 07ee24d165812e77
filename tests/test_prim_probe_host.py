"""jg_tune_set("prim_probe", op | pattern << 4 | bits << 8 | n << 16) refuses a bad argument before it touches
the device (csrc/jg_prim_probe.hip, jg_prim_probe_host.h unpack): every case here is JG_ERR_ARG on a machine
without a GPU, where anything that reached the device would be JG_ERR_HIP instead."""
import pytest

N_CAP = 1 << 25

BAD = {
    "op_9": (9, 0, 8, 100),
    "op_15": (15, 0, 8, 100),
    "scan_pattern_4": (0, 4, 8, 100),
    "async_scan_pattern_4": (3, 4, 8, 100),
    "scan_pattern_15": (2, 15, 8, 100),
    "sort_pattern_6": (5, 6, 8, 100),
    "sort_pairs_pattern_6": (6, 6, 8, 100),
    "flags_pattern_5": (7, 5, 8, 100),
    "scratch_flags_pattern_5": (8, 5, 8, 100),
    "bits_0_sort": (5, 0, 0, 100),
    "bits_0_scan": (0, 0, 0, 100),
    "bits_65": (6, 0, 65, 100),
    "bits_255": (5, 0, 255, 100),
    "n_minus_1": (0, 0, 8, -1),
    "n_minus_2_pow_40": (5, 0, 8, -(1 << 40)),
    "n_cap_plus_1": (1, 0, 8, N_CAP + 1),
    "n_2_pow_40": (7, 0, 8, 1 << 40),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_argument(name):
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    jg.load()
    with pytest.raises(jg.JanusGpuError) as e:
        _lib.prim_probe(*BAD[name])
    assert e.value.code == _lib.JG_ERR_ARG and "prim_probe" in str(e.value)


def test_raw_values_outside_the_packing():
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    jg.load()
    for value in (-1, -(1 << 63), (1 << 63) - 1):
        with pytest.raises(jg.JanusGpuError) as e:
            _lib.tune_set("prim_probe", value)
        assert e.value.code == _lib.JG_ERR_ARG


def test_packing_helper(monkeypatch):
    """_lib.prim_probe packs op | pattern << 4 | bits << 8 | n << 16 and hands it to tune_set under the probe's key."""
    from janusgraph_amd import _lib
    seen = []
    monkeypatch.setattr(_lib, "tune_set", lambda key, value: seen.append((key, value)))
    _lib.prim_probe(6, 5, 64, N_CAP)
    _lib.prim_probe(0, 0, 1, 0)
    assert seen == [("prim_probe", 6 | 5 << 4 | 64 << 8 | N_CAP << 16), ("prim_probe", 1 << 8)]
