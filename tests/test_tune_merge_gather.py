"""The launch-time knobs of the merge kernel's gather half (jg_tune_set; no GPU needed)."""
import pytest


def test_merge_hot_and_off32_ranges():
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    jg.load()
    try:
        for k, v in (("merge_hot", 0), ("merge_hot", 128), ("merge_hot", 1 << 30), ("merge_hot", -1),
                     ("merge_off32", 0), ("merge_off32", 1)):
            _lib.tune_set(k, v)
        for k, v in (("merge_hot", -2), ("merge_hot", (1 << 30) + 1), ("merge_off32", 2), ("merge_off32", -1)):
            with pytest.raises(jg.JanusGpuError) as e:
                _lib.tune_set(k, v)
            assert e.value.code == -1
    finally:
        _lib.tune_set("merge_hot", -1)
        _lib.tune_set("merge_off32", 1)
