"""The chunk limits of the one-shot edgestore build (jg_tune_set; no GPU needed)."""
import pytest

DEFAULTS = {"edgestore_chunk_entries": 4 << 20, "edgestore_chunk_bytes": 64 << 20}  # add_in_chunks, jg_decode.hip


def test_chunk_limit_ranges():
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    jg.load()
    try:
        for key in DEFAULTS:
            for v in (1, 1000, 1 << 40):
                _lib.tune_set(key, v)
            for v in (0, -1):
                with pytest.raises(jg.JanusGpuError) as e:
                    _lib.tune_set(key, v)
                assert e.value.code == -1
    finally:
        for key, v in DEFAULTS.items():
            _lib.tune_set(key, v)
