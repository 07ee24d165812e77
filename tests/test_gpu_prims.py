"""The device primitives of csrc/jg_prim.hip, each alone against plain host code, at the sizes where their tile
structure changes (jg_tune_set("prim_probe", ...), csrc/jg_prim_probe.hip).

About forty call sites (the CSR build, the path DAGs, the census, top-k, peer pressure, label scopes, the decoder,
the halo plan) rest on exclusive_scan, exclusive_scan_async, radix_sort and compact_indices at sizes their data
decides.  One probe call generates an input on the host, runs one primitive on the device and compares the result
element for element with std::stable_sort, a running int64 sum or a loop over the flags; a case passes when the call
returns.  The sizes are the smallest at which each mechanism changes:
  scans   kScanTile = 2048 elements per block: two levels above 2048, three above 2048^2 (2048^2 + 2049: a partial
          last tile on both upper levels); out[n], the total, is checked with the rest, and the asynchronous scans
          get exactly scan_scratch_size(n) of scratch with a canary run behind it;
  sorts   kRadixTile = 4096 keys per block, 1024 per wave in 16 rounds of 64; the count table's scan goes to two
          levels from 9 tiles (32769 keys) on; bits 1, 5, 8, 9, 16, 33, 40, 64 give 1, 1, 1, 2, 2, 5, 5, 8 passes,
          both parities of the copy-back from the temporaries;
  flags   the scans' sizes up to 4097 and 2048^2 + 1; the scratch overload is called on n / 2 and then on n flags
          with the same two buffers.
Not the full product but a cross: every size with the random pattern (the sorts at bits 5, 33 and 64), every bits
at 4097 and 32769 keys, every pattern at the tile edge (2049 for scans and flags, 4097 keys at 16 bits).
"""
import pytest

pytestmark = pytest.mark.gpu

T2 = 2048 * 2048
SCAN_SIZES = (0, 1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4097, T2 - 1, T2, T2 + 1, T2 + 2049)
SORT_SIZES = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 32768, 32769, 100003)
SORT_BITS = (1, 5, 8, 9, 16, 33, 40, 64)
FLAG_SIZES = tuple(n for n in SCAN_SIZES if n <= 4097) + (T2 + 1,)

SCAN_OPS = {0: "scan_i32", 1: "scan_i64", 2: "scan_u32", 3: "scan_async_u8", 4: "scan_async_u32"}
SORT_OPS = {5: "sort_keys", 6: "sort_pairs"}
FLAG_OPS = {7: "compact", 8: "compact_scratch"}
SCAN_PATTERNS = ("random", "zero", "max", "last_only")
FLAG_PATTERNS = ("random", "none", "all", "first_only", "last_only")
SORT_PATTERNS = ("random", "equal", "ascending", "descending", "top_digit", "two_values")


def cross():
    cases = {}  # (op, pattern, bits, n) -> id; a dict, so a case two arms of the cross reach runs once

    def add(names, op, patterns, p, bits, n):
        cases.setdefault((op, p, bits, n), f"{names[op]}-{patterns[p]}-" + (f"b{bits}-" if op in SORT_OPS else "") + f"n{n}")

    for op in SCAN_OPS:
        for n in SCAN_SIZES:
            add(SCAN_OPS, op, SCAN_PATTERNS, 0, 8, n)
        for p in range(len(SCAN_PATTERNS)):
            add(SCAN_OPS, op, SCAN_PATTERNS, p, 8, 2049)
    for op in SORT_OPS:
        for bits in (5, 33, 64):
            for n in SORT_SIZES:
                add(SORT_OPS, op, SORT_PATTERNS, 0, bits, n)
        for bits in SORT_BITS:
            for n in (4097, 32769):
                add(SORT_OPS, op, SORT_PATTERNS, 0, bits, n)
        for p in range(len(SORT_PATTERNS)):
            add(SORT_OPS, op, SORT_PATTERNS, p, 16, 4097)
    for op in FLAG_OPS:
        for n in FLAG_SIZES:
            add(FLAG_OPS, op, FLAG_PATTERNS, 0, 8, n)
        for p in range(len(FLAG_PATTERNS)):
            add(FLAG_OPS, op, FLAG_PATTERNS, p, 8, 2049)
    return cases


CASES = cross()


@pytest.fixture(scope="module")
def ctx():
    """The probe runs on the calling thread's current device: a context is held open around it."""
    import janusgraph_amd as jg
    c = jg.Context((0,))
    yield c
    c.close()


def test_the_cross_is_what_it_says():
    assert len(CASES) == 5 * (16 + 3) + 2 * (3 * 16 + (8 - 3) * 2 + 5) + 2 * (13 + 4) == 255
    assert len(set(CASES.values())) == len(CASES)


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES.values()))
def test_primitive(ctx, case):
    from janusgraph_amd import _lib
    _lib.prim_probe(*case)
