"""The C-ABI library loads here (no GPU) and exports exactly what include/janusgpu.h declares."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "janusgpu.h")


def header_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(jg_\w+)\s*\(", text, flags=re.M)))


def test_header_declares_the_drop_in_surface():
    fns = header_functions()
    for f in ["jg_ctx_create", "jg_graph_build", "jg_pagerank", "jg_bfs", "jg_shortest_distance",
              "jg_connected_components", "jg_graph_destroy", "jg_last_error", "jg_ctx_last_stats"]:
        assert f in fns


def test_library_exports_every_declared_symbol():
    import janusgraph_amd._lib as L
    lib = L.load()
    fns = header_functions()
    assert sorted(fns) == sorted(L.EXPORTS)
    for f in fns:
        assert hasattr(lib, f), f
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(fns) <= exported


def test_abi_version_and_no_gpu_error_is_a_status():
    import janusgraph_amd as jg
    lib = jg.load()
    assert lib.jg_abi_version() == 3
    # asked in a child process: torch carries a HIP runtime of its own, and once that one has opened the
    # device in this process the library's finds none (every GPU test after this one then fails)
    probe = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                           ["-c", "import torch, sys; sys.exit(0 if torch.cuda.is_available() else 1)"],
                           capture_output=True, timeout=300)
    has_gpu = probe.returncode == 0
    if has_gpu:
        pytest.skip("a GPU is present")
    with pytest.raises(jg.JanusGpuError) as e:
        jg.Context((0,))
    assert e.value.code in (-3, -1)


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof/offsetof of jg_graph_info and jg_stats from gcc == the ctypes mirrors."""
    import ctypes
    import janusgraph_amd._lib as L
    src = tmp_path / "layout.c"
    fields_i = [f for f, _ in L.GraphInfo._fields_]
    fields_s = [f for f, _ in L.Stats._fields_]
    body = ["#include <stdio.h>", "#include <stddef.h>", '#include "janusgpu.h"', "int main(void){",
            'printf("%zu\\n", sizeof(jg_graph_info));', 'printf("%zu\\n", sizeof(jg_stats));']
    body += [f'printf("%zu\\n", offsetof(jg_graph_info, {f}));' for f in fields_i]
    body += [f'printf("%zu\\n", offsetof(jg_stats, {f}));' for f in fields_s]
    body += ["return 0;}"]
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [ctypes.sizeof(L.GraphInfo), ctypes.sizeof(L.Stats)]
    want += [getattr(L.GraphInfo, f).offset for f in fields_i] + [getattr(L.Stats, f).offset for f in fields_s]
    assert vals == want


def test_header_compiles_as_plain_c():
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-x", "c", HEADER])


def test_tune_keys_validate_without_a_gpu():
    """jg_tune_set accepts every documented knob and reports bad keys / values as JG_ERR_ARG."""
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    jg.load()
    for k, v in (("merge_temporal", 1), ("band1_bit", 3), ("merge_pack", 1), ("merge_stage0", -1), ("merge_stage1", -1),
                 ("bfs_grid_mult", 4), ("bfs_batch0", 10), ("msbfs_skip", 1), ("cc_first", 1), ("msbfs_sparse", 1),
                 ("cc_uf_sharded", 0), ("cc_uf_sharded", 1), ("cc_uf_search", 0), ("cc_uf_search", 1), ("cc_sparse", 0), ("cc_sparse", 1), ("msbfs_td", 2),
                 ("msbfs_td", 1), ("bfs_td_split", 2), ("bfs_td_split_levels", 2), ("bfs_td_split_min", 65536),
                 ("bfs_td_split_max", 1 << 20), ("bfs_tail_grid", 0), ("bfs_tail_grid", 64),
                 # retired knobs (variants measured slower and removed): accepted as no-ops
                 ("bfs_persistent", 1), ("light_lds", 0), ("pull_unroll", 4), ("pull_nt", 1), ("pull_overlap", 0),
                 ("msbfs_exit", 0), ("msbfs_exit", 2), ("msbfs_exit", 1), ("msbfs_exit_live", 1000), ("msbfs_exit_live", 950),
                 ("msbfs_td_noprobe", 0), ("msbfs_td_noprobe", 2), ("msbfs_exit_first", 3), ("msbfs_exit_first", 16),
                 ("msbfs_scan_queue", 0), ("msbfs_scan_queue", 1001), ("msbfs_scan_queue", 50),
                 ("msbfs_td_rowapply", 0), ("msbfs_td_rowapply", 4), ("bfs_narrow", 0), ("bfs_narrow", 1),
                 ("nb_alpha", 14), ("nb_alpha", 30), ("nb_first", 16), ("halo", 1), ("pull_split", 1), ("band0_sub", 64),
                 ("band0_bit", 0), ("band0_deg", 96), ("band1_bit", 0), ("band1_deg", -1), ("band2_deg", -1),
                 ("band2_bit", 0), ("sd_delta", 0), ("sd_delta", 64), ("sd_delta", -1),
                 ("sd_dist32", 0), ("sd_dist32", 1), ("sd_dist32", 2)):
        _lib.tune_set(k, v)
    # unknown keys (including the variants deleted in round 5: measured slower or equal) and bad values
    for k, v in (("band1_bit", 2), ("no_such_knob", 1), ("merge_pack", 20),
                 ("merge_stage0", 100), ("merge_stage4", 64), ("merge_diag", 0), ("merge_nt", 0), ("msbfs_srcsplit", 0),
                 ("msbfs_bu", 0), ("fin_pipe", 1), ("relabel_out_ties", 0), ("band_sliced_build", 0),
                 ("bfs_grid_mult", 0), ("bfs_batch0", 0), ("sd_delta", -2), ("cc_first", 0), ("cc_first", 65), ("bfs_tail_grid", -1),
                 ("msbfs_exit", 3), ("msbfs_exit_live", 1001), ("msbfs_td_noprobe", -1), ("msbfs_exit_first", 0),
                 ("msbfs_scan_queue", 1002), ("msbfs_td_rowapply", -1), ("nb_first", 3), ("nb_alpha", 0),
                 ("bfs_narrow", 2), ("msbfs_td", 3), ("bfs_td_split", 3), ("bfs_td_split_levels", -1),
                 ("bfs_td_split_min", 0), ("bfs_td_split_max", 1 << 31), ("sd_dist32", 3)):
        with pytest.raises(jg.JanusGpuError) as e:
            _lib.tune_set(k, v)
        assert e.value.code == -1
