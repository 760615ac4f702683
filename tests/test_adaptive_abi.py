"""The C-ABI of adaptive sampling (include/ptamd.h): exported symbols, the header's declarations against ptamd.device.EXPORTS, the two records as the
C compiler lays them out and as ptamd.device declares them to ctypes, and the refusals that need no device.  Runs without a GPU."""
import ctypes
import os
import re
import subprocess

from ptamd import device as D

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ["pt_set_adaptive", "pt_adaptive", "pt_adaptive_params_get", "pt_render_adaptive", "pt_adaptive_stats_get", "pt_read_adaptive",
           "pt_write_adaptive", "pt_adaptive_device_ptr", "pt_debug_adaptive_timing"]

PROBE = r"""
#include "ptamd.h"
#include <stddef.h>
#include <stdio.h>
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(pt_adaptive_params), offsetof(pt_adaptive_params, threshold), offsetof(pt_adaptive_params, min_samples),
        offsetof(pt_adaptive_params, round_samples), offsetof(pt_adaptive_params, max_samples), offsetof(pt_adaptive_params, _reserved));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(pt_adaptive_stats), offsetof(pt_adaptive_stats, rounds), offsetof(pt_adaptive_stats, blocks),
        offsetof(pt_adaptive_stats, active_blocks), offsetof(pt_adaptive_stats, nonfinite), offsetof(pt_adaptive_stats, min_count),
        offsetof(pt_adaptive_stats, max_count), offsetof(pt_adaptive_stats, samples_total), offsetof(pt_adaptive_stats, max_block_error),
        offsetof(pt_adaptive_stats, _reserved));
    printf("%zu %zu %zu %zu %zu\n", sizeof(pt_denoise_params), sizeof(pt_temporal_params), sizeof(pt_variance_params), sizeof(pt_response_params),
        sizeof(pt_firefly_params));
    return 0;
}
"""


def test_library_exports_the_symbols():
    lib = ctypes.CDLL(D.DEVICE_LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert not [s for s in SYMBOLS if s not in D.EXPORTS]


def test_the_header_declares_what_the_binding_exports():
    """every pt_*adaptive* function the header declares is in EXPORTS and in the library, and the other way round"""
    header = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    declared = set(re.findall(r"^(?:int|void\*|uint32_t)\s+(pt_\w*adaptive\w*)\(", header, re.M))
    assert declared == set(SYMBOLS) == {s for s in D.EXPORTS if "adaptive" in s}
    assert "const pt_adaptive_params* params); /* NULL: off */" in header


def test_record_layout_as_the_c_compiler_sees_it(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in lines[0].split()] == [32, 0, 4, 8, 12, 16]
    assert [int(x) for x in lines[1].split()] == [56, 0, 4, 8, 12, 16, 20, 24, 32, 36]
    assert [int(x) for x in lines[2].split()] == [32, 32, 32, 32, 32]  # the records of before keep their size


def test_ctypes_structures_agree():
    P, S = D.AdaptiveParams, D.AdaptiveStats
    assert ctypes.sizeof(P) == 32 and ctypes.sizeof(S) == 56
    assert [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16]
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 32, 36]
    assert P._reserved.size == 16 and S._reserved.size == 20 and S.samples_total.size == 8


def test_null_contexts_are_refused_without_a_device():
    lib = D.lib()
    prm, st = D.AdaptiveParams(0.01, 0, 0, 0), D.AdaptiveStats()
    timing = (ctypes.c_double * 4)()
    assert lib.pt_set_adaptive(None, ctypes.byref(prm)) == -1  # PT_ERR_INVALID
    assert lib.pt_set_adaptive(None, None) == -1
    assert lib.pt_adaptive_params_get(None, ctypes.byref(prm)) == -1
    assert lib.pt_render_adaptive(None, 1) == -1
    assert lib.pt_adaptive_stats_get(None, ctypes.byref(st)) == -1
    assert lib.pt_read_adaptive(None, None, None, None, None, None) == -1
    assert lib.pt_write_adaptive(None, None, None, None) == -1
    assert lib.pt_debug_adaptive_timing(None, timing) == -1
    assert lib.pt_adaptive(None) == 0
    assert not lib.pt_adaptive_device_ptr(None, 0)
