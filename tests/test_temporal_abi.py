"""The C-ABI of the sample base and the temporal history (include/ptamd.h): exported symbols, record sizes as the C compiler lays them out
and as ptamd.device declares them to ctypes.  Runs without a GPU."""
import ctypes
import os
import subprocess

from ptamd import device as D

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ["pt_temporal_accumulate", "pt_temporal_reset", "pt_temporal_frames", "pt_read_temporal", "pt_write_temporal", "pt_temporal_device_ptr",
           "pt_set_sample_base", "pt_sample_base"]

PROBE = r"""
#include "ptamd.h"
#include <stddef.h>
#include <stdio.h>
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(pt_temporal_params), offsetof(pt_temporal_params, max_history), offsetof(pt_temporal_params, k_normal),
        offsetof(pt_temporal_params, sigma_depth), sizeof(pt_denoise_params), offsetof(pt_denoise_params, input), offsetof(pt_denoise_params, _reserved),
        offsetof(pt_denoise_params, sigma_lum));
    printf("%d %d\n", (int)PT_DENOISE_INPUT_ACCUM, (int)PT_DENOISE_INPUT_TEMPORAL);
    return 0;
}
"""


def test_library_exports_the_new_symbols():
    lib = ctypes.CDLL(D.DEVICE_LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert not [s for s in SYMBOLS if s not in D.EXPORTS]


def test_record_layouts_as_the_c_compiler_sees_them(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in lines[0].split()] == [32, 0, 4, 8, 32, 20, 24, 16]
    assert [int(x) for x in lines[1].split()] == [0, 1]


def test_ctypes_structures_agree():
    assert ctypes.sizeof(D.TemporalParams) == 32
    assert (D.TemporalParams.max_history.offset, D.TemporalParams.k_normal.offset, D.TemporalParams.sigma_depth.offset) == (0, 4, 8)
    assert ctypes.sizeof(D.DenoiseParams) == 32
    assert D.DenoiseParams.input.offset == 20 and D.DenoiseParams._reserved.offset == 24 and D.DenoiseParams._reserved.size == 8
    assert [n for n, _ in D.DenoiseParams._fields_][:5] == ["iterations", "output", "k_normal", "sigma_depth", "sigma_lum"]
    assert (D.DENOISE_INPUT_ACCUM, D.DENOISE_INPUT_TEMPORAL) == (0, 1)
    prm = D.DenoiseParams(5, D.DENOISE_HDR, 1.0, 2.0, 3.0)  # the five positional fields of before; the new one defaults to the accumulator
    assert prm.input == D.DENOISE_INPUT_ACCUM and prm.sigma_lum == 3.0
