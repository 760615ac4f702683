"""The C-ABI of the temporal variance (include/ptamd.h): exported symbols, the record as the C compiler lays it out and as ptamd.device
declares it to ctypes, the value of the new input.  Runs without a GPU."""
import ctypes
import os
import subprocess

from ptamd import device as D

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ["pt_set_temporal_variance", "pt_temporal_variance", "pt_read_temporal_variance", "pt_write_temporal_variance",
           "pt_temporal_variance_device_ptr"]

PROBE = r"""
#include "ptamd.h"
#include <stddef.h>
#include <stdio.h>
int main(void)
{
    printf("%zu %zu %zu %zu %zu\n", sizeof(pt_variance_params), offsetof(pt_variance_params, sigma_variance), offsetof(pt_variance_params, relative_floor),
        offsetof(pt_variance_params, full_history), offsetof(pt_variance_params, _reserved));
    printf("%d %d %d\n", (int)PT_DENOISE_INPUT_ACCUM, (int)PT_DENOISE_INPUT_TEMPORAL, (int)PT_DENOISE_INPUT_TEMPORAL_VARIANCE);
    printf("%zu %zu\n", sizeof(pt_denoise_params), sizeof(pt_temporal_params));
    return 0;
}
"""


def test_library_exports_the_five_symbols():
    lib = ctypes.CDLL(D.DEVICE_LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert not [s for s in SYMBOLS if s not in D.EXPORTS]


def test_record_layout_as_the_c_compiler_sees_it(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in lines[0].split()] == [32, 0, 4, 8, 12]
    assert [int(x) for x in lines[1].split()] == [0, 1, 2]
    assert [int(x) for x in lines[2].split()] == [32, 32]  # the records of before keep their size


def test_ctypes_structure_agrees():
    assert ctypes.sizeof(D.VarianceParams) == 32
    assert (D.VarianceParams.sigma_variance.offset, D.VarianceParams.relative_floor.offset, D.VarianceParams.full_history.offset) == (0, 4, 8)
    assert D.VarianceParams._reserved.offset == 12 and D.VarianceParams._reserved.size == 20
    assert D.DENOISE_INPUT_TEMPORAL_VARIANCE == 2
    assert D._denoise_input(False, None) == D.DENOISE_INPUT_ACCUM and D._denoise_input(True, None) == D.DENOISE_INPUT_TEMPORAL
    assert D._denoise_input(False, D.DENOISE_INPUT_TEMPORAL_VARIANCE) == 2
