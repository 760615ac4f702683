"""The C-ABI of the temporal response (include/ptamd.h): exported symbols, the record as the C compiler lays it out and as ptamd.device
declares it to ctypes, the defaults, the records of before.  Runs without a GPU."""
import ctypes
import os
import subprocess

import response_ref as P
from ptamd import device as D

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ["pt_set_temporal_response", "pt_temporal_response", "pt_read_temporal_fast", "pt_write_temporal_fast", "pt_read_temporal_response",
           "pt_temporal_fast_device_ptr"]

PROBE = r"""
#include "ptamd.h"
#include <stddef.h>
#include <stdio.h>
int main(void)
{
    printf("%zu %zu %zu %zu %zu\n", sizeof(pt_response_params), offsetof(pt_response_params, fast_history), offsetof(pt_response_params, sigma_response),
        offsetof(pt_response_params, relative_floor), offsetof(pt_response_params, _reserved));
    printf("%d %u %.9g %.9g\n", (int)PT_RESPONSE_RADIUS, (unsigned)PT_RESPONSE_DEFAULT_FAST_HISTORY, (double)PT_RESPONSE_DEFAULT_SIGMA_RESPONSE,
        (double)PT_RESPONSE_DEFAULT_RELATIVE_FLOOR);
    printf("%zu %zu %zu\n", sizeof(pt_denoise_params), sizeof(pt_temporal_params), sizeof(pt_variance_params));
    return 0;
}
"""


def test_library_exports_the_six_symbols():
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
    radius, fast, sigma, floor = lines[1].split()
    assert (int(radius), int(fast)) == (P.RADIUS, P.FAST_HISTORY) == (3, 4)
    assert float(sigma) == P.SIGMA_RESPONSE == 2.0 and abs(float(floor) - P.RELATIVE_FLOOR) < 1e-8  # (0.02f, printed as a float)
    assert [int(x) for x in lines[2].split()] == [32, 32, 32]  # the records of before keep their size


def test_ctypes_structure_agrees():
    assert ctypes.sizeof(D.ResponseParams) == 32
    assert (D.ResponseParams.fast_history.offset, D.ResponseParams.sigma_response.offset, D.ResponseParams.relative_floor.offset) == (0, 4, 8)
    assert D.ResponseParams._reserved.offset == 12 and D.ResponseParams._reserved.size == 20
    assert ctypes.sizeof(D.TemporalParams) == 32 and ctypes.sizeof(D.DenoiseParams) == 32 and ctypes.sizeof(D.VarianceParams) == 32
