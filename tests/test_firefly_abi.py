"""The C-ABI of the firefly clamp (include/ptamd.h): exported symbols, the header's declarations against ptamd.device.EXPORTS, the record as the C
compiler lays it out and as ptamd.device declares it to ctypes, the defaults, and the refusals that need no device.  Runs without a GPU."""
import ctypes
import os
import re
import subprocess

import firefly_ref as F
from ptamd import device as D

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ["pt_set_firefly_clamp", "pt_firefly_clamp", "pt_read_firefly", "pt_firefly_counts", "pt_firefly_device_ptr"]

PROBE = r"""
#include "ptamd.h"
#include <stddef.h>
#include <stdio.h>
int main(void)
{
    printf("%zu %zu %zu %zu\n", sizeof(pt_firefly_params), offsetof(pt_firefly_params, rank), offsetof(pt_firefly_params, scale),
        offsetof(pt_firefly_params, _reserved));
    printf("%d %u %u %.9g\n", (int)PT_FIREFLY_RADIUS, (unsigned)PT_FIREFLY_MAX_RANK, (unsigned)PT_FIREFLY_DEFAULT_RANK, (double)PT_FIREFLY_DEFAULT_SCALE);
    printf("%zu %zu %zu %zu\n", sizeof(pt_denoise_params), sizeof(pt_temporal_params), sizeof(pt_variance_params), sizeof(pt_response_params));
    return 0;
}
"""


def test_library_exports_the_five_symbols():
    lib = ctypes.CDLL(D.DEVICE_LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert not [s for s in SYMBOLS if s not in D.EXPORTS]


def test_the_header_declares_what_the_binding_exports():
    """every pt_*firefly* function the header declares is in EXPORTS and in the library, and the other way round"""
    header = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    declared = set(re.findall(r"^(?:int|void\*|uint32_t)\s+(pt_\w*firefly\w*)\(", header, re.M))
    assert declared == set(SYMBOLS) == {s for s in D.EXPORTS if "firefly" in s}
    assert "const pt_firefly_params* params); /* NULL: off */" in header


def test_record_layout_as_the_c_compiler_sees_it(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in lines[0].split()] == [32, 0, 4, 8]
    radius, max_rank, rank, scale = lines[1].split()
    assert (int(radius), int(max_rank)) == (F.RADIUS, F.MAX_RANK) == (D.FIREFLY_RADIUS, D.FIREFLY_MAX_RANK) == (2, 4)
    assert (int(rank), float(scale)) == (F.RANK, F.SCALE)  # the scan's choice (tests/test_firefly_ref.py)
    assert [int(x) for x in lines[2].split()] == [32, 32, 32, 32]  # the records of before keep their size


def test_ctypes_structure_agrees():
    assert ctypes.sizeof(D.FireflyParams) == 32
    assert (D.FireflyParams.rank.offset, D.FireflyParams.scale.offset) == (0, 4)
    assert D.FireflyParams._reserved.offset == 8 and D.FireflyParams._reserved.size == 24


def test_null_contexts_are_refused_without_a_device():
    lib = D.lib()
    prm = D.FireflyParams(0, 0.0)
    counts = (ctypes.c_uint32 * 2)()
    assert lib.pt_set_firefly_clamp(None, ctypes.byref(prm)) == -1  # PT_ERR_INVALID
    assert lib.pt_set_firefly_clamp(None, None) == -1
    assert lib.pt_read_firefly(None, None, counts) == -1
    assert lib.pt_firefly_counts(None, counts) == -1
    assert lib.pt_firefly_clamp(None) == 0
    assert not lib.pt_firefly_device_ptr(None)
