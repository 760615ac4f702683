"""The C-ABI of the guide chain (include/ptamd.h, "guide chain"): exported symbols, the constant and the error codes as the C compiler sees
them, the records of before, what the entry points answer without a context, and the scene the feature is measured on.  Runs without a GPU."""
import ctypes
import os
import subprocess

import numpy as np

import chain_ref as CH
from ptamd import device as D, layout as L, scenes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ["pt_set_guide_chain", "pt_guide_chain", "pt_debug_guide_chain_terminals", "pt_debug_read_guide_chain_terminals"]

PROBE = r"""
#include "ptamd.h"
#include <stdio.h>
int main(void)
{
    printf("%u %d %d %d\n", (unsigned)PT_GUIDE_CHAIN_MAX, (int)PT_ERR_INVALID, (int)PT_ERR_STATE, (int)PT_ERR_UNSUPPORTED);
    printf("%zu %zu %zu %zu %zu\n", sizeof(pt_denoise_params), sizeof(pt_temporal_params), sizeof(pt_variance_params), sizeof(pt_response_params),
        sizeof(pt_config));
    return 0;
}
"""


def test_library_exports_the_symbols():
    lib = ctypes.CDLL(D.DEVICE_LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert not [s for s in SYMBOLS if s not in D.EXPORTS]


def test_constant_codes_and_the_records_of_before(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in lines[0].split()] == [CH.CHAIN_MAX, -1, -3, -4] and D.GUIDE_CHAIN_MAX == CH.CHAIN_MAX == 4
    assert [int(x) for x in lines[1].split()] == [32, 32, 32, 32, ctypes.sizeof(D.Config)]  # struct sizes unchanged
    assert ctypes.sizeof(D.DenoiseParams) == ctypes.sizeof(D.TemporalParams) == ctypes.sizeof(D.VarianceParams) == ctypes.sizeof(D.ResponseParams) == 32


def test_without_a_context():
    lib = D.lib()
    assert lib.pt_set_guide_chain(None, 2) == -1 and lib.pt_set_guide_chain(None, 9) == -1  # PT_ERR_INVALID
    assert lib.pt_guide_chain(None) == 0
    assert lib.pt_debug_guide_chain_terminals(None, 1) == -1 and lib.pt_debug_read_guide_chain_terminals(None, None) == -1


def test_the_scene_behind_glass():
    for rough, kind in ((False, L.MAT_BASIC_REFRACTIVE), (True, L.MAT_REFRACTIVE)):
        b = scenes.cornell_behind_glass(64, 64, rough=rough)
        flat = b.flat
        types = flat.materials["type"][flat.triangles["materialIndex"]]
        glass = np.flatnonzero(types == kind)
        assert len(glass) == 2 and len(flat.triangles) == len(scenes.cornell_box(64, 64).flat.triangles) + 2
        p = flat.vertices["vertex"][flat.triangles["indices"][glass].reshape(-1), :3]
        assert np.allclose(p.min(0), (-0.6, 0.2, -0.6)) and np.allclose(p.max(0), (0.6, 1.8, -0.6))
        n = flat.vertices["normal"][flat.triangles["indices"][glass].reshape(-1), :3]
        assert np.allclose(n, (0, 0, -1))  # towards the camera
        ior = flat.materials["refractiveIndexRough" if rough else "refractiveIndexBasic"][flat.triangles["materialIndex"][glass]]
        assert np.allclose(ior, 1.5)
