"""The C-ABI of the guide reflections (include/ptamd.h, "guide reflections"): exported symbols, the records of before as the C compiler sees them,
what the entry points answer without a context, and the three scenes the feature is tested on.  Runs without a GPU."""
import ctypes
import os
import subprocess

import numpy as np

import mirror_ref as M
from ptamd import device as D, layout as L, scenes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ["pt_set_guide_reflections", "pt_guide_reflections"]

PROBE = r"""
#include "ptamd.h"
#include <stdio.h>
int main(void)
{
    int (*set)(pt_ctx*, int) = pt_set_guide_reflections;
    int (*get)(const pt_ctx*) = pt_guide_reflections;
    printf("%d %d %d %d\n", (int)PT_ERR_INVALID, (int)PT_ERR_STATE, (int)PT_ERR_UNSUPPORTED, set != 0 && get != 0);
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


def test_the_records_of_before(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L" + os.path.dirname(D.DEVICE_LIB_PATH), "-lptamd", "-Wl,-rpath," + os.path.dirname(D.DEVICE_LIB_PATH)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in lines[0].split()] == [-1, -3, -4, 1]
    assert [int(x) for x in lines[1].split()] == [32, 32, 32, 32, ctypes.sizeof(D.Config)]  # struct sizes unchanged
    assert ctypes.sizeof(D.DenoiseParams) == ctypes.sizeof(D.TemporalParams) == ctypes.sizeof(D.VarianceParams) == ctypes.sizeof(D.ResponseParams) == 32


def test_without_a_context():
    lib = D.lib()
    assert lib.pt_set_guide_reflections(None, 1) == -1 and lib.pt_set_guide_reflections(None, 0) == -1  # PT_ERR_INVALID
    assert lib.pt_guide_reflections(None) == 0


def _mirror_triangles(flat):
    mirror = np.flatnonzero(M.is_mirror(flat.materials[flat.triangles["materialIndex"]]))
    idx = flat.triangles["indices"][mirror].reshape(-1)
    return mirror, flat.vertices["vertex"][idx, :3], flat.vertices["normal"][idx, :3], flat.materials[flat.triangles["materialIndex"][mirror]]


def test_the_mirror_wall():
    for smoothness in (1.0, 0.97):
        b = scenes.cornell_mirror_wall(64, 64, smoothness=smoothness)
        mirror, p, n, mat = _mirror_triangles(b.flat)
        assert len(mirror) == 2 and len(b.flat.triangles) == len(scenes.cornell_box(64, 64).flat.triangles) + 2
        assert np.allclose(p.min(0), (-0.8, 0.2, 0.99)) and np.allclose(p.max(0), (0.8, 1.8, 0.99))
        assert np.allclose(n, (0, 0, -1))  # into the room
        assert (mat["type"] == L.MAT_PBR).all() and (mat["metallic"] != 0).all() and (mat["smoothness"] > np.float32(0.94)).all()
        assert np.allclose(mat["colour"][:, :3], 0.9) and np.allclose(mat["smoothness"], smoothness)
    # below shading's threshold, or a dielectric: not a mirror
    assert len(_mirror_triangles(scenes.cornell_mirror_wall(64, 64, smoothness=0.94).flat)[0]) == 0
    assert not M.is_mirror(np.asarray([L.material_pbr_dielectric((0.9, 0.9, 0.9), 1.0)])).any()
    assert not np.isin(b.flat.materials["type"], (L.MAT_REFRACTIVE, L.MAT_BASIC_REFRACTIVE)).any()  # a mirror and no glass


def test_the_corridor():
    b = scenes.mirror_corridor(64, 36)
    mirror, p, n, mat = _mirror_triangles(b.flat)
    assert len(mirror) == 4
    side = p[:, 0] < 0  # (the tree's builder orders the triangles)
    left, right = p[side], p[~side]
    assert len(left) == len(right) == 6
    assert np.allclose(left.min(0), (-0.99, 0.05, -0.95)) and np.allclose(left.max(0), (-0.99, 1.95, 0.95)) and np.allclose(n[side], (1, 0, 0))
    assert np.allclose(right.min(0), (0.99, 0.05, -0.95)) and np.allclose(right.max(0), (0.99, 1.95, 0.95)) and np.allclose(n[~side], (-1, 0, 0))
    assert np.allclose(mat["colour"][:, :3], scenes.CORRIDOR_TINT) and (mat["metallic"] != 0).all() and (mat["smoothness"] == 1).all()


def test_the_blob_room():
    b = scenes.mirror_blob_room(64, 36)
    flat = b.flat
    mirror, p, n, mat = _mirror_triangles(flat)
    assert len(mirror) == 20 * 4 ** 3 and (mat["metallic"] != 0).all() and (mat["smoothness"] > np.float32(0.94)).all()
    assert flat.num_instances == 2
    dets = [np.linalg.det(t.reshape(4, 4)[:3, :3].astype(np.float64)) for t in flat.top_nodes["invTransform"][:flat.num_instances]]
    assert min(dets) < 0 < max(dets)  # the blob's instance is mirrored, the room's is not
    m = flat.top_nodes["invTransform"][int(np.argmin(dets))].reshape(4, 4)[:3, :3].astype(np.float64)
    factors = np.sort(1.0 / np.linalg.svd(m, compute_uv=False))
    assert np.allclose(factors, (0.9, 1.2, 1.4), rtol=1e-5)  # three different scale factors
    spread = np.linalg.norm(n.reshape(-1, 3, 3)[:, 0] - n.reshape(-1, 3, 3)[:, 1], axis=1)
    assert (spread > 1e-3).mean() > 0.9  # interpolated normals: the vertices of a triangle carry different ones
