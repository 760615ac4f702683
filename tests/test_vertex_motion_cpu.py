"""Vertex motion without a GPU (include/ptamd.h, "vertex motion"): the host's rows (pt_debug_vertex_motion_rows) against their float64 restatement,
the restatement's own sanity on a rigidly moved sphere, the preconditions of the GPU deposit test stated on the oracle's hits, and the C-ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import orclib as O
import vertex_motion_ref as V
from ptamd import device as D, host as H, scenes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ["pt_set_vertex_motion", "pt_vertex_motion", "pt_debug_vertex_motion_rows"]


# ---------------------------------------------------------------- 1. the rows
def _inverse_world(scale, axis=None, angle=0.0, location=(0.0, 0.0, 0.0), shear=None):
    """the column-major float32 invTransform of world = T R S (times an optional shear matrix)"""
    w = np.eye(4)
    w[:3, :3] = np.diag(np.asarray(scale, np.float64))
    if shear is not None:
        w[:3, :3] = np.asarray(shear, np.float64) @ w[:3, :3]
    if axis is not None:
        a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        w[:3, :3] = (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K) @ w[:3, :3]
    w[:3, 3] = location
    return np.linalg.inv(w).T.reshape(16).astype(np.float32)


def _pairs():
    """the (name, previous, current) invTransforms of the instance-motion record test, rebuilt here: translations, a rotation, scales of 1 / 1024 and
    8, hand-made mirror / shear / 30 : 1 matrices, and every leaf of scenes.transform_zoo("general") against itself moved on"""
    one = (1.0, 1.0, 1.0)
    out = [("translation", _inverse_world(one), _inverse_world(one, location=(0.25, 0.0, 0.1))),
           ("far translation", _inverse_world(one, location=(300.0, -2.0, 7.0)), _inverse_world(one, location=(300.5, -2.0, 7.25))),
           ("rotation", _inverse_world(one, (0, 1, 0), 0.2, (1.0, 0.5, 2.0)), _inverse_world(one, (0, 1, 0), 0.7, (1.0, 0.5, 2.0))),
           ("rotation + translation", _inverse_world(one, (1, 1, 0), 1.1, (1.0, 0.5, 2.0)), _inverse_world(one, (0, 1, 0), 0.7, (1.3, 0.4, 2.0))),
           ("scale 1/1024", _inverse_world((1 / 1024,) * 3, location=(0.0, 0.0, -0.05)), _inverse_world((1 / 1024,) * 3, (0, 0, 1), 0.3, (0.001, 0.0, -0.05))),
           ("scale 8", _inverse_world((8.0,) * 3, location=(3.0, 4.5, 14.0)), _inverse_world((8.0,) * 3, (1, 0, 0), 0.4, (3.5, 4.5, 13.0))),
           ("scale 1/1024 to 8", _inverse_world((1 / 1024,) * 3), _inverse_world((8.0,) * 3, location=(1.0, 2.0, 3.0))),
           ("mirror", _inverse_world((-0.8, 0.8, 0.8), (0, 1, 0), 0.7, (1.3, -0.4, 2.2)), _inverse_world((-0.8, 0.8, 0.8), (0, 1, 0), 0.9, (1.2, -0.4, 2.2))),
           ("30 : 1", _inverse_world((0.1, 1.0, 3.0), (0, 0, 1), 0.4, (1.8, -0.4, 3.5)), _inverse_world((0.1, 1.0, 3.0), (0, 0, 1), 0.6, (1.9, -0.4, 3.4))),
           ("shear", _inverse_world((1.0, 3.0, 0.5), (1, 0, 1), 0.9, (2.6, 0.2, 5.0), shear=[[1, 0.4, 0], [0, 1, 0.2], [0, 0, 1]]),
            _inverse_world((1.0, 3.0, 0.5), (1, 0, 1), 1.0, (2.7, 0.2, 5.0), shear=[[1, 0.4, 0], [0, 1, 0.2], [0, 0, 1]]))]
    b = scenes.transform_zoo("general", level=1)
    before = b.flat.top_nodes.copy()
    for node in range(2, 9):
        b.scene.set_transform(node, location=(0.1 * node, -0.3, 2.0 + 0.4 * node), orientation_wxyz=scenes._axis_angle((1, node, 0), 0.3 * node))
    after = b.scene.flatten().top_nodes
    leaves = np.flatnonzero((before["isLeaf"] != 0) & (after["isLeaf"] != 0))
    moved = [k for k in leaves if not np.array_equal(before["invTransform"][k], after["invTransform"][k])]
    assert len(moved) >= 7
    out += [(f"zoo leaf {k}", before["invTransform"][k].copy(), after["invTransform"][k].copy()) for k in moved]
    return out


def test_rows_match_the_float64_restatement():
    """every row within 2 ulp of the row's largest entry (the criterion of test_records_match_the_float64_restatement), w == 0"""
    pairs = _pairs()
    inv = np.stack([m for _, p, c in pairs for m in (p, c)])
    names = [f"{n} ({which})" for n, _, _ in pairs for which in ("previous", "current")]
    got = D.debug_vertex_motion_rows(inv)
    assert got.shape == (len(inv), 3, 4) and got.dtype == np.float32
    want = V.vertex_motion_rows(inv)
    worst = 0.0
    for k, name in enumerate(names):
        assert np.all(got[k, :, 3].view(np.uint32) == 0), name  # w: +0
        for row in range(3):
            ulp = float(np.spacing(np.float32(np.abs(want[k, row]).max())))
            err = float(np.abs(got[k, row].astype(np.float64) - want[k, row]).max()) / ulp
            worst = max(worst, err)
            assert err <= 2.0, (name, row, err)
        assert np.any(got[k, :, :3] != 0), name
    print(f"worst error of L: {worst:.2f} ulp of the row's largest entry")
    assert D.debug_vertex_motion_rows(np.zeros((0, 16), np.float32)).shape == (0, 3, 4)


@pytest.mark.parametrize("what", ["singular", "dependent", "nan", "inf"])
def test_a_bad_matrix_is_refused_with_a_message(what):
    good = _inverse_world((1.0, 1.0, 1.0), location=(1.0, 2.0, 3.0))
    bad = good.copy()
    if what == "singular":
        bad[0:3] = 0.0  # a zero column
    elif what == "dependent":
        bad[4:7] = bad[0:3]  # two equal columns
    else:
        bad[5] = np.nan if what == "nan" else np.inf
    with pytest.raises(D.PtError) as e:
        D.debug_vertex_motion_rows(np.stack([good, bad]))
    assert "failed (-1)" in str(e.value) and "entry 1" in str(e.value) and ("singular" in str(e.value) or "finite" in str(e.value))


# ---------------------------------------------------------------- 2. the restatement itself
def test_a_rigid_move_deposits_the_analytic_displacement():
    """The sphere, under a transform that float32 holds exactly (scales 1, 1/2, 1/4: L is exact), was at p' = R p + s in its own space.  The float64
    deposits are W (x_then - x_now) to 1e-12 x extent with both points formed as the library forms them, and W ((R - I) x_now + s) up to the rounding
    of the moved vertices to float32 (1e-6 x extent).  The room and the misses deposit nothing."""
    room = V.DeformingRoom(location=(0.0, 0.75, 0.125), scale=(1.0, 0.5, 0.25))
    now = room.flat0
    a = 0.3
    Rm = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    s = np.array([0.05, -0.02, 0.1])
    then = room.shape(room.p0.astype(np.float64) @ Rm.T + s)
    o, d = V.pixel_centre_rays(room.camera, room.width, room.height)
    hits = O.intersect_batch(O.BoundScene(now), o, d, threads=4)
    motion, pn, extra = V.deposits(now, then, None, o, d, hits, np.float64)
    on_blob = (hits["prim"] >= 0) & (hits["inst"] == V.BLOB_LEAF)
    assert on_blob.sum() > 30 and (~on_blob).sum() > 1000
    extent = V.scene_extent(now)
    Wl = np.diag([1.0, 0.5, 0.25])
    u, v = hits["u"].astype(np.float64)[on_blob, None], hits["v"].astype(np.float64)[on_blob, None]
    x_now = V._object_points(now, hits["prim"][on_blob], u, v, np.float64)
    x_then = V._object_points(then, hits["prim"][on_blob], u, v, np.float64)
    err = float(np.abs(motion[on_blob, :3] - (x_then - x_now) @ Wl.T).max())
    err_rigid = float(np.abs(motion[on_blob, :3] - (x_now @ (Rm - np.eye(3)).T + s) @ Wl.T).max())
    print(f"rigid move: {on_blob.sum()} pixels, error {err:.3e} against the library's points, {err_rigid:.3e} against R x + s; extent {extent}")
    assert err <= 1e-12 * extent and err_rigid <= 1e-6 * extent
    assert np.abs(motion[on_blob, :3]).max() > 0.02 and not motion[~on_blob].any() and not motion[:, 3].any()
    # the normals turn with R (smooth normals regenerated by the refit: the same up to their own rounding)
    n_obj_now = extra["normal_unflipped"][on_blob] @ Wl  # back through the normal transform: n_world ~ W^-T n_object
    n_obj_now /= np.linalg.norm(n_obj_now, axis=1, keepdims=True)
    want = (n_obj_now @ Rm.T) @ np.linalg.inv(Wl).T
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(extra["then_unflipped"][on_blob] - want).max() < 1e-4


# ---------------------------------------------------------------- 3. what the GPU deposit test stands on
@pytest.mark.parametrize("builder", ["BVH_BINNED_SAH", "BVH_SPATIAL_SPLIT"])
def test_the_deposit_scene_has_deformed_undeformed_and_missed_pixels(builder):
    """tests/test_gpu_vertex_motion.py::test_guide_deposits_of_a_refitted_mesh, on the oracle's hits for the camera's pixel-centre rays: more than 100
    pixels on the deformed sphere, more than 100 on geometry that kept its bits, a miss, and fewer than 1e-2 of the hits at grazing incidence"""
    room = V.DeformingRoom(getattr(H, builder))
    flat_a, flat_b = room.flat0, room.frame(1)
    changed_vertex = np.any(flat_a.vertices["vertex"] != flat_b.vertices["vertex"], 1) | np.any(flat_a.vertices["normal"] != flat_b.vertices["normal"], 1)
    changed_tri = changed_vertex[flat_b.triangles["indices"]].any(1)
    assert np.array_equal(changed_tri, room.blob_triangles(flat_b)) or changed_tri[room.blob_triangles(flat_b)].mean() > 0.9
    assert not changed_tri[~room.blob_triangles(flat_b)].any()
    o, d = V.pixel_centre_rays(room.camera, room.width, room.height)
    hits = O.intersect_batch(O.BoundScene(flat_b), o, d, threads=4)
    hit = hits["prim"] >= 0
    deformed = hit & changed_tri[np.where(hit, hits["prim"], 0)]
    motion, pn, extra = V.deposits(flat_b, flat_a, None, o, d, hits, np.float64)
    grazing = hit & (np.abs(extra["n_dot_d"]) < 1e-6)
    print(f"{builder}: {deformed.sum()} deformed, {(hit & ~deformed).sum()} undeformed, {(~hit).sum()} missed pixels; grazing {grazing.mean():.2e}; "
          f"largest displacement {np.abs(motion[deformed, :3]).max():.3f}")
    assert deformed.sum() > 100 and (hit & ~deformed).sum() > 100 and (~hit).sum() >= 1
    assert grazing.mean() < 1e-2
    assert np.abs(motion[deformed, :3]).max() > 0.02 and not motion[~deformed].any()


# ---------------------------------------------------------------- 4. the C-ABI
PROBE = r"""
#include "ptamd.h"
#include <stdio.h>
int main(void)
{
    int (*set)(pt_ctx*, int) = pt_set_vertex_motion;
    int (*get)(const pt_ctx*, uint32_t*) = pt_vertex_motion;
    int (*rows)(const float*, uint32_t, float*) = pt_debug_vertex_motion_rows;
    float inv[16] = { 0.5f, 0, 0, 0, 0, 4, 0, 0, 0, 0, 1, 0, 3, 2, 1, 1 }, out[13];
    uint32_t deformed = 7;
    out[12] = 77.0f;
    const int is_set = get(0, &deformed); /* no context: not set, and the count is written all the same */
    printf("%d %d %d %u\n", rows(inv, 1, out), set != 0, is_set, deformed);
    for (int k = 0; k < 13; k++)
        printf("%g ", out[k]);
    printf("\n");
    return 0;
}
"""


def test_library_exports_the_new_symbols():
    lib = ctypes.CDLL(D.DEVICE_LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert not [s for s in SYMBOLS if s not in D.EXPORTS]
    assert D.lib().pt_vertex_motion(None, None) == 0  # the binding loads, and answers, without a device


def test_the_rows_are_48_bytes_as_the_c_compiler_sees_them(tmp_path):
    """the header's prototypes compile as C and link, and one entry fills 12 floats and not one more"""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    libdir = os.path.dirname(os.path.abspath(D.DEVICE_LIB_PATH))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + libdir, "-lptamd",
                    "-Wl,-rpath," + libdir], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert lines[0].split() == ["0", "1", "0", "0"]
    got = [float(x) for x in lines[1].split()]
    assert got == [2, 0, 0, 0, 0, 0.25, 0, 0, 0, 0, 1, 0, 77]  # the inverse's linear part; the translation does not enter
