"""Instance motion without a GPU (include/ptamd.h, "instance motion"): the host's record conversion (pt_debug_motion_records) against its float64
restatement, the restatement's own sanity on the synthetic moved sphere (tests/motion_ref.py), and the C-ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import motion_ref as M
import temporal_ref as T
from ptamd import device as D, scenes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ["pt_set_instance_motion", "pt_instance_motion", "pt_read_motion_guides", "pt_write_motion_guides", "pt_motion_guides_device_ptr",
           "pt_debug_motion_records"]


# ---------------------------------------------------------------- 1. the record conversion
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
    """(name, previous, current) invTransforms: translations, a rotation, scales of 1 / 1024 and 8, hand-made mirror / shear / 30 : 1 matrices, and every
    leaf of scenes.transform_zoo("general") -- mirrored, sheared, 30 : 1 non-uniform -- against itself moved on"""
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
    assert len(moved) >= 7  # (the sheared child follows its parent)
    out += [(f"zoo leaf {k}", before["invTransform"][k].copy(), after["invTransform"][k].copy()) for k in moved]
    return out


def test_records_match_the_float64_restatement():
    pairs = _pairs()
    prev, cur = np.stack([p for _, p, _ in pairs]), np.stack([c for _, _, c in pairs])
    got = D.debug_motion_records(prev, cur)
    assert got.shape == (len(pairs), 6, 4) and got.dtype == np.float32
    want, exact = M.motion_records(prev, cur), M.records_exact(prev, cur)
    worst = 0.0
    for k, (name, p, _) in enumerate(pairs):
        assert np.array_equal(got[k, 3:].view(np.uint32), p.reshape(4, 4).T[:3].view(np.uint32)), name  # the previous rows, untouched
        for row in range(3):
            ulp = float(np.spacing(np.float32(np.abs(exact[k, row]).max())))  # at the magnitude of the row's largest entry
            err = float(np.abs(got[k, row].astype(np.float64) - want[k, row].astype(np.float64)).max()) / ulp
            worst = max(worst, err)
            assert err <= 2.0, (name, row, err)
        assert np.any(got[k, :3] != 0), name
    print(f"worst error of (A | t): {worst:.2f} ulp of the row's largest entry")


def test_identical_bits_give_exact_zeros():
    pairs = _pairs()
    same = np.stack([c for _, _, c in pairs])
    got = D.debug_motion_records(same, same.copy())
    assert np.all(got[:, :3].view(np.uint32) == 0)  # +0, every bit
    assert np.array_equal(got[:, 3:].view(np.uint32), M.motion_records(same, same)[:, 3:].view(np.uint32))
    nudged = same.copy()
    nudged[:, 12] = np.nextafter(nudged[:, 12], np.float32(np.inf))  # one bit of one translation
    assert np.all(np.any(D.debug_motion_records(nudged, same)[:, :3] != 0, axis=(1, 2)))


@pytest.mark.parametrize("what", ["singular", "nan", "inf"])
def test_a_bad_previous_matrix_is_refused_with_a_message(what):
    good = _inverse_world((1.0, 1.0, 1.0), location=(1.0, 2.0, 3.0))
    bad = good.copy()
    if what == "singular":
        bad[0:3] = 0.0  # a zero column
    else:
        bad[5] = np.nan if what == "nan" else np.inf
    with pytest.raises(D.PtError) as e:
        D.debug_motion_records(np.stack([good, bad]), np.stack([good, good]))
    assert "failed (-1)" in str(e.value) and "entry 1" in str(e.value) and ("singular" in str(e.value) or "finite" in str(e.value))
    D.debug_motion_records(np.stack([good, good]), np.stack([good, bad]))  # the CURRENT matrix is the upload's business


# ---------------------------------------------------------------- 2. the restatement itself
@pytest.mark.parametrize("turn", [False, True])
@pytest.mark.parametrize("width,height", T.SIZES)
def test_no_motion_is_the_plain_restatement(width, height, turn):
    case = M.make_moved_case("pan", width, height, turn=turn)
    for dt in (np.float64, np.float32):
        plain = T.run_case(case, dt)
        for got in (M.run_case(case, dt, with_motion=False), M.run_case(M.make_moved_case("pan", width, height, turn=turn, zero_motion=True), dt)):
            for a, b in zip(got, plain):
                assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("turn", [False, True])
@pytest.mark.parametrize("width,height", [(70, 45), (150, 83)])
def test_the_moved_sphere_keeps_its_history_with_motion_only(width, height, turn):
    """mean confidence Wsum over the sphere's pixels: > 0.5 with the motion sums, < 0.05 and at least ten times less without"""
    case = M.make_moved_case("pan", width, height, turn=turn)
    sphere = case["sphere"]
    assert sphere.sum() > 100
    cn_with, _, w_with = M.run_case(case)
    cn_without, _, w_without = M.run_case(case, with_motion=False)
    a, b = float(w_with[sphere].mean()), float(w_without[sphere].mean())
    print(f"{width}x{height} turn={turn}: mean Wsum on the sphere {a:.3f} with motion, {b:.4f} without; "
          f"mean count {cn_with[sphere, 3].mean():.1f} / {cn_without[sphere, 3].mean():.1f}")
    assert a > 0.5 and b < 0.05 and a >= 10.0 * b
    away = ~sphere
    assert np.array_equal(w_with[away], w_without[away]) and np.array_equal(cn_with[away], cn_without[away])  # nothing else moved


# ---------------------------------------------------------------- 3. the C-ABI
PROBE = r"""
#include "ptamd.h"
#include <stdio.h>
int main(void)
{
    int (*set)(pt_ctx*, const float*, uint32_t) = pt_set_instance_motion;
    int (*get)(const pt_ctx*, uint32_t*) = pt_instance_motion;
    int (*rd)(pt_ctx*, float*, float*) = pt_read_motion_guides;
    int (*wr)(pt_ctx*, const float*, const float*) = pt_write_motion_guides;
    void* (*ptr)(pt_ctx*, int) = pt_motion_guides_device_ptr;
    int (*rec)(const float*, const float*, uint32_t, float*) = pt_debug_motion_records;
    float prev[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 }, cur[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -2, 0, 0.5f, 1 }, out[25];
    out[24] = 77.0f;
    printf("%d %d\n", rec(prev, cur, 1, out), set && get && rd && wr && ptr);
    for (int k = 0; k < 25; k++)
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


def test_the_record_is_96_bytes_as_the_c_compiler_sees_it(tmp_path):
    """the header's prototypes compile as C and link, and one record fills 24 floats and not one more"""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    libdir = os.path.dirname(os.path.abspath(D.DEVICE_LIB_PATH))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + libdir, "-lptamd",
                    "-Wl,-rpath," + libdir], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert lines[0].split() == ["0", "1"]
    got = [float(x) for x in lines[1].split()]
    # prev = identity, cur = a translation by (-2, 0, 0.5) in the inverse: P - I = that translation
    assert got == [0, 0, 0, -2, 0, 0, 0, 0, 0, 0, 0, 0.5, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 77]
    assert D.MOTION_RECORD_BYTES == 96 == 24 * 4
