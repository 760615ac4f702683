"""The temporal luminance variance on the device (pt_set_temporal_variance, k_temporal<., true>, k_atrous<., true>; include/ptamd.h "temporal
variance") against its numpy restatement (tests/variance_ref.py): synthetic inputs through write_accum / write_guides / write_temporal /
write_temporal_variance, the refusals, the C++ example."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import gpu_util as U
import motion_ref as M
import temporal_ref as T
import variance_ref as V
from ptamd import device as D, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GUIDED = D.DENOISE_INPUT_TEMPORAL_VARIANCE


def history_variance(case, seed=31):
    """a variance plane for the case's history: random, non-negative, from exact zeros to 10"""
    rng = np.random.default_rng(seed)
    h, w = case["height"], case["width"]
    v = rng.uniform(0.0, 10.0, (h, w)) * (rng.uniform(size=(h, w)) > 0.15)
    v[0, 0], v[h - 1, w - 1] = 0.0, 10.0
    return v.astype(np.float32)


def load(ctx, case, history=True, variance=None):
    """the inputs of one accumulate into the context; `variance`: the history's plane (the mode must be on)"""
    ctx.write_accum(case["accum"], case["spp"])
    ctx.write_guides(case["albedo_hits"], case["normal_depth"], case["gspp"])
    if "motion" in case:
        ctx.write_motion_guides(case["motion"], case["prev_normal"])
    ctx.set_camera(case["camera"])
    if history:
        ctx.write_temporal(case["hist_cn"], case["hist_nd"], case["hist_camera"])
        if variance is not None:
            ctx.write_temporal_variance(variance)


def read(ctx, case):
    h, w = case["height"], case["width"]
    cn, nd = ctx.read_temporal()
    return cn.reshape(h, w, 4), nd.reshape(h, w, 4)


def restated(case, hist_v, dtype):
    return V.accumulate(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], case["camera"],
                        (case["hist_cn"], case["hist_nd"], case["hist_camera"], hist_v), motion=case.get("motion"), prev_normal=case.get("prev_normal"), dtype=dtype)


def variance_bound(ref64, ref32):
    """8 x what single precision costs the restatement on this input + 1e-6 x the largest variance of the float64 result"""
    assert ref32.dtype == np.float32 and ref64.dtype == np.float64
    return 8.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + 1e-6 * float(ref64.max())


def make_ctx(gpu, case, moving):
    if not moving:
        return gpu.Context(case["width"], case["height"])
    flat = scenes.cornell_box(64, 64).flat  # a motion can only be set on a context that holds a scene: every leaf where it was
    ctx = U.make_ctx(gpu, flat, case["width"], case["height"])
    ctx.set_instance_motion(flat.top_nodes)
    assert ctx.instance_motion == (True, 0)
    return ctx


def check_accumulate(gpu, case, name, moving=False):
    """One accumulate with the mode on: the variance plane within the bound of the float64 restatement; colour_count and normal_depth with the
    bits of the same call with the mode off; a second run gives the same bits."""
    hist_v = history_variance(case)
    off = make_ctx(gpu, case, moving)
    load(off, case)
    off.temporal_accumulate()
    cn_off, nd_off = read(off, case)
    assert off.temporal_variance is False and off.temporal_variance_device_ptr == 0
    off.close()
    ctx = make_ctx(gpu, case, moving)
    ctx.set_temporal_variance()
    assert ctx.temporal_variance is True
    load(ctx, case, variance=hist_v)
    assert np.array_equal(ctx.read_temporal_variance(), hist_v.ravel())
    ctx.temporal_accumulate()
    cn, nd = read(ctx, case)
    var = ctx.read_temporal_variance().reshape(case["height"], case["width"])
    ref64, ref32 = restated(case, hist_v, np.float64)[2], restated(case, hist_v, np.float32)[2]
    bound = variance_bound(ref64, ref32)
    err = float(np.abs(var.astype(np.float64) - ref64).max())
    U.record_margin(f"temporal variance vs restatement: {name}", error=err, bound=bound, largest=float(ref64.max()))
    print(f"{name}: variance error {err:.3e}, bound {bound:.3e}, largest {ref64.max():.3e}")
    assert np.all(var >= 0.0) and np.all(np.isfinite(var))
    assert err <= bound
    assert (var != hist_v).mean() > 0.5 and (var > 0).mean() > 0.2  # neither the history's plane handed through nor zeros
    assert np.array_equal(cn.view(np.uint32), cn_off.view(np.uint32)) and np.array_equal(nd.view(np.uint32), nd_off.view(np.uint32))
    load(ctx, case, variance=hist_v)  # (the sets flipped: the inputs go into what is now the newest one)
    ctx.temporal_accumulate()
    cn2, nd2 = read(ctx, case)
    assert np.array_equal(ctx.read_temporal_variance().view(np.uint32), var.ravel().view(np.uint32))
    assert np.array_equal(cn2.view(np.uint32), cn.view(np.uint32)) and np.array_equal(nd2.view(np.uint32), nd.view(np.uint32))
    ctx.close()


@pytest.mark.parametrize("width,height", T.SIZES)
@pytest.mark.parametrize("pose", ["pan", "big"])
def test_accumulate_matches_the_restatement(gpu, pose, width, height):
    """16 x 16 is smaller than the 32 x 8 tile, 70 x 45 no multiple of it, 150 x 83 several tiles each way"""
    check_accumulate(gpu, T.make_case(pose, width, height), f"{pose} {width}x{height}")


def test_accumulate_with_fireflies(gpu):
    """a 1e4 firefly in the current frame and one in the history: (l - mu)^2 of 1e7 and more, the same form of bound"""
    check_accumulate(gpu, T.make_case("pan", 70, 45, firefly=True), "pan 70x45, fireflies")


def test_accumulate_on_the_motion_route(gpu):
    """k_temporal<true, true>: the moved and turned sphere of the motion tests, non-zero motion sums"""
    case = M.make_moved_case("pan", 70, 45, turn=True)
    assert np.abs(case["motion"]).max() > 0.1
    check_accumulate(gpu, case, "moved sphere 70x45, motion route", moving=True)


def test_no_history_gives_a_plane_of_zeros(gpu):
    """the camera turned away (every lambda <= 0), and the first call after a reset"""
    case = T.make_case("turn", 70, 45)
    ctx = gpu.Context(70, 45)
    ctx.set_temporal_variance()
    load(ctx, case, variance=history_variance(case))
    ctx.temporal_accumulate()
    assert not ctx.read_temporal_variance().any()
    ctx.write_temporal_variance(history_variance(case))
    ctx.temporal_reset()
    assert ctx.temporal_frames == 0 and ctx.temporal_variance is True  # the reset keeps the mode
    ctx.temporal_accumulate()
    assert ctx.temporal_frames == 1
    assert not ctx.read_temporal_variance().any()
    cn, _ = read(ctx, case)
    assert np.all(cn[..., 3] == 1.0)
    ctx.close()


# ---------------------------------------------------------------- the filter
@pytest.fixture(scope="module")
def filter_cases(gpu):
    """per size: a context that holds the current frame, a history with counts 0 .. 39 (s covers 0, fractions and 1), fireflies in both, and
    the history's variance plane -- shared by the iteration counts, and left unchanged by them"""
    made = {}

    def get(width, height):
        if (width, height) not in made:
            case = T.make_case("history", width, height, firefly=True)
            counts = case["hist_cn"][..., 3]
            assert counts.min() == 0 and (counts == 1).any() and ((counts > 1) & (counts < V.FULL_HISTORY)).any() and counts.max() > V.FULL_HISTORY
            hist_v = history_variance(case)
            ctx = gpu.Context(width, height)
            ctx.set_temporal_variance()
            load(ctx, case, variance=hist_v)
            made[(width, height)] = (ctx, case, hist_v)
        return made[(width, height)]
    yield get
    for ctx, *_ in made.values():
        ctx.close()


def guided_bound(case, hist_cn, hist_v, iterations):
    """(float64 restatement, float32 restatement as float64, bound) in the form of tests/test_gpu_denoise.py's hdr_bound"""
    ref64 = V.denoise_hdr(hist_cn, hist_v, case["albedo_hits"], case["normal_depth"], case["gspp"], iterations, np.float64)
    ref32 = V.denoise_hdr(hist_cn, hist_v, case["albedo_hits"], case["normal_depth"], case["gspp"], iterations, np.float32)
    assert ref32.dtype == np.float32
    ref32 = ref32.astype(np.float64)
    return ref64, ref32, 8.0 * float(np.abs(ref32 - ref64).max()) + 1e-6 * float(hist_cn[..., :3].max())


SIZES_ITERATIONS = [(70, 45, i) for i in (1, 2, 3, 5, 6)] + [(150, 83, i) for i in (1, 3, 5)] + [(16, 16, i) for i in (2, 5)]


@pytest.mark.parametrize("width,height,iterations", SIZES_ITERATIONS)
def test_filter_matches_the_restatement(filter_cases, width, height, iterations):
    """HDR output against the float64 restatement, absolute (the fireflies set that bound) and relative (the ordinary pixels), as
    tests/test_gpu_denoise.py holds the plain filter; iterations 1-2 run the LDS variant, 3 and more the direct loads."""
    ctx, case, hist_v = filter_cases(width, height)
    out = ctx.denoise(iterations, hdr=True, input=GUIDED)
    ref, ref32, bound = guided_bound(case, case["hist_cn"], hist_v, iterations)
    err = float(np.abs(out[..., :3].astype(np.float64) - ref).max())
    U.record_margin(f"variance-guided filter vs restatement: {width}x{height}, {iterations} iterations", error=err, bound=bound)
    print(f"{width}x{height} iterations {iterations}: error {err:.3e}, bound {bound:.3e}")
    assert np.all(out[..., 3] == 1.0)
    assert err <= bound
    scale = np.abs(ref) + 1e-3
    rel, rel_bound = float((np.abs(out[..., :3] - ref) / scale).max()), 8.0 * float((np.abs(ref32 - ref) / scale).max()) + 1e-6
    U.record_margin(f"variance-guided filter vs restatement, relative: {width}x{height}, {iterations} iterations", error=rel, bound=rel_bound)
    print(f"    relative: error {rel:.3e}, bound {rel_bound:.3e}")
    assert rel <= rel_bound
    # the variance did something: not the plain filter over the same history
    plain = ctx.denoise(iterations, hdr=True, input_temporal=True)
    assert np.abs(out[..., :3] - plain[..., :3]).max() > 10 * bound
    assert np.array_equal(ctx.denoise(iterations, hdr=True, input=GUIDED).view(np.uint32), out.view(np.uint32))  # run to run


def test_zero_iterations_and_the_tone_curve(filter_cases):
    ctx, case, _ = filter_cases(70, 45)
    assert np.array_equal(ctx.denoise(0, hdr=True, input=GUIDED), ctx.denoise(0, hdr=True, input_temporal=True))
    assert np.array_equal(ctx.denoise(0, input=GUIDED), ctx.denoise(0, input_temporal=True))
    out = ctx.denoise(3, input=GUIDED)
    assert out[..., :3].max() <= 1.0 and out[..., :3].min() >= 0.0 and np.all(out[..., 3] == 1.0)
    assert not np.array_equal(out, ctx.denoise(3, input_temporal=True))


@pytest.mark.parametrize("iterations", [2, 5])
def test_a_history_of_one_frame_is_filtered_like_the_plain_filter(gpu, iterations):
    """every count 1: s == 0, and the output is PT_DENOISE_INPUT_TEMPORAL's on the same context, within the bound of the restatement"""
    case = T.make_case("history", 70, 45, firefly=True)
    hist_cn = case["hist_cn"].copy()
    hist_cn[..., 3] = 1.0
    hist_v = history_variance(case)
    ctx = gpu.Context(70, 45)
    ctx.set_temporal_variance()
    load(ctx, dict(case, hist_cn=hist_cn), variance=hist_v)
    guided, plain = ctx.denoise(iterations, hdr=True, input=GUIDED), ctx.denoise(iterations, hdr=True, input_temporal=True)
    _, _, bound = guided_bound(case, hist_cn, hist_v, iterations)
    err = float(np.abs(guided.astype(np.float64) - plain).max())
    U.record_margin(f"variance-guided filter, all counts 1, vs the plain filter: 70x45, {iterations} iterations", error=err, bound=bound)
    print(f"all counts 1, {iterations} iterations: difference {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    ctx.close()


# ---------------------------------------------------------------- state
def test_three_chained_accumulates(gpu):
    """A -> B -> C -> D with three accumulate calls and no write in between: the new plane's ping-pong.  The bound is computed on the
    restatement chained the same way."""
    width, height = 70, 45
    steps = [T.make_case("pan", width, height, seed=21), T.make_case("pan2", width, height, seed=22), T.make_case("pan", width, height, seed=23)]
    hist_v = history_variance(steps[0])
    ctx = gpu.Context(width, height)
    ctx.set_temporal_variance()
    load(ctx, steps[0], variance=hist_v)
    planes = []
    for k, case in enumerate(steps):
        if k:
            load(ctx, case, history=False)
        ctx.temporal_accumulate()
        planes.append(ctx.temporal_variance_device_ptr)
    assert ctx.temporal_frames == 4
    assert planes[0] and planes[0] == planes[2] and planes[1] and planes[1] != planes[0]
    var = ctx.read_temporal_variance().reshape(height, width)

    def chain(dtype):
        first = steps[0]
        hist = (first["hist_cn"], first["hist_nd"], first["hist_camera"], hist_v)
        for case in steps:
            cn, nd, v = V.accumulate(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], case["camera"], hist, dtype=dtype)
            hist = (cn, nd, case["camera"], v)
        return v
    ref64, ref32 = chain(np.float64), chain(np.float32)
    bound = variance_bound(ref64, ref32)
    err = float(np.abs(var.astype(np.float64) - ref64).max())
    U.record_margin("temporal variance vs restatement: chained A-B-C-D 70x45", error=err, bound=bound)
    print(f"chained: variance error {err:.3e}, bound {bound:.3e}")
    assert err <= bound and (var > 0).mean() > 0.5
    ctx.close()


def test_refusals_and_what_they_leave_alone(gpu):
    INVALID, STATE, UNSUPPORTED = -1, -3, -4
    case = T.make_case("pan", 16, 16)
    hist_v = history_variance(case)
    ctx = gpu.Context(16, 16)
    for bad in (dict(sigma_variance=-1.0), dict(relative_floor=-0.5), dict(full_history=-3.0), dict(sigma_variance=float("nan")),
                dict(relative_floor=float("inf")), dict(full_history=1.5), dict(full_history=float("nan"))):
        assert U.status(lambda: ctx.set_temporal_variance(**bad)) == INVALID, bad
        assert ctx.temporal_variance is False
    # mode off: no plane to read or write, no guided filter
    load(ctx, case)
    assert U.status(ctx.read_temporal_variance) == STATE
    assert U.status(lambda: ctx.write_temporal_variance(hist_v)) == STATE
    assert U.status(lambda: ctx.denoise(3, input=GUIDED)) == STATE
    assert U.status(lambda: ctx.denoise(3, input=3)) == INVALID
    # a history exists: the mode cannot change, either way
    assert ctx.temporal_frames == 1
    assert U.status(ctx.set_temporal_variance) == STATE
    assert ctx.temporal_variance is False
    ctx.temporal_reset()
    ctx.set_temporal_variance(full_history=2.0)
    assert ctx.temporal_variance is True
    # mode on, no history
    assert U.status(ctx.read_temporal_variance) == STATE
    assert U.status(lambda: ctx.write_temporal_variance(hist_v)) == STATE
    assert U.status(lambda: ctx.denoise(3, input=GUIDED)) == STATE
    load(ctx, case, variance=hist_v)
    assert U.status(lambda: ctx.set_temporal_variance(False)) == STATE  # forgetting, too
    assert U.status(ctx.set_temporal_variance) == STATE
    assert ctx.temporal_variance is True and ctx.temporal_frames == 1
    assert np.array_equal(ctx.read_temporal_variance(), hist_v.ravel())  # the refused calls changed nothing
    assert ctx.denoise(3, input=GUIDED).shape == (16, 16, 4)
    ctx.write_temporal(case["hist_cn"], case["hist_nd"], case["hist_camera"])  # a new history: nothing is known about its spread
    assert not ctx.read_temporal_variance().any()
    ctx.temporal_reset()
    ctx.set_temporal_variance(False)
    assert ctx.temporal_variance is False and ctx.temporal_variance_device_ptr == 0
    ctx.temporal_accumulate()  # the plain kernel again
    assert U.status(ctx.read_temporal_variance) == STATE
    ctx.close()
    for kw in (dict(rng_mode=D.RNG_LFSR113_PARITY), dict(max_active_rays=1024)):
        other = gpu.Context(64, 64, **kw)
        assert U.status(other.set_temporal_variance) == UNSUPPORTED
        assert other.temporal_variance is False
        other.close()


def test_cpp_converge_example(gpu):
    """examples/converge_cornell.cpp: 32 frames of 1 spp under a static camera.  At the last frame the variance-guided filter is closer to the
    converged image than the plain filter and than the unfiltered history -- the two frame-32 conditions of tests/test_variance_ref.py."""
    r = subprocess.run([os.path.join(ROOT, "examples", "converge_cornell"), "32", "256"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    rows = {}
    for line in r.stdout.splitlines():
        fields = dict(kv.split("=") for kv in line.split() if "=" in kv)
        if "frame" in fields:
            rows[int(fields["frame"])] = tuple(float(fields[k]) for k in ("history", "plain", "guided"))
        elif "frames" in fields:
            assert int(fields["frames"]) == 32 and int(fields["temporal_frames"]) == 32 and int(fields["variance"]) == 1
    assert sorted(rows) == [1, 8, 32]
    alone, plain, guided = rows[32]
    U.record_margin("converge_cornell, 32 frames of 1 spp", rmse_history=alone, rmse_plain=plain, rmse_guided=guided)
    assert guided < plain and guided < alone
    assert rows[32][0] < rows[1][0]  # the history converged
