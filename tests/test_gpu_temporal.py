"""The temporal history on the device (pt_temporal_accumulate, pt_set_sample_base, PT_DENOISE_INPUT_TEMPORAL; include/ptamd.h "temporal
history") against its numpy restatement (tests/temporal_ref.py): synthetic inputs through write_accum / write_guides / write_temporal,
rendered frames, the refusals, the C++ example."""
import math
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import gpu_util as U
import temporal_ref as T
from ptamd import device as D, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def load(ctx, case, history=True):
    """the inputs of one accumulate into the context: accumulator, guides, camera and (optionally) the history"""
    ctx.write_accum(case["accum"], case["spp"])
    ctx.write_guides(case["albedo_hits"], case["normal_depth"], case["gspp"])
    ctx.set_camera(case["camera"])
    if history:
        ctx.write_temporal(case["hist_cn"], case["hist_nd"], case["hist_camera"])


def read(ctx, case):
    cn, nd = ctx.read_temporal()
    return cn.reshape(case["height"], case["width"], 4), nd.reshape(case["height"], case["width"], 4)


def current_d(case, dtype=np.float64):
    return R.prepare(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], dtype)[0]


def check_against_restatement(gpu, case, name):
    """one accumulate of `case` on a fresh context: colour_count within the bound of the float64 restatement (absolute, rgb and N alike),
    normal_depth = prepare's (n, z), the history did something, and a second run gives the same bits"""
    ctx = gpu.Context(case["width"], case["height"])
    load(ctx, case)
    assert ctx.temporal_frames == 1
    ctx.temporal_accumulate()
    assert ctx.temporal_frames == 2
    cn, nd = read(ctx, case)
    ref, bound = T.bound(case)
    err_rgb = float(np.abs(cn[..., :3].astype(np.float64) - ref[..., :3]).max())
    err_n = float(np.abs(cn[..., 3].astype(np.float64) - ref[..., 3]).max())
    U.record_margin(f"temporal vs restatement: {name}", error_rgb=err_rgb, error_count=err_n, bound=bound)
    print(f"{name}: rgb error {err_rgb:.3e}, count error {err_n:.3e}, bound {bound:.3e}")
    _, _, n, z = R.prepare(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], np.float64)
    assert np.allclose(nd[..., :3], n, rtol=1e-6, atol=1e-6) and np.allclose(nd[..., 3], z, rtol=1e-6, atol=0)
    assert err_rgb <= bound and err_n <= bound
    assert np.abs(cn[..., :3] - current_d(case)).max() > 10 * bound  # not the current frame handed through
    load(ctx, case)  # (the sets flipped: the history goes into what is now the newest one)
    ctx.temporal_accumulate()
    cn2, nd2 = read(ctx, case)
    assert np.array_equal(cn2.view(np.uint32), cn.view(np.uint32)) and np.array_equal(nd2.view(np.uint32), nd.view(np.uint32))
    ctx.close()
    return cn, ref, bound


@pytest.mark.parametrize("width,height", T.SIZES)
@pytest.mark.parametrize("pose", ["pan", "big"])
def test_accumulate_matches_the_restatement(gpu, pose, width, height):
    """16 x 16 is smaller than the 32 x 8 tile, 70 x 45 no multiple of it, 150 x 83 several tiles each way"""
    check_against_restatement(gpu, T.make_case(pose, width, height), f"{pose} {width}x{height}")


def test_accumulate_with_fireflies(gpu):
    """a 1e4 firefly in the current frame and one in the history, same absolute bound"""
    check_against_restatement(gpu, T.make_case("pan", 70, 45, firefly=True), "pan 70x45, fireflies")


@pytest.mark.parametrize("width,height", T.SIZES)
def test_static_camera(gpu, width, height):
    """Same camera, every N_h >= 1, history guides equal to the current ones: fx is an exact integer in float64 and round-off picks the side of
    floor(); the bilinear weights make that harmless."""
    case = T.make_case("history", width, height, all_counted=True, same_guides=True)
    cn, ref, bound = check_against_restatement(gpu, case, f"static {width}x{height}")
    assert np.abs(cn[..., 3] - np.minimum(case["hist_cn"][..., 3] + 1, T.MAX_HISTORY)).max() <= bound + 1e-2


def test_no_history(gpu):
    """The camera turned away, and the first call after a reset: d_out is the current d and N = 1 everywhere.  "The current d" is the device's
    own (its division is good to an ulp, not correctly rounded): both routes must give the same bits, and those agree with numpy's float32."""
    case = T.make_case("turn", 70, 45)
    ctx = gpu.Context(70, 45)
    load(ctx, case)
    ctx.temporal_accumulate()
    turned, nd_turned = read(ctx, case)
    ctx.temporal_reset()
    assert ctx.temporal_frames == 0
    ctx.temporal_accumulate()
    assert ctx.temporal_frames == 1
    first, nd_first = read(ctx, case)
    fresh = gpu.Context(70, 45)
    load(fresh, case, history=False)
    fresh.temporal_accumulate()
    never, _ = read(fresh, case)
    for cn in (turned, first, never):
        assert np.all(cn[..., 3] == 1.0)
        assert np.allclose(cn[..., :3], current_d(case, np.float32), rtol=1e-6, atol=0)
    assert np.array_equal(turned.view(np.uint32), first.view(np.uint32)) and np.array_equal(never.view(np.uint32), first.view(np.uint32))
    assert np.array_equal(nd_turned.view(np.uint32), nd_first.view(np.uint32))
    ctx.close()
    fresh.close()


def test_chained(gpu):
    """A -> B -> C with two accumulate calls and no write in between: ping-pong and the remembered camera.  The bound is computed on the
    restatement chained the same way."""
    width, height = 70, 45
    b, c = T.make_case("pan", width, height, seed=21), T.make_case("pan2", width, height, seed=22)
    ctx = gpu.Context(width, height)
    load(ctx, b)  # history made under A
    ctx.temporal_accumulate()
    load(ctx, c, history=False)
    ctx.temporal_accumulate()
    assert ctx.temporal_frames == 3
    cn, nd = read(ctx, c)

    def chain(dtype):
        o1, nd1, _ = T.run_case(b, dtype)
        return T.accumulate(c["accum"], c["spp"], c["albedo_hits"], c["normal_depth"], c["gspp"], c["camera"], (o1, nd1, b["camera"]), dtype=dtype)
    ref, ref32 = chain(np.float64)[0], chain(np.float32)[0]
    largest = max(float(x["accum"][..., :3].max()) for x in (b, c))
    bound = 8.0 * float(np.abs(ref32.astype(np.float64) - ref).max()) + 1e-6 * max(largest, float(b["hist_cn"][..., :3].max()))
    err = float(np.abs(cn.astype(np.float64) - ref).max())
    U.record_margin("temporal vs restatement: chained A-B-C 70x45", error=err, bound=bound)
    print(f"chained: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.abs(cn[..., 3]).max() > 2.0  # counts carried through both steps
    ctx.close()


def test_filter_reads_the_history(gpu):
    width, height = 70, 45
    case = T.make_case("pan", width, height)
    plain = gpu.Context(width, height)
    load(plain, case, history=False)
    unflagged = plain.denoise(3, hdr=True)
    ctx = gpu.Context(width, height)
    load(ctx, case)
    ctx.temporal_accumulate()
    cn, _ = read(ctx, case)
    out = ctx.denoise(3, hdr=True, input_temporal=True)

    def want(dtype):
        _, a, n, z = R.prepare(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], dtype)
        return R.atrous(cn[..., :3].astype(dtype), n, z, 3) * a
    ref, ref32 = want(np.float64), want(np.float32)
    assert ref32.dtype == np.float32
    bound = 8.0 * float(np.abs(ref32.astype(np.float64) - ref).max()) + 1e-6 * float(cn[..., :3].max())
    err = float(np.abs(out[..., :3].astype(np.float64) - ref).max())
    U.record_margin("denoise over the history vs restatement: 70x45, 3 iterations", error=err, bound=bound)
    print(f"filter over the history: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound and np.all(out[..., 3] == 1.0)
    assert np.abs(out[..., :3] - unflagged[..., :3]).max() > 10 * bound
    # zero iterations: the history re-modulated
    a = R.prepare(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], np.float64)[1]
    assert np.allclose(ctx.denoise(0, hdr=True, input_temporal=True)[..., :3], cn[..., :3] * a, rtol=1e-6, atol=0)
    assert ctx.denoise(0, input_temporal=True)[..., :3].max() <= 1.0
    # without the flag a history changes nothing
    assert np.array_equal(ctx.denoise(3, hdr=True).view(np.uint32), unflagged.view(np.uint32))
    assert np.array_equal(ctx.denoise(3).view(np.uint32), plain.denoise(3).view(np.uint32))
    ctx.close()
    plain.close()


def test_sample_base(gpu):
    b = scenes.cornell_box(64, 64)
    based = U.make_ctx(gpu, b, 64, 64)
    based.set_sample_base(5)
    assert based.sample_base == 5
    based.clear()
    based.render(1)
    based.render_guides(1)
    assert based.sample_base == 5 and based.samples_per_pixel == 1 and based.guide_samples == 1  # the counts do not include the base
    shifted = U.make_ctx(gpu, b, 64, 64)
    zeros = np.zeros((64 * 64, 4), np.float32)
    shifted.write_accum(zeros, 5)
    shifted.write_guides(zeros, zeros, 5)
    shifted.render(1)
    shifted.render_guides(1)
    assert based.read_accum().any()
    assert np.array_equal(based.read_accum().view(np.uint32), shifted.read_accum().view(np.uint32))
    for x, y in zip(based.read_guides(), shifted.read_guides()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    never = U.make_ctx(gpu, b, 64, 64)
    never.render(1)
    never.render_guides(1)
    assert not np.array_equal(based.read_accum(), never.read_accum())  # sample 5 is not sample 0
    based.set_sample_base(0)
    based.clear()
    assert based.sample_base == 0
    based.render(1)
    based.render_guides(1)
    assert np.array_equal(based.read_accum().view(np.uint32), never.read_accum().view(np.uint32))
    for x, y in zip(based.read_guides(), never.read_guides()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for c in (based, shifted, never):
        c.close()


def orbit_camera(degrees, width=64, height=64):
    """the Cornell box's camera turned about the vertical axis through the room's centre"""
    t = math.radians(degrees)
    return scenes._camera(width, height, (-3.9 * math.sin(t), 1.0, -3.9 * math.cos(t)), (0.0, 1.0, 0.0), 40.0)


def test_rendered_orbit_is_closer_to_the_converged_image_over_the_history(gpu):
    """Twelve 1-spp frames on an arc of 2 degrees per frame, the sample base set to the frame number: the last frame filtered over the history
    must be closer (tone-mapped RMSE) to a 256-spp render of the last camera than the same frame filtered alone."""
    b = scenes.cornell_box(64, 64)
    ctx = U.make_ctx(gpu, b, 64, 64)
    frames = 12
    for f in range(frames):
        cam = orbit_camera(2.0 * (f - frames + 1))
        ctx.set_sample_base(f)
        ctx.set_camera(cam)
        ctx.clear()
        ctx.render(1)
        ctx.render_guides(1)
        ctx.temporal_accumulate()
    assert ctx.temporal_frames == frames
    over_history = ctx.denoise(5, hdr=True, input_temporal=True)[..., :3]
    alone = ctx.denoise(5, hdr=True)[..., :3]
    cn, _ = ctx.read_temporal()
    ref = U.make_ctx(gpu, b, 64, 64, camera=cam)
    ref.set_sample_base(1000)
    ref.render(256)
    want = U.tonemap(ref.read_accum()[:, :3].reshape(64, 64, 3), 256, cam)
    e_temporal, e_alone = U.rmse(U.tonemap(over_history, 1, cam), want), U.rmse(U.tonemap(alone, 1, cam), want)
    U.record_margin("rendered orbit, cornell 64x64, 12 frames of 1 spp", rmse_over_history=e_temporal, rmse_alone=e_alone, ratio=e_temporal / e_alone,
                    mean_count=float(cn[:, 3].mean()))
    print(f"orbit: tone-mapped RMSE against 256 spp: over the history {e_temporal:.3e}, alone {e_alone:.3e}, ratio {e_temporal / e_alone:.3f}; "
          f"mean history count {cn[:, 3].mean():.2f}")
    assert cn[:, 3].mean() > 2.0  # the orbit kept its history
    assert e_temporal < e_alone
    ctx.close()
    ref.close()


def test_refusals_and_what_leaves_the_history_alone(gpu):
    INVALID, STATE, UNSUPPORTED = -1, -3, -4
    case = T.make_case("pan", 16, 16)
    bare = gpu.Context(16, 16)
    bare.write_accum(case["accum"], 1)
    bare.write_guides(case["albedo_hits"], case["normal_depth"], 1)
    assert U.status(bare.temporal_accumulate) == STATE  # no camera
    assert U.status(lambda: bare.denoise(3, hdr=True, input_temporal=True)) == STATE  # no history
    bare.set_camera(case["camera"])
    bare.temporal_accumulate()
    bare.close()
    ctx = gpu.Context(16, 16)
    ctx.set_camera(case["camera"])
    ctx.write_guides(case["albedo_hits"], case["normal_depth"], 1)
    assert U.status(ctx.temporal_accumulate) == STATE  # no colour sample
    ctx.write_accum(case["accum"], 1)
    ctx.write_guides(case["albedo_hits"], case["normal_depth"], 0)
    assert U.status(ctx.temporal_accumulate) == STATE  # no guide sample
    ctx.write_guides(case["albedo_hits"], case["normal_depth"], 1)
    assert U.status(lambda: ctx.temporal_accumulate(max_history=4097)) == INVALID
    assert U.status(lambda: ctx.temporal_accumulate(sigma_depth=-1.0)) == INVALID
    assert U.status(lambda: ctx.temporal_accumulate(k_normal=-1.0)) == INVALID
    ctx.set_tiles([(0, 0, 8, 16)])
    assert U.status(ctx.temporal_accumulate) == UNSUPPORTED
    ctx.set_tiles([])
    assert ctx.temporal_frames == 0  # a refused call is no call
    ctx.temporal_accumulate(max_history=4096)
    ctx.write_temporal(case["hist_cn"], case["hist_nd"], case["hist_camera"])
    assert ctx.temporal_frames == 1
    ctx.clear()  # clears accumulator and guides, not the history
    ctx.set_camera(case["camera"])
    assert ctx.temporal_frames == 1 and ctx.samples_per_pixel == 0
    cn, nd = ctx.read_temporal()
    assert np.array_equal(cn.reshape(16, 16, 4), case["hist_cn"]) and np.array_equal(nd.reshape(16, 16, 4), case["hist_nd"])
    assert U.status(lambda: ctx.denoise(3, input_temporal=True)) == STATE  # a history, but no sample of the current frame
    assert ctx.temporal_device_ptr(0) and ctx.temporal_device_ptr(1) and ctx.temporal_device_ptr(0) != ctx.temporal_device_ptr(1)
    ctx.close()
    parity = gpu.Context(16, 16, rng_mode=D.RNG_LFSR113_PARITY)
    assert U.status(lambda: parity.set_sample_base(3)) == UNSUPPORTED
    assert parity.sample_base == 0
    parity.close()


def test_cpp_orbit_example(gpu, tmp_path):
    """examples/orbit_cornell.cpp: three images of one size; the one filtered over the history has less high-frequency energy than the one
    filtered alone."""
    paths = [tmp_path / n for n in ("raw.ppm", "filtered.ppm", "temporal.ppm")]
    r = subprocess.run([os.path.join(ROOT, "examples", "orbit_cornell"), "12"] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split() if "=" in kv)
    assert int(fields["frames"]) == 12 and int(fields["spp"]) == 1 and int(fields["temporal_frames"]) == 12
    raw, filtered, temporal = (U.read_ppm(p) for p in paths)
    assert raw.shape == filtered.shape == temporal.shape == (256, 256, 3)
    assert not np.array_equal(filtered, temporal) and not np.array_equal(raw, temporal)
    lr, lf, lt = (U.mean_abs_laplacian(x) for x in (raw, filtered, temporal))
    print(f"mean |Laplacian|: raw {lr:.4f}, filtered alone {lf:.4f}, filtered over the history {lt:.4f}")
    assert lt < lf
