"""The temporal response on the device (pt_set_temporal_response, k_temporal<., ., true>, k_temporal_response; include/ptamd.h "temporal
response") against its numpy restatement (tests/response_ref.py): synthetic inputs through write_accum / write_guides / write_temporal /
write_temporal_fast, the bits it owes a context with the mode off, the refusals, and a light that jumps in a rendered room."""
import os
import subprocess

import numpy as np
import pytest

import gpu_util as U
import orclib as O
import response_ref as P
import temporal_ref as T
from ptamd import device as D, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def load(ctx, case, history=True, fast=True):
    """the inputs of one accumulate into the context; fast: the history's fast image too (the mode must be on)"""
    ctx.write_accum(case["accum"], case["spp"])
    ctx.write_guides(case["albedo_hits"], case["normal_depth"], case["gspp"])
    if "motion" in case:
        ctx.write_motion_guides(case["motion"], case["prev_normal"])
    ctx.set_camera(case["camera"])
    if history:
        ctx.write_temporal(case["hist_cn"], case["hist_nd"], case["hist_camera"])
        if fast:
            ctx.write_temporal_fast(case["hist_fast"])


def make_ctx(gpu, case):
    if "motion" not in case:
        return gpu.Context(case["width"], case["height"])
    flat = scenes.cornell_box(64, 64).flat  # a motion can only be set on a context that holds a scene: every leaf where it was
    ctx = U.make_ctx(gpu, flat, case["width"], case["height"])
    ctx.set_instance_motion(flat.top_nodes)
    assert ctx.instance_motion == (True, 0)
    return ctx


def read_all(ctx, case):
    h, w = case["height"], case["width"]
    cn, nd = ctx.read_temporal()
    return cn.reshape(h, w, 4), nd.reshape(h, w, 4), ctx.read_temporal_fast().reshape(h, w, 4), ctx.read_temporal_response().reshape(h, w)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name,kw", P.GPU_CASES, ids=[n for n, _ in P.GPU_CASES])
def test_accumulate_matches_the_restatement(gpu, name, kw):
    """colour_count (mixed), fast and s against the float64 restatement, each within 8 x what float32 costs the restatement on that input +
    1e-6 x the largest colour; normal_depth with the bits of a context with the mode off; a second run with the same bits.  16 x 16 is
    smaller than the 32 x 8 tile (halo beyond every edge), 70 x 45 no multiple of it, 150 x 83 several tiles each way, 5 x 3 narrower than
    the window; tests/test_response_ref.py holds the spread of s on these very cases."""
    case = P.make_case(**kw)
    ctx = make_ctx(gpu, case)
    ctx.set_temporal_response()
    assert ctx.temporal_response is True
    load(ctx, case)
    assert np.array_equal(bits(ctx.read_temporal_fast()), bits(case["hist_fast"]).reshape(-1, 4))
    ctx.temporal_accumulate()
    cn, nd, fast, s = read_all(ctx, case)
    (ref_cn, _, ref_fast, ref_s), (b_cn, b_fast, b_s) = P.bounds(case)
    for what, got, ref, bound in (("colour_count", cn, ref_cn, b_cn), ("fast", fast, ref_fast, b_fast), ("s", s, ref_s, b_s)):
        err = float(np.abs(got.astype(np.float64) - ref).max())
        U.record_margin(f"temporal response vs restatement: {name}, {what}", error=err, bound=bound)
        print(f"{name}: {what} error {err:.3e}, bound {bound:.3e}")
        assert np.all(np.isfinite(got))
        assert err <= bound, what
    assert np.all(s >= 0) and np.all(s <= 1)
    zero, between, one = P.fractions(s)
    print(f"{name}: device s == 0 {zero:.3f}, 0 < s < 1 {between:.3f}, s == 1 {one:.3f}")
    off = make_ctx(gpu, case)
    load(off, case, fast=False)
    off.temporal_accumulate()
    cn_off, nd_off = off.read_temporal()
    off.close()
    assert np.array_equal(bits(nd), bits(nd_off).reshape(nd.shape))
    unmixed = s == 0  # where nothing was mixed colour_count is the plain kernel's, bit for bit
    assert np.array_equal(bits(cn)[unmixed], bits(cn_off).reshape(cn.shape)[unmixed])
    load(ctx, case)  # (the sets flipped: the inputs go into what is now the newest one)
    ctx.temporal_accumulate()
    again = read_all(ctx, case)
    for a, b in zip(again, (cn, nd, fast, s)):
        assert np.array_equal(bits(a), bits(b))
    ctx.close()


def frame_case(pose, seed, width=70, height=45):
    """a current frame alone (no history is taken from it)"""
    return T.make_case(pose, width, height, seed=seed)


@pytest.mark.parametrize("variance", [False, True], ids=["response", "response+variance"])
def test_a_short_history_has_the_bits_of_the_mode_off(gpu, variance):
    """While pt_temporal_frames() <= fast_history the two histories are one: colour_count has the bits of a context with the mode off, fast
    the bits of colour_count, s is 0.  Four accumulates from nothing, the camera still, then panning: the default fast_history of 4.  With
    the variance mode on as well the variance plane has the bits of a variance-only context."""
    width, height = 70, 45
    steps = [frame_case("history", 41), frame_case("history", 42), frame_case("pan", 43), frame_case("pan2", 44), frame_case("pan", 45), frame_case("history", 46)]
    on, off = gpu.Context(width, height), gpu.Context(width, height)
    on.set_temporal_response()
    if variance:
        on.set_temporal_variance()
        off.set_temporal_variance()
    parted = False
    for k, case in enumerate(steps):
        for ctx in (on, off):
            load(ctx, case, history=False)
            ctx.temporal_accumulate()
        assert on.temporal_frames == off.temporal_frames == k + 1
        cn, nd = on.read_temporal()
        cn_off, nd_off = off.read_temporal()
        fast, s = on.read_temporal_fast(), on.read_temporal_response()
        assert np.array_equal(bits(nd), bits(nd_off))
        if k + 1 <= P.FAST_HISTORY:
            assert not s.any()
            assert np.array_equal(bits(cn), bits(cn_off)) and np.array_equal(bits(fast), bits(cn))
            if variance:
                assert np.array_equal(bits(on.read_temporal_variance()), bits(off.read_temporal_variance()))
        else:  # the long history goes on growing, the fast one is capped
            assert fast[:, 3].max() <= P.FAST_HISTORY and cn_off[:, 3].max() > P.FAST_HISTORY
            assert not np.array_equal(bits(fast), bits(cn))
            parted = True
    assert parted
    on.close(), off.close()


def test_the_variance_plane_is_the_variance_modes_own(gpu):
    """one accumulate over a written history, both modes on, s anywhere in [0, 1]: the variance plane has the bits of a variance-only context
    (k_temporal<., true> wrote it; the mix does not touch it)"""
    case = P.make_case("pan", 70, 45)
    rng = np.random.default_rng(5)
    hist_v = rng.uniform(0.0, 10.0, (45, 70)).astype(np.float32)
    planes = []
    for response in (True, False):
        ctx = gpu.Context(70, 45)
        ctx.set_temporal_variance()
        if response:
            ctx.set_temporal_response()
        load(ctx, case, fast=response)
        ctx.write_temporal_variance(hist_v)
        ctx.temporal_accumulate()
        planes.append(ctx.read_temporal_variance())
        if response:
            assert min(P.fractions(ctx.read_temporal_response())) >= 0.05
        ctx.close()
    assert planes[0].any() and np.array_equal(bits(planes[0]), bits(planes[1]))


def test_write_temporal_zeroes_the_fast_history(gpu):
    """... of the set it writes; the fast history then restarts from the current frame: fast = (d, 1) after the next accumulate"""
    case = P.make_case("pan", 70, 45)
    ctx = gpu.Context(70, 45)
    ctx.set_temporal_response()
    load(ctx, case)
    assert ctx.read_temporal_fast().any() and ctx.temporal_fast_device_ptr
    ctx.write_temporal(case["hist_cn"], case["hist_nd"], case["hist_camera"])
    assert not ctx.read_temporal_fast().any()
    ctx.temporal_accumulate()
    first = gpu.Context(70, 45)  # what a first frame gives: (d, 1)
    load(first, case, history=False)
    first.temporal_accumulate()
    assert np.array_equal(bits(ctx.read_temporal_fast()), bits(first.read_temporal()[0]))
    assert np.all(ctx.read_temporal_fast()[:, 3] == 1.0)
    first.close(), ctx.close()


def test_refusals_and_what_they_leave_alone(gpu):
    INVALID, STATE, UNSUPPORTED = -1, -3, -4
    case = P.make_case("pan", 16, 16)
    ctx = gpu.Context(16, 16)
    assert ctx.temporal_response is False and ctx.temporal_fast_device_ptr == 0
    for bad in (dict(fast_history=4097), dict(sigma_response=-1.0), dict(relative_floor=-0.5), dict(sigma_response=float("nan")),
                dict(relative_floor=float("inf")), dict(sigma_response=float("inf")), dict(relative_floor=float("nan"))):
        assert U.status(lambda: ctx.set_temporal_response(**bad)) == INVALID, bad
        assert ctx.temporal_response is False
    # mode off: nothing to read or write
    load(ctx, case, fast=False)
    assert U.status(ctx.read_temporal_fast) == STATE
    assert U.status(lambda: ctx.write_temporal_fast(case["hist_fast"])) == STATE
    assert U.status(ctx.read_temporal_response) == STATE
    # a history exists: the mode cannot change, either way
    assert ctx.temporal_frames == 1
    assert U.status(ctx.set_temporal_response) == STATE
    assert ctx.temporal_response is False
    ctx.temporal_reset()
    ctx.set_temporal_response(fast_history=4096)
    ctx.set_temporal_response(fast_history=2, sigma_response=1.5, relative_floor=0.05)
    assert ctx.temporal_response is True
    # mode on, no history
    assert U.status(ctx.read_temporal_fast) == STATE
    assert U.status(lambda: ctx.write_temporal_fast(case["hist_fast"])) == STATE
    assert U.status(ctx.read_temporal_response) == STATE
    load(ctx, case)
    assert U.status(lambda: ctx.set_temporal_response(False)) == STATE  # forgetting, too
    assert U.status(ctx.set_temporal_response) == STATE
    assert U.status(lambda: ctx.set_temporal_response(fast_history=5000)) == INVALID
    assert ctx.temporal_response is True and ctx.temporal_frames == 1
    assert np.array_equal(bits(ctx.read_temporal_fast()), bits(case["hist_fast"]).reshape(-1, 4))  # the refused calls changed nothing
    ctx.temporal_accumulate()  # the parameters that were set are the ones in force
    (ref_cn, _, ref_fast, ref_s), (b_cn, b_fast, b_s) = P.bounds(case, fast_history=2, sigma_response=1.5, relative_floor=0.05)
    cn, _, fast, s = read_all(ctx, case)
    assert np.abs(s - ref_s).max() <= b_s and np.abs(fast - ref_fast).max() <= b_fast and np.abs(cn - ref_cn).max() <= b_cn
    assert fast[..., 3].max() == 2.0
    ctx.temporal_reset()
    assert ctx.temporal_response is True  # the reset keeps the mode
    ctx.set_temporal_response(False)
    assert ctx.temporal_response is False and ctx.temporal_fast_device_ptr == 0
    ctx.temporal_accumulate()  # the plain kernel again
    assert U.status(ctx.read_temporal_fast) == STATE
    ctx.close()
    for kw in (dict(rng_mode=D.RNG_LFSR113_PARITY), dict(max_active_rays=1024)):
        other = gpu.Context(64, 64, **kw)
        assert U.status(other.set_temporal_response) == UNSUPPORTED
        assert other.temporal_response is False
        other.close()


def test_the_buffers_go_with_the_context(gpu):
    """pt_debug_live_resources returns to its baseline after a context with the mode on is destroyed: two fast images and two scratch planes
    more than the history's own four while it lives"""
    case = P.make_case("pan", 16, 16)
    base = gpu.live_resources()
    counts = []
    for response in (False, True):
        ctx = gpu.Context(16, 16)
        if response:
            ctx.set_temporal_response()
        load(ctx, case, fast=response)
        ctx.temporal_accumulate()
        counts.append(gpu.live_resources()[0])
        ctx.close()
        assert gpu.live_resources() == base
    assert counts[1] == counts[0] + 4


# ---------------------------------------------------------------- end to end: a light that jumps in a rendered room
def test_a_rendered_light_that_jumps_is_followed(gpu):
    """cornell_moving_light at 64 x 64, 48 frames of 1 spp under a static camera; after frame 16 the light is re-posed from x = -0.5 to +0.5
    through upload_dynamic_async + frame_tick.  Tone-mapped RMSE of the re-modulated history against the oracle's 256 spp of the state the frame
    shows: with the mode on at most 0.75 x the mode-off history's at frames 32 and 48, at most 1.02 x at frame 16, both rendered here.
    The guide pass takes 16 samples per frame (first hits alone: cheap next to the frame).  The response answers a LONG history that is wrong, and how
    long the history grows is the guides' doing: with one jittered guide sample per frame depth and normal flicker at every edge, the confidence-scaled
    count of this room stays near 8 at frame 16 and 12 at frame 48 instead of 16 and 32, the plain history forgets the old light by itself and there is
    nothing to win.  Measured on an MI355X, ratios at frames 32 / 48 by guide samples per frame: 1: 0.99 / 1.00; 2: 0.92 / 0.99; 4: 0.70 / 0.87;
    8: 0.59 / 0.67; 16: 0.54 / 0.57 (the float64 prototype on pixel-centre guides: 0.49 / 0.52); at frame 16 every one of them is 1.000."""
    frames, jump_after, checkpoints, guide_samples = 48, 16, (16, 32, 48), 16
    b = scenes.cornell_moving_light(64, 64, -0.5)
    flat_before = b.flat
    sc = U.oracle_scene(b)
    ref, _ = O.render(sc, b.camera, 64, 64, 256, first_sample=1000, threads=8)
    want_before = U.tonemap(ref[:, :3].reshape(64, 64, 3), 256, b.camera)
    scenes.move_light(b, 0.5)
    flat_after = b.scene.flatten_dynamic(flat_before)[0]
    ref, _ = O.render(O.BoundScene(flat_after), b.camera, 64, 64, 256, first_sample=1000, threads=8)
    want_after = U.tonemap(ref[:, :3].reshape(64, 64, 3), 256, b.camera)
    want = {16: want_before, 32: want_after, 48: want_after}

    def loop(response):
        ctx = U.make_ctx(gpu, flat_before, 64, 64, camera=b.camera)
        if response:
            ctx.set_temporal_response()
        out = {}
        for f in range(frames):
            if f == jump_after:
                ctx.upload_dynamic_async(flat_after)
                ctx.frame_tick()
            ctx.set_sample_base(f)
            ctx.clear()
            ctx.render(1)
            ctx.render_guides(guide_samples)
            ctx.temporal_accumulate()
            if f + 1 in checkpoints:
                image = ctx.denoise(0, hdr=True, input_temporal=True)[..., :3]  # the history times the current albedo
                out[f + 1] = U.rmse(U.tonemap(image.astype(np.float64), 1, b.camera), want[f + 1])
        if response:
            out["mean s"] = float(ctx.read_temporal_response().mean())
        ctx.close()
        return out
    on, off = loop(True), loop(False)
    for f in checkpoints:
        print(f"frame {f}: mode off {off[f]:.3e}, mode on {on[f]:.3e}, ratio {on[f] / off[f]:.3f}")
    U.record_margin("rendered light jump, cornell_moving_light 64x64, 48 frames of 1 spp", **{f"rmse_off_{f}": off[f] for f in checkpoints},
                    **{f"rmse_on_{f}": on[f] for f in checkpoints}, mean_s_last=on["mean s"])
    assert on[16] <= 1.02 * off[16]
    assert on[32] <= 0.75 * off[32] and on[48] <= 0.75 * off[48]


def test_cpp_moving_light_example(gpu):
    """examples/moving_light.cpp: the C++ class, its own 64 x 64 room, the light swung after 16 frames, 16 guide samples per frame.  The same
    conditions as above, 16 and 32 frames after the jump; measured 0.43 and 0.48 (and 0.77 four frames after it)."""
    r = subprocess.run([os.path.join(ROOT, "examples", "moving_light"), "16", "256"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    rows = {}
    for line in r.stdout.splitlines():
        fields = dict(kv.split("=") for kv in line.split() if "=" in kv)
        if "after" in fields:
            rows[int(fields["after"])] = (float(fields["plain"]), float(fields["response"]))
        elif "before" in fields:
            assert int(fields["before"]) == 16 and int(fields["temporal_frames"]) == 48
    assert sorted(rows) == [4, 16, 32]
    U.record_margin("moving_light, 16 + 32 frames of 1 spp", **{f"rmse_plain_{k}": v[0] for k, v in rows.items()}, **{f"rmse_response_{k}": v[1] for k, v in rows.items()})
    for after in (16, 32):
        assert rows[after][1] <= 0.75 * rows[after][0], after
    assert rows[4][1] <= rows[4][0]
