"""The restatement of the temporal response (tests/response_ref.py) held against what it must be: its fixed point, its ranges, the plain
accumulate it reduces to, numpy's own mean and variance over the clipped window, the spread of its test cases, and -- on the oracle alone --
the lighting change it is there for.  Runs without a GPU."""
import functools
import math

import numpy as np
import pytest

import denoise_ref as R
import gpu_util as U
import orclib as O
import response_ref as P
import temporal_ref as T
from ptamd import scenes
from test_denoise_ref import pixel_centre_rays


def test_a_constant_image_is_a_fixed_point():
    """the frame and both histories hold one colour: whatever the guides and the counts say, every blend and the mix return it, and s == 0"""
    colour = np.array([0.3, 1.7, 0.05])
    for pose in ("history", "pan", "big"):
        case = T.make_case(pose, 23, 17)
        albedo = case["albedo_hits"][..., :3].astype(np.float64) / case["gspp"]
        accum = np.zeros((17, 23, 4))
        accum[..., :3] = colour * np.maximum(albedo, R.ALBEDO_FLOOR)  # d = c / max(a, floor) == colour
        hist = case["hist_cn"].astype(np.float64)
        hist[..., :3] = colour
        fast = hist.copy()
        fast[..., 3] = np.minimum(fast[..., 3], P.FAST_HISTORY)
        out, _, f, s = P.accumulate(accum, 1, case["albedo_hits"], case["normal_depth"], 1, case["camera"],
                                    (hist, case["hist_nd"], case["hist_camera"], fast))
        assert np.abs(out[..., :3] - colour).max() < 1e-12 and np.abs(f[..., :3] - colour).max() < 1e-12
        assert not s.any()


@pytest.mark.parametrize("name,kw", P.GPU_CASES, ids=[n for n, _ in P.GPU_CASES])
def test_ranges_and_spread_of_every_device_case(name, kw):
    """s lies in [0, 1]; N_out lies between N_f and N_l; fast is the plain accumulate of the fast image under its own cap.  And the cases
    exercise the whole mix: the float64 restatement puts at least 5 % of the pixels in each of s == 0, 0 < s < 1 and s == 1 -- wherever that
    can be: with the camera turned away ("turn": every lambda <= 0) no pixel has a history and s is 0 throughout, and on 5 x 3 every window
    holds 12 to 15 of the 15 pixels, so s takes three values at most (what is asserted there is that the mix is not idle)."""
    case = P.make_case(**kw)
    for dt in (np.float64, np.float32):
        out, nd, fast, s = P.run_case(case, dt)
        assert s.dtype == dt and np.all(s >= 0) and np.all(s <= 1) and np.all(np.isfinite(s))
        hist = (case["hist_cn"], case["hist_nd"], case["hist_camera"])
        mo = dict(motion=case["motion"], prev_normal=case["prev_normal"]) if "motion" in case else {}
        args = (case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], case["camera"])
        plain = T.accumulate(*args, hist, dtype=dt, **mo)[0]
        plain_fast = T.accumulate(*args, (case["hist_fast"], hist[1], hist[2]), max_history=P.FAST_HISTORY, dtype=dt, **mo)[0]
        assert np.array_equal(fast, plain_fast)
        lo, hi = np.minimum(plain[..., 3], fast[..., 3]), np.maximum(plain[..., 3], fast[..., 3])
        slack = 4 * np.finfo(dt).eps * hi
        assert np.all(out[..., 3] >= lo - slack) and np.all(out[..., 3] <= hi + slack)
        assert np.array_equal(out[s == 0], plain[s == 0])
    zero, between, one = P.fractions(P.run_case(case, np.float64)[3])
    print(f"{name}: s == 0 {zero:.3f}, 0 < s < 1 {between:.3f}, s == 1 {one:.3f}")
    if kw["pose"] == "turn":
        assert zero == 1.0
    elif (kw["width"], kw["height"]) == (5, 3):
        assert kw["pose"] == "big" or between + one > 0
    else:
        assert min(zero, between, one) >= 0.05


def test_equal_histories_give_the_plain_accumulate_exactly():
    """fast == long under the same cap: the two blends are one, t == 0, and colour_count has the plain accumulate's bits -- in both precisions"""
    for pose in ("pan", "big"):
        case = T.make_case(pose, 70, 45, firefly=True)
        hist = (case["hist_cn"], case["hist_nd"], case["hist_camera"])
        args = (case["accum"], 1, case["albedo_hits"], case["normal_depth"], 1, case["camera"])
        for dt in (np.float64, np.float32):
            plain = T.accumulate(*args, hist, dtype=dt)
            out, nd, fast, s = P.accumulate(*args, hist + (case["hist_cn"],), fast_history=T.MAX_HISTORY, dtype=dt)
            assert not s.any()
            assert np.array_equal(out, plain[0]) and np.array_equal(nd, plain[1]) and np.array_equal(fast, plain[0])
    first = P.accumulate(*args, None)
    assert np.array_equal(first[0], first[2]) and not first[3].any() and np.all(first[0][..., 3] == 1)


def brute_force_mix(l_f, l_l):
    """steps 3 and 4 pixel by pixel, with numpy's own mean and variance over the clipped window"""
    H, W = l_f.shape
    s = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            win = (slice(max(y - P.RADIUS, 0), min(y + P.RADIUS, H - 1) + 1), slice(max(x - P.RADIUS, 0), min(x + P.RADIUS, W - 1) + 1))
            n_p = l_f[win].size
            mu_f, mu_l, sd = l_f[win].mean(), l_l[win].mean(), l_f[win].std()
            t = abs(mu_f - mu_l) / (P.SIGMA_RESPONSE * sd / math.sqrt(n_p) + P.RELATIVE_FLOOR * (max(mu_f, mu_l) + 1e-3))
            s[y, x] = min(max(t - 1.0, 0.0), 1.0)
    return s


@pytest.mark.parametrize("width,height", [(5, 3), (3, 5), (1, 1), (7, 7), (16, 16), (40, 9)])
def test_the_window_is_clipped_to_the_image(width, height):
    """an image narrower than the radius (5 x 3: every window is cut on two or three sides), one pixel, exactly one window, and images whose
    interior sees whole windows"""
    rng = np.random.default_rng(width * 100 + height)
    l_l = rng.gamma(0.6, 1.5, (height, width))
    l_f = l_l + np.linspace(0.0, 4.0, width)[None, :] * rng.uniform(0.5, 1.0, (height, width))
    total, count = P.window_sums(l_f)
    for y in range(height):
        for x in range(width):
            ny = min(y + P.RADIUS, height - 1) - max(y - P.RADIUS, 0) + 1
            nx = min(x + P.RADIUS, width - 1) - max(x - P.RADIUS, 0) + 1
            assert count[y, x] == nx * ny
    s = P.mix_factor(l_f, l_l)
    assert np.abs(s - brute_force_mix(l_f, l_l)).max() < 1e-12
    assert s.max() > 0 or width * height == 1  # (one pixel: no offset at x = 0, t == 0)


# ---------------------------------------------------------------- the oracle: a light that jumps, a steady light, a camera arc
FRAMES, JUMP_AFTER = 48, 16
CHECKPOINTS = (16, 20, 32, 48)


def guides_of(bundle, camera):
    sc = U.oracle_scene(bundle)
    o, dirs = pixel_centre_rays(camera, 64, 64)
    ah, nd = (x.reshape(64, 64, 4) for x in R.guide_deposits(bundle.flat, dirs, O.intersect_batch(sc, o, dirs, threads=8)))
    return sc, ah, nd


def converged(sc, camera):
    hi, _ = O.render(sc, camera, 64, 64, 256, first_sample=1000, threads=8)
    return U.tonemap(hi[:, :3].reshape(64, 64, 3), 256, camera)


def run_histories(states, frames):
    """states(f) -> (oracle scene, albedo_hits, normal_depth, camera) of frame f (0-based).  One 1-spp oracle frame per first_sample, blended by
    temporal_ref (the plain history) and by response_ref.  Yields (f + 1, plain colour_count, response colour_count, mean s, albedo)."""
    plain, resp = None, None
    for f in range(frames):
        sc, ah, nd, cam = states(f)
        frame, _ = O.render(sc, cam, 64, 64, 1, first_sample=f, threads=8)
        frame = frame.reshape(64, 64, 4)
        cn, gd, _ = T.accumulate(frame, 1, ah, nd, 1, cam, plain)
        plain = (cn, gd, cam)
        out, gd2, fast, s = P.accumulate(frame, 1, ah, nd, 1, cam, resp)
        resp = (out, gd2, cam, fast)
        a = R.prepare(np.zeros((64, 64, 4)), 1, ah, nd, 1)[1]
        yield f + 1, cn, out, float(s.mean()), a


@functools.lru_cache(maxsize=None)
def light_table(x_before, x_after):
    """{frame: (plain RMSE, response RMSE, mean s)}: tone-mapped RMSE of the re-modulated history against 256 spp of the state the frame shows"""
    b = scenes.cornell_moving_light(64, 64, x_before)
    before = guides_of(b, b.camera)
    want_before = converged(before[0], b.camera)
    if x_after != x_before:
        scenes.move_light(b, x_after)
        after = guides_of(b, b.camera)
        want_after = converged(after[0], b.camera)
    else:
        after, want_after = before, want_before
    out = {}
    for f, cn, mixed, s, a in run_histories(lambda f: (before if f < JUMP_AFTER else after) + (b.camera,), FRAMES):
        if f in CHECKPOINTS:
            want = want_before if f <= JUMP_AFTER else want_after
            out[f] = tuple(U.rmse(U.tonemap(x[..., :3] * a, 1, b.camera), want) for x in (cn, mixed)) + (s,)
    return out


def show(title, table):
    for f in sorted(table):
        plain, resp, s = table[f]
        print(f"{title}, frame {f:2d}: plain history {plain:.3e}, with the response {resp:.3e} (ratio {resp / plain:.3f}), mean s {s:.1e}")


def test_the_response_follows_a_light_that_jumps():
    """cornell_moving_light at 64 x 64, 1 spp per frame, the light at x = -0.5 for 16 frames, then at +0.5; the defaults.  Just before the jump
    the response costs at most 2 %; at frames 32 and 48 its RMSE is at most 0.75 x the plain history's.  Measured:
    ratios 1.000, 0.49 and 0.52 at frames 16, 32 and 48 (0.68 at frame 20)."""
    table = light_table(-0.5, 0.5)
    show("light jumps -0.5 -> +0.5", table)
    assert table[16][1] <= 1.02 * table[16][0]
    for f in (32, 48):
        assert table[f][1] <= 0.75 * table[f][0], f


def test_a_steady_light_is_left_alone():
    table = light_table(-0.5, -0.5)
    show("steady light", table)
    assert table[48][1] <= 1.02 * table[48][0]


def test_a_camera_arc_is_left_alone():
    """the camera on an arc of 2 degrees per frame about the room's centre, 24 frames: reprojection noise is not a lighting change"""
    b = scenes.cornell_moving_light(64, 64, 0.0)
    frames = 24

    @functools.lru_cache(maxsize=None)
    def state(f):
        a = math.radians(2.0 * f)
        cam = scenes._camera(64, 64, (3.9 * math.sin(a), 1.0, -3.9 * math.cos(a)), (0.0, 1.0, 0.0), 40.0)
        return guides_of(b, cam) + (cam,)
    for f, cn, mixed, s, a in run_histories(state, frames):
        pass
    sc, _, _, cam = state(frames - 1)
    want = converged(sc, cam)
    plain, resp = (U.rmse(U.tonemap(x[..., :3] * a, 1, cam), want) for x in (cn, mixed))
    print(f"camera arc, frame {frames}: plain history {plain:.3e}, with the response {resp:.3e} (ratio {resp / plain:.4f}), mean s {s:.1e}")
    assert resp <= 1.02 * plain
