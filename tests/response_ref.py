"""numpy restatement of the temporal response (pt_set_temporal_response; include/ptamd.h, "temporal response"): a short, fast history kept beside
the long one, and the mix of the two where their 7 x 7 low-passed luminances disagree by more than the fast one's own noise explains.
Parameterised by dtype like temporal_ref, on which it is built: float64 is the reference the device is held against, float32 measures what single
precision costs the same arithmetic on the same input.  Also the case generator the response tests share."""
import numpy as np

import denoise_ref as R
import motion_ref as M
import temporal_ref as T

RADIUS = 3  # PT_RESPONSE_RADIUS: the window is 7 x 7, clipped to the image
FAST_HISTORY, SIGMA_RESPONSE, RELATIVE_FLOOR = 4, 2.0, 0.02  # the defaults of pt_response_params


def window_sums(img, radius=RADIUS):
    """(sum of img over the (2 radius + 1)^2 window clipped to the image, the number of pixels in it), both (H, W) of img's dtype"""
    dt = img.dtype.type
    H, W = img.shape
    padded = np.zeros((H + 2 * radius, W + 2 * radius), img.dtype)
    padded[radius:radius + H, radius:radius + W] = img
    inside = np.zeros_like(padded)
    inside[radius:radius + H, radius:radius + W] = dt(1)
    total, count = np.zeros((H, W), img.dtype), np.zeros((H, W), img.dtype)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            total += padded[dy:dy + H, dx:dx + W]
            count += inside[dy:dy + H, dx:dx + W]
    return total, count


def mix_factor(l_f, l_l, sigma_response=0.0, relative_floor=0.0):
    """s (H, W) from the two luminance planes: steps 3 and 4 of the header.  Two passes: the mean, then the squared distances from it."""
    dt = l_f.dtype.type
    sigma_response, relative_floor = dt(sigma_response or SIGMA_RESPONSE), dt(relative_floor or RELATIVE_FLOOR)
    H, W = l_f.shape
    sum_f, n_p = window_sums(l_f)
    sum_l, _ = window_sums(l_l)
    mu_f, mu_l = sum_f / n_p, sum_l / n_p
    # second pass: (l_f(q) - mu_f(p))^2 over the window of p, tap by tap
    padded = np.zeros((H + 2 * RADIUS, W + 2 * RADIUS), l_f.dtype)
    padded[RADIUS:RADIUS + H, RADIUS:RADIUS + W] = l_f
    inside = np.zeros((H + 2 * RADIUS, W + 2 * RADIUS), bool)
    inside[RADIUS:RADIUS + H, RADIUS:RADIUS + W] = True
    var_f = np.zeros((H, W), l_f.dtype)
    for dy in range(2 * RADIUS + 1):
        for dx in range(2 * RADIUS + 1):
            delta = padded[dy:dy + H, dx:dx + W] - mu_f
            var_f += np.where(inside[dy:dy + H, dx:dx + W], delta * delta, dt(0))
    var_f = var_f / n_p
    t = np.abs(mu_f - mu_l) / (sigma_response * np.sqrt(var_f) / np.sqrt(n_p) + relative_floor * (np.maximum(mu_f, mu_l) + dt(1e-3)))
    s = np.clip(t - dt(1), dt(0), dt(1))
    assert s.dtype == l_f.dtype
    return s


def accumulate(accum, spp, albedo_hits, normal_depth, gspp, camera, history=None, max_history=T.MAX_HISTORY, fast_history=0, sigma_response=0.0,
               relative_floor=0.0, dtype=np.float64, **kw):
    """One pt_temporal_accumulate with the response on.  history: None or (colour_count, normal_depth, camera, fast), fast the (H, W, 4) fast
    history of that set.  Returns (colour_count -- mixed --, normal_depth, fast, s).  Both histories are temporal_ref.accumulate's: the long one with
    max_history, the fast one with fast_history as its cap and the fast image as the history's colours."""
    dt = dtype
    fast_history = fast_history or FAST_HISTORY
    long_hist = None if history is None else tuple(history[:3])
    fast_hist = None if history is None else (history[3], history[1], history[2])
    cn_l, nd, _ = T.accumulate(accum, spp, albedo_hits, normal_depth, gspp, camera, long_hist, max_history=max_history, dtype=dt, **kw)
    cn_f, _, _ = T.accumulate(accum, spp, albedo_hits, normal_depth, gspp, camera, fast_hist, max_history=fast_history, dtype=dt, **kw)
    if history is None:
        return cn_l, nd, cn_f, np.zeros(cn_l.shape[:2], dt)
    s = mix_factor(R.luminance(cn_f[..., :3]), R.luminance(cn_l[..., :3]), sigma_response, relative_floor)
    out = cn_l + s[..., None] * (cn_f - cn_l)
    assert out.dtype == dt and cn_f.dtype == dt
    return out, nd, cn_f, s


# ---------------------------------------------------------------- the cases
OFFSET = 1.6  # the largest offset of the fast history's colours, at the right edge of the image


def with_fast_history(case, fast_history=FAST_HISTORY):
    """`case` (temporal_ref.make_case, motion_ref.make_moved_case) with a fast history: the long one's colours plus a smooth offset that rises from
    0 at the left edge to OFFSET at the right one (a quarter of a cosine wave down the image on top, so rows differ), counts capped at
    fast_history.  Small offsets leave s at 0, large ones drive it to 1, and the ramp between holds the fractions."""
    h, w = case["height"], case["width"]
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = OFFSET * (xx + 0.5) / w * (0.85 + 0.15 * np.cos(0.5 * np.pi * (yy + 0.5) / h))
    fast = case["hist_cn"].astype(np.float64)
    fast[..., :3] += ramp[..., None]
    fast[..., 3] = np.minimum(fast[..., 3], fast_history)
    return dict(case, hist_fast=fast.astype(np.float32))


def make_case(pose, width, height, moved=False, **kw):
    base = M.make_moved_case(pose, width, height, turn=True, **kw) if moved else T.make_case(pose, width, height, **kw)
    return with_fast_history(base)


def run_case(case, dtype=np.float64, **params):
    hist = (case["hist_cn"], case["hist_nd"], case["hist_camera"], case["hist_fast"])
    mo = dict(motion=case["motion"], prev_normal=case["prev_normal"]) if "motion" in case else {}
    return accumulate(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], case["camera"], hist, dtype=dtype, **mo, **params)


def bounds(case, **params):
    """(float64 restatement (colour_count, normal_depth, fast, s), the bound of each of colour_count, fast and s) in temporal_ref.bound's form:
    8 x what single precision costs the restatement on this input + 1e-6 x the largest input colour"""
    ref64, ref32 = run_case(case, np.float64, **params), run_case(case, np.float32, **params)
    largest = max(float(case["accum"][..., :3].max() / case["spp"]), float(case["hist_cn"][..., :3].max()), float(case["hist_fast"][..., :3].max()))
    out = []
    for k in (0, 2, 3):
        assert ref32[k].dtype == np.float32 and ref64[k].dtype == np.float64
        out.append(8.0 * float(np.abs(ref32[k].astype(np.float64) - ref64[k]).max()) + 1e-6 * largest)
    return ref64, tuple(out)


def fractions(s):
    """the fractions of pixels with s == 0, 0 < s < 1 and s == 1"""
    return float((s == 0).mean()), float(((s > 0) & (s < 1)).mean()), float((s == 1).mean())


# the cases the device test runs: (name, make_case arguments)
SIZES = T.SIZES + [(5, 3)]
GPU_CASES = [(f"{pose} {w}x{h}", dict(pose=pose, width=w, height=h)) for pose in ("history", "pan", "big", "turn") for (w, h) in SIZES]
GPU_CASES += [("pan 70x45, fireflies", dict(pose="pan", width=70, height=45, firefly=True)),
              ("moved sphere 70x45, motion route", dict(pose="pan", width=70, height=45, moved=True))]
