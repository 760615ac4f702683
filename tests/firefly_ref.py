"""numpy restatement of the firefly clamp (pt_set_firefly_clamp; include/ptamd.h, "firefly clamp"): every pixel's demodulated colour bounded by
scale x (the rank-th largest luminance among its finite 5 x 5 neighbours + 1e-3).  Parameterised by dtype like temporal_ref, on whose cases it is
built: float64 is the reference the device is held against, float32 measures what single precision costs the same arithmetic on the same input.
Also the planted cases the firefly tests share."""
import numpy as np

import denoise_ref as R
import temporal_ref as T

RADIUS, MAX_RANK = 2, 4  # PT_FIREFLY_RADIUS, PT_FIREFLY_MAX_RANK
RANK, SCALE = 1, 8.0  # PT_FIREFLY_DEFAULT_RANK, PT_FIREFLY_DEFAULT_SCALE: chosen by tests/test_firefly_ref.py's scan
FLOOR = 1e-3
BAR = 9.0  # the demodulated colour of the planted bar
R_CPU = 0.71  # mirror_blob_room, 1 spp, the defaults: the filtered on / off ratio pooled over the scan's bases (tests/test_firefly_ref.py measures it)


def demodulated(accum, spp, albedo_hits, gspp, dtype=np.float64):
    """(d (H, W, 3), L (H, W), finite (H, W)) of (H, W, 4) sums: demodulatedMean, its Rec.709 luminance, and whether all four are finite"""
    dt = dtype
    with np.errstate(all="ignore"):
        c = np.asarray(accum).astype(dt)[..., :3] / dt(spp)
        a = np.maximum(np.asarray(albedo_hits).astype(dt)[..., :3] / dt(gspp), dt(R.ALBEDO_FLOOR))
        d = c / a
        lum = R.luminance(d)
    return d, lum, np.isfinite(d).all(-1) & np.isfinite(lum)


def clamp_plane(d, lum, finite, rank=0, scale=0.0):
    """The operator on a demodulated image.  Returns (plane (H, W, 4) = (d_out.rgb, s), cap (H, W), n_q (H, W)) in d's dtype."""
    dt = d.dtype.type
    rank, scale = int(rank or RANK), dt(scale or SCALE)
    assert 1 <= rank <= MAX_RANK
    H, W = lum.shape
    never = dt(-np.inf)
    padded = np.full((H + 2 * RADIUS, W + 2 * RADIUS), never, d.dtype)
    padded[RADIUS:RADIUS + H, RADIUS:RADIUS + W] = np.where(finite, lum, never)  # out-of-image and non-finite entries never count
    taps = [padded[dy:dy + H, dx:dx + W] for dy in range(2 * RADIUS + 1) for dx in range(2 * RADIUS + 1) if (dy, dx) != (RADIUS, RADIUS)]
    ordered = -np.sort(-np.stack(taps, -1), axis=-1)  # descending; ties are ordinary values
    n_q = (ordered > never).sum(-1)
    r = ordered[..., rank - 1]
    with np.errstate(all="ignore"):
        cap = np.where(n_q >= rank, scale * (np.where(n_q >= rank, r, dt(0)) + dt(FLOOR)), dt(np.inf)).astype(d.dtype)
        over = finite & (lum > cap)
        s = np.where(over, cap / np.where(over, lum, dt(1)), dt(1)).astype(d.dtype)
        rgb = np.where(over[..., None], d * s[..., None], d)
    plane = np.concatenate([rgb, s[..., None]], -1)
    plane[~finite] = dt(0)
    assert plane.dtype == d.dtype
    return plane, cap, n_q


def evaluate(accum, spp, albedo_hits, gspp, rank=0, scale=0.0, dtype=np.float64):
    """pt_read_firefly on (H, W, 4) sums: dict(plane, counts=(clamped, nonfinite), cap, lum, finite, n_q, d)"""
    d, lum, finite = demodulated(accum, spp, albedo_hits, gspp, dtype)
    plane, cap, n_q = clamp_plane(d, lum, finite, rank, scale)
    clamped = finite & (lum > cap)
    return dict(plane=plane, counts=(int(clamped.sum()), int((~finite).sum())), cap=cap, lum=lum, finite=finite, n_q=n_q, d=d, clamped=clamped)


def run_case(case, dtype=np.float64, **params):
    return evaluate(case["accum"], case["spp"], case["albedo_hits"], case["gspp"], dtype=dtype, **params)


def bounds(case, ref64=None, **params):
    """(float64 restatement, bound) in temporal_ref.bound's form: 8 x what float32 costs the restatement on this input + 1e-6 x the largest value
    of the float64 OUTPUT plane; absolute, for rgb and s alike"""
    ref64 = run_case(case, np.float64, **params) if ref64 is None else ref64
    ref32 = run_case(case, np.float32, **params)
    assert ref32["plane"].dtype == np.float32 and ref64["plane"].dtype == np.float64
    return ref64, 8.0 * float(np.abs(ref32["plane"].astype(np.float64) - ref64["plane"]).max()) + 1e-6 * float(ref64["plane"].max())


def near(case, ref64=None, **params):
    """flat indices of the finite pixels whose L lies within 1e-4 relative of Cap: where float32 may count a clamp the float64 restatement does not"""
    ref64 = run_case(case, np.float64, **params) if ref64 is None else ref64
    with np.errstate(all="ignore"):
        close = ref64["finite"] & np.isfinite(ref64["cap"]) & (np.abs(ref64["lum"] - ref64["cap"]) <= 1e-4 * ref64["cap"])
    return np.flatnonzero(close)


def accumulate_case(case, dtype=np.float64, clamp=True, history=True, rank=0, scale=0.0, **params):
    """pt_temporal_accumulate with the mode on: temporal_ref.accumulate fed the restated plane (an accumulator of d_out over an albedo of 1, one
    sample each: demodulatedMean of it is d_out's own bits)"""
    if not clamp:
        return T.run_case(case, dtype, history=history, **params)
    plane = run_case(case, dtype, rank=rank, scale=scale)["plane"]
    fed = np.concatenate([plane[..., :3], np.zeros_like(plane[..., :1])], -1)
    ones = np.full(np.asarray(case["albedo_hits"]).shape, case["gspp"], dtype)  # (an albedo of exactly 1)
    hist = (case["hist_cn"], case["hist_nd"], case["hist_camera"]) if history else None
    return T.accumulate(fed, 1, ones, case["normal_depth"], case["gspp"], case["camera"], hist, dtype=dtype, **params)


def temporal_bound(case, **params):
    """(float64 restatement colour_count of accumulate_case, bound) in temporal_ref.bound's form, the largest input colour being the restated plane's"""
    ref64, ref32 = accumulate_case(case, np.float64, **params)[0], accumulate_case(case, np.float32, **params)[0]
    assert ref32.dtype == np.float32
    plane = run_case(case, np.float64, rank=params.get("rank", 0), scale=params.get("scale", 0.0))["plane"]
    largest = max(float(plane[..., :3].max()), float(case["hist_cn"][..., :3].max()))
    return ref64, 8.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + 1e-6 * largest


def filtered(case, iterations, dtype=np.float64, **params):
    """pt_denoise (HDR, accumulator input, iterations > 0) with the mode on: the restated plane through denoise_ref's filter, times the albedo"""
    plane = run_case(case, dtype, **params)["plane"]
    with np.errstate(all="ignore"):
        _, a, n, z = R.prepare(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], dtype)
    return R.atrous(plane[..., :3], n, z, iterations) * a


def filter_bound(case, iterations, **params):
    """(float64 restatement, bound) in the form of tests/test_gpu_denoise.py's hdr_bound, the largest input being the re-modulated restated plane's"""
    ref64, ref32 = filtered(case, iterations, np.float64, **params), filtered(case, iterations, np.float32, **params)
    assert ref32.dtype == np.float32
    with np.errstate(all="ignore"):
        a = R.prepare(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"])[1]
    largest = float((run_case(case, np.float64, **params)["plane"][..., :3] * a).max())
    return ref64, 8.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + 1e-6 * largest


# ---------------------------------------------------------------- the cases
SIZES = T.SIZES + [(5, 3), (2, 1), (1, 1)]
SMALL = [(5, 3), (2, 1), (1, 1)]
PARAMS = [dict(), dict(rank=3, scale=2.0)]  # the defaults, and a pair under which enough pixels clamp


def plant(case):
    """`case` (temporal_ref.make_case) with, where the image has room for them: two adjacent 1e4 spikes; a spike in a corner and one on an edge; a NaN
    pixel beside a spike and an Inf pixel; a bar 3 pixels wide at 10 x its surround; a block of exact zeros.  Returns the case with `planted`, the
    (y, x) of each."""
    h, w = case["height"], case["width"]
    accum = case["accum"].copy()
    spp = case["spp"]
    spike = np.array([1e4, 0.5e4, 0.2e4])  # in d: the accumulator holds it times the pixel's albedo
    planted = {}

    def put(name, y, x, value):
        if 0 <= y < h and 0 <= x < w:
            accum[y, x, :3] = value * np.maximum(case["albedo_hits"][y, x, :3] / case["gspp"], R.ALBEDO_FLOOR) * spp
            planted.setdefault(name, []).append((y, x))
    put("corner", 0, 0, spike)
    if w >= 16 and h >= 16:
        put("pair", h // 3, w // 2, spike), put("pair", h // 3, w // 2 + 1, spike)
        put("edge", h // 2, w - 1, spike)
        put("nan", h // 3 + 1, w // 2, np.nan)  # beside the pair
        put("inf", h - 2, 1, np.inf)
        for y in range(2, 12):  # the bar: 3 wide, d = 9 in every component -- 10 x the mean of the gamma(0.6, 1.5) colours around it
            for x in (4, 5, 6):
                accum[y, x, :3] = BAR * np.maximum(case["albedo_hits"][y, x, :3] / case["gspp"], R.ALBEDO_FLOOR) * spp
                planted.setdefault("bar", []).append((y, x))
        accum[h - 6:h - 2, w - 9:w - 4, :3] = 0.0
        planted["zeros"] = [(y, x) for y in range(h - 6, h - 2) for x in range(w - 9, w - 4)]
    elif w >= 5 and h >= 3:
        put("nan", 1, 3, np.nan)
    return dict(case, accum=accum, planted=planted)


def make_case(width, height, pose="pan", seed=11):
    return plant(T.make_case(pose, width, height, seed=seed))


def make_smooth_case(width, height, pose="pan"):
    """nothing clamps: a smooth ramp of colour over a constant albedo"""
    case = T.make_case(pose, width, height)
    yy, xx = np.mgrid[0:height, 0:width]
    accum = np.zeros((height, width, 4), np.float32)
    for k in range(3):
        accum[..., k] = (0.2 + 0.1 * k + 0.5 * (xx + 0.5) / width + 0.3 * (yy + 0.5) / height) * case["spp"]
    ah = np.zeros((height, width, 4), np.float32)
    ah[..., :3] = 0.5 * case["gspp"]
    ah[..., 3] = case["gspp"]
    return dict(case, accum=accum, albedo_hits=ah, planted={})


CASES = [(f"{w}x{h}" + (", rank 3 scale 2" if prm else ""), dict(width=w, height=h), prm) for (w, h) in SIZES for prm in PARAMS]
