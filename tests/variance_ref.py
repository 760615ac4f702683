"""numpy restatement of the temporal luminance variance (pt_set_temporal_variance; include/ptamd.h, "temporal variance"): the plane that
pt_temporal_accumulate keeps beside the history, and the variance-guided a-trous filter of PT_DENOISE_INPUT_TEMPORAL_VARIANCE.  Parameterised by
dtype like temporal_ref and denoise_ref, on which it is built: float64 is the reference the device is held against, float32 measures what single
precision costs the same arithmetic on the same input."""
import numpy as np

import denoise_ref as R
import motion_ref as M
import temporal_ref as T

# the defaults of include/ptamd.h (pt_variance_params)
SIGMA_VARIANCE, RELATIVE_FLOOR, FULL_HISTORY = 2.0, 0.1, 16.0
BINOMIAL = (0.25, 0.5, 0.25)


# ---------------------------------------------------------------- temporal side
def _unit_sum(nsum, dt):
    """denoise_ref.prepare's normalisation of a normal sum (zero stays zero)"""
    ln = np.sqrt((nsum * nsum).sum(-1, keepdims=True))
    return np.where(ln > 0, nsum / np.where(ln > 0, ln, dt(1)), dt(0))


def _history_taps(normal_depth, gspp, camera, hist_cn, hist_nd, hist_camera, motion, prev_normal, k_normal, sigma_depth, dt):
    """The (up to) four taps temporal_ref.accumulate (motion_ref.accumulate, where the two motion sums are given) meets the history at, with its
    weights: a list of (ty, tx, w), ty / tx clipped into the image and w == 0 where the tap does not count."""
    k_normal, sigma_depth = dt(k_normal or R.K_NORMAL), dt(sigma_depth or R.SIGMA_DEPTH)
    nd = np.asarray(normal_depth).astype(dt)
    z = nd[..., 3] / dt(gspp)
    H, W = z.shape
    n = _unit_sum(nd[..., :3] if motion is None else np.asarray(prev_normal).astype(dt).reshape(H, W, 4)[..., :3], dt)
    m = dt(0) if motion is None else np.asarray(motion).astype(dt).reshape(H, W, 4)[..., :3] / dt(gspp)
    E, S, u, v = T.camera_vectors(camera, dt)
    Eh, Sh, uh, vh = T.camera_vectors(hist_camera, dt)
    yy, xx = np.mgrid[0:H, 0:W]
    px = ((xx.astype(dt) + dt(0.5)) / dt(W))[..., None]
    py = ((yy.astype(dt) + dt(0.5)) / dt(H))[..., None]
    taps = []
    with np.errstate(all="ignore"):
        dirv = S + u * px + v * py - E
        D = dirv / np.sqrt(T._dot(dirv, dirv))[..., None]
        q = (E + z[..., None] * D + m) - Eh
        s0 = Sh - Eh
        uxv = np.cross(uh, vh)
        det = T._dot(s0, uxv)
        lam = T._dot(q, uxv) / det
        alpha = T._dot(s0, np.cross(q, vh)) / det
        beta = T._dot(s0, np.cross(uh, q)) / det
        front = lam > 0
        lam = np.where(front, lam, dt(1))
        fx = np.clip(dt(W) * alpha / lam - dt(0.5), dt(-2), dt(W + 1))
        fy = np.clip(dt(H) * beta / lam - dt(0.5), dt(-2), dt(H + 1))
        zq = np.sqrt(T._dot(q, q))
        flx, fly = np.floor(fx), np.floor(fy)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        ax, ay = fx - flx, fy - fly
        for j in (0, 1):
            for i in (0, 1):
                tx, ty = x0 + i, y0 + j
                inside = front & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                cy, cx = np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)
                ch, gh = hist_cn[cy, cx], hist_nd[cy, cx]
                counts = inside & (ch[..., 3] > 0)
                b = (ax if i else dt(1) - ax) * (ay if j else dt(1) - ay)
                e_n = k_normal * np.maximum(dt(0), dt(1) - T._dot(n, gh[..., :3]))
                e_z = np.abs(zq - gh[..., 3]) / (sigma_depth * (np.minimum(zq, gh[..., 3]) + dt(1e-6)))
                taps.append((cy, cx, np.where(counts, b * np.exp(-(e_n + e_z)), dt(0)).astype(dt)))
    return taps


def accumulate(accum, spp, albedo_hits, normal_depth, gspp, camera, history=None, motion=None, prev_normal=None, max_history=T.MAX_HISTORY,
               k_normal=0.0, sigma_depth=0.0, dtype=np.float64):
    """One pt_temporal_accumulate with the variance mode on.  history: None or (colour_count, normal_depth, camera, variance (H, W)); motion,
    prev_normal: the two (H, W, 4) motion sums, or None.  Returns (colour_count, normal_depth, variance): the first two are temporal_ref.accumulate's
    (motion_ref.accumulate's), the third
        v_out = (1 - alpha) (v_h + alpha (l - mu)^2),  alpha = 1 / N_out,  l = L(d),  mu = L(h),  v_h = sum w v_tap / Wsum
    over the colour's own taps and weights, and 0 where the pixel found no history."""
    dt = dtype
    plain = None if history is None else history[:3]
    if motion is None:
        out, out_nd, _ = T.accumulate(accum, spp, albedo_hits, normal_depth, gspp, camera, plain, max_history, k_normal, sigma_depth, dt)
    else:
        out, out_nd, _ = M.accumulate(accum, spp, albedo_hits, normal_depth, gspp, camera, plain, motion, prev_normal, max_history, k_normal, sigma_depth, dt)
    H, W = out.shape[:2]
    if history is None:
        return out, out_nd, np.zeros((H, W), dt)
    hist_cn, hist_nd = (np.asarray(x).astype(dt).reshape(H, W, 4) for x in history[:2])
    hist_v = np.asarray(history[3]).astype(dt).reshape(H, W)
    d = R.prepare(accum, spp, albedo_hits, normal_depth, gspp, dt)[0]
    sd, sv, sw = np.zeros((H, W, 3), dt), np.zeros((H, W), dt), np.zeros((H, W), dt)
    for cy, cx, w in _history_taps(normal_depth, gspp, camera, hist_cn, hist_nd, history[2], motion, prev_normal, k_normal, sigma_depth, dt):
        sd += w[..., None] * hist_cn[cy, cx, :3]
        sv += w * hist_v[cy, cx]
        sw += w
    use = sw >= dt(1e-12)
    safe = np.where(use, sw, dt(1))
    mu, v_h = R.luminance(sd / safe[..., None]), sv / safe
    alpha = dt(1) / out[..., 3]
    delta = R.luminance(d) - mu
    v_out = np.where(use, (dt(1) - alpha) * (v_h + alpha * delta * delta), dt(0))
    assert v_out.dtype == dt
    return out, out_nd, v_out


# ---------------------------------------------------------------- filter side
def history_weight(count, full_history=0.0):
    """s(p) = min((N - 1) / (full_history - 1), 1), and 0 below N = 1 (a count pt_temporal_accumulate never writes)"""
    dt = count.dtype.type
    return np.clip((count - dt(1)) / (dt(full_history or FULL_HISTORY) - dt(1)), dt(0), dt(1))


def initial_variance(variance, count):
    """V_0 = v / N, the variance of the history's MEAN (N below 1 taken as 1)"""
    return variance / np.maximum(count, count.dtype.type(1))


def _neighbourhood(V):
    """g^2: the 3 x 3 binomial mean of V over the neighbours at distance 1 inside the image"""
    dt = V.dtype.type
    H, W = V.shape
    num, den = np.zeros_like(V), np.zeros_like(V)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if abs(dy) >= H or abs(dx) >= W:
                continue
            p = (slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
            q = (slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx)))
            k = dt(BINOMIAL[dy + 1]) * dt(BINOMIAL[dx + 1])
            num[p] += k * V[q]
            den[p] += k
    return num / den


def atrous(d, V, count, n, z, iterations, k_normal=0.0, sigma_depth=0.0, sigma_lum=0.0, sigma_variance=0.0, relative_floor=0.0, full_history=0.0):
    """denoise_ref.atrous with the luminance term moved from the relative one to the variance one as the history grows; V (H, W) is V_0,
    count (H, W) the history's N.  Returns (d (H, W, 3), V (H, W)) after `iterations` passes."""
    k_normal, sigma_depth, sigma_lum = k_normal or R.K_NORMAL, sigma_depth or R.SIGMA_DEPTH, sigma_lum or R.SIGMA_LUM
    dt = d.dtype.type
    sigma_variance, relative_floor = dt(sigma_variance or SIGMA_VARIANCE), dt(relative_floor or RELATIVE_FLOOR)
    s = history_weight(count.astype(d.dtype), full_history)
    H, W = z.shape
    for i in range(iterations):
        step = 2 ** i
        lum = R.luminance(d)
        g = np.sqrt(_neighbourhood(V))
        num, num_v, den = np.zeros_like(d), np.zeros_like(z), np.zeros_like(z)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                if abs(oy) >= H or abs(ox) >= W:
                    continue
                p = (slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox)))
                q = (slice(max(0, oy), H - max(0, -oy)), slice(max(0, ox), W - max(0, -ox)))
                e_n = dt(k_normal) * np.maximum(dt(0), dt(1) - (n[p] * n[q]).sum(-1))
                e_z = np.abs(z[p] - z[q]) / (dt(sigma_depth) * (np.minimum(z[p], z[q]) + dt(1e-6)))
                diff, top = np.abs(lum[p] - lum[q]), np.maximum(lum[p], lum[q]) + dt(1e-3)
                e_plain = diff / (dt(sigma_lum) * dt(2.0 ** -i) * top)
                e_var = diff / (sigma_variance * g[p] + relative_floor * top)
                e_l = s[p] * e_var + (dt(1) - s[p]) * e_plain
                w = dt(R.KERNEL[dy + 2]) * dt(R.KERNEL[dx + 2]) * np.exp(-(e_n + e_z + e_l))
                num[p] += w[..., None] * d[q]
                num_v[p] += w * w * V[q]
                den[p] += w
        d, V = num / den[..., None], num_v / (den * den)
    return d, V


def denoise_hdr(hist_cn, variance, albedo_hits, normal_depth, gspp, iterations, dtype=np.float64, **params):
    """the PT_DENOISE_HDR output (H, W, 3) of PT_DENOISE_INPUT_TEMPORAL_VARIANCE: the history's d filtered under the current guides, times the
    current albedo"""
    dt = dtype
    hist_cn, variance = np.asarray(hist_cn).astype(dt), np.asarray(variance).astype(dt)
    H, W = variance.shape
    _, a, n, z = R.prepare(np.zeros((H, W, 4), dt), 1, albedo_hits, normal_depth, gspp, dt)
    d, count = hist_cn[..., :3], hist_cn[..., 3]
    if iterations == 0:
        return d * a
    return atrous(d, initial_variance(variance, count), count, n, z, iterations, **params)[0] * a
