"""numpy restatement of pt_temporal_accumulate (include/ptamd.h, "temporal history"), parameterised by dtype like denoise_ref: float64 is the
reference the device is held against, float32 measures what single precision costs the same arithmetic on the same input -- independently
of the code under test.  Also the synthetic scene the temporal tests share: an analytic ray-cast that gives consistent (n, z) for any camera."""
import numpy as np

import denoise_ref as R
from ptamd import layout as L, scenes

MAX_HISTORY = 32
SPP, GSPP = 1, 1
SIZES = [(16, 16), (70, 45), (150, 83)]


# ---------------------------------------------------------------- the restatement
def camera_vectors(camera, dt):
    """(E, S, u, v) of a pt_camera record as 3-vectors of dtype dt"""
    cam = np.asarray(camera, L.CAMERA).reshape(1)[0]
    return tuple(np.asarray(cam[k], np.float32)[:3].astype(dt) for k in ("eyePoint", "screenPoint", "u", "v"))


def _dot(a, b):
    return (a * b).sum(-1)


def accumulate(accum, spp, albedo_hits, normal_depth, gspp, camera, history=None, max_history=MAX_HISTORY, k_normal=0.0, sigma_depth=0.0,
               dtype=np.float64, motion=None, prev_normal=None, variance=False):
    """One pt_temporal_accumulate.  accum, albedo_hits, normal_depth: (H, W, 4) sums; history: None or (colour_count (H, W, 4),
    normal_depth (H, W, 4), camera it was made under).  Returns (colour_count, normal_depth, Wsum), all of `dtype`.
    motion, prev_normal (include/ptamd.h, "instance motion"): the two (H, W, 4) motion sums -- q = (X + m / gspp) - E', and the taps' normal term
    compares with n_then, the prev_normal sum normalised by denoise_ref.prepare's own normalisation.
    variance (pt_set_temporal_variance): the history carries a fourth element, its variance plane (H, W), and the third result is the new plane
        v_out = (1 - alpha) (v_h + alpha (l - mu)^2),  alpha = 1 / N_out,  l = L(d),  mu = L(h),  v_h = sum w v_tap / Wsum
    over the colour's own taps and weights, 0 where the pixel found no history."""
    dt = dtype
    k_normal, sigma_depth = dt(k_normal or R.K_NORMAL), dt(sigma_depth or R.SIGMA_DEPTH)
    d, _, n, z = R.prepare(accum, spp, albedo_hits, normal_depth, gspp, dt)
    H, W = z.shape
    out_nd = np.concatenate([n, z[..., None]], -1)
    if history is None:
        return np.concatenate([d, np.ones((H, W, 1), dt)], -1), out_nd, np.zeros((H, W), dt)
    hist_cn, hist_nd, hist_camera = history[:3]
    hist_cn, hist_nd = np.asarray(hist_cn).astype(dt).reshape(H, W, 4), np.asarray(hist_nd).astype(dt).reshape(H, W, 4)
    hist_v = np.asarray(history[3]).astype(dt).reshape(H, W) if variance else np.zeros((H, W), dt)
    n_then = n  # what the history's normals are compared with
    if motion is not None:
        m = np.asarray(motion).astype(dt).reshape(H, W, 4)[..., :3] / dt(gspp)
        n_then = R.prepare(accum, spp, albedo_hits, np.asarray(prev_normal).reshape(H, W, 4), gspp, dt)[2]
    E, S, u, v = camera_vectors(camera, dt)
    Eh, Sh, uh, vh = camera_vectors(hist_camera, dt)
    yy, xx = np.mgrid[0:H, 0:W]
    px = ((xx.astype(dt) + dt(0.5)) / dt(W))[..., None]
    py = ((yy.astype(dt) + dt(0.5)) / dt(H))[..., None]
    with np.errstate(all="ignore"):
        dirv = S + u * px + v * py - E
        D = dirv / np.sqrt(_dot(dirv, dirv))[..., None]
        X = E + z[..., None] * D
        if motion is not None:
            X = X + m  # where the surface was
        q = X - Eh
        s0 = Sh - Eh
        uxv = np.cross(uh, vh)
        det = _dot(s0, uxv)
        lam = _dot(q, uxv) / det
        alpha = _dot(s0, np.cross(q, vh)) / det
        beta = _dot(s0, np.cross(uh, q)) / det
        front = lam > 0
        lam = np.where(front, lam, dt(1))
        fx = np.clip(dt(W) * alpha / lam - dt(0.5), dt(-2), dt(W + 1))
        fy = np.clip(dt(H) * beta / lam - dt(0.5), dt(-2), dt(H + 1))
        zq = np.sqrt(_dot(q, q))
        flx, fly = np.floor(fx), np.floor(fy)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        ax, ay = fx - flx, fy - fly
        sd, sn, sv, sw = np.zeros((H, W, 3), dt), np.zeros((H, W), dt), np.zeros((H, W), dt), np.zeros((H, W), dt)
        for j in (0, 1):
            for i in (0, 1):
                tx, ty = x0 + i, y0 + j
                inside = front & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                cy, cx = np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)
                ch, gh = hist_cn[cy, cx], hist_nd[cy, cx]
                counts = inside & (ch[..., 3] > 0)
                b = (ax if i else dt(1) - ax) * (ay if j else dt(1) - ay)
                e_n = k_normal * np.maximum(dt(0), dt(1) - _dot(n_then, gh[..., :3]))
                e_z = np.abs(zq - gh[..., 3]) / (sigma_depth * (np.minimum(zq, gh[..., 3]) + dt(1e-6)))
                w = np.where(counts, b * np.exp(-(e_n + e_z)), dt(0)).astype(dt)
                sd += w[..., None] * ch[..., :3]
                sn += w * ch[..., 3]
                sv += w * hist_v[cy, cx]
                sw += w
        use = sw >= dt(1e-12)
        safe = np.where(use, sw, dt(1))
        h = sd / safe[..., None]
        N = np.minimum(sn + dt(1), dt(max_history))
        d_out = np.where(use[..., None], h + (d - h) / N[..., None], d)
        N_out = np.where(use, N, dt(1))
        a, delta = dt(1) / N_out, R.luminance(d) - R.luminance(h)
        v_out = np.where(use, (dt(1) - a) * (sv / safe + a * delta * delta), dt(0))
    out = np.concatenate([d_out, N_out[..., None]], -1)
    assert out.dtype == dt and out_nd.dtype == dt and v_out.dtype == dt
    return out, out_nd, (v_out if variance else sw)


# ---------------------------------------------------------------- the synthetic scene
SPHERE_C, SPHERE_R = np.array([0.3, 0.5, 1.5]), 0.5


def ray_cast(camera, width, height):
    """(n (H, W, 3), z (H, W)) in float64 of the first hit through every pixel centre: a floor y = 0 for |x| < 4, a back wall z = 3 below
    y = 2.2, a sphere of radius 0.5 at (0.3, 0.5, 1.5), sky elsewhere (n = -D, z = 1e6)."""
    E, S, u, v = camera_vectors(camera, np.float64)
    yy, xx = np.mgrid[0:height, 0:width]
    dirv = S + u * ((xx + 0.5) / width)[..., None] + v * ((yy + 0.5) / height)[..., None] - E
    D = dirv / np.linalg.norm(dirv, axis=-1, keepdims=True)
    n = -D.copy()
    z = np.full((height, width), R.SKY_DEPTH)
    with np.errstate(all="ignore"):
        t = -E[1] / D[..., 1]  # floor
        hit = (D[..., 1] < 0) & (t > 0) & (np.abs(E[0] + t * D[..., 0]) < 4.0) & (t < z)
        z = np.where(hit, t, z)
        n = np.where(hit[..., None], np.array([0.0, 1.0, 0.0]), n)
        t = (3.0 - E[2]) / D[..., 2]  # back wall
        hit = (D[..., 2] > 0) & (t > 0) & (E[1] + t * D[..., 1] < 2.2) & (t < z)
        z = np.where(hit, t, z)
        n = np.where(hit[..., None], np.array([0.0, 0.0, -1.0]), n)
        oc = E - SPHERE_C  # sphere
        bq = (oc * D).sum(-1)
        disc = bq * bq - ((oc * oc).sum() - SPHERE_R ** 2)
        t = -bq - np.sqrt(np.maximum(disc, 0.0))
        hit = (disc > 0) & (t > 0) & (t < z)
        z = np.where(hit, t, z)
        n = np.where(hit[..., None], (E + t[..., None] * D - SPHERE_C) / SPHERE_R, n)
    return n, z


HISTORY_EYE, HISTORY_TARGET = (0.0, 1.0, -3.9), (0.0, 1.0, 0.0)
POSES = {"history": (HISTORY_EYE, HISTORY_TARGET),
         "pan": ((0.15, 1.05, -3.8), (0.1, 0.9, 0.0)),
         "pan2": ((0.3, 1.1, -3.7), (0.2, 0.8, 0.0)),  # a second small step beyond "pan" (the chained test)
         "big": ((1.5, 1.4, -3.0), (0.0, 0.6, 0.0)),
         "turn": (HISTORY_EYE, (3.0, 1.0, -3.9))}


def camera(pose, width, height):
    eye, target = POSES[pose]
    return scenes._camera(width, height, eye, target, 40.0)


def guide_sums(camera_, width, height, gspp=GSPP):
    """normal_depth sums (H, W, 4) float32 of the ray-cast under `camera_`, and the sky mask"""
    n, z = ray_cast(camera_, width, height)
    nd = np.zeros((height, width, 4), np.float32)
    nd[..., :3] = n * gspp
    nd[..., 3] = z * gspp
    return nd, z >= R.SKY_DEPTH


def make_case(pose, width, height, seed=11, firefly=False, all_counted=False, same_guides=False, spp=SPP, gspp=GSPP):
    """Inputs of one accumulate as the device holds them (float32): the current frame under POSES[pose] (accum, albedo_hits, normal_depth,
    camera) and a history made under the history camera (colour_count, normal_depth, camera).  all_counted: every history count >= 1;
    same_guides: the history's guides are the current frame's own (n, z) (for pose "history": the static camera)."""
    rng = np.random.default_rng(seed)
    cam, hcam = camera(pose, width, height), camera("history", width, height)
    nd, sky = guide_sums(cam, width, height, gspp)
    albedo = 0.1 + 0.8 * rng.uniform(size=(height, width, 3))
    yy, xx = np.mgrid[0:height, 0:width]
    albedo[(xx + 2 * yy) % 11 == 0, 1] = 4e-4  # below the floor of the demodulation
    albedo[sky] = 1.0
    colour = albedo * rng.gamma(0.6, 1.5, (height, width, 3))
    accum = np.zeros((height, width, 4), np.float32)
    accum[..., :3] = colour * spp
    ah = np.zeros((height, width, 4), np.float32)
    ah[..., :3] = albedo * gspp
    ah[..., 3] = np.where(sky, 0, gspp)
    hist_cn = np.zeros((height, width, 4), np.float32)
    hist_cn[..., :3] = rng.gamma(0.6, 1.5, (height, width, 3))
    counts = np.floor(rng.uniform(0, 40, (height, width)))
    counts[rng.uniform(size=(height, width)) < 0.1] = 0
    if all_counted:
        counts = np.maximum(counts, 1)
    hist_cn[..., 3] = counts
    if firefly:
        accum[height // 3, width // 2, :3] = (1e4 * spp, 0.5e4 * spp, 0.2e4 * spp)
        hist_cn[height // 2, width // 3, :3] = (0.3e4, 1e4, 0.6e4)
        hist_cn[height // 2, width // 3, 3] = max(hist_cn[height // 2, width // 3, 3], 3)
    if same_guides:
        _, _, n, z = R.prepare(accum, spp, ah, nd, gspp, np.float32)
        hist_nd = np.concatenate([n, z[..., None]], -1).astype(np.float32)
    else:
        hn, hz = ray_cast(hcam, width, height)
        hist_nd = np.concatenate([hn, hz[..., None]], -1).astype(np.float32)
    return dict(accum=accum, albedo_hits=ah, normal_depth=nd, camera=cam, spp=spp, gspp=gspp, hist_cn=hist_cn, hist_nd=hist_nd, hist_camera=hcam,
                width=width, height=height)


def run_case(case, dtype=np.float64, history=True, **params):
    hist = (case["hist_cn"], case["hist_nd"], case["hist_camera"]) if history else None
    return accumulate(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], case["camera"], hist, dtype=dtype, **params)


def bound(case, ref64=None, **params):
    """(float64 restatement colour_count, bound): 8 x what single precision costs the restatement on this input + 1e-6 x the largest input
    colour -- the form of tests/test_gpu_denoise.py's hdr_bound; absolute, for the rgb part and for N alike"""
    ref64 = run_case(case, np.float64, **params)[0] if ref64 is None else ref64
    ref32 = run_case(case, np.float32, **params)[0]
    assert ref32.dtype == np.float32
    largest = max(float(case["accum"][..., :3].max() / case["spp"]), float(case["hist_cn"][..., :3].max()))
    return ref64, 8.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + 1e-6 * largest
