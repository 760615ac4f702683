"""numpy restatement of the instance motion (include/ptamd.h, "instance motion"): the host's record conversion and the two guide deposits,
parameterised by dtype like temporal_ref, whose accumulate takes the two motion sums -- float64 is the reference the device is held against, float32
measures what single precision costs the same arithmetic on the same input.  Also the synthetic moved-sphere case the motion tests share."""
import contextlib

import numpy as np

import denoise_ref as R
import temporal_ref as T

SHIFT = np.array([0.25, 0.0, 0.1])  # the sphere's move between the history and the current frame
TURN = 0.5  # ... and, optionally, its turn about y (radians)


# ---------------------------------------------------------------- the accumulate: temporal_ref.accumulate with its two motion inputs
def run_case(case, dtype=np.float64, with_motion=True, **params):
    hist = (case["hist_cn"], case["hist_nd"], case["hist_camera"])
    mo = dict(motion=case["motion"], prev_normal=case["prev_normal"]) if with_motion else {}
    return T.accumulate(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], case["camera"], hist, dtype=dtype, **mo, **params)


def bound(case, **params):
    """(float64 restatement colour_count, bound) in temporal_ref.bound's form: 8 x what single precision costs the restatement on this input +
    1e-6 x the largest input colour"""
    ref64 = run_case(case, np.float64, **params)[0]
    ref32 = run_case(case, np.float32, **params)[0]
    assert ref32.dtype == np.float32
    largest = max(float(case["accum"][..., :3].max() / case["spp"]), float(case["hist_cn"][..., :3].max()))
    return ref64, 8.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + 1e-6 * largest


# ---------------------------------------------------------------- the host's record conversion
def _matrix(m16):
    """the 4 x 4 matrix of 16 column-major floats, float64"""
    return np.asarray(m16, np.float32).astype(np.float64).reshape(4, 4).T


def motion_records(prev_inv, cur_inv):
    """(n, 6, 4) float32 from (n, 16) float32 previous and current invTransforms: P = inverse(prev) * cur in float64 (world now -> world then),
    rows (A | t) of P - I rounded to float32 -- exact zeros where prev has cur's bits --, then prev's rows 0..2."""
    prev = np.ascontiguousarray(prev_inv, np.float32).reshape(-1, 16)
    cur = np.ascontiguousarray(cur_inv, np.float32).reshape(-1, 16)
    out = np.zeros((len(prev), 6, 4), np.float32)
    for i, (p, c) in enumerate(zip(prev, cur)):
        out[i, 3:] = p.reshape(4, 4).T[:3]
        if np.array_equal(p.view(np.uint32), c.view(np.uint32)):
            continue
        P = np.linalg.inv(_matrix(p)) @ _matrix(c)
        out[i, :3] = (P - np.eye(4))[:3].astype(np.float32)
    return out


def records_exact(prev_inv, cur_inv):
    """the (A | t) rows in float64, before the rounding: (n, 3, 4)"""
    prev = np.ascontiguousarray(prev_inv, np.float32).reshape(-1, 16)
    cur = np.ascontiguousarray(cur_inv, np.float32).reshape(-1, 16)
    return np.stack([(np.linalg.inv(_matrix(p)) @ _matrix(c) - np.eye(4))[:3] for p, c in zip(prev, cur)])


# ---------------------------------------------------------------- the two guide deposits
def motion_deposits(flat, prev_top_nodes, o, d, hits, dtype=np.float64, thin_lens=False):
    """What ONE guide sample deposits into the two motion sums for rays (o, d) ((n, 3) each) with hit records `hits` (dict t, u, v, prim, inst;
    inst = top-level leaf index) on the state `flat`, whose instances had prev_top_nodes' invTransform before: (motion (n, 4), prev_normal (n, 4))."""
    dt = dtype
    n = len(d)
    O, Draw = np.asarray(o, np.float32).astype(dt), np.asarray(d, np.float32).astype(dt)
    D = Draw / np.sqrt((Draw * Draw).sum(1))[:, None] if thin_lens else Draw
    prim = np.asarray(hits["prim"])
    motion, pn = np.zeros((n, 4), dt), np.zeros((n, 4), dt)
    pn[:, :3] = -D
    extra = dict(n_dot_d=np.full(n, np.nan, dt), normal_unflipped=np.zeros((n, 3), dt), then_unflipped=np.zeros((n, 3), dt))
    k = np.flatnonzero(prim >= 0)
    if k.size == 0:
        return motion, pn, extra
    inst = np.asarray(hits["inst"])[k]
    rec = motion_records(prev_top_nodes["invTransform"][inst], flat.top_nodes["invTransform"][inst]).astype(dt)
    X = O[k] + Draw[k] * np.asarray(hits["t"], np.float32).astype(dt)[k, None]
    motion[k, :3] = np.einsum("kij,kj->ki", rec[:, :3, :3], X) + rec[:, :3, 3]
    idx = flat.triangles[prim[k]]["indices"]
    u, v = np.asarray(hits["u"], dt)[k, None], np.asarray(hits["v"], dt)[k, None]
    vn = flat.vertices["normal"][:, :3].astype(dt)
    n0, n1, n2 = vn[idx[:, 0]], vn[idx[:, 1]], vn[idx[:, 2]]
    sn = R._unit(n0 + (n1 - n0) * u + (n2 - n0) * v)  # object space

    def world(m16):  # normalTransform: (M^T v)_j = sum_i m[4 j + i] v_i
        m = m16.astype(dt).reshape(-1, 4, 4)
        return R._unit(np.einsum("kji,ki->kj", m[:, :3, :3], sn))
    N = world(flat.top_nodes["invTransform"][inst])
    n_dot_d = (N * D[k]).sum(1)
    n_then = world(prev_top_nodes["invTransform"][inst])
    pn[k, :3] = np.where(n_dot_d[:, None] > 0, -n_then, n_then)  # flipped if and only if N is
    extra["n_dot_d"][k], extra["normal_unflipped"][k], extra["then_unflipped"][k] = n_dot_d, N, n_then
    return motion, pn, extra


# ---------------------------------------------------------------- the synthetic moved-sphere case
@contextlib.contextmanager
def sphere_at(centre):
    """temporal_ref.ray_cast with its sphere somewhere else"""
    saved = T.SPHERE_C
    T.SPHERE_C = np.asarray(centre, np.float64)
    try:
        yield
    finally:
        T.SPHERE_C = saved


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def make_moved_case(pose, width, height, turn=False, zero_motion=False, **kw):
    """temporal_ref.make_case(pose, all_counted=True) -- a history with the sphere at SPHERE_C -- whose current frame has the sphere at SPHERE_C + SHIFT,
    optionally turned by TURN about y; `motion` / `prev_normal` sums filled analytically on the sphere's pixels (case["sphere"]), 0 and the current
    normal sums elsewhere.  zero_motion: the sums that make the motion kernel the plain one (0, normal_depth.xyz)."""
    c0, c1 = T.SPHERE_C, T.SPHERE_C + SHIFT
    with sphere_at(c1):
        case = T.make_case(pose, width, height, all_counted=True, **kw)
        _, z = T.ray_cast(case["camera"], width, height)
    if not kw.get("same_guides"):
        hn, hz = T.ray_cast(case["hist_camera"], width, height)  # the history saw the sphere where it was
        case["hist_nd"] = np.concatenate([hn, hz[..., None]], -1).astype(np.float32)
    E, S, u, v = T.camera_vectors(case["camera"], np.float64)
    yy, xx = np.mgrid[0:height, 0:width]
    dirv = S + u * ((xx + 0.5) / width)[..., None] + v * ((yy + 0.5) / height)[..., None] - E
    D = dirv / np.linalg.norm(dirv, axis=-1, keepdims=True)
    X = E + z[..., None] * D
    sphere = (z < R.SKY_DEPTH) & (np.abs(np.linalg.norm(X - c1, axis=-1) - T.SPHERE_R) < 1e-9)
    back = _rot_y(-TURN if turn else 0.0)  # object point p: then at c0 + p, now at c1 + Ry(TURN) p
    rel = X - c1
    x_then = c0 + rel @ back.T
    n_then = (rel / T.SPHERE_R) @ back.T
    gspp = case["gspp"]
    motion = np.zeros((height, width, 4), np.float32)
    prev_normal = np.zeros((height, width, 4), np.float32)
    prev_normal[..., :3] = case["normal_depth"][..., :3]
    if not zero_motion:
        motion[sphere, :3] = ((x_then - X) * gspp)[sphere]
        prev_normal[sphere, :3] = (n_then * gspp)[sphere]
    case.update(motion=motion, prev_normal=prev_normal, sphere=sphere)
    return case
