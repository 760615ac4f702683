"""numpy restatement of the first-hit guide deposits and of the edge-avoiding a-trous filter (include/ptamd.h, "guides and denoiser"),
parameterised by dtype: float64 is the reference the device is held against, float32 measures what single precision costs the same
arithmetic on the same input -- independently of the code under test."""
import numpy as np

from ptamd import layout as L

SKY_DEPTH = 1e6
ALBEDO_FLOOR = 1e-3
KERNEL = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
# the defaults of include/ptamd.h (PT_DENOISE_DEFAULT_*)
K_NORMAL, SIGMA_DEPTH, SIGMA_LUM = 64.0, 0.05, 0.7
# ... and of pt_variance_params
SIGMA_VARIANCE, RELATIVE_FLOOR, FULL_HISTORY = 2.0, 0.1, 16.0
BINOMIAL = (0.25, 0.5, 0.25)


# ---------------------------------------------------------------- guide deposits
def _sample_linear_repeat(tex, s, t, layer, dt):
    """NORMALIZED_COORDS | ADDRESS_REPEAT | FILTER_LINEAR on tex[layers][h][w][4] (csrc/pt_shade.h, sampleLinearRepeat)"""
    tex = np.asarray(tex)
    if tex.dtype == np.uint8:  # B, G, R, A bytes
        tex = tex[..., [2, 1, 0, 3]].astype(dt) / dt(255)
    tex = tex.astype(dt)
    layers, h, w, _ = tex.shape
    s, t = s.astype(dt), t.astype(dt)
    u = (s - np.floor(s)) * dt(w)
    v = (t - np.floor(t)) * dt(h)
    i0 = np.floor(u - dt(0.5)).astype(np.int64)
    j0 = np.floor(v - dt(0.5)).astype(np.int64)
    i1, j1 = i0 + 1, j0 + 1
    i0 = np.where(i0 < 0, i0 + w, i0)
    i1 = np.where(i1 > w - 1, i1 - w, i1)
    j0 = np.where(j0 < 0, j0 + h, j0)
    j1 = np.where(j1 > h - 1, j1 - h, j1)
    a = ((u - dt(0.5)) - np.floor(u - dt(0.5)))[:, None]
    b = ((v - dt(0.5)) - np.floor(v - dt(0.5)))[:, None]
    layer = np.clip(np.rint(layer).astype(np.int64), 0, layers - 1)
    return ((1 - a) * (1 - b) * tex[layer, j0, i0] + a * (1 - b) * tex[layer, j0, i1]
            + (1 - a) * b * tex[layer, j1, i0] + a * b * tex[layer, j1, i1])


def _unit(v):
    return v / np.sqrt((v * v).sum(1, keepdims=True))


def guide_deposits(flat, d, hits, material_textures=None, dtype=np.float64, thin_lens=False):
    """What ONE guide sample deposits for rays of direction `d` ((n, 3)) with hit records `hits` (dict t, u, v, prim, inst; inst = top-level
    leaf index): (albedo_hits (n, 4), normal_depth (n, 4))."""
    dt = dtype
    n = len(d)
    D = np.asarray(d, dt)
    scale = np.ones(n, dt)
    if thin_lens:
        scale = np.sqrt((D * D).sum(1))
        D = D / scale[:, None]
    prim = np.asarray(hits["prim"])
    hit = prim >= 0
    ah = np.ones((n, 4), dt)
    ah[:, 3] = 0
    nd = np.empty((n, 4), dt)
    nd[:, :3] = -D
    nd[:, 3] = SKY_DEPTH
    k = np.flatnonzero(hit)
    if k.size == 0:
        return ah, nd
    tri = flat.triangles[prim[k]]
    idx = tri["indices"]
    u, v = np.asarray(hits["u"], dt)[k, None], np.asarray(hits["v"], dt)[k, None]
    vn = flat.vertices["normal"][:, :3].astype(dt)
    n0, n1, n2 = vn[idx[:, 0]], vn[idx[:, 1]], vn[idx[:, 2]]
    sn = _unit(n0 + (n1 - n0) * u + (n2 - n0) * v)  # object space
    # normalTransform (math.cl:22-29): (M^T v)_j = sum_i m[4 j + i] v_i, m = the column-major inverse world matrix of the instance
    m = flat.top_nodes["invTransform"][np.asarray(hits["inst"])[k]].astype(dt).reshape(-1, 4, 4)
    N = _unit(np.einsum("kji,ki->kj", m[:, :3, :3], sn))
    N = np.where((N * D[k]).sum(1, keepdims=True) > 0, -N, N)
    mat = flat.materials[tri["materialIndex"]]
    albedo = np.ones((k.size, 3), dt)
    plain = (mat["type"] == L.MAT_PBR) | (mat["type"] == L.MAT_DIFFUSE)
    albedo[plain] = mat["colour"][plain, :3].astype(dt)
    textured = (mat["type"] == L.MAT_DIFFUSE) & (mat["textureId"] != -1)
    if textured.any():
        if material_textures is None:
            albedo[textured] = 1.0  # (opaque white: what the fetch returns without a texture array)
        else:
            tc = flat.vertices["texCoord"].astype(dt)
            t0, t1, t2 = tc[idx[:, 0]], tc[idx[:, 1]], tc[idx[:, 2]]
            uv = (t0 + (t1 - t0) * u + (t2 - t0) * v)[textured]
            c = _sample_linear_repeat(material_textures, uv[:, 0], uv[:, 1], mat["textureId"][textured].astype(dt), dt)
            albedo[textured] = np.where(c[:, 3:4] == 0, 1.0, c[:, :3])
    ah[k, :3] = albedo
    ah[k, 3] = 1
    nd[k, :3] = N
    nd[k, 3] = np.asarray(hits["t"], dt)[k] * scale[k]
    return ah, nd


# ---------------------------------------------------------------- filter
def luminance(rgb):
    dt = rgb.dtype.type
    return dt(0.2126) * rgb[..., 0] + dt(0.7152) * rgb[..., 1] + dt(0.0722) * rgb[..., 2]


def tap_weight(n_p, n_q, z_p, z_q, l_p, l_q, i, k_normal, sigma_depth, sigma_lum, guided=None):
    """w_i(p, q) = exp(-(e_n + e_z + e_l)) of iteration i; arrays of one dtype, which the arithmetic stays in.  guided: None, or
    (s_p, sigma_variance g_p, relative_floor) of the variance-guided filter: e_l = s e_var + (1 - s) e_plain"""
    dt = z_p.dtype.type
    e_n = dt(k_normal) * np.maximum(dt(0), dt(1) - (n_p * n_q).sum(-1))
    e_z = np.abs(z_p - z_q) / (dt(sigma_depth) * (np.minimum(z_p, z_q) + dt(1e-6)))
    diff, top = np.abs(l_p - l_q), np.maximum(l_p, l_q) + dt(1e-3)
    e_l = diff / (dt(sigma_lum) * dt(2.0 ** -i) * top)
    if guided is not None:
        s, sigma_g, relative_floor = guided
        e_l = s * (diff / (sigma_g + relative_floor * top)) + (dt(1) - s) * e_l
    return np.exp(-(e_n + e_z + e_l))


def prepare(accum, spp, albedo_hits, normal_depth, gspp, dtype=np.float64):
    """(d0, a, n, z) as (H, W, .) arrays of `dtype` from (H, W, 4) sums"""
    dt = dtype
    accum, ah, nd = (np.asarray(x).astype(dt) for x in (accum, albedo_hits, normal_depth))
    c = accum[..., :3] / dt(spp)
    a = np.maximum(ah[..., :3] / dt(gspp), dt(ALBEDO_FLOOR))
    nsum = nd[..., :3]
    ln = np.sqrt((nsum * nsum).sum(-1, keepdims=True))
    n = np.where(ln > 0, nsum / np.where(ln > 0, ln, dt(1)), dt(0))
    z = nd[..., 3] / dt(gspp)
    return c / a, a, n, z


def history_weight(count, full_history=0.0):
    """s(p) = min((N - 1) / (full_history - 1), 1), and 0 below N = 1 (a count pt_temporal_accumulate never writes)"""
    dt = count.dtype.type
    return np.clip((count - dt(1)) / (dt(full_history or FULL_HISTORY) - dt(1)), dt(0), dt(1))


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


def atrous(d, n, z, iterations, k_normal=0.0, sigma_depth=0.0, sigma_lum=0.0, variance=None):
    """`iterations` passes of the 5 x 5 B3-spline filter with step doubling over d (H, W, 3) under the guides n (H, W, 3), z (H, W).
    variance: None, or (V, count, sigma_variance, relative_floor, full_history) -- the filter of PT_DENOISE_INPUT_TEMPORAL_VARIANCE, whose luminance
    term moves from the relative one to the variance one as the history grows; V (H, W) is V_0, count (H, W) the history's N.  Returns (d, V) then."""
    k_normal, sigma_depth, sigma_lum = k_normal or K_NORMAL, sigma_depth or SIGMA_DEPTH, sigma_lum or SIGMA_LUM
    dt = d.dtype.type
    H, W = z.shape
    guided = None
    if variance is not None:
        V, count, sigma_variance, relative_floor, full_history = variance
        sigma_variance, relative_floor = dt(sigma_variance or SIGMA_VARIANCE), dt(relative_floor or RELATIVE_FLOOR)
        hw = history_weight(count.astype(d.dtype), full_history)
    for i in range(iterations):
        s = 2 ** i
        lum = luminance(d)
        num, den = np.zeros_like(d), np.zeros_like(z)
        if variance is not None:
            g, num_v = np.sqrt(_neighbourhood(V)), np.zeros_like(z)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                if abs(oy) >= H or abs(ox) >= W:
                    continue
                p = (slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox)))
                q = (slice(max(0, oy), H - max(0, -oy)), slice(max(0, ox), W - max(0, -ox)))
                if variance is not None:
                    guided = (hw[p], sigma_variance * g[p], relative_floor)
                w = dt(KERNEL[dy + 2]) * dt(KERNEL[dx + 2]) * tap_weight(n[p], n[q], z[p], z[q], lum[p], lum[q], i, k_normal, sigma_depth, sigma_lum, guided)
                num[p] += w[..., None] * d[q]
                den[p] += w
                if variance is not None:
                    num_v[p] += w * w * V[q]
        d = num / den[..., None]
        if variance is not None:
            V = num_v / (den * den)
    return d if variance is None else (d, V)


def denoise_hdr(accum, spp, albedo_hits, normal_depth, gspp, iterations, dtype=np.float64, **params):
    """the PT_DENOISE_HDR output (H, W, 3): linear mean radiance, filtered"""
    d0, a, n, z = prepare(accum, spp, albedo_hits, normal_depth, gspp, dtype)
    if iterations == 0:
        return np.asarray(accum).astype(dtype)[..., :3] / dtype(spp)
    return atrous(d0, n, z, iterations, **params) * a
