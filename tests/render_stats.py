"""Production renders against the reference's own kernels, statistically: the shared pieces of tests/golden/make_render_stats.py (the fixture of the
reference's side), tests/test_render_stats_cpu.py (the oracle in counter mode) and tests/test_gpu_render_stats.py (the device library).

A render is split into K independent groups of n samples per pixel; each group is reduced to the mean luminance of the 72 blocks of 6 x 3 pixels of the
48 x 27 image and the whole-image mean of each channel.  Two sides that draw from one distribution give group means whose Welch t statistics are t-distributed:
per block, their signed mean over the blocks (a bias too small for any one block shows in all of them), and for the whole image.  The generators of the two
sides differ (clRNG's LFSR113 | the counter PRNG), so nothing here is a bit comparison."""
import numpy as np
from scipy import stats as S

import orclib as O
from ptamd import scenes

W, H = 48, 27
BW, BH = 6, 3
BLOCKS = (W // BW) * (H // BH)
K = 32
N_START = 64  # samples per group to start from; the fixture's generator doubles it per scene until the conditions below hold
LUMA = np.array([0.2126, 0.7152, 0.0722], np.float64)
SE_LIMIT = 0.005  # standard error of a difference of whole-image means, relative to the mean
LEVEL_BLOCKS = 1e-3  # family-wise over the blocks of all scenes
LEVEL_SIGNED = 1e-4
LEVEL_IMAGE = 1e-4


def scene_builders():
    import test_oracle_vs_ref as T
    b = {k: T.CASES[k] for k in ("pbr", "glass", "instanced_sky", "instanced_thin_lens")}
    b["cornell"] = lambda: scenes.cornell_box(W, H)
    return b


SCENES = ("cornell", "glass", "instanced_sky", "instanced_thin_lens", "pbr")


_fixture = None


def fixture():
    """tests/golden/render_stats.npz (tests/golden/make_render_stats.py): {scene: {"groups": (K, 75) float32, "n", "se", "control"}}, read once"""
    global _fixture
    if _fixture is None:
        import golden_io
        z = golden_io.load_npz("render_stats.npz")
        assert int(z["K"]) == K
        _fixture = {s: {"groups": z[s + "/groups"], "n": int(z[s + "/n"]), "se": float(z[s + "/se"]), "control": z[s + "/control"]} for s in SCENES}
    return _fixture


def bound_scene(bundle):
    return O.BoundScene(bundle.flat, sky=bundle.sky, material_textures=bundle.material_textures)


def reduce_group(sums, n):
    """(W * H, >= 3) float32 sums of n samples -> float32 [72 block means of the luminance, 3 whole-image channel means]"""
    rgb = np.asarray(sums)[:, :3].astype(np.float64).reshape(H, W, 3) / n
    lum = rgb @ LUMA
    blocks = lum.reshape(H // BH, BH, W // BW, BW).mean(axis=(1, 3)).ravel()
    return np.concatenate([blocks, rgb.mean(axis=(0, 1))]).astype(np.float32)


def reference_groups(bundle, k, n, first_group=0):
    """Groups first_group .. first_group + k - 1 of the reference's kernels (oracle/_ref): successive ranges of n samples of one LFSR113 stream set"""
    sc = bound_scene(bundle)
    st = O.QueueState(W, H, (W * H + 63) // 64 * 64)
    streams = O.create_streams(W * H, use_ref=True)
    out = []
    for g in range(first_group + k):
        st.accum[:] = 0
        for _ in range(n):
            O.trace_rays("ref", sc, bundle.camera, st, streams)
        if g >= first_group:
            out.append(reduce_group(st.accum, n))
    return np.array(out)


def oracle_groups(bundle, k, n, seed=1, threads=8):
    """the oracle in counter mode: groups are first_sample ranges of one seed"""
    sc = bound_scene(bundle)
    return np.array([reduce_group(O.render(sc, bundle.camera, W, H, n, seed=seed, first_sample=g * n, threads=threads)[0], n) for g in range(k)])


def welch(a, b):
    """Welch's t of the columns of a against b (rows: groups): (t, degrees of freedom, two-sided p).  A column without variance on either side -- every
    group the same number -- has t = 0 if the two numbers agree to fp32 rounding of a mean (1e-6 relative) and is infinite otherwise."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    va, vb = a.var(axis=0, ddof=1) / len(a), b.var(axis=0, ddof=1) / len(b)
    d = a.mean(axis=0) - b.mean(axis=0)
    se2 = va + vb
    flat = se2 == 0
    same = np.abs(d) <= 1e-6 * np.maximum(np.abs(a.mean(axis=0)), np.abs(b.mean(axis=0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(flat, np.where(same, 0.0, np.inf * np.sign(d)), d / np.sqrt(se2))
        df = np.where(flat, len(a) + len(b) - 2.0, se2 ** 2 / (va ** 2 / (len(a) - 1) + vb ** 2 / (len(b) - 1)))
    return t, df, 2.0 * S.t.sf(np.abs(t), df)


def luminance_of_means(groups):
    return np.asarray(groups, np.float64)[:, BLOCKS:BLOCKS + 3] @ LUMA


def compare(a, b):
    """The three statistics of two sets of groups (rows of reduce_group)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    t, df, p = welch(a[:, :BLOCKS], b[:, :BLOCKS])
    signed = float(t.mean() * np.sqrt(BLOCKS / np.mean(df / (df - 2.0))))  # var(t_df) = df / (df - 2): standard normal for independent blocks
    ti, dfi, pi = welch(luminance_of_means(a)[:, None], luminance_of_means(b)[:, None])
    tc, _, pc = welch(a[:, BLOCKS:], b[:, BLOCKS:])
    return {"block_t": t, "block_p": p, "block_p_min": float(p.min()), "block_t_max": float(np.abs(t).max()), "signed": signed,
            "image_t": float(ti[0]), "image_p": float(pi[0]), "channel_p_min": float(pc.min())}


def gates():
    return {"block_p": LEVEL_BLOCKS / (BLOCKS * len(SCENES)), "signed": float(S.norm.isf(LEVEL_SIGNED / 2)), "image_p": LEVEL_IMAGE}


def verdict(c):
    """{statistic: inside its level}"""
    g = gates()
    return {"blocks": c["block_p_min"] >= g["block_p"], "signed": abs(c["signed"]) <= g["signed"], "image": c["image_p"] >= g["image_p"] and c["channel_p_min"] >= g["image_p"]}


def assert_same_distribution(what, got, ref):
    c = compare(got, ref)
    g = gates()
    print(f"{what}: min block p {c['block_p_min']:.3e} (max |t| {c['block_t_max']:.2f}; gate {g['block_p']:.2e}), signed mean of block t {c['signed']:+.2f} "
          f"(gate {g['signed']:.2f}), whole image t {c['image_t']:+.2f} p {c['image_p']:.3e}, channels min p {c['channel_p_min']:.3e} (gate {g['image_p']:.0e})")
    v = verdict(c)
    assert v["blocks"], (what, "a block's mean left the reference's distribution", c["block_p_min"], int(np.argmin(c["block_p"])))
    assert v["signed"], (what, "the blocks lean one way", c["signed"])
    assert v["image"], (what, "whole-image mean", c["image_t"], c["image_p"], c["channel_p_min"])
    return c


def relative_se_of_difference(groups):
    """standard error of the difference of two whole-image luminance means of len(groups) groups each, over the mean"""
    m = luminance_of_means(groups)
    return float(np.sqrt(2.0 * m.var(ddof=1) / len(m)) / m.mean())
