"""The edge-avoiding a-trous filter and the guide deposits as tests/denoise_ref.py restates them (include/ptamd.h, "guides and denoiser"):
facts any implementation of the contract has, and -- on the oracle alone -- that the documented defaults make a 4-spp image better."""
import ctypes

import numpy as np

import denoise_ref as R
import gpu_util as U
import orclib as O
from ptamd import device as D, scenes


def _guides(h, w, seed=0):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    z = rng.uniform(0.5, 5.0, (h, w))
    return n, z


def test_a_constant_image_is_a_fixed_point_under_any_guides():
    n, z = _guides(23, 31)
    d = np.full((23, 31, 3), 0.37)
    out = R.atrous(d, n, z, 5)
    assert np.abs(out - d).max() < 1e-15


def test_zero_iterations_is_the_input():
    rng = np.random.default_rng(1)
    accum = rng.uniform(0, 8, (9, 11, 4))
    ah = rng.uniform(0, 4, (9, 11, 4))
    nd = rng.normal(size=(9, 11, 4))
    assert np.array_equal(R.denoise_hdr(accum, 4, ah, nd, 4, 0), accum[..., :3] / 4.0)
    d, n, z = rng.uniform(0, 1, (9, 11, 3)), nd[..., :3], np.abs(nd[..., 3])
    assert R.atrous(d, n, z, 0) is d


def _two_regions(edge):
    """left half 0.2, right half 0.8 (+ noise that averages out), the halves told apart by `edge` alone"""
    h, w = 32, 64
    rng = np.random.default_rng(2)
    d = np.empty((h, w, 3))
    d[:, : w // 2] = 0.2
    d[:, w // 2:] = 0.8
    d += rng.uniform(-0.05, 0.05, d.shape)
    n = np.zeros((h, w, 3))
    n[..., 2] = 1.0
    z = np.full((h, w), 2.0)
    if edge == "normal":
        n[:, w // 2:] = (1.0, 0.0, 0.0)
    else:
        z[:, w // 2:] = 4.0
    return d, n, z


def test_normal_and_depth_edges_keep_two_regions_apart():
    for edge in ("normal", "depth"):
        d, n, z = _two_regions(edge)
        w = d.shape[1]
        # sigma_lum large: the luminance term must not be what keeps the regions apart
        out = R.atrous(d, n, z, 5, sigma_lum=1e6)
        left, right = d[:, : w // 2].mean(), d[:, w // 2:].mean()
        tol = 0.01 * abs(right - left)
        assert abs(out[:, : w // 2].mean() - left) < tol and abs(out[:, w // 2:].mean() - right) < tol, edge
        # ... and inside a region the noise is gone: the filter does something
        assert out[:, : w // 2].std() < 0.25 * d[:, : w // 2].std(), edge


def test_weights_are_symmetric():
    rng = np.random.default_rng(3)
    n, z = _guides(1, 4096, seed=4)
    n, z = n[0], z[0]
    z[::7] = R.SKY_DEPTH
    lum = rng.uniform(0, 3, 4096)
    p, q = slice(0, 2048), slice(2048, 4096)
    for i in range(6):
        a = R.tap_weight(n[p], n[q], z[p], z[q], lum[p], lum[q], i, R.K_NORMAL, R.SIGMA_DEPTH, R.SIGMA_LUM)
        b = R.tap_weight(n[q], n[p], z[q], z[p], lum[q], lum[p], i, R.K_NORMAL, R.SIGMA_DEPTH, R.SIGMA_LUM)
        assert np.array_equal(a, b) and (a > 0).any() and (a <= 1).all()


def pixel_centre_rays(camera, width, height):
    """pinhole rays through the pixel centres, row-major"""
    cam = np.asarray(camera, D.L.CAMERA).reshape(())
    eye, scr, u, v = (cam[k][:3].astype(np.float64) for k in ("eyePoint", "screenPoint", "u", "v"))
    yy, xx = np.mgrid[0:height, 0:width]
    s = scr + u * ((xx.reshape(-1, 1) + 0.5) / width) + v * ((yy.reshape(-1, 1) + 0.5) / height)
    d = s - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.repeat(eye[None], len(d), 0).astype(np.float32), d.astype(np.float32)


def test_the_defaults_make_a_4spp_cornell_box_better():
    """Oracle alone: cornell_box(64, 64) rendered at 4 and at 256 spp, guides restated from pixel-centre pinhole rays.  The denoised 4-spp
    image must be closer to the 256-spp one (tone-mapped RMSE) than the raw 4-spp image -- a do-nothing filter gives ratio 1, one that blurs
    across the walls' and boxes' edges more than that.  Measured with the defaults (k_normal 64, sigma_depth 0.05, sigma_lum 0.7):
    RMSE 7.5e-4 raw, 5.6e-4 denoised, ratio 0.74 (the exposure makes the tone-mapped room dark: its mean is 7.3e-4)."""
    b = scenes.cornell_box(64, 64)
    sc = U.oracle_scene(b)
    lo, _ = O.render(sc, b.camera, 64, 64, 4, threads=8)
    hi, _ = O.render(sc, b.camera, 64, 64, 256, threads=8)
    o, d = pixel_centre_rays(b.camera, 64, 64)
    hits = O.intersect_batch(sc, o, d, threads=8)
    ah, nd = R.guide_deposits(b.flat, d, hits)
    out = R.denoise_hdr(lo.reshape(64, 64, 4), 4, ah.reshape(64, 64, 4), nd.reshape(64, 64, 4), 1, 5)
    ref = U.tonemap(hi[:, :3].reshape(64, 64, 3), 256, b.camera)
    raw = U.rmse(U.tonemap(lo[:, :3].reshape(64, 64, 3), 4, b.camera), ref)
    den = U.rmse(U.tonemap(out, 1, b.camera), ref)
    print(f"tone-mapped RMSE against 256 spp: raw 4 spp {raw:.4f}, denoised {den:.4f}, ratio {den / raw:.3f}")
    assert den < raw


def test_denoise_params_is_32_bytes():
    assert ctypes.sizeof(D.DenoiseParams) == 32
