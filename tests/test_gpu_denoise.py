"""The edge-avoiding a-trous denoiser on the device (pt_denoise, include/ptamd.h "guides and denoiser") against its numpy restatement
(tests/denoise_ref.py): synthetic inputs through write_accum / write_guides, a rendered frame, the refusals, the C++ example."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import gpu_util as U
from ptamd import device as D, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SPP, GSPP = 4, 2


def synthetic(width, height, seed=5):
    """Sums as the device holds them: seeded random colour with exact zeros and one 1e4 firefly; piecewise-smooth normals and depth
    (a tilted floor, a curved wall, a box in front of them) with sky regions; albedo with components below the 1e-3 floor."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    fx, fy = xx / max(width - 1, 1), yy / max(height - 1, 1)
    n = np.zeros((height, width, 3))
    z = np.zeros((height, width))
    floor = fy > 0.55
    n[floor] = (0.0, 1.0, 0.0)
    z[floor] = (1.0 + 4.0 * (1.0 - fy))[floor]
    wall = ~floor
    ang = (fx - 0.5) * 1.2
    n[wall] = np.stack([np.sin(ang), 0 * ang, -np.cos(ang)], -1)[wall]
    z[wall] = (3.0 + 0.5 * np.cos(ang))[wall]
    box = (abs(fx - 0.3) < 0.12) & (abs(fy - 0.6) < 0.2)
    n[box] = (0.6, 0.0, -0.8)
    z[box] = 1.5 + 0.3 * fx[box]
    sky = ((fx > 0.8) & (fy < 0.3)) | ((fx - 0.1) ** 2 + (fy - 0.1) ** 2 < 0.01)
    n[sky] = np.stack([-(fx - 0.5), -(fy - 0.5), -np.ones_like(fx)], -1)[sky]
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    z[sky] = R.SKY_DEPTH
    albedo = 0.1 + 0.8 * rng.uniform(size=(height, width, 3)) * (0.5 + 0.5 * np.sin(9 * fx)[..., None] ** 2)
    albedo[(xx + 2 * yy) % 11 == 0, 1] = 4e-4  # below the floor of the demodulation
    albedo[(xx * 3 + yy) % 13 == 0] = 2e-4
    albedo[sky] = 1.0
    colour = albedo * rng.gamma(0.6, 1.5, (height, width, 3))
    colour[rng.uniform(size=(height, width)) < 0.15] = 0.0  # exact zeros: paths that found no light
    colour[height // 3, width // 2] = (1e4, 0.5e4, 0.2e4)  # a firefly
    accum = np.zeros((height, width, 4), np.float32)
    accum[..., :3] = colour * SPP
    ah = np.zeros((height, width, 4), np.float32)
    ah[..., :3] = albedo * GSPP
    ah[..., 3] = np.where(sky, 0, GSPP)
    nd = np.zeros((height, width, 4), np.float32)
    nd[..., :3] = n * GSPP * rng.uniform(0.7, 1.0, (height, width, 1))  # sums of differing unit normals are shorter than their count
    nd[..., 3] = z * GSPP
    nd[height - 1, 0, :3] = 0.0  # a normal sum of zero stays zero
    return accum, ah, nd


@pytest.fixture(scope="module")
def cases(gpu):
    """inputs and a context per size, shared by the iteration counts"""
    made = {}

    def get(width, height):
        if (width, height) not in made:
            accum, ah, nd = synthetic(width, height)
            ctx = gpu.Context(width, height)
            ctx.write_accum(accum, SPP)
            ctx.write_guides(ah, nd, GSPP)
            made[(width, height)] = (ctx, accum, ah, nd)
        return made[(width, height)]
    yield get
    for ctx, *_ in made.values():
        ctx.close()


def hdr_bound(accum, ah, nd, spp, gspp, iterations):
    """(float64 restatement, bound): 8 x what single precision costs the restatement on this input + 1e-6 x the input's largest value"""
    ref64 = R.denoise_hdr(accum, spp, ah, nd, gspp, iterations, np.float64)
    ref32 = R.denoise_hdr(accum, spp, ah, nd, gspp, iterations, np.float32)
    assert ref32.dtype == np.float32
    return ref64, 8.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + 1e-6 * float(accum[..., :3].max() / spp)


SIZES_ITERATIONS = [(70, 45, i) for i in (1, 2, 3, 5, 6)] + [(150, 83, i) for i in (1, 2, 3, 5)] + [(16, 16, i) for i in (1, 2, 3, 5)]


@pytest.mark.parametrize("width,height,iterations", SIZES_ITERATIONS)
def test_filter_matches_the_restatement_on_synthetic_inputs(cases, width, height, iterations):
    """HDR output against the float64 restatement.  70 x 45 is no multiple of the 32 x 8 tile and narrower than the reach of iteration 5,
    150 x 83 is several tiles each way; iterations 1-2 run the LDS variant, 3 and more hand over to the direct loads."""
    ctx, accum, ah, nd = cases(width, height)
    out = ctx.denoise(iterations, hdr=True)
    ref, bound = hdr_bound(accum, ah, nd, SPP, GSPP, iterations)
    err = float(np.abs(out[..., :3].astype(np.float64) - ref).max())
    U.record_margin(f"denoise vs restatement: {width}x{height}, {iterations} iterations", error=err, bound=bound)
    print(f"{width}x{height} iterations {iterations}: error {err:.3e}, bound {bound:.3e}")
    assert np.all(out[..., 3] == 1.0)
    assert err <= bound
    # The firefly sets that bound (absolute, at values of thousands).  The same yardstick in relative terms holds the ordinary pixels too:
    # 8 x the largest relative difference between the float32 and the float64 restatement, + 1e-6.
    ref32 = R.denoise_hdr(accum, SPP, ah, nd, GSPP, iterations, np.float32).astype(np.float64)
    scale = np.abs(ref) + 1e-3
    rel, rel_bound = float((np.abs(out[..., :3] - ref) / scale).max()), 8.0 * float((np.abs(ref32 - ref) / scale).max()) + 1e-6
    U.record_margin(f"denoise vs restatement, relative: {width}x{height}, {iterations} iterations", error=rel, bound=rel_bound)
    print(f"    relative: error {rel:.3e}, bound {rel_bound:.3e}")
    assert rel <= rel_bound
    # the filter did something, and not the same thing at every iteration count
    mean = accum[..., :3] / SPP
    assert np.abs(out[..., :3] - mean).max() > 10 * bound


def srgb(x):
    return np.where(x <= 0.0031308, x * 12.92, 1.055 * np.abs(x) ** (1.0 / 2.4) - 0.055)


def test_rendered_frame_zero_iterations_is_resolve_and_five_match_the_restatement(gpu):
    b = scenes.cornell_box(64, 64)
    ctx = U.make_ctx(gpu, b, 64, 64)
    ctx.render(4)
    ctx.render_guides(4)
    assert np.array_equal(ctx.denoise(0), ctx.resolve())  # bit for bit
    accum = ctx.read_accum().reshape(64, 64, 4)
    ah, nd = (x.reshape(64, 64, 4) for x in ctx.read_guides())
    assert np.allclose(ctx.denoise(0, hdr=True)[..., :3], accum[..., :3] / 4.0, rtol=1e-6)
    ref, bound = hdr_bound(accum, ah, nd, 4, 4, 5)
    hdr = ctx.denoise(5, hdr=True)
    err_hdr = float(np.abs(hdr[..., :3].astype(np.float64) - ref).max())
    want = srgb(U.tonemap(ref, 1, b.camera))  # gpu_util.tonemap is pre-gamma; pt_resolve's image is sRGB-encoded
    out = ctx.denoise(5)
    err = float(np.abs(out[..., :3].astype(np.float64) - want).max())
    U.record_margin("denoise vs restatement: cornell 64x64 4 spp, 5 iterations", error_hdr=err_hdr, bound_hdr=bound, error_tonemapped=err,
                    bound_tonemapped=12.92 * bound)
    print(f"cornell: hdr error {err_hdr:.3e} (bound {bound:.3e}), tone-mapped error {err:.3e} (bound {12.92 * bound:.3e})")
    assert err_hdr <= bound
    assert err <= 12.92 * bound
    assert not np.array_equal(out, ctx.resolve())
    ctx.close()


def test_refusals_and_clear(gpu):
    INVALID, STATE, UNSUPPORTED = -1, -3, -4
    b = scenes.cornell_box(32, 32)
    ctx = U.make_ctx(gpu, b, 32, 32)
    ctx.render(1)
    assert U.status(lambda: ctx.denoise(3)) == STATE  # no guide sample yet
    ctx.clear()
    ctx.render_guides(1)
    assert U.status(lambda: ctx.denoise(3)) == STATE  # no colour sample yet
    ctx.render(1)
    assert ctx.denoise(3).shape == (32, 32, 4)
    assert U.status(lambda: ctx.denoise(7)) == INVALID
    ctx.set_tiles([(0, 0, 16, 32)])
    assert U.status(lambda: ctx.denoise(3)) == UNSUPPORTED
    ctx.set_tiles([])
    ctx.clear()
    assert ctx.guide_samples == 0 and ctx.samples_per_pixel == 0
    a, g = ctx.read_guides()
    assert not a.any() and not g.any()
    ctx.close()
    parity = U.make_ctx(gpu, b, 32, 32, rng_mode=D.RNG_LFSR113_PARITY)
    assert U.status(lambda: parity.render_guides(1)) == UNSUPPORTED
    parity.close()
    bare = gpu.Context(32, 32)
    assert U.status(lambda: bare.render_guides(1)) == STATE  # no scene, no camera
    bare.close()


def test_cpp_denoise_example(gpu, tmp_path):
    """examples/denoise_cornell.cpp: RayTracer::getOutput and getDenoisedOutput of one 4-spp frame -- two images of one size that differ,
    the denoised one with less high-frequency energy."""
    raw, den = tmp_path / "raw.ppm", tmp_path / "denoised.ppm"
    r = subprocess.run([os.path.join(ROOT, "examples", "denoise_cornell"), "4", str(raw), str(den)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split() if "=" in kv)
    assert int(fields["spp"]) == 4 and int(fields["guide_samples"]) == 4 and 0.3 < float(fields["coverage"]) <= 1.0
    a, b = U.read_ppm(raw), U.read_ppm(den)
    assert a.shape == b.shape == (256, 256, 3) and not np.array_equal(a, b)
    la, lb = U.mean_abs_laplacian(a), U.mean_abs_laplacian(b)
    print(f"mean |Laplacian|: raw {la:.4f}, denoised {lb:.4f}")
    assert lb < la
