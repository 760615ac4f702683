"""First-hit guide buffers (pt_render_guides, include/ptamd.h "guides and denoiser") against the oracle's hits and the numpy restatement of
the deposits (tests/denoise_ref.py); that the sums are reproducible whatever the schedule, and that the pass leaves the render alone."""
import numpy as np
import pytest

import denoise_ref as R
import gpu_util as U
import orclib as O
from ptamd import scenes

pytestmark = pytest.mark.gpu


def _scene(name):
    if name == "cornell":
        return scenes.cornell_box(64, 64)
    if name == "crowd_general":
        return scenes.instanced_crowd(64, 36, nx=2, nz=2, level=2, transform="general")
    if name == "textured_floor":
        return scenes.blob_room(64, 36, level=2, textured_floor=True)
    if name == "zoo_room":  # a mirrored, a sheared, a non-uniformly scaled and a small instance: the world-space normal behind such transforms
        return scenes.zoo_room(64, 36)
    return scenes.glass_first()


@pytest.mark.parametrize("name", ["cornell", "crowd_general", "textured_floor", "glass_first", "zoo_room"])
def test_guides_match_the_oracle_at_one_sample(gpu, name):
    """Guide VALUES for the rays of sample 0 (ctx.gen_rays) against deposits restated from the oracle's hits: albedo / coverage and
    normal to 1e-5 absolute, distance to 2e-4 relative; at most 1 % of the pixels outside (hit / miss and nearest-triangle ties at
    silhouettes: the allowance compare_hits grants)."""
    b = _scene(name)
    n = b.width * b.height
    ctx = U.make_ctx(gpu, b, b.width, b.height)
    o, d, pixel = ctx.gen_rays(0, n)
    assert np.array_equal(np.sort(pixel), np.arange(n))
    hits = O.intersect_batch(U.oracle_scene(b), o, d, threads=8)
    want_a, want_g = R.guide_deposits(b.flat, d, hits, b.material_textures)
    ctx.render_guides(1)
    assert ctx.guide_samples == 1
    got_a, got_g = ctx.read_guides()
    got_a, got_g = got_a[pixel].astype(np.float64), got_g[pixel].astype(np.float64)
    ok = (np.abs(got_a - want_a).max(1) <= 1e-5) & (np.abs(got_g[:, :3] - want_g[:, :3]).max(1) <= 1e-5) \
        & np.isclose(got_g[:, 3], want_g[:, 3], rtol=2e-4, atol=1e-6)
    frac = 1.0 - float(ok.mean())
    U.record_margin(f"guides vs oracle: {name}", outside_fraction=frac, gate=1e-2, pixels=n, hits=float(want_a[:, 3].sum()),
                    textured=float((np.abs(want_a[:, :3] - want_a[:, :1]).max(1) > 0).mean()))
    assert want_a[:, 3].sum() > 0.3 * n  # the scene is in view
    assert frac <= 1e-2, (name, frac)
    ctx.close()


def _close(got, want):
    """1e-5 relative, against the magnitude of a sample's deposit (components of unit normals and albedos pass through zero)"""
    return np.abs(got - want) <= 1e-5 * np.maximum(np.abs(want), 1.0)


def _tiles(width, height, parity, size=16):
    return [(x, y, min(x + size, width), min(y + size, height)) for y in range(0, height, size) for x in range(0, width, size)
            if ((x // size) + (y // size)) % 2 == parity]


def test_several_guide_samples_sum_in_sample_order_whatever_the_schedule(gpu):
    b = scenes.cornell_box(70, 45)
    n = 70 * 45
    ctx = U.make_ctx(gpu, b, 70, 45, samples_in_flight=16)
    want_a, want_g = np.zeros((n, 4)), np.zeros((n, 4))
    for s in range(5):  # the device's own hits for guide sample s: the rays pt_render traces for sample index s
        o, d, pixel, hits = ctx.primary_pass(s, 1, n)
        a, g = R.guide_deposits(b.flat, d, hits)
        want_a[pixel] += a
        want_g[pixel] += g
    ctx.render_guides(5)
    assert ctx.guide_samples == 5 and ctx.samples_per_pixel == 0
    got_a, got_g = ctx.read_guides()
    assert _close(got_a, want_a).all() and _close(got_g, want_g).all()
    assert got_a[:, 3].max() == 5  # coverage counts samples

    # 2 + 3 samples: guide indices continue from pt_guide_samples
    split = U.make_ctx(gpu, b, 70, 45, samples_in_flight=16)
    split.render_guides(2)
    split.render_guides(3)
    sa, sg = split.read_guides()
    assert np.allclose(sa, got_a, rtol=1e-6, atol=0) and np.allclose(sg, got_g, rtol=1e-6, atol=1e-6)
    # again, bit for bit; and with queues smaller than a batch (the guide pass has a scratch queue of its own)
    for kw in (dict(), dict(ext_queue_fraction=0.30, shadow_queue_fraction=0.62)):
        other = U.make_ctx(gpu, b, 70, 45, samples_in_flight=16, **kw)
        other.render_guides(5)
        oa, og = other.read_guides()
        assert np.array_equal(oa, got_a) and np.array_equal(og, got_g), kw
        other.close()
    # two contexts owning complementary 16 x 16 tiles: their images add up to the whole one
    parts = []
    for parity in (0, 1):
        t = U.make_ctx(gpu, b, 70, 45, samples_in_flight=16)
        t.set_tiles(_tiles(70, 45, parity))
        t.render_guides(5)
        parts.append(t.read_guides())
        t.close()
    assert np.array_equal(parts[0][0] + parts[1][0], got_a) and np.array_equal(parts[0][1] + parts[1][1], got_g)
    assert (parts[0][0][:, :3].sum(1) == 0).any() and (parts[1][0][:, :3].sum(1) == 0).any()  # each left the other's pixels alone
    ctx.close()
    split.close()


def test_the_guide_pass_leaves_the_render_alone(gpu):
    b = scenes.cornell_box(64, 64)
    counters = ("rays_extension", "rays_shadow", "rays_generated", "shade_hits", "deposits", "deposits_shadow", "samples")
    results = []
    for with_guides in (False, True):
        ctx = U.make_ctx(gpu, b, 64, 64)
        ctx.render(4)
        if with_guides:
            ctx.render_guides(4)
        ctx.render(4)
        st = ctx.stats()
        results.append((ctx.read_accum(), ctx.samples_per_pixel, [st[k] for k in counters], ctx.guide_samples))
        ctx.close()
    assert np.array_equal(results[0][0], results[1][0])
    assert results[0][1] == results[1][1] == 8 and results[0][2] == results[1][2]
    assert (results[0][3], results[1][3]) == (0, 4)
