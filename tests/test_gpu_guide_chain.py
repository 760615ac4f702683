"""The guide chain on the device (pt_set_guide_chain, k_guide_chain; include/ptamd.h "guide chain") against its numpy restatement
(tests/chain_ref.py) on the device's own camera rays; the bits it owes a context with the chain off, run to run, over calls and over tilings;
the refusals, the lifetime of its buffers, and what it buys a history of 1-spp frames behind glass.  All at 64 x 36."""
import gc

import numpy as np
import pytest

import chain_ref as CH
import gpu_util as U
import orclib as O
from ptamd import device as D, layout as L, scenes
from test_chain_ref import glass_box_room, gpu_scene

pytestmark = pytest.mark.gpu
W, H = 64, 36
ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -4  # PT_ERR_* (include/ptamd.h; tests/test_chain_abi.py holds them against the header)
N = W * H

# fraction of (pixel, sample) entries whose chain ends on the restatement's primitive and instance (first run on an MI355X), and the ratio of
# test_a_history_of_frames_behind_glass_is_better
MEASURED = {
    "guide chain: glass_box, K = 4: entries ending on the restatement's primitive": 1.0,
    "guide chain: glass_box, K = 1: entries ending on the restatement's primitive": 1.0,
    "guide chain: behind_rough_glass, K = 4: entries ending on the restatement's primitive": 1.0,
    "guide chain: zoo_room, K = 4: entries ending on the restatement's primitive": 1.0,
    "guide chain: glass_first_thin_lens, K = 4: entries ending on the restatement's primitive": 1.0,
}
R_DEV = 0.94  # measured on the first run (the docstring of test_a_history_of_frames_behind_glass_is_better has the figures and their spread)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def thin_lens_glass_first():
    b = gpu_scene("glass_first", W, H)
    b.camera = scenes._camera(W, H, (0.0, 1.0, -0.95), (0.0, 1.0, 1.0), 40.0, thin_lens=True, focal_length_mm=50.0, aperture_fstops=2.0)
    return b


def chain_ctx(gpu, b, K, **kw):
    ctx = U.make_ctx(gpu, b, W, H, **kw)
    ctx.set_guide_chain(K)
    assert ctx.guide_chain == K
    return ctx


def first_hit_is_glass(ctx, b, samples):
    """per pixel: some sample's stage-0 hit is REFRACTIVE / BASIC_REFRACTIVE (the device's own rays and hits)"""
    glass = np.zeros(N, bool)
    types = b.flat.materials["type"][b.flat.triangles["materialIndex"]]
    for s in range(samples):
        o, d, pixel = ctx.gen_rays(s, N)
        prim = ctx.intersect(o, d)["prim"]
        g = np.zeros(N, bool)
        g[prim >= 0] = np.isin(types[prim[prim >= 0]], (L.MAT_REFRACTIVE, L.MAT_BASIC_REFRACTIVE))
        glass[pixel] |= g
    return glass


def _tiles(parity, size=16):
    return [(x, y, min(x + size, W), min(y + size, H)) for y in range(0, H, size) for x in range(0, W, size) if ((x // size) + (y // size)) % 2 == parity]


@pytest.mark.parametrize("K", [1, 4])
def test_sums_keep_their_bits(gpu, K):
    """glass-box room, three guide samples: pixels whose stage-0 hit is never glass carry the bits of a chain-off context; a second run, (2) + (1)
    samples and two complementary tilings give the bits of the whole."""
    b = glass_box_room(W, H)
    off = U.make_ctx(gpu, b, W, H)
    glass = first_hit_is_glass(off, b, 3)
    assert 200 < glass.sum() < N - 200
    off.render_guides(3)
    off_a, off_g = off.read_guides()
    off.close()
    ctx = chain_ctx(gpu, b, K)
    ctx.render_guides(3)
    a, g = ctx.read_guides()
    ctx.close()
    assert np.array_equal(bits(a)[~glass], bits(off_a)[~glass]) and np.array_equal(bits(g)[~glass], bits(off_g)[~glass])
    assert (g[glass, 3] > off_g[glass, 3]).mean() > 0.9  # behind the glass the distance is that of what lies behind
    again = chain_ctx(gpu, b, K)
    again.render_guides(3)
    split = chain_ctx(gpu, b, K)
    split.render_guides(2)
    split.render_guides(1)
    for other in (again, split):
        oa, og = other.read_guides()
        assert np.array_equal(bits(oa), bits(a)) and np.array_equal(bits(og), bits(g))
        other.close()
    parts = []
    for parity in (0, 1):
        t = chain_ctx(gpu, b, K)
        t.set_tiles(_tiles(parity))
        t.render_guides(3)
        parts.append(t.read_guides())
        t.close()
    assert np.array_equal(bits(parts[0][0] + parts[1][0]), bits(a)) and np.array_equal(bits(parts[0][1] + parts[1][1]), bits(g))
    assert (parts[0][0][:, :3].sum(1) == 0).any() and (parts[1][0][:, :3].sum(1) == 0).any()  # each left the other's pixels alone


CASES = [("glass_box", 4), ("glass_box", 1), ("behind_rough_glass", 4), ("zoo_room", 4), ("glass_first_thin_lens", 4)]


@pytest.mark.parametrize("name,K", CASES, ids=[f"{n}-K{k}" for n, k in CASES])
def test_chain_matches_the_restatement(gpu, name, K):
    """Three guide samples, each alone (sample base s, cleared sums), against chain_ref on the device's own rays of that sample.  The fraction of
    (pixel, sample) entries whose chain ends on the restatement's primitive and instance (the device's, through the terminal records of
    pt_debug_guide_chain_terminals) is gated through fraction_gate, legacy floor 0.97.  On agreeing entries albedo and hits are exact, the normal is
    within the first-hit test's 1e-5 and the distance within its 2e-4 relative (1e-6 absolute) times the number of segments -- or, where that is
    more, within 8 x the float32 restatement's own error against the float64 one ON THESE RAYS (computed here, per case): a chain through a curved,
    sheared body amplifies rounding, and float32 is what the device has."""
    thin = name == "glass_first_thin_lens"
    b = thin_lens_glass_first() if thin else gpu_scene(name, W, H)
    sc = U.oracle_scene(b)
    ctx = chain_ctx(gpu, b, K)
    ctx.debug_guide_chain_terminals(True)
    agree, depth, tir = [], [], []
    worst_n = worst_d = tol_n_used = tol_d_used = 0.0
    for s in range(3):
        ctx.set_sample_base(s)
        ctx.clear()
        o, d, pixel = ctx.gen_rays(s, N)
        assert np.array_equal(np.sort(pixel), np.arange(N))
        want_a, want_g, info = CH.chain(b.flat, sc, o, d, K, b.material_textures, thin_lens=thin)
        _, g32, info32 = CH.chain(b.flat, sc, o, d, K, b.material_textures, dtype=np.float32, thin_lens=thin)
        ctx.render_guides(1)
        assert ctx.guide_samples == 1
        got_a, got_g = (x[pixel].astype(np.float64) for x in ctx.read_guides())
        term = ctx.read_guide_chain_terminals()[pixel]
        same = (term[:, 0] == info["prim"]) & (term[:, 1] == info["inst"])
        agree.append(same)
        depth.append(term[:, 2])
        tir.append(term[:, 3])
        # the float32 restatement's own error, on the entries where it follows the float64 one
        s32 = (info32["prim"] == info["prim"]) & (info32["inst"] == info["inst"])
        hit32 = s32 & (info["prim"] >= 0)
        f32_n = float(np.abs(g32[s32, :3] - want_g[s32, :3]).max())
        f32_d = float((np.abs(g32[hit32, 3] - want_g[hit32, 3]) / want_g[hit32, 3]).max())
        tol_n = max(1e-5, 8.0 * f32_n)
        hit = same & (info["prim"] >= 0)
        assert np.array_equal(got_a[same, 3], want_a[same, 3])
        assert np.array_equal(got_a[same, :3].astype(np.float32), want_a[same, :3].astype(np.float32))
        assert np.array_equal(term[same, 2], info["depth"][same]) and np.array_equal(term[same, 3] == 1, info["tir"][same])
        err_n = np.abs(got_g[same, :3] - want_g[same, :3]).max(1)
        err_d = np.abs(got_g[hit, 3] - want_g[hit, 3])
        bound_d = np.maximum(2e-4 * info["segments"][hit], 8.0 * f32_d) * want_g[hit, 3] + 1e-6 * info["segments"][hit]
        worst_n, worst_d = max(worst_n, float(err_n.max())), max(worst_d, float((err_d / want_g[hit, 3]).max()))
        tol_n_used, tol_d_used = max(tol_n_used, tol_n), max(tol_d_used, 8.0 * f32_d)
        print(f"{name} K={K} sample {s}: agree {same.mean():.4f}, normal err {err_n.max():.2e} (tol {tol_n:.2e}), distance rel "
              f"{(err_d / want_g[hit, 3]).max():.2e} (float32's own {f32_d:.2e}), float32 follows {s32.mean():.4f}")
        assert (err_n <= tol_n).all(), (name, s, float(err_n.max()), tol_n)
        assert (err_d <= bound_d).all(), (name, s, float((err_d / want_g[hit, 3]).max()))
        miss = same & (info["prim"] < 0)
        assert (got_g[miss, 3] == D.GUIDE_SKY_DEPTH).all()
    agree, depth, tir = np.concatenate(agree), np.concatenate(depth), np.concatenate(tir)
    hist = np.bincount(depth, minlength=K + 1)
    print(f"{name} K={K}: stages {hist.tolist()}, total internal reflections {int(tir.sum())}")
    U.record_margin(f"guide chain vs restatement: {name}, K = {K}", normal_error=worst_n, normal_tolerance=tol_n_used, distance_error=worst_d,
                    float32_distance_x8=tol_d_used, stages=hist.tolist(), reflections=int(tir.sum()))
    assert depth.min() >= 0 and hist[1] > 0
    if K >= 2 and name in ("glass_box", "zoo_room"):  # a body has a way in and a way out; the two panes are one interface each
        assert hist[2] > 0
    if name == "glass_box" and K == 4:
        assert tir.sum() >= 1
    U.fraction_gate(f"guide chain: {name}, K = {K}: entries ending on the restatement's primitive", agree, MEASURED, legacy=0.97)
    ctx.close()


def test_a_scene_without_glass_runs_the_kernels_of_before(gpu):
    """cornell_box, chain on: both sums carry the chain-off bits, nothing is recorded by a chain kernel, pt_stats is untouched"""
    b = scenes.cornell_box(W, H)
    counters = ("rays_extension", "rays_shadow", "rays_generated", "shade_hits", "deposits", "deposits_shadow", "samples", "team_launches", "packet_launches")
    out = []
    for K in (0, 4):
        ctx = chain_ctx(gpu, b, K)
        ctx.debug_guide_chain_terminals(True)
        ctx.render(2)
        before = ctx.stats()
        ctx.render_guides(3)
        after = ctx.stats()
        assert [before[k] for k in counters] == [after[k] for k in counters]
        assert (ctx.read_guide_chain_terminals() == -1).all()  # k_guide_chain did not run
        out.append(ctx.read_guides() + (ctx.read_accum(),))
        ctx.close()
    for x, y in zip(*out):
        assert np.array_equal(bits(x), bits(y))


def test_refusals(gpu):
    b = glass_box_room(W, H)
    ctx = U.make_ctx(gpu, b, W, H)
    assert ctx.guide_chain == 0
    assert U.status(lambda: ctx.set_guide_chain(D.GUIDE_CHAIN_MAX + 1)) == ERR_INVALID
    ctx.set_guide_chain(2)
    ctx.render_guides(1)
    ctx.set_guide_chain(2)  # the value it has: accepted
    for K in (0, 3):  # a change while samples are in the sums: sums of two definitions must not mix
        assert U.status(lambda: ctx.set_guide_chain(K)) == ERR_STATE
    assert ctx.guide_chain == 2
    ctx.clear()
    ctx.set_guide_chain(3)
    # the chain and the motions refuse each other, in either order
    assert U.status(lambda: ctx.set_instance_motion(b.flat.top_nodes)) == ERR_UNSUPPORTED
    assert U.status(lambda: ctx.set_vertex_motion(True)) == ERR_UNSUPPORTED
    ctx.set_instance_motion(None)  # forgetting is not refused
    ctx.set_vertex_motion(False)
    ctx.set_guide_chain(0)
    ctx.set_instance_motion(b.flat.top_nodes)
    assert U.status(lambda: ctx.set_guide_chain(1)) == ERR_UNSUPPORTED
    ctx.set_guide_chain(0)
    assert U.status(lambda: ctx.set_guide_chain(5)) == ERR_INVALID
    ctx.close()
    # parity mode: the refusal of pt_render_guides
    parity = U.make_ctx(gpu, b, W, H, rng_mode=D.RNG_LFSR113_PARITY)
    assert U.status(lambda: parity.set_guide_chain(1)) == ERR_UNSUPPORTED
    parity.set_guide_chain(0)
    parity.close()




def test_the_chain_buffers_go_with_the_context(gpu):
    gc.collect()
    base = D.live_resources()
    b = glass_box_room(W, H)
    plain = U.make_ctx(gpu, b, W, H)
    plain.render_guides(1)
    without = D.live_resources()
    plain.close()
    assert D.live_resources() == base
    ctx = chain_ctx(gpu, b, 4)
    ctx.render_guides(2)
    ctx.debug_guide_chain_terminals(True)
    ctx.render_guides(1)
    assert D.live_resources()[0] == without[0] + 5  # the second queue's two planes, two distance planes, the terminal records
    ctx.debug_guide_chain_terminals(False)
    assert D.live_resources()[0] == without[0] + 4
    ctx.close()
    assert D.live_resources() == base


def test_a_history_of_frames_behind_glass_is_better(gpu):
    """glass-box room, twelve 1-spp frames under a static camera (sample base = frame number), three guide samples per frame like every case of this
    file, history + five iterations over it: tone-mapped RMSE over the pixels whose first hit is glass against the oracle's 1024 spp, chain (K = 4)
    against first-hit guides.  Gate: (1 + r_dev) / 2, r_dev = R_DEV the ratio measured on the first run ("no better" is 1 and fails).
    Measured on an MI355X (365 glass pixels of 2304): first-hit 7.66e-5, chain 7.21e-5, r_dev = 0.94; pixels outside the glass 0.97 x.  The kernels
    and the counter PRNG are deterministic, so the test repeats that figure; it is NOT a large margin, and other noise realisations (sample bases
    100 k + frame, k = 1..7) give 0.74 .. 1.06, pooled over the eight 0.95 with 1.014 outside: at this size and frame count the error over a few
    hundred glass pixels is mostly variance.  With ONE guide sample per frame -- what this test ran at first, against the set-up its file states --
    the chain LOSES on this view: 8.27e-5 -> 9.12e-5, 1.10 (1.01 .. 1.16 over eight realisations, pooled 1.09; outside 1.03; history count 8.31
    against 8.07): a single jittered guide ray per frame crosses the new edges inside a box 15 pixels wide from frame to frame, 43 % of the box's
    entries end in total internal reflection (a second flat region), and -- supposed, not shown -- the wall albedo (0.12, 0.45, 0.15) demodulates
    the front face's Fresnel reflection and changes under a pixel between frames.  A caller behind a small glass body wants more than one guide
    sample per frame (they cost a fraction of the frame: DESIGN.md section 9).  Where the glass is a pane in front of the room one is enough:
    examples/glass_cornell, 256 x 256, orbiting camera, twelve frames: RMSE through the glass 0.0216 -> 0.0113."""
    b = glass_box_room(W, H)
    sc = U.oracle_scene(b)
    hi, _ = O.render(sc, b.camera, W, H, 1024, threads=8)
    ref = U.tonemap(hi[:, :3], 1024, b.camera)
    errs = {}
    for K in (0, 4):
        ctx = chain_ctx(gpu, b, K)
        if K == 0:
            glass = first_hit_is_glass(ctx, b, 1)
        for frame in range(12):
            ctx.set_sample_base(frame)
            ctx.clear()
            ctx.render(1)
            ctx.render_guides(3)
            ctx.temporal_accumulate()
        out = ctx.denoise(5, hdr=True, input_temporal=True).reshape(N, 4)[:, :3].astype(np.float64)
        img = U.tonemap(out, 1, b.camera)
        errs[K] = (U.rmse(img[glass], ref[glass]), U.rmse(img[~glass], ref[~glass]))
        ctx.close()
    ratio, outside = errs[4][0] / errs[0][0], errs[4][1] / errs[0][1]
    U.record_margin("guide chain: 12 frames behind glass, glass-box room 64x36", first_hit=errs[0][0], chain=errs[4][0], ratio=ratio, r_dev=R_DEV,
                    outside_ratio=outside, glass_pixels=int(glass.sum()))
    print(f"glass pixels {int(glass.sum())}: first-hit {errs[0][0]:.3e}, chain {errs[4][0]:.3e}, ratio {ratio:.3f}; outside ratio {outside:.4f}")
    assert R_DEV is not None, "r_dev has not been measured yet"
    assert errs[4][0] < (1 + R_DEV) / 2 * errs[0][0]
