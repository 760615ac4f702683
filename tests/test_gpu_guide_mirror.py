"""Guide reflections on the device (pt_set_guide_reflections, k_guide_chain<true>; include/ptamd.h "guide reflections") against their numpy restatement
(tests/mirror_ref.py) on the device's own camera rays; the bits they owe a context with reflections off, run to run, over calls and over tilings; which
kernels run; the refusals, the lifetime of the tint planes, and what they buy a history of 1-spp frames in front of a mirror wall.  All at 64 x 36 with
three guide samples."""
import gc

import numpy as np
import pytest

import denoise_ref as R
import gpu_util as U
import mirror_ref as M
import orclib as O
from ptamd import device as D, layout as L, scenes
from test_denoise_ref import pixel_centre_rays
from test_mirror_ref import TEMPORAL_R, arc_camera, mirror_scene, on_mirror

pytestmark = pytest.mark.gpu
W, H = 64, 36
N = W * H
ERR_STATE, ERR_UNSUPPORTED = -3, -4  # PT_ERR_* (include/ptamd.h; tests/test_mirror_abi.py holds them against the header)

# fraction of (pixel, sample) entries whose chain ends on the restatement's primitive and instance (first run on an MI355X)
MEASURED = {
    "guide reflections: mirror_wall, K = 1: entries ending on the restatement's primitive": 1.0,
    "guide reflections: mirror_wall, K = 4: entries ending on the restatement's primitive": 1.0,
    "guide reflections: mirror_corridor, K = 4: entries ending on the restatement's primitive": 1.0,
    "guide reflections: mirror_blob_room, K = 4: entries ending on the restatement's primitive": 0.9998553240740741,
    "guide reflections: glass_box, K = 4: entries ending on the restatement's primitive": 1.0,
    "guide reflections: mirror_wall_thin_lens, K = 4: entries ending on the restatement's primitive": 1.0,
}
R_DEV = 0.56  # test_a_history_in_front_of_the_mirror_follows_the_virtual_image: the device's ratio on the first run (figures in its docstring)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mirror_ctx(gpu, b, K, reflections=True, **kw):
    ctx = U.make_ctx(gpu, b, W, H, **kw)
    ctx.set_guide_chain(K)
    ctx.set_guide_reflections(reflections)
    assert ctx.guide_chain == K and ctx.guide_reflections == bool(reflections)
    return ctx


def thin_lens_mirror_wall():
    b = scenes.cornell_mirror_wall(W, H)
    b.camera = scenes._camera(W, H, (0.0, 1.0, -0.8), (0.0, 1.0, 0.99), 40.0, thin_lens=True, focal_length_mm=50.0, aperture_fstops=2.0)
    return b


def _tiles(parity, size=16):
    return [(x, y, min(x + size, W), min(y + size, H)) for y in range(0, H, size) for x in range(0, W, size) if ((x // size) + (y // size)) % 2 == parity]


def meets_a_reflection(ctx, b, sc, K, samples):
    """per pixel: some sample's chain hits a MIRROR or meets a total internal reflection (the device's own rays through the restatement)"""
    met = np.zeros(N, bool)
    for s in range(samples):
        o, d, pixel = ctx.gen_rays(s, N)
        met[pixel] |= M.chain(b.flat, sc, o, d, K, b.material_textures)[2]["met"]
    return met


@pytest.mark.parametrize("K", [1, 4])
def test_sums_keep_their_bits(gpu, K):
    """cornell_mirror_wall, three guide samples: pixels none of whose samples meets a mirror carry the bits of a reflections-off context with the same
    K; a second run, (2) + (1) samples and two complementary tilings give the bits of the whole."""
    b = scenes.cornell_mirror_wall(W, H)
    sc = U.oracle_scene(b)
    off = mirror_ctx(gpu, b, K, reflections=False)
    met = meets_a_reflection(off, b, sc, K, 3)
    assert 200 < met.sum() < N - 200
    off.render_guides(3)
    off_a, off_g = off.read_guides()
    off.close()
    ctx = mirror_ctx(gpu, b, K)
    ctx.render_guides(3)
    a, g = ctx.read_guides()
    ctx.close()
    assert np.array_equal(bits(a)[~met], bits(off_a)[~met]) and np.array_equal(bits(g)[~met], bits(off_g)[~met])
    assert (g[met, 3] > off_g[met, 3]).mean() > 0.9  # in the mirror the distance is that of what it shows
    again = mirror_ctx(gpu, b, K)
    again.render_guides(3)
    split = mirror_ctx(gpu, b, K)
    split.render_guides(2)
    split.render_guides(1)
    for other in (again, split):
        oa, og = other.read_guides()
        assert np.array_equal(bits(oa), bits(a)) and np.array_equal(bits(og), bits(g))
        other.close()
    parts = []
    for parity in (0, 1):
        t = mirror_ctx(gpu, b, K)
        t.set_tiles(_tiles(parity))
        t.render_guides(3)
        parts.append(t.read_guides())
        t.close()
    assert np.array_equal(bits(parts[0][0] + parts[1][0]), bits(a)) and np.array_equal(bits(parts[0][1] + parts[1][1]), bits(g))
    assert (parts[0][0][:, :3].sum(1) == 0).any() and (parts[1][0][:, :3].sum(1) == 0).any()  # each left the other's pixels alone


@pytest.mark.parametrize("name", ["cornell_box", "glass_first"])
def test_nothing_to_reflect_keeps_every_bit(gpu, name):
    """cornell_box (the chain-off kernels run) and glass_first (glass, no total internal reflection from the camera: the reflecting kernel runs): both
    sums equal those of a reflections-off context bit for bit"""
    b = scenes.cornell_box(W, H) if name == "cornell_box" else scenes.glass_first(W, H)
    out = []
    for reflections in (False, True):
        ctx = mirror_ctx(gpu, b, 4, reflections=reflections)
        ctx.debug_guide_chain_terminals(True)
        ctx.render_guides(3)
        out.append(ctx.read_guides() + (ctx.read_guide_chain_terminals(),))
        ctx.close()
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))
    ran = (out[1][2][:, 2] >= 0).any()
    assert ran == (name == "glass_first")
    assert np.array_equal(out[0][2], out[1][2])  # (no reflection anywhere: the fourth word is 0 under either meaning)


CASES = [("mirror_wall", 1), ("mirror_wall", 4), ("mirror_corridor", 4), ("mirror_blob_room", 4), ("glass_box", 4), ("mirror_wall_thin_lens", 4)]


@pytest.mark.parametrize("name,K", CASES, ids=[f"{n}-K{k}" for n, k in CASES])
def test_reflections_match_the_restatement(gpu, name, K):
    """Three guide samples, each alone (sample base s, cleared sums), against mirror_ref on the device's own rays of that sample.  The fraction of
    (pixel, sample) entries whose chain ends on the restatement's primitive and instance is gated through fraction_gate, legacy floor 0.97.  On agreeing
    entries hits, the stage and the number of reflections are exact; the albedo is within 2 ulp per followed mirror of the float64 product (exact where
    no mirror was followed); the normal is within 1e-5 and the distance within 2e-4 relative (1e-6 absolute) times the number of segments -- or, where
    that is more, within 8 x the float32 restatement's own error against the float64 one ON THESE RAYS."""
    thin = name == "mirror_wall_thin_lens"
    b = thin_lens_mirror_wall() if thin else mirror_scene(name, W, H)
    sc = U.oracle_scene(b)
    ctx = mirror_ctx(gpu, b, K)
    ctx.debug_guide_chain_terminals(True)
    agree, depth, count, prims = [], [], [], []
    worst_n = worst_d = worst_a = tol_n_used = tol_d_used = 0.0
    for s in range(3):
        ctx.set_sample_base(s)
        ctx.clear()
        o, d, pixel = ctx.gen_rays(s, N)
        assert np.array_equal(np.sort(pixel), np.arange(N))
        want_a, want_g, info = M.chain(b.flat, sc, o, d, K, b.material_textures, thin_lens=thin)
        _, g32, info32 = M.chain(b.flat, sc, o, d, K, b.material_textures, dtype=np.float32, thin_lens=thin)
        ctx.render_guides(1)
        assert ctx.guide_samples == 1
        got_a, got_g = (x[pixel].astype(np.float64) for x in ctx.read_guides())
        term = ctx.read_guide_chain_terminals()[pixel]
        same = (term[:, 0] == info["prim"]) & (term[:, 1] == info["inst"])
        agree.append(same)
        depth.append(term[:, 2])
        count.append(term[:, 3])
        prims.append(term[:, 0])
        s32 = (info32["prim"] == info["prim"]) & (info32["inst"] == info["inst"])
        hit32 = s32 & (info["prim"] >= 0)
        f32_n = float(np.abs(g32[s32, :3] - want_g[s32, :3]).max())
        f32_d = float((np.abs(g32[hit32, 3] - want_g[hit32, 3]) / want_g[hit32, 3]).max())
        tol_n = max(1e-5, 8.0 * f32_n)
        hit = same & (info["prim"] >= 0)
        assert np.array_equal(got_a[same, 3], want_a[same, 3])
        assert np.array_equal(term[same, 2], info["depth"][same]) and np.array_equal(term[same, 3], info["reflections"][same])
        want32 = want_a[same, :3].astype(np.float32)
        ulps = np.abs(got_a[same, :3] - want32.astype(np.float64)) / np.spacing(want32).astype(np.float64)
        worst_a = max(worst_a, float(ulps.max()))
        assert (ulps <= 2.0 * info["mirrors"][same, None]).all(), (name, s, float(ulps.max()))
        err_n = np.abs(got_g[same, :3] - want_g[same, :3]).max(1)
        err_d = np.abs(got_g[hit, 3] - want_g[hit, 3])
        bound_d = np.maximum(2e-4 * info["segments"][hit], 8.0 * f32_d) * want_g[hit, 3] + 1e-6 * info["segments"][hit]
        worst_n, worst_d = max(worst_n, float(err_n.max())), max(worst_d, float((err_d / want_g[hit, 3]).max()))
        tol_n_used, tol_d_used = max(tol_n_used, tol_n), max(tol_d_used, 8.0 * f32_d)
        print(f"{name} K={K} sample {s}: agree {same.mean():.4f}, albedo {ulps.max():.2f} ulp, normal err {err_n.max():.2e} (tol {tol_n:.2e}), distance rel "
              f"{(err_d / want_g[hit, 3]).max():.2e} (float32's own {f32_d:.2e}), float32 follows {s32.mean():.4f}")
        assert (err_n <= tol_n).all(), (name, s, float(err_n.max()), tol_n)
        assert (err_d <= bound_d).all(), (name, s, float((err_d / want_g[hit, 3]).max()))
        miss = same & (info["prim"] < 0)
        assert (got_g[miss, 3] == D.GUIDE_SKY_DEPTH).all()
    agree, depth, count, prims = (np.concatenate(x) for x in (agree, depth, count, prims))
    hist = np.bincount(depth, minlength=K + 1)
    print(f"{name} K={K}: stages {hist.tolist()}, reflections followed {np.bincount(count, minlength=K + 1).tolist()}")
    U.record_margin(f"guide reflections vs restatement: {name}, K = {K}", albedo_ulps=worst_a, normal_error=worst_n, normal_tolerance=tol_n_used,
                    distance_error=worst_d, float32_distance_x8=tol_d_used, stages=hist.tolist(), reflections=np.bincount(count, minlength=K + 1).tolist())
    assert depth.min() >= 0 and hist[1:].sum() > 0 and count.max() >= 1
    if name == "mirror_corridor":
        assert ((depth == 4) & on_mirror(b.flat, prims)).sum() > 100  # chains that reach stage K on a mirror
    if name == "glass_box":
        types = b.flat.materials["type"][b.flat.triangles["materialIndex"]]
        off = mirror_ctx(gpu, b, K, reflections=False)
        off.debug_guide_chain_terminals(True)
        off.set_sample_base(2)
        off.render_guides(1)
        ended = off.read_guide_chain_terminals()
        off.close()
        glass_off = np.isin(types[ended[ended[:, 0] >= 0, 0]], (L.MAT_REFRACTIVE, L.MAT_BASIC_REFRACTIVE)).sum()
        glass_on = np.isin(types[term[term[:, 0] >= 0, 0]], (L.MAT_REFRACTIVE, L.MAT_BASIC_REFRACTIVE)).sum()
        print(f"glass_box: chains of sample 2 ending on glass {int(glass_off)} -> {int(glass_on)}")
        assert ended[:, 3].sum() >= 1 and glass_on < glass_off
    U.fraction_gate(f"guide reflections: {name}, K = {K}: entries ending on the restatement's primitive", agree, MEASURED, legacy=0.97)
    ctx.close()


def test_a_mirror_without_glass_runs_the_chain(gpu):
    """cornell_mirror_wall holds no glass: with reflections off the chain-off kernels run whatever K (today's behaviour, today's bits); with reflections
    on and K > 0 the terminal records show that the chain ran; K == 0 with reflections on is inert, in either order of the setters"""
    b = scenes.cornell_mirror_wall(W, H)
    out = {}
    for K, reflections, chain_first in ((0, False, True), (4, False, True), (0, True, True), (0, True, False), (4, True, True), (4, True, False)):
        ctx = U.make_ctx(gpu, b, W, H)
        for setter in ((ctx.set_guide_chain, K), (ctx.set_guide_reflections, reflections))[::1 if chain_first else -1]:
            setter[0](setter[1])
        ctx.debug_guide_chain_terminals(True)
        ctx.render_guides(3)
        out[K, reflections, chain_first] = ctx.read_guides() + (ctx.read_guide_chain_terminals(),)
        ctx.close()
    plain = out[0, False, True]
    for key in ((4, False, True), (0, True, True), (0, True, False)):
        assert (out[key][2] == -1).all()  # k_guide_chain did not run
        assert np.array_equal(bits(out[key][0]), bits(plain[0])) and np.array_equal(bits(out[key][1]), bits(plain[1]))
    a, g, term = out[4, True, True]
    assert (term[:, 2] >= 0).all() and (term[:, 3] == 1).sum() > 300  # every pixel's chain ended somewhere; the mirror's were reflected once
    assert not np.array_equal(bits(a), bits(plain[0]))
    other = out[4, True, False]
    assert np.array_equal(bits(other[0]), bits(a)) and np.array_equal(bits(other[1]), bits(g)) and np.array_equal(other[2], term)


def test_refusals(gpu):
    b = scenes.cornell_mirror_wall(W, H)
    ctx = U.make_ctx(gpu, b, W, H)
    assert ctx.guide_reflections is False
    ctx.set_guide_chain(2)
    ctx.set_guide_reflections(True)
    ctx.render_guides(1)
    ctx.set_guide_reflections(True)  # the value it has: accepted
    assert U.status(lambda: ctx.set_guide_reflections(False)) == ERR_STATE  # sums of two definitions must not mix
    assert ctx.guide_reflections is True and ctx.guide_samples == 1  # a refused call changes nothing
    ctx.clear()
    ctx.set_guide_reflections(False)
    ctx.render_guides(1)
    ctx.set_guide_reflections(False)
    assert U.status(lambda: ctx.set_guide_reflections(True)) == ERR_STATE
    assert ctx.guide_reflections is False
    ctx.close()
    # parity mode: the refusal of pt_set_guide_chain
    parity = U.make_ctx(gpu, b, W, H, rng_mode=D.RNG_LFSR113_PARITY)
    assert U.status(lambda: parity.set_guide_reflections(True)) == ERR_UNSUPPORTED
    assert parity.guide_reflections is False
    parity.set_guide_reflections(False)
    parity.close()


def test_stats_and_the_tint_planes_go_with_the_context(gpu):
    gc.collect()
    base = D.live_resources()
    b = scenes.cornell_mirror_wall(W, H)
    plain = U.make_ctx(gpu, b, W, H)
    plain.render_guides(1)
    without = D.live_resources()
    plain.close()
    assert D.live_resources() == base
    off = mirror_ctx(gpu, b, 4, reflections=False)  # no glass, no reflections: nothing of the chain is allocated
    off.render_guides(1)
    assert D.live_resources() == without
    off.close()
    ctx = mirror_ctx(gpu, b, 4)
    ctx.render_guides(2)
    ctx.render_guides(1)
    assert D.live_resources()[0] == without[0] + 6  # the second queue's two planes, two distance planes, two tint planes
    ctx.close()
    assert D.live_resources() == base
    # pt_stats is none of the pass's business
    counters = ("rays_extension", "rays_shadow", "rays_generated", "shade_hits", "deposits", "deposits_shadow", "samples", "team_launches", "packet_launches")
    ctx = mirror_ctx(gpu, b, 4)
    ctx.render(2)
    before = ctx.stats()
    ctx.render_guides(3)
    after = ctx.stats()
    assert [before[k] for k in counters] == [after[k] for k in counters]
    ctx.close()
    assert D.live_resources() == base


def history_in_front_of_the_mirror(gpu, b, sc, base=0):
    """the 12-frame arc (test_mirror_ref.arc_camera), 1 spp and three guide samples per frame, sample base `base` + frame: for reflections off and on
    (K = 4 both) the RMSE of the unfiltered history over the last frame's mirror pixels, tone-mapped, against 1024 spp, and the history counts in / outside"""
    last = arc_camera(11, W, H)
    hi, _ = O.render(sc, last, W, H, 1024, threads=8)
    ref = U.tonemap(hi[:, :3], 1024, last)
    mirror = M.chain(b.flat, sc, *pixel_centre_rays(last, W, H), 0)[2]["first_mirror"]  # the CPU figure's own pixels: by pixel-centre rays
    out = {}
    for reflections in (False, True):
        ctx = mirror_ctx(gpu, b, 4, reflections=reflections)
        for frame in range(12):
            ctx.set_camera(arc_camera(frame, W, H))
            ctx.set_sample_base(base + frame)
            ctx.clear()
            ctx.render(1)
            ctx.render_guides(3)
            ctx.temporal_accumulate()
        cn, _ = ctx.read_temporal()
        a, g = ctx.read_guides()
        albedo = R.prepare(ctx.read_accum(), 1, a, g, 3)[1]
        img = U.tonemap(cn[:, :3].astype(np.float64) * albedo, 1, last)
        out[reflections] = (U.rmse(img[mirror], ref[mirror]), float(cn[mirror, 3].mean()), float(cn[~mirror, 3].mean()), int(mirror.sum()))
        ctx.close()
    return out


def test_a_history_in_front_of_the_mirror_follows_the_virtual_image(gpu):
    """cornell_mirror_wall, the 12-frame arc of 2 degrees per frame that ends on the room's axis, 1 spp and three guide samples per frame (sample base =
    frame number), the UNFILTERED history: tone-mapped RMSE over the pixels whose first hit is the mirror against the oracle's 1024 spp, reflections on
    against off (K = 4 both).  Gate: (1 + r_t) / 2, r_t = TEMPORAL_R the ratio the restatement measures on the CPU (tests/test_mirror_ref.py) -- half
    of the gain is margin, because the glass chain's device runs moved their ratio by +-0.15 with jittered guides.
    The mirror pixels are the CPU figure's: those whose PIXEL-CENTRE ray hits the mirror first (440 of 2304).  The pixels on the mirror's outline are
    not among them: its upper edge shows the reflection of the ceiling light, a few pixels of high variance that decide the RMSE of any set they are in
    (with them, by a jittered first-hit mask of 475 pixels, the same run gives 3.22e-4 -> 7.47e-4).
    Measured on an MI355X: first-hit 1.270e-4 (history count 10.03 in the mirror / 5.32 outside), reflections 7.13e-5 (3.94 / 4.97), R_DEV = 0.56.  The
    kernels and the counter PRNG are deterministic, so the test repeats that figure; it is NOT a robust margin.  Other noise realisations (sample bases
    1000 k + frame, k = 1..7) give 0.79, 0.76, 0.84, 1.20, 1.28, 1.05, 0.86; pooled over the eight 1.03: after twelve 1-spp frames the RMSE of an
    unfiltered history over 440 pixels is mostly variance, and a history rightly cut to four frames is noisier than a ghosted one of ten.  What repeats in
    every realisation is the history count: 9.98 .. 10.03 in the mirror with first-hit guides (the ghosting), 3.94 .. 4.04 with reflections, against
    4.94 .. 4.99 outside.  The cost repeats too: the outline's pixels lose their history as well, and a firefly of the current frame shows there."""
    b = scenes.cornell_mirror_wall(W, H)
    sc = U.oracle_scene(b)
    out = history_in_front_of_the_mirror(gpu, b, sc)
    (e0, in0, out0, px), (e1, in1, out1, _) = out[False], out[True]
    ratio = e1 / e0
    U.record_margin("guide reflections: 12 frames in front of the mirror wall 64x36", first_hit=e0, reflections=e1, ratio=ratio, r_t=TEMPORAL_R, r_dev=R_DEV,
                    count_in_first_hit=in0, count_out_first_hit=out0, count_in=in1, count_out=out1, mirror_pixels=px)
    print(f"mirror pixels {px}: first-hit {e0:.3e} (history count {in0:.2f} in / {out0:.2f} outside), reflections {e1:.3e} ({in1:.2f} / {out1:.2f}), "
          f"ratio {ratio:.3f}")
    assert e1 < (1 + TEMPORAL_R) / 2 * e0
