"""k_shade through pt_shade_batch over the shade grid (tests/shade_grid.py) against the oracle, entry by entry, counter PRNG under identical keys: the
material corners (smoothness 0 / 1 / either side of kMaxSmoothness, ior 1 / kAirIor, f0 0 / 1, total internal reflection), grazing and back-side
incidence either side of kEPS and of the 0.05 cutoff, hits at vertices and edge midpoints, turned, mirrored and quarter-turned instances, and the
axis-aligned normals on which the reference's tangent frame is NaN.  tests/test_shade_grid_cpu.py holds the oracle to the reference on the same entries and
shows that the grid is conditioned: a disagreement beyond the gates here is not round-off.

The gates per stratum are those of test_gpu_gen_shade.py::test_shade_batch_matches_oracle_per_material; the measured fractions are read from
profiles/round6/parity_margins.json (gpu_util.fraction_gate: 0.98 x measured, never below 0.97)."""
import json
import os
import time

import numpy as np
import pytest

import gpu_util as U
import orclib as O
import shade_grid as G

pytestmark = pytest.mark.gpu

W, H = 64, 48  # one pixel per entry: 3072 >= the largest family
_PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "round6", "parity_margins.json")
# The "fraction" entries of that file are the MEASUREMENT of the first green MI355X run of this file on the committed kernel, frozen: the gate is 0.98 x
# them.  The file is a copy of what a session writes, and copying a later session's output over it re-bases every gate on that session -- do that only
# for a kernel change that is meant to move a fraction, and say so; a fraction that fell is a finding, not a new baseline.  (The "measured" / "gate" fields
# of an entry record how the session that wrote it was gated, not how this file gates.)
with open(_PROFILE) as _f:
    MEASURED = {k[len("fraction: "):]: v["fraction"] for k, v in json.load(_f).items() if k.startswith("fraction: shade grid")}

RAY = (("nox", "origin", 0), ("noy", "origin", 1), ("noz", "origin", 2), ("ndx", "direction", 0), ("ndy", "direction", 1), ("ndz", "direction", 2),
       ("nthr_r", "multiplier", 0), ("nthr_g", "multiplier", 1), ("nthr_b", "multiplier", 2))
SHADOW = (("sox", "origin", 0), ("soy", "origin", 1), ("soz", "origin", 2), ("sdx", "direction", 0), ("sdy", "direction", 1), ("sdz", "direction", 2),
          ("sc_r", "multiplier", 0), ("sc_g", "multiplier", 1), ("sc_b", "multiplier", 2))


def _shade_on_gpu(gpu, g, flags=0):
    S = g.scene
    assert g.n <= W * H and int(g.rays["outputPixel"].max()) < W * H and g.prim.max() < len(S.flat.triangles)
    ctx = U.make_ctx(gpu, S.flat, W, H, camera=S.camera, sky=S.sky, tex=S.tex, seed=4, flags=flags)
    t0 = time.time()
    got = ctx.shade_batch(g.rays["origin"][:, :3], g.rays["direction"][:, :3], g.rays["multiplier"][:, :3], g.rays["outputPixel"], g.rays["flags"],
                          g.rays["numBounces"], g.t, g.uv[:, 0], g.uv[:, 1], g.prim, g.inst, sample=2)
    dt = time.time() - t0
    ctx.close()
    return got, dt


def _compare(tag, g, got, want):
    """the stratum gates; returns (flips, worst continuation fraction, worst shadow fraction) over the strata"""
    g_o, g_s = got["out_alive"].astype(bool), got["shadow_alive"].astype(bool)
    # every live output is finite, the axis-aligned strata included
    for names, alive in ((RAY, g_o), (SHADOW + (("slen", None, None),), g_s)):
        for a, _, _ in names:
            assert np.isfinite(got[a][alive]).all(), (tag, a, sorted(set(g.labels["corner"][alive & ~np.isfinite(got[a])]))[:6])
    assert np.isfinite(got["radiance"]).all(), tag
    worst_flips, worst_ray, worst_shadow = (0, 0), 1.0, 1.0
    for label, sl in G.strata(g):
        size = len(sl)
        assert size >= 64, (tag, label, size)
        flips = int((g_o[sl] != want.ray_alive[sl]).sum()), int((g_s[sl] != want.shadow_alive[sl]).sum())
        print(f"{tag}/{label}: {size} entries, flips {flips}")
        assert max(flips) <= max(1, size // 64), (tag, label, flips)
        worst_flips = max(worst_flips, flips, key=max)
        both = sl[want.ray_alive[sl] & g_o[sl]]
        worst = 1.0
        for a, f, c in RAY:
            close = np.isclose(got[a][both], want.ray[f][both, c], rtol=2e-3, atol=2e-4)
            worst = min(worst, float(close.mean()) if close.size else 1.0)
        U.fraction_gate(f"shade grid {tag}/{label}: continuation rays, worst field", np.array([worst]), MEASURED, legacy=0.97)
        worst_ray = min(worst_ray, worst)
        if worst < 1.0 and label.startswith("family"):  # which entries, which fields, by how much: the record a fraction below 1 needs
            for a, f, c in RAY:
                for k in both[~np.isclose(got[a][both], want.ray[f][both, c], rtol=2e-3, atol=2e-4)]:
                    print(f"  off: {tag} entry {k} {[g.labels[d][k] for d in g.labels]} {a}: {got[a][k]!r} against {want.ray[f][k, c]!r}")
        assert np.array_equal(got["nflags"][both] & 2, want.ray["flags"][both] & 2), (tag, label, "LASTSPECULAR")
        sb = sl[want.shadow_alive[sl] & g_s[sl]]
        worst = 1.0
        for a, f, c in SHADOW:
            close = np.isclose(got[a][sb], want.shadow[f][sb, c], rtol=2e-3, atol=2e-4)
            worst = min(worst, float(close.mean()) if close.size else 1.0)
        if sb.size:
            worst = min(worst, float(np.isclose(got["slen"][sb], want.shadow["rayLength"][sb], rtol=1e-4, atol=1e-5).mean()))
        U.fraction_gate(f"shade grid {tag}/{label}: shadow rays, worst field", np.array([worst]), MEASURED, legacy=0.97)
        worst_shadow = min(worst_shadow, worst)
        rad_close = np.isclose(got["radiance"][sl], want.radiance[sl], rtol=2e-3, atol=1e-4).all(axis=1)
        U.fraction_gate(f"shade grid {tag}/{label}: radiance deposited by shade", rad_close, MEASURED, legacy=0.98)
    return worst_flips, worst_ray, worst_shadow


def _structure(g, got):
    """what must hold per family whatever the numbers are"""
    g_o, g_s = got["out_alive"].astype(bool), got["shadow_alive"].astype(bool)
    fam, corner = g.labels["family"], g.labels["corner"]
    glass = np.isin(fam, ("rough glass", "basic glass"))
    assert not g_s[glass].any(), "no next event estimation on refractive materials"
    assert g_o[fam == "basic glass"].all(), "basic glass: the green channel is not absorbed, the survival probability is 1"
    assert (got["nflags"][glass & g_o] & 2).all(), "a refractive bounce is specular"
    miss = fam == "miss"
    assert not g_o[miss].any() and not g_s[miss].any() and (got["radiance"][miss].sum(axis=1) > 0).all()
    em = fam == "emissive"
    assert not g_o[em].any() and not g_s[em].any(), "an emissive hit ends the path (shading.cl:387-397)"
    spec = em & (corner == "after a specular bounce")
    assert np.allclose(got["radiance"][spec], g.rays["multiplier"][spec, :3] * g.colour[spec], rtol=1e-6) and (got["radiance"][em & ~spec] == 0).all()
    assert (got["radiance"][~em & ~miss] == 0).all(), "only emissive hits and sky misses deposit in shade"
    pbr = np.isin(fam, ("pbr dielectric", "pbr metal"))
    rough = pbr & np.array([c.startswith(("s=0 ", "s=0.3", "s=0.94-")) or c in ("s=0", "s=0.94-") for c in corner])
    assert not (got["nflags"][rough & g_o] & 2).any(), "smoothness <= kMaxSmoothness never sets LASTSPECULAR"
    always = pbr & ~rough & ((fam == "pbr metal") | np.array([c.endswith("f0=1") for c in corner]))  # F = 1: the specular branch every time
    assert (got["nflags"][always & g_o] & 2).all() and (not always.any() or (always & g_o).sum() >= 32)
    smooth = pbr & ~rough
    assert not smooth.any() or (got["nflags"][smooth & g_o] & 2).any()
    if g.alpha0.any():  # an alpha-0 texel passes the ray straight through: same direction, same throughput, survival 1
        a0 = g.alpha0
        assert g_o[a0].all() and a0.sum() >= 64
        d = g.rays["direction"][a0, :3]
        assert np.allclose(np.stack([got["ndx"], got["ndy"], got["ndz"]], 1)[a0], d / np.linalg.norm(d, axis=1, keepdims=True), rtol=0, atol=1e-6)
        assert np.allclose(np.stack([got["nthr_r"], got["nthr_g"], got["nthr_b"]], 1)[a0], g.rays["multiplier"][a0, :3], rtol=1e-6)
        assert (got["nflags"][a0] & 2 == 0).all()


@pytest.mark.parametrize("family", G.FAMILIES)
def test_shade_grid_matches_oracle(gpu, family):
    """k_shade<false, false> over one material family of the grid: the stratum gates, finiteness, the structural facts"""
    g = G.grid(family)
    want = G.shade(g, sample=2, seed=4, width=W, height=H)
    got, dt = _shade_on_gpu(gpu, g)
    flips, worst_ray, worst_shadow = _compare(family, g, got, want)
    _structure(g, got)
    deg = g.degenerate & got["out_alive"].astype(bool)
    print(f"shade grid {family}: {g.n} entries in {dt:.2f} s, worst stratum flips {flips}, worst field fraction {worst_ray:.4f} (continuation) "
          f"{worst_shadow:.4f} (shadow), {int(deg.sum())} live continuation rays off degenerate tangent frames")
    assert deg.sum() >= (32 if g.degenerate.any() else 0)


@pytest.mark.parametrize("family", ["pbr dielectric", "pbr metal", "diffuse"])
def test_shade_grid_general_kernel_weighted_lights(gpu, family):
    """k_shade<false, true> (FLAG_SOLID_ANGLE_LIGHTS) on the PBR (dielectric: f0 0 / 0.04 / 1; metal) and diffuse corners against the oracle under
    LIGHTS_SOLID_ANGLE: the same gates (diffuse: the two diffuse materials, without the misses and the emissive hits the default kernel's case has)"""
    g = G.grid(family)
    if family == "diffuse":
        g = G.take(g, np.flatnonzero(g.labels["family"] == "diffuse"))
    tag = "general " + family
    want = G.shade(g, sample=2, seed=4, light_sampling=O.LIGHTS_SOLID_ANGLE, width=W, height=H)
    got, dt = _shade_on_gpu(gpu, g, flags=gpu.FLAG_SOLID_ANGLE_LIGHTS)
    flips, worst_ray, worst_shadow = _compare(tag, g, got, want)
    _structure(g, got)
    print(f"shade grid {tag}: {g.n} entries in {dt:.2f} s, worst stratum flips {flips}, worst field fraction {worst_ray:.4f} / {worst_shadow:.4f}")


def test_axis_aligned_room_renders_like_the_oracle(gpu):
    """64x36, 8 spp, sky bound: the room of exact axis normals (PBR x walls, a rough-glass wall, an instanced turned PBR box).  The accumulator is
    finite; the image is the oracle's at the gates of test_production_render_matches_oracle."""
    flat, cam, sky = G.axis_aligned_room(64, 36)
    spp = 8
    ctx = U.make_ctx(gpu, flat, 64, 36, camera=cam, sky=sky, seed=3, samples_in_flight=1)
    ctx.render(spp)
    a, st = ctx.read_accum(), ctx.stats()
    ctx.close()
    assert np.isfinite(a).all()
    a = a[:, :3]
    ref, cnt = O.render(O.BoundScene(flat, sky=sky), cam, 64, 36, spp, seed=3, threads=8)
    ref = ref[:, :3]
    assert st["rays_generated"] == cnt["raysGenerated"] == 64 * 36 * spp
    for k, ck in (("rays_extension", "raysExtension"), ("rays_shadow", "raysShadow"), ("shade_hits", "shadeHits")):
        assert abs(st[k] - cnt[ck]) <= 1e-3 * cnt[ck] + 2, (k, st[k], cnt[ck])
    U.image_margins("shade grid: axis-aligned PBR / rough-glass room vs the oracle path by path, 64x36, 8 spp", a, ref, spp, cam, 1e-3, 1e-3)
    close = np.isclose(a, ref, rtol=1e-3, atol=1e-3 * ref.max()).all(axis=1)
    U.fraction_gate("shade grid: axis-aligned PBR / rough-glass room, 64x36, 8 spp: pixels within 1e-3", close, MEASURED, legacy=0.97)
