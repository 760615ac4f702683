"""k_shade through pt_shade_batch over the shade grid (tests/shade_grid.py) against the oracle, entry by entry, counter PRNG under identical keys: the
material corners (smoothness 0 / 1 / either side of kMaxSmoothness, ior 1 / kAirIor, f0 0 / 1, total internal reflection), grazing and back-side
incidence either side of kEPS and of the 0.05 cutoff, hits at vertices and edge midpoints, turned, mirrored and quarter-turned instances, and the
axis-aligned normals on which the reference's tangent frame is NaN.  tests/test_shade_grid_cpu.py holds the oracle to the reference on the same entries and
shows that the grid is conditioned: a disagreement beyond the gates here is not round-off.

Under neeMisShading (k_shade<false, true> with FLAG_INTEGRATOR_MIS) the hook carries the path's density word both ways: the same families with a seeded
incoming density, the density written for the next bounce held to the oracle's, the emissive-under-MIS family of the grid, the COMPARE_SHADING split.

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


def _shade_on_gpu(gpu, g, flags=0, in_pdf=None):
    """in_pdf: the incoming density handed to the hook (None: the hook's own default, 0 for every entry)"""
    S = g.scene
    assert g.n <= W * H and int(g.rays["outputPixel"].max()) < W * H and g.prim.max() < len(S.flat.triangles)
    ctx = U.make_ctx(gpu, S.flat, W, H, camera=S.camera, sky=S.sky, tex=S.tex, seed=4, flags=flags)
    t0 = time.time()
    got = ctx.shade_batch(g.rays["origin"][:, :3], g.rays["direction"][:, :3], g.rays["multiplier"][:, :3], g.rays["outputPixel"], g.rays["flags"],
                          g.rays["numBounces"], g.t, g.uv[:, 0], g.uv[:, 1], g.prim, g.inst, sample=2, **({} if in_pdf is None else dict(in_pdf=in_pdf)))
    dt = time.time() - t0
    ctx.close()
    return got, dt


def _compare(tag, g, got, want, npdf=False):
    """the stratum gates; returns (flips, worst continuation fraction, worst shadow fraction) over the strata.
    npdf: the density written for the next bounce is held to the oracle's too, on the entries alive on both sides, at the fields' tolerance"""
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
        if npdf:
            close = np.isclose(got["npdf"][both], want.ray["pdf"][both], rtol=2e-3, atol=2e-4)
            U.fraction_gate(f"shade grid {tag}/{label}: density for the next bounce", close, MEASURED, legacy=0.97)
            if not close.all() and label.startswith("family"):
                for k in both[~close]:
                    print(f"  off: {tag} entry {k} {[g.labels[d][k] for d in g.labels]} npdf: {got['npdf'][k]!r} against {want.ray['pdf'][k]!r}")
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


def _structure(g, got, mis=False):
    """what must hold per family whatever the numbers are (mis: under neeMisShading an emissive hit after a non-specular bounce may deposit)"""
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
    assert np.allclose(got["radiance"][spec], g.rays["multiplier"][spec, :3] * g.colour[spec], rtol=1e-6)
    if mis:  # a balance-heuristic weight in [0, 1) of throughput x colour; nothing without a density of at least kEPS, nothing at bounce 0
        cap = np.where((g.rays["numBounces"] == 0)[:, None], 1.0, g.rays["multiplier"][:, :3]) * g.colour
        rad = got["radiance"][em & ~spec]
        assert (rad >= 0).all() and (rad <= cap[em & ~spec] * (1 + 1e-6)).all()
        assert (got["radiance"][em & ~spec & ((g.rays["numBounces"] == 0) | (g.rays["pdf"] < G.K_EPS))] == 0).all()
    else:
        assert (got["radiance"][em & ~spec] == 0).all()
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


def _density_structure(g, got, want, mis_entries=None):
    """The density k_shade writes for the next bounce, whatever its value: 0 on glass and on the alpha-0 pass-through (materials that take no part in MIS,
    shading.cl:175); finite on every other live continuation; positive wherever the instance leaves the shading normal alone (the identity placement),
    outside the degenerate tangent frames.  It is NOT positive everywhere, in the reference either: the shading normal stays in object space, so under
    a turned instance a DIFFUSE bounce's dot(shadingNormal, reflection) / pi is negative for some directions, and a perfect mirror's D_GGX (alpha = 0) is
    0 wherever the turned halfway vector leaves f above kEPS (tests/test_shade_grid_cpu.py pins both bit for bit against the reference's own build).
    There the sign is the oracle's.  mis_entries: the entries shaded by neeMisShading (all by default); the others carry density 0."""
    mis_entries = np.ones(g.n, bool) if mis_entries is None else mis_entries
    g_o = got["out_alive"].astype(bool)
    fam = g.labels["family"]
    passive = np.isin(fam, ("rough glass", "basic glass")) | g.alpha0 | ~mis_entries
    assert (got["npdf"][g_o & passive] == 0).all(), "glass, the alpha-0 pass-through and neeIsShading carry no density"
    other = g_o & ~passive
    assert np.isfinite(got["npdf"][other]).all()
    sound = other & ~g.degenerate
    identity = sound & np.char.endswith(g.labels["placement"], "/identity")
    assert (got["npdf"][identity] > 0).all(), sorted(set(g.labels["corner"][identity & ~(got["npdf"] > 0)]))
    both = sound & want.ray_alive & (np.abs(want.ray["pdf"]) > 1e-3)  # (five times the comparison's atol: round-off does not carry a density across 0)
    assert np.array_equal(got["npdf"][both] > 0, want.ray["pdf"][both] > 0)
    assert not sound.any() or (identity.sum() >= 16 and (got["npdf"][sound] > 0).sum() >= 64), (int(identity.sum()), int((got["npdf"][sound] > 0).sum()))
    return int(sound.sum()), int((got["npdf"][sound] <= 0).sum())


@pytest.mark.parametrize("family", G.FAMILIES)
def test_shade_grid_mis_matches_oracle(gpu, family):
    """k_shade<false, true> under FLAG_INTEGRATOR_MIS over one material family, the bounce-1 entries carrying a seeded incoming density in [0, 10]
    (shade_grid.seed_in_pdf) through the hook: the stratum gates of the default kernel's test, unchanged, plus the density written for the next bounce
    against the oracle's on the entries alive on both sides; finiteness; the structural facts, those of the density among them."""
    g = G.seed_in_pdf(G.grid(family))
    want = G.shade(g, sample=2, seed=4, integrator=O.INTEGRATOR_MIS, width=W, height=H)
    got, dt = _shade_on_gpu(gpu, g, flags=gpu.FLAG_INTEGRATOR_MIS, in_pdf=g.rays["pdf"])
    tag = "mis " + family
    flips, worst_ray, worst_shadow = _compare(tag, g, got, want, npdf=True)
    _structure(g, got, mis=True)
    n_density, n_not_positive = _density_structure(g, got, want)
    if family == "diffuse":  # the seeded density reaches the emissive branch: this family's emissive hits after a diffuse bounce deposit
        em = g.labels["corner"] == "after a diffuse bounce"
        assert np.array_equal((got["radiance"][em] != 0).any(1), (want.radiance[em] != 0).any(1)) and (got["radiance"][em] != 0).any(1).sum() >= 16
    print(f"shade grid {tag}: {g.n} entries in {dt:.2f} s, worst stratum flips {flips}, worst field fraction {worst_ray:.4f} (continuation) "
          f"{worst_shadow:.4f} (shadow), {n_density} densities for the next bounce, {n_not_positive} of them not positive")


def test_shade_grid_mis_pbr_light_sample_draws_once_more(gpu):
    """neeMisShading draws one more number per PBR light sample (shading.cl:131) than neeIsShading: on a PBR entry with a live shadow ray every later
    draw moves, so the continuation ray of the MIS kernel leaves in another direction than the default kernel's on the SAME entry and keys -- except off a
    perfect mirror (smoothness 1: the GGX halfway vector is the normal whatever was drawn), which is left out.  Without a shadow ray there is no extra
    draw: there both kernels sample the same direction."""
    moved = 0
    for family in ("pbr dielectric", "pbr metal"):
        g = G.seed_in_pdf(G.grid(family))
        mis, _ = _shade_on_gpu(gpu, g, flags=gpu.FLAG_INTEGRATOR_MIS, in_pdf=g.rays["pdf"])
        plain, _ = _shade_on_gpu(gpu, g)
        assert np.array_equal(mis["shadow_alive"], plain["shadow_alive"]), "the light sample's three cosine tests see the same draws"
        assert (plain["npdf"] == 0).all(), "the default kernel carries no density"
        rough = ~np.char.startswith(g.labels["corner"], "s=1")
        d_mis, d_plain = (np.stack([r["ndx"], r["ndy"], r["ndz"]], 1) for r in (mis, plain))
        live = mis["out_alive"].astype(bool) & plain["out_alive"].astype(bool) & rough & ~g.degenerate
        drew = live & mis["shadow_alive"].astype(bool)
        assert drew.sum() >= 32 and (np.abs(d_mis[drew] - d_plain[drew]).max(1) > 1e-4).all(), (family, int(drew.sum()))
        moved += int(drew.sum())
        same = live & ~mis["shadow_alive"].astype(bool)
        unmoved = np.isclose(d_mis[same], d_plain[same], rtol=2e-3, atol=2e-4).all(1)  # (two instantiations of one source: the fields' tolerance)
        assert same.sum() >= 64 and unmoved.mean() >= 0.97, (family, int(same.sum()), float(unmoved.mean()))
        print(f"shade grid mis {family}: {int(drew.sum())} continuation rays moved by the extra draw, {int(same.sum())} without one unmoved")
    assert moved >= 64, moved  # (a live shadow ray AND a live continuation ray off a rough PBR corner: some 3 % of a family)


def test_shade_grid_mis_emissive(gpu):
    """The one branch only neeMisShading has (shading.cl:69-90, pt_shade.h shadeHit), over the emissive-under-MIS family: incoming densities 0, either
    neighbour of kEPS, 1/pi, 1, a GGX peak, 1e7; solid angles far below kEPS, 2 % either side of it, mid-range and clamped at 2 pi; head-on, oblique,
    grazing and back-side hits; every placement and a uniformly scaled one (area in object space, distance in world space); a bounce-0 control.
    The deposit per stratum against the oracle at the radiance tolerance of the other tests; deposit-or-not equal to the oracle's on EVERY entry (the
    grid is conditioned: tests/test_shade_grid_cpu.py); never above throughput x colour; exactly 0 behind the light, below kEPS of density and at
    bounce 0; and nothing at all from the default kernel on the same entries."""
    g = G.grid("emissive mis")
    want = G.shade(g, sample=2, seed=4, integrator=O.INTEGRATOR_MIS, width=W, height=H)
    got, dt = _shade_on_gpu(gpu, g, flags=gpu.FLAG_INTEGRATOR_MIS, in_pdf=g.rays["pdf"])
    rad, lab = got["radiance"], g.labels
    assert np.isfinite(rad).all() and not got["out_alive"].any() and not got["shadow_alive"].any(), "an emissive hit ends the path"
    dep, dep_want = (rad != 0).any(1), (want.radiance != 0).any(1)
    wrong = np.flatnonzero(dep != dep_want)
    for k in wrong[:16]:
        print(f"  off: entry {k} {[lab[d][k] for d in lab]} solid angle {g.solid_angle[k]:.6g} deposit {rad[k]} against {want.radiance[k]}")
    assert wrong.size == 0, f"{wrong.size} entries decide deposit / no deposit unlike the oracle"
    assert dep.sum() >= 512
    cap = g.rays["multiplier"][:, :3] * g.colour
    assert (rad >= 0).all() and (rad <= cap * (1 + 1e-6)).all(), "a balance-heuristic weight lies in [0, 1]"
    for name, stratum in (("behind the light", lab["solid_angle"] == G.BACK_SIDE), ("density kEPS-", lab["in_pdf"] == "kEPS-"),
                          ("density 0", lab["in_pdf"] == "0"), ("bounce 0", lab["in_pdf"] == "0 at bounce 0 (control)"),
                          ("solid angle below kEPS", np.isin(lab["solid_angle"], ("1e-6", "kEPS/1.02")))):
        assert stratum.sum() >= 64 and (rad[stratum] == 0).all(), name
    worst = 1.0
    for label, sl in G.strata(g):
        assert len(sl) >= 64, (label, len(sl))
        close = np.isclose(rad[sl], want.radiance[sl], rtol=2e-3, atol=1e-4).all(axis=1)
        worst = min(worst, U.fraction_gate(f"shade grid mis emissive/{label}: radiance deposited by shade", close, MEASURED, legacy=0.98))
        if label.startswith("family"):
            for k in sl[~close]:
                print(f"  off: entry {k} {[lab[d][k] for d in lab]} radiance {rad[k]} against {want.radiance[k]}")
    plain, _ = _shade_on_gpu(gpu, g, in_pdf=g.rays["pdf"])
    assert (plain["radiance"] == 0).all() and not plain["out_alive"].any(), "neeIsShading: next event estimation has counted this light already"
    print(f"shade grid mis emissive: {g.n} entries in {dt:.2f} s, {int(dep.sum())} deposits, worst stratum fraction {worst:.4f}")


def test_shade_grid_compare_shading_splits_on_the_pixel(gpu):
    """FLAG_COMPARE_SHADING over the PBR dielectric family against the oracle's INTEGRATOR_COMPARE: neeMisShading where pixel % width < width / 2,
    neeIsShading elsewhere.  The reference's COMPARE_SHADING build remaps only the CAMERA ray's x at generation, so that both halves look at the left
    half's view (kernel.cl:48-51); the queue entry keeps the true outputPixel, and shade selects on outputPixel % scrWidth (kernel.cl:249).  The hook's
    pixel IS that outputPixel -- it keys the PRNG, addresses the accumulator and makes this selection -- so the hook expresses both halves faithfully.
    The grid numbers its entries' pixels 0 .. n-1 (take() renumbers them likewise): at width 64 the entries alternate between the halves in runs of 32,
    half of the family in each, every stratum in both."""
    g = G.seed_in_pdf(G.grid("pbr dielectric"))
    left = (g.rays["outputPixel"] % W) < W // 2
    assert abs(int(left.sum()) - g.n // 2) <= 32
    for label, sl in G.strata(g):
        assert min(left[sl].sum(), (~left[sl]).sum()) >= 16, label
    want = G.shade(g, sample=2, seed=4, integrator=O.INTEGRATOR_COMPARE, width=W, height=H)
    got, dt = _shade_on_gpu(gpu, g, flags=gpu.FLAG_COMPARE_SHADING, in_pdf=g.rays["pdf"])
    flips, worst_ray, worst_shadow = _compare("compare pbr dielectric", g, got, want, npdf=True)
    _structure(g, got, mis=True)
    _density_structure(g, got, want, mis_entries=left)
    g_o = got["out_alive"].astype(bool)
    assert (want.ray["pdf"][want.ray_alive & ~left] == 0).all() and (got["npdf"][g_o & left & ~g.degenerate] != 0).sum() >= 64
    print(f"shade grid compare pbr dielectric: {g.n} entries in {dt:.2f} s, {int(left.sum())} in the MIS half, worst stratum flips {flips}, "
          f"worst field fraction {worst_ray:.4f} / {worst_shadow:.4f}")


def test_shade_grid_mis_with_weighted_lights(gpu):
    """FLAG_INTEGRATOR_MIS | FLAG_SOLID_ANGLE_LIGHTS over the PBR metal family against the oracle under INTEGRATOR_MIS and LIGHTS_SOLID_ANGLE: the same gates"""
    g = G.seed_in_pdf(G.grid("pbr metal"))
    want = G.shade(g, sample=2, seed=4, integrator=O.INTEGRATOR_MIS, light_sampling=O.LIGHTS_SOLID_ANGLE, width=W, height=H)
    got, dt = _shade_on_gpu(gpu, g, flags=gpu.FLAG_INTEGRATOR_MIS | gpu.FLAG_SOLID_ANGLE_LIGHTS, in_pdf=g.rays["pdf"])
    flips, worst_ray, worst_shadow = _compare("mis general pbr metal", g, got, want, npdf=True)
    _structure(g, got, mis=True)
    _density_structure(g, got, want)
    print(f"shade grid mis general pbr metal: {g.n} entries in {dt:.2f} s, worst stratum flips {flips}, worst field fraction {worst_ray:.4f} / {worst_shadow:.4f}")


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
