"""The shade grid (tests/shade_grid.py) on the CPU: the oracle against the reference's own shade kernel entry by entry, the finiteness of everything
the oracle emits, and the conditioning of the grid -- the condition under which the gates of tests/test_gpu_shade_grid.py mean something.  Each of
them under both integrators: neeIsShading, and neeMisShading with the incoming density every entry carries and the emissive-under-MIS family."""
import numpy as np
import pytest

import orclib as O
import shade_grid as G


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _finite(rec, shadow):
    ok = np.isfinite(rec["origin"][:, :3]).all(1) & np.isfinite(rec["direction"][:, :3]).all(1) & np.isfinite(rec["multiplier"][:, :3]).all(1)
    return ok & np.isfinite(rec["rayLength"]) if shadow else ok


@pytest.fixture(scope="module")
def counter_mode():
    """every family shaded once by the strict oracle in counter mode (shared, read-only)"""
    return {f: (g, G.shade(g)) for f, g in ((f, G.grid(f)) for f in G.FAMILIES)}


MIS_FAMILIES = G.FAMILIES + ("emissive mis",)


def mis_grid(family):
    """the grid of `family` as every MIS test sees it: the five material families with a seeded incoming density on their bounce-1 entries, the
    emissive-under-MIS family with its own ladder"""
    return G.grid(family) if family == "emissive mis" else G.seed_in_pdf(G.grid(family))


@pytest.fixture(scope="module")
def mis_mode():
    """every family and the emissive-under-MIS family shaded once by the strict oracle under INTEGRATOR_MIS in counter mode (shared, read-only)"""
    return {f: (g, G.shade(g, integrator=O.INTEGRATOR_MIS)) for f, g in ((f, mis_grid(f)) for f in MIS_FAMILIES)}


def test_grid_covers_what_it_says():
    """every stratum holds at least 64 entries; the corners are the ones the materials were asked for; both sides of kMaxSmoothness are one float apart;
    the emissive-under-MIS family (_emissive_mis_family_covers_what_it_says)"""
    assert np.float32(G.BELOW) < G.K_MAX_SMOOTHNESS < np.float32(G.ABOVE) and np.nextafter(G.BELOW, np.float32(1)) == G.K_MAX_SMOOTHNESS
    total = 0
    for f in G.FAMILIES:
        g = G.grid(f)
        total += g.n
        assert g.n <= 3000
        for label, idx in G.strata(g):
            assert len(idx) >= 64, (f, label, len(idx))
        want = {m[1] for m in G.MATERIALS if m[0] == f}
        assert want <= set(g.labels["corner"]), want - set(g.labels["corner"])
        seeded = f in ("pbr dielectric", "pbr metal", "rough glass")
        assert (g.degenerate.sum() >= 64) == seeded, (f, int(g.degenerate.sum()))
        assert {p.split("/")[0] for p in g.labels["placement"][g.degenerate]} <= {"axis"}
        if seeded:  # under every placement: the shading normal stays in object space, whatever the instance's rotation
            assert {p.split("/")[1] for p in g.labels["placement"][g.degenerate]} == set(G.PLACEMENTS)
    g = G.grid("diffuse")
    assert g.alpha0.sum() >= 64 and ((g.labels["corner"] == "textured") & ~g.alpha0).sum() >= 64
    assert (g.labels["family"] == "miss").sum() == G.N_MISS and (g.labels["family"] == "emissive").sum() == 2 * G.N_EMISSIVE
    print(f"{total} entries")
    # a seeded density: bounce 0 keeps 0, bounce 1 gets U(0, 10); nothing else of the grid moves
    s = G.seed_in_pdf(g)
    assert (g.rays["pdf"] == 0).all() and (s.rays["pdf"][s.rays["numBounces"] == 0] == 0).all()
    seeded = s.rays["pdf"][s.rays["numBounces"] != 0]
    assert (seeded >= 0).all() and seeded.max() <= 10 and seeded.max() > 9 and ((seeded > 0) & (seeded < G.K_EPS)).sum() == 0
    held = (s.rays["numBounces"] != 0) & (s.rays["pdf"] == 0)  # (seed_in_pdf: the emissive hits at cosines of 5e-5 and below keep 0)
    assert set(s.labels["family"][held]) <= {"emissive"} and held.sum() <= 64 and ((s.labels["family"] == "emissive") & (s.rays["pdf"] > 0)).sum() >= 64
    t = s.rays.copy()
    t["pdf"] = 0
    assert np.array_equal(t, g.rays) and np.array_equal(s.prim, g.prim)
    _emissive_mis_family_covers_what_it_says()


def _emissive_mis_family_covers_what_it_says():
    """The emissive-under-MIS family: sizes, the exact neighbours of kEPS in the incoming density, the solid-angle rungs realised (float64 from the fp32
    inputs), the scaled placement, and on either side of either threshold at least 64 entries that the threshold ALONE decides: every other condition
    of the deposit holds for them, they deposit on the one side (by the oracle) and do not on the other."""
    g = G.grid("emissive mis")
    assert g.n == G.N_EMISSIVE_MIS + G.N_EMISSIVE_MIS_CONTROL <= 3000 and g.hit.all()
    for label, idx in G.strata(g):
        assert len(idx) >= 64, (label, len(idx))
    assert {"in_pdf", "solid_angle"} <= set(g.labels) and (g.rays["flags"] == 0).all()
    ctl = g.labels["in_pdf"] == "0 at bounce 0 (control)"
    assert np.array_equal(ctl, g.rays["numBounces"] == 0) and ctl.sum() == G.N_EMISSIVE_MIS_CONTROL and (g.rays["numBounces"][~ctl] == 1).all()
    assert (g.rays["pdf"][ctl] == 0).all() and (g.rays["multiplier"][ctl, :3] == 1).all() and (g.solid_angle[ctl] > 1.01e-4).all()
    thr = g.rays["multiplier"][~ctl, :3]
    assert thr.min() >= 0.1 and thr.max() <= 1
    # the density ladder, bit for bit
    pdf = g.rays["pdf"]
    eps = np.float32(1e-4)
    rung = {name: val for name, val in G.IN_PDF_LADDER}
    assert set(g.labels["in_pdf"][~ctl]) == set(rung) and len(rung) == 7
    for name, val in rung.items():
        assert (pdf[g.labels["in_pdf"] == name] == val).all() and pdf[g.labels["in_pdf"] == name].dtype == np.float32
    assert rung["kEPS-"] < eps < rung["kEPS+"] and np.nextafter(rung["kEPS-"], np.float32(1)) == eps == np.nextafter(rung["kEPS+"], np.float32(0))
    assert rung["0"] == 0 and rung["1"] == 1 and abs(rung["1/pi"] * np.pi - 1) < 1e-6 and rung["1e7"] == 1e7
    assert abs(rung["GGX peak of s=0.94"] - 1 / (np.pi * 0.06 ** 2)) < 1e-3 * 88 and abs(G.d_ggx(1.0, 0.06) - 88.42) < 0.01
    # the solid-angle ladder as realised
    sa, lab = g.solid_angle, g.labels["solid_angle"]
    back = lab == G.BACK_SIDE
    assert np.array_equal(back, sa < 0) and np.array_equal(back, np.char.startswith(g.labels["incidence"], "cos=-")) and back.sum() >= 64
    for name, val in G.SOLID_ANGLE_LADDER:
        assert np.allclose(sa[lab == name], val, rtol=2e-3, atol=0), name  # (the cosine of the 2e-4 rung is good to 1e-3 in fp32 inputs)
    assert (sa[lab == "1e-6"] < 1e-5).all() and (sa[lab == "20, clamped to 2 pi"] > 2 * np.pi).all()
    assert sa[lab == "kEPS/1.02"].max() < 1e-4 < sa[lab == "kEPS*1.02"].min()
    assert {"cos=0.01", "cos=0.0002"} <= set(g.labels["incidence"]), "grazing front-side hits"
    # every placement of the grid and the scaled one, on both meshes
    assert set(g.labels["placement"]) == {f"{m}/{p}" for m in ("axis", "tilt") for p in (*G.PLACEMENTS, *G.EXTRA_PLACEMENTS)}
    for key, w in g.scene.where.items():
        if key[1] in G.EXTRA_PLACEMENTS:
            assert np.allclose(w["M"][:3, :3], 0.5 * np.eye(3), atol=1e-6), "a pure uniform scale that is not 1"
    # the thresholds: who deposits, by the oracle
    dep = (G.shade(g, integrator=O.INTEGRATOR_MIS).radiance != 0).any(1)
    assert np.array_equal(dep, (sa > 1e-4) & ~(pdf < eps) & ~ctl), "the deposit is the conjunction of the two thresholds"
    pdf_ok, sa_ok = ~ctl & (pdf > eps), ~back & (sa > 1e-4)
    for name, side, deposits in (("solid angle above", pdf_ok & (lab == "kEPS*1.02"), True), ("solid angle below", pdf_ok & (lab == "kEPS/1.02"), False),
                                 ("density above", sa_ok & (g.labels["in_pdf"] == "kEPS+"), True),
                                 ("density below", sa_ok & (g.labels["in_pdf"] == "kEPS-"), False)):
        assert side.sum() >= 64 and (dep[side] == deposits).all(), (name, int(side.sum()), int(dep[side].sum()))
        print(f"{name} kEPS: {int(side.sum())} entries the threshold alone decides, {int(dep[side].sum())} deposit")
    assert (dep & (lab == "20, clamped to 2 pi")).sum() >= 64 and (dep & (g.labels["placement"] == "axis/scaled 0.5")).sum() >= 32


@pytest.mark.parametrize("family", MIS_FAMILIES)
def test_oracle_mis_equals_the_reference_compare_build_bit_for_bit(family):
    """neeMisShading entry by entry: the reference's COMPARE_SHADING build shades outputPixel % width < width / 2 with it, so the queue is handed over
    with width = twice its length and height 1 -- every entry's pixel lies in the MIS half.  The oracle runs INTEGRATOR_COMPARE_AS_COMPILED under the
    same width (the reference's uninitialised DIFFUSE density read as what its build makes of it, dot(shadingNormal, rayDirection) / pi: oracle.cpp,
    neeShading -- the grid meets diffuse surfaces from behind and under turned instances, where that is positive; whole images had read it as 0).  LFSR113, stream k for
    slot k on both sides, the incoming density of mis_grid: flags, every field of every live continuation ray -- the density written for the next
    bounce among them -- and of every live shadow ray, the accumulator and the stream states (= the number of draws, the extra one per PBR light sample
    included) are equal BIT FOR BIT on every entry outside the degenerate tangent frames; inside them the reference's continuation is non-finite and the
    oracle's finite, shadow ray and radiance are equal.  No other stratum is non-finite in the reference under MIS either."""
    if not O.have_ref_mis():
        pytest.skip("oracle/_ref not built (reference tree absent)")
    g = mis_grid(family)
    width = 2 * ((g.n + 63) // 64 * 64)
    ref = G.shade(g, "ref", width=width, height=1, compare_build=True)
    orc = G.shade(g, "oracle", rng_mode=O.RNG_LFSR113, width=width, height=1, integrator=O.INTEGRATOR_COMPARE_AS_COMPILED)
    sound = ~g.degenerate
    assert np.array_equal(ref.ray["flags"][sound], orc.ray["flags"][sound])
    assert np.array_equal(ref.shadow["flags"], orc.shadow["flags"])
    assert np.array_equal(ref.ray["numBounces"][sound], orc.ray["numBounces"][sound])
    live = ref.ray_alive & sound
    assert live.sum() >= (64 if family != "emissive mis" else 0)
    for f, _ in G.RAY_FIELDS:
        assert np.array_equal(_bits(ref.ray[f][live][:, :3]), _bits(orc.ray[f][live][:, :3])), f
        assert np.array_equal(_bits(ref.shadow[f][ref.shadow_alive][:, :3]), _bits(orc.shadow[f][ref.shadow_alive][:, :3])), f
    assert np.array_equal(_bits(ref.ray["pdf"][live]), _bits(orc.ray["pdf"][live])), "the density written for the next bounce"
    assert np.array_equal(_bits(ref.shadow["rayLength"][ref.shadow_alive]), _bits(orc.shadow["rayLength"][ref.shadow_alive]))
    assert np.array_equal(_bits(ref.radiance), _bits(orc.radiance))
    assert np.array_equal(ref.streams[sound], orc.streams[sound])
    bad_ray, bad_shadow = ref.ray_alive & ~(_finite(ref.ray, False) & np.isfinite(ref.ray["pdf"])), ref.shadow_alive & ~_finite(ref.shadow, True)
    assert not bad_shadow.any() and np.isfinite(ref.radiance).all()
    assert np.array_equal(bad_ray, ref.ray_alive & g.degenerate), (int(bad_ray.sum()), int((ref.ray_alive & g.degenerate).sum()))
    if g.degenerate.any():
        assert _finite(orc.ray, False)[orc.ray_alive & g.degenerate].all() and (orc.ray_alive & g.degenerate).sum() >= 32
    if family == "emissive mis":
        assert ((ref.radiance != 0).any(1)).sum() >= 512 and not ref.ray_alive.any() and not ref.shadow_alive.any()
    if family == "diffuse":  # the seeded density reaches the branch: emissive hits after a diffuse bounce deposit under MIS, and only at bounce 1
        em = (g.labels["corner"] == "after a diffuse bounce")
        assert not (ref.radiance[em] != 0).any(1)[g.rays["numBounces"][em] == 0].any() and (ref.radiance[em] != 0).any(1).sum() >= 16
    if family in ("pbr dielectric", "pbr metal"):  # the extra draw: the same entries under the IS build end on other stream states
        plain = G.shade(g, "ref", width=width, height=1)
        moved = (plain.streams != ref.streams).any(1) if plain.streams.ndim > 1 else plain.streams != ref.streams
        assert (moved & ref.shadow_alive).sum() >= 64


def test_fixed_mis_oracle_differs_from_the_as_compiled_one_only_in_the_diffuse_density(mis_mode):
    """INTEGRATOR_MIS takes the DIFFUSE continuation's density from the direction it has just sampled; INTEGRATOR_MIS_AS_COMPILED stores what
    the reference's build makes of its read-before-assignment (shading.cl:590-592), the cosine of the INCOMING direction over pi.  Counter mode, every family: that word of the live DIFFUSE
    continuations that are no alpha-0 pass-through is all that differs -- no flag, no other field, no deposit, no other live ray's density (a
    continuation that ended has no fields)."""
    for f, (g, a) in mis_mode.items():
        b = G.shade(g, integrator=O.INTEGRATOR_MIS_AS_COMPILED)
        assert np.array_equal(a.ray["flags"], b.ray["flags"]) and np.array_equal(a.shadow["flags"], b.shadow["flags"]), f
        for fld, _ in G.RAY_FIELDS:
            assert np.array_equal(_bits(a.ray[fld]), _bits(b.ray[fld])) and np.array_equal(_bits(a.shadow[fld]), _bits(b.shadow[fld])), (f, fld)
        assert np.array_equal(_bits(a.shadow["rayLength"]), _bits(b.shadow["rayLength"])) and np.array_equal(_bits(a.radiance), _bits(b.radiance)), f
        diffuse = a.ray_alive & (g.labels["family"] == "diffuse") & ~g.alpha0
        assert np.array_equal(_bits(a.ray["pdf"][a.ray_alive & ~diffuse]), _bits(b.ray["pdf"][a.ray_alive & ~diffuse])), f
        assert (b.ray["pdf"][diffuse] != a.ray["pdf"][diffuse]).all(), f
        assert diffuse.sum() >= (64 if f == "diffuse" else 0) and (f == "diffuse" or not diffuse.any())


def test_every_live_output_of_the_mis_oracle_is_finite(mis_mode):
    """counter mode, INTEGRATOR_MIS, every family and the emissive-under-MIS one: continuation rays with the density they carry on, shadow rays,
    deposits.  D_GGX is finite at smoothness exactly 1 too: alpha^2 = 0 gives 0 / (pi f^2) = 0 while f > kEPS and the constant 1 below it."""
    for f, (g, r) in mis_mode.items():
        ok = _finite(r.ray, False) & np.isfinite(r.ray["pdf"])
        assert ok[r.ray_alive].all(), (f, g.labels["corner"][r.ray_alive & ~ok][:8])
        assert _finite(r.shadow, True)[r.shadow_alive].all(), f
        assert np.isfinite(r.radiance).all(), f
        assert (r.ray_alive & g.degenerate).sum() >= (32 if g.degenerate.any() else 0), "the degenerate frames go on as paths"


@pytest.mark.parametrize("exact_rungs", [True, False], ids=["the ladder's exact rungs", "the conditioned rungs"])
@pytest.mark.parametrize("family", G.FAMILIES)
def test_oracle_equals_the_reference_shade_bit_for_bit(family, exact_rungs):
    """On the ladder exactly as written -- cos = 0 is 0, +-1 is +-1, rough glass included: this comparison is deterministic and needs no conditioning --
    and on the grid the conditioning and GPU tests use (three rungs moved off round-off's reach, shade_grid.py).  LFSR113, stream k for slot k on
    both sides: flags, every field of every live continuation and shadow ray, the accumulator and the stream states
    (= the number of draws) are equal BIT FOR BIT (a NaN would have to be the same NaN) on every entry outside the degenerate tangent frames.  Inside
    them -- PBR and rough glass on an object-space normal of exactly +-x -- every live continuation ray of the reference is non-finite and every one of
    the oracle is finite (oracle.cpp, orient: FIXED); the shadow ray and the radiance, which shade settles before it samples the continuation, are equal
    there too.  No other stratum of the grid is non-finite in the reference."""
    if not O.have_ref():  # (asked here, not at collection: the session's build makes oracle/_ref where the reference tree is)
        pytest.skip("oracle/_ref not built (reference tree absent)")
    g = G.grid(family, exact_rungs=exact_rungs)
    assert ("cos=0" in set(g.labels["incidence"])) == exact_rungs and ("cos=1" in set(g.labels["incidence"])) == (exact_rungs or family != "rough glass")
    ref, orc = G.shade(g, "ref"), G.shade(g, "oracle", rng_mode=O.RNG_LFSR113)
    sound = ~g.degenerate
    assert np.array_equal(ref.ray["flags"][sound], orc.ray["flags"][sound])
    assert np.array_equal(ref.shadow["flags"], orc.shadow["flags"])
    assert np.array_equal(ref.ray["numBounces"][sound], orc.ray["numBounces"][sound])
    live = ref.ray_alive & sound
    assert live.sum() >= 64
    for f, _ in G.RAY_FIELDS:
        assert np.array_equal(_bits(ref.ray[f][live][:, :3]), _bits(orc.ray[f][live][:, :3])), f
        assert np.array_equal(_bits(ref.shadow[f][ref.shadow_alive][:, :3]), _bits(orc.shadow[f][ref.shadow_alive][:, :3])), f
    assert np.array_equal(_bits(ref.shadow["rayLength"][ref.shadow_alive]), _bits(orc.shadow["rayLength"][ref.shadow_alive]))
    assert np.array_equal(_bits(ref.radiance), _bits(orc.radiance))
    assert np.array_equal(ref.streams[sound], orc.streams[sound])
    # the reference's own non-finite outputs: the degenerate tangent frames, all of them, and nothing else
    bad_ray, bad_shadow = ref.ray_alive & ~_finite(ref.ray, False), ref.shadow_alive & ~_finite(ref.shadow, True)
    assert not bad_shadow.any() and np.isfinite(ref.radiance).all()
    assert np.array_equal(bad_ray, ref.ray_alive & g.degenerate), (int(bad_ray.sum()), int((ref.ray_alive & g.degenerate).sum()))
    if g.degenerate.any():
        assert np.array_equal(ref.ray_alive[g.degenerate], np.ones(int(g.degenerate.sum()), bool)), "no comparison ends a NaN path"
        assert _finite(orc.ray, False)[orc.ray_alive & g.degenerate].all() and (orc.ray_alive & g.degenerate).sum() >= 32


def test_rough_glass_at_exactly_normal_incidence_ends_paths_as_the_reference_does():
    """SURVEY 8a quirk 10, pinned.  G_SmithBeckmannCorrelated takes tan(acos(x)) of x = |N . I| and of x = |N . O| (refract.cl:116-134); at exactly normal
    incidence both are 1 to round-off, and where one rounds to 1 + 1 ulp the term is NaN, the weight 0 and the path ends.  Entry k of grid(seed,
    exact_rungs=True) and of grid(seed) is the same hit record under the same LFSR113 stream, at cos = +-1 in the first and +-0.9999 in the second: a path
    that goes on at 0.9999 with a throughput factor >= 1 (survival probability 1: no roulette can end it) and ENDS at exactly +-1 ended by that NaN.  The
    reference's own kernel does this, the oracle does exactly the same (every flag, every live field and every stream state of the rung equal bit for
    bit), and it happens only where the object-space shading normal is also the world's (identity; the quarter turn's z faces)."""
    if not O.have_ref():
        pytest.skip("oracle/_ref not built (reference tree absent)")
    events = 0
    for seed in (1, 2, 3, 4):
        ge, gc = G.grid("rough glass", seed=seed, exact_rungs=True), G.grid("rough glass", seed=seed)
        assert all(np.array_equal(getattr(ge, k), getattr(gc, k)) for k in ("prim", "inst", "uv", "t")), "the same hit records"
        rung = np.isin(ge.labels["incidence"], ("cos=1", "cos=-1")) & ~ge.degenerate
        assert rung.sum() >= 128
        ref, orc, off = G.shade(ge, "ref"), G.shade(ge, "oracle", rng_mode=O.RNG_LFSR113), G.shade(gc, "ref")
        assert np.array_equal(ref.ray["flags"][rung], orc.ray["flags"][rung]) and np.array_equal(ref.streams[rung], orc.streams[rung])
        live = rung & ref.ray_alive
        for f, _ in G.RAY_FIELDS:
            assert np.array_equal(_bits(ref.ray[f][live][:, :3]), _bits(orc.ray[f][live][:, :3])), f
        ended = rung & ~ref.ray_alive & off.ray_alive & (off.ray["multiplier"][:, :3].max(1) >= 1)
        assert np.array_equal(ended, rung & ~orc.ray_alive & off.ray_alive & (off.ray["multiplier"][:, :3].max(1) >= 1))
        assert all(p.endswith(("/identity", "/quarter turn z")) for p in ge.labels["placement"][ended]), ge.labels["placement"][ended]
        events += int(ended.sum())
    assert events >= 1, "no path of four grids ended at exactly normal incidence"
    print(f"{events} paths end at exactly normal incidence and go on at cos = 0.9999")


def test_every_live_output_of_the_oracle_is_finite(counter_mode):
    """counter mode, the whole grid: continuation rays, shadow rays, deposits"""
    for f, (g, r) in counter_mode.items():
        assert _finite(r.ray, False)[r.ray_alive].all(), (f, g.labels["corner"][r.ray_alive & ~_finite(r.ray, False)][:8])
        assert _finite(r.shadow, True)[r.shadow_alive].all(), f
        assert np.isfinite(r.radiance).all(), f
        assert (r.ray_alive & g.degenerate).sum() >= (32 if g.degenerate.any() else 0), "the degenerate frames go on as paths"


def test_axis_aligned_room_renders_finite():
    """64x36, 8 spp: a room of exact axis normals whose x walls are PBR, with a rough-glass wall and an instanced, turned PBR box"""
    flat, cam, sky = G.axis_aligned_room()
    acc, cnt = O.render(O.BoundScene(flat, sky=sky), cam, 64, 36, 8, seed=1, threads=4)
    assert np.isfinite(acc).all() and acc[:, :3].mean() > 0 and cnt["shadeHits"] > 64 * 36 * 8


@pytest.fixture(scope="module")
def fast_oracle():
    """the -O3 -march=native build of the oracle (bench.py's CPU baseline), made where it is missing or stale"""
    O.build(fast=True, ref=False)
    return O.oracle(fast=True)


def _nee_ggx_f(g, r):
    """D_GGX's argument f = (N.H)^2 (alpha^2 - 1) + 1 (pbr_brdf.cl:101) of the MIS light sample's density, float64, for the PBR entries with a live
    shadow ray (H: the halfway vector of -D and the shadow ray's direction; N: the object-space shading normal): (entries, f)"""
    idx = np.flatnonzero(r.shadow_alive & np.isin(g.labels["family"], ("pbr dielectric", "pbr metal")))
    smooth = np.array([dict(G.SMOOTHNESS)[c.split()[0][2:]] for c in g.labels["corner"][idx]], np.float64)
    d = g.rays["direction"][idx, :3].astype(np.float64)
    h = -d / np.linalg.norm(d, axis=1, keepdims=True) + r.shadow["direction"][idx, :3].astype(np.float64)
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    n = g.shading_normal[idx].astype(np.float64)
    ndoth = (n / np.linalg.norm(n, axis=1, keepdims=True) * h).sum(1)
    return idx, ndoth * ndoth * ((1 - smooth) ** 2 - 1) + 1


def test_grid_is_conditioned(counter_mode, mis_mode, fast_oracle):
    """Two correct builds of the same code -- strict (no contraction, baseline x86-64) and -O3 -march=native (FMA contraction) -- agree over the whole grid
    under either integrator (MIS: with the seeded incoming density, and over the emissive-under-MIS family too): no alive / finished flip, no
    deposit-or-not flip, every field -- the density written for the next bounce included -- within the tolerances the GPU test uses.  The grid holds no
    value within round-off of a threshold; a disagreement between k_shade and the oracle beyond the GPU test's gates is then not round-off.
    Under MIS two more computed values meet kEPS: the solid angle of an emissive hit, and f in D_GGX (below it the density jumps to the constant 1).
    Neither comes within a hundred times its round-off of kEPS on any entry (float64 from the fp32 inputs)."""
    differing = 0
    for integrator, shaded in ((O.INTEGRATOR_IS, counter_mode), (O.INTEGRATOR_MIS, mis_mode)):
        for f, (g, a) in shaded.items():
            b = G.shade(g, fast=True, integrator=integrator)
            differing += int((_bits(a.ray["direction"][a.ray_alive][:, :3]) != _bits(b.ray["direction"][a.ray_alive][:, :3])).any(1).sum())
            assert np.array_equal(a.ray_alive, b.ray_alive) and np.array_equal(a.shadow_alive, b.shadow_alive), f
            assert np.array_equal(a.ray["flags"], b.ray["flags"]), f
            assert np.array_equal((a.radiance != 0).any(1), (b.radiance != 0).any(1)), (f, "deposit or not")
            for fld, _ in G.RAY_FIELDS:
                assert np.allclose(a.ray[fld][a.ray_alive][:, :3], b.ray[fld][a.ray_alive][:, :3], rtol=2e-3, atol=2e-4), (f, fld)
                assert np.allclose(a.shadow[fld][a.shadow_alive][:, :3], b.shadow[fld][a.shadow_alive][:, :3], rtol=2e-3, atol=2e-4), (f, fld)
            assert np.allclose(a.ray["pdf"][a.ray_alive], b.ray["pdf"][a.ray_alive], rtol=2e-3, atol=2e-4), (f, "pdf")
            assert np.allclose(a.shadow["rayLength"][a.shadow_alive], b.shadow["rayLength"][a.shadow_alive], rtol=1e-4, atol=1e-5), f
            assert np.allclose(a.radiance, b.radiance, rtol=2e-3, atol=1e-4), f
    # the comparison means something only if the two builds ARE two: on a host whose -march=native contracts nothing they would be one build
    assert differing >= 200, f"only {differing} continuation directions differ in any bit between the strict and the -march=native oracle: no second build"

    # the solid angle: a quotient of fp32 products, good to some 1e-6 relative, 1e-3 at the cosine rung 2e-4 (an absolute 1e-7 of a dot product)
    g = mis_mode["emissive mis"][0]
    assert (np.abs(g.solid_angle / 1e-4 - 1) > 0.015).all(), float(np.abs(g.solid_angle / 1e-4 - 1).min())
    assert (np.abs(g.solid_angle[~np.isin(g.labels["incidence"], ("cos=0.0002",))] / 1e-4 - 1) > 0.0195).all()
    # f: 1 - (N.H)^2 where alpha = 0, good to an absolute 2e-7; above alpha^2 >= 9e-4 for every other corner
    seen = 0
    for f in ("pbr dielectric", "pbr metal"):
        g, a = mis_mode[f]
        idx, ggx_f = _nee_ggx_f(g, a)
        assert idx.size >= 64 and (np.abs(ggx_f - 1e-4) > 2e-5).all(), (f, float(np.abs(ggx_f - 1e-4).min()))
        mirror = np.char.startswith(g.labels["corner"][idx], "s=1")
        assert (ggx_f[~mirror] >= 8.9e-4).all() and mirror.sum() >= 32
        seen += int((ggx_f[mirror] < 1e-4).sum())
        print(f"{f}: {idx.size} MIS light samples, f within [{ggx_f.min():.3g}, {ggx_f.max():.3g}], {int((ggx_f[mirror] < 1e-4).sum())} below kEPS")
    print(f"{seen} light samples take D_GGX's constant branch")
