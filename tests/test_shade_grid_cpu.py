"""The shade grid (tests/shade_grid.py) on the CPU: the oracle against the reference's own shade kernel entry by entry, the finiteness of everything
the oracle emits, and the conditioning of the grid -- the condition under which the gates of tests/test_gpu_shade_grid.py mean something."""
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


def test_grid_covers_what_it_says():
    """every stratum holds at least 64 entries; the corners are the ones the materials were asked for; both sides of kMaxSmoothness are one float apart"""
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


def test_grid_is_conditioned(counter_mode, fast_oracle):
    """Two correct builds of the same code -- strict (no contraction, baseline x86-64) and -O3 -march=native (FMA contraction) -- agree over the whole grid:
    no alive / finished flip, every field within the tolerances the GPU test uses.  The grid holds no value within round-off of a threshold; a
    disagreement between k_shade and the oracle beyond the GPU test's gates is then not round-off."""
    differing = 0
    for f, (g, a) in counter_mode.items():
        b = G.shade(g, fast=True)
        differing += int((_bits(a.ray["direction"][a.ray_alive][:, :3]) != _bits(b.ray["direction"][a.ray_alive][:, :3])).any(1).sum())
        assert np.array_equal(a.ray_alive, b.ray_alive) and np.array_equal(a.shadow_alive, b.shadow_alive), f
        assert np.array_equal(a.ray["flags"], b.ray["flags"]), f
        for fld, _ in G.RAY_FIELDS:
            assert np.allclose(a.ray[fld][a.ray_alive][:, :3], b.ray[fld][a.ray_alive][:, :3], rtol=2e-3, atol=2e-4), (f, fld)
            assert np.allclose(a.shadow[fld][a.shadow_alive][:, :3], b.shadow[fld][a.shadow_alive][:, :3], rtol=2e-3, atol=2e-4), (f, fld)
        assert np.allclose(a.shadow["rayLength"][a.shadow_alive], b.shadow["rayLength"][a.shadow_alive], rtol=1e-4, atol=1e-5), f
        assert np.allclose(a.radiance, b.radiance, rtol=2e-3, atol=1e-4), f

    # the comparison means something only if the two builds ARE two: on a host whose -march=native contracts nothing they would be one build
    assert differing >= 100, f"only {differing} continuation directions differ in any bit between the strict and the -march=native oracle: no second build"
