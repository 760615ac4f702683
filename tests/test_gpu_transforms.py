"""The traversal kernels (pt_trace.h, pt_team.h, pt_packet.h, pt_packet_multi.h; shared steps in pt_walk.h) where the other GPU tests never take them:
mirrored, sheared and strongly non-uniformly scaled instances, instances a thousand times smaller and eight times larger than their neighbours, whole
scenes in units a million times smaller and larger, directions of any length, axis-parallel rays in a large scene, zero-area triangles inside a mesh --
against the oracle, which tests/test_transforms_cpu.py holds against float64 brute force on the same inputs and proves exactly equivariant under a
change of units.  An absolute epsilon or an assumption about a transform's sign in one of these kernels fails here."""
import functools

import numpy as np
import pytest

import gpu_util as U
import orclib as O
from ptamd import host as H, scenes

pytestmark = pytest.mark.gpu

MODES = U.MODES
# fractions of pixels within tolerance of the oracle as measured on the MI355X (profiles/round6/parity_margins.json): gpu_util.fraction_gate holds every such
# comparison against 0.98 x its entry here, and never below 0.97
MEASURED = {
    'zoo room vs the oracle, IS, copied: pixels within 1e-3 of the oracle': 1.0000,
    'zoo room vs the oracle, IS, entered: pixels within 1e-3 of the oracle': 1.0000,
    'zoo room vs the oracle, MIS, copied: pixels within 1e-3 of the oracle': 1.0000,
    'zoo room vs the oracle, MIS, entered: pixels within 1e-3 of the oracle': 1.0000,
}
N_RAYS = 20000
COPIED = dict(edge_flip_frac=5e-4, t_outlier_frac=5e-4, uv_atol=5e-2)  # world-space copies round a triangle's edges in another space than the reference
BUILDERS = {"sah": H.BVH_BINNED_SAH, "fast": H.BVH_BINNED_FAST, "sbvh": H.BVH_SPATIAL_SPLIT}


@functools.lru_cache(maxsize=None)
def _zoo(kind, thin=False):
    return scenes.transform_zoo(kind, 96, 54, thin_lens=thin)


@functools.lru_cache(maxsize=None)
def _grid():
    return scenes.instanced_grid(64, 36, level=3, sky_size=(16, 8), rotate=True)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(bundle, origins, directions, shadow-ray lengths, the oracle's closest hits, the oracle's occlusion verdicts) at unit scale: computed once, shared, never written to"""
    if name == "grid":
        b = _grid()
        o, d = U.random_rays(N_RAYS, 5, (-4, 0.05, -4), (4, 3, 4))
    else:
        b = _zoo(name)
        o, d = U.zoo_rays(b, N_RAYS, 51)
    tmax = np.random.default_rng(1).uniform(0.05, 6, len(o)).astype(np.float32)
    sc = U.oracle_scene(b)
    want, occ = O.intersect_batch(sc, o, d, threads=8), O.intersect_batch(sc, o, d, tmax=tmax, any_hit=True, threads=8)["prim"]
    for a in (o, d, tmax, occ, *want.values()):
        a.setflags(write=False)
    return b, o, d, tmax, want, occ


def _against_the_oracle(flat, mode, got, want, occ_got, occ_want, grid=False):
    """The tolerances the existing tests give the same route (tests/test_gpu_intersect.py): entered instances compare_hits' defaults, world-space copies a few
    edge-grazing rays; occlusion verdicts may differ for three rays beyond those."""
    if U.entered(mode):
        info = U.compare_hits(flat, got, want)
        slack = 3
    elif grid:
        info = U.compare_hits(flat, got, want, edge_flip_frac=5e-4)
        slack = 3 + info["edge_flips"]
    else:
        info = U.compare_hits(flat, got, want, **COPIED)
        slack = 3 + info["edge_flips"] + int(5e-4 * len(occ_want))
    assert info["flips"] == 0 and info["n"] > 0.3 * len(occ_want)
    assert (occ_got != occ_want).sum() <= slack, int((occ_got != occ_want).sum())
    assert 0.05 < occ_want.mean() < 0.95
    return info


def _check_route(ctx, kind, mode):
    folded, general = U.zoo_route(kind, mode)
    U.check_kernel_used(ctx, mode, folded, general)
    assert (ctx.stats()["entered_instances"] == 0) == (not U.entered(mode)), "instances entered where they should be copied (or the other way round)"
    return "copied" if not U.entered(mode) else "folded" if folded else "general" if general else "parked"


# ---- (a) the zoo against the oracle, every kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["general", "uniform", "mixed"])
def test_zoo_against_the_oracle(gpu, kind, mode):
    """Closest hit and any hit of all nine modes on mirrors, a point reflection, scale ratios up to 30 : 1 and a shear ("general"), on uniform scales from
    1 / 1024 to 8 ("uniform") and on those beside one mirror ("mixed"); ctx.stats() must show the route the conversion's rules give the scene."""
    b, o, d, tmax, want, occ = _case(kind)
    ctx = U.make_ctx(gpu, b, 64, 36, flags=U.mode_flags(gpu, mode))
    got = ctx.intersect(o, d)
    occ_got = ctx.intersect(o, d, tmax=tmax, any_hit=True)["prim"]
    _against_the_oracle(b.flat, mode, got, want, occ_got, occ)
    hit = want["prim"] >= 0
    assert len(np.unique(want["inst"][hit])) >= len(b.targets) + 1  # every blob is hit, and the ground
    _check_route(ctx, kind, mode)
    ctx.close()


def test_the_zoo_cases_cover_every_instance_route(gpu):
    """Copied, folded, general and parked each occur among the cases above -- read from ctx.stats() of every (scene, mode), not from the table of expectations."""
    seen = set()
    for kind in ("general", "uniform", "mixed"):
        for mode in MODES:
            ctx = U.make_ctx(gpu, _zoo(kind), 64, 36, flags=U.mode_flags(gpu, mode))
            st = ctx.stats()
            ctx.close()
            seen.add("copied" if st["entered_instances"] == 0 else "folded" if st["folded_instances"] else "general" if st["general_route"] else "parked")
    assert seen == {"copied", "folded", "general", "parked"}, seen


# ---- (b) packets and bundles on the zoo ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entered", [False, True], ids=["copied", "entered"])
@pytest.mark.parametrize("thin", [False, True], ids=["pinhole", "thin_lens"])
@pytest.mark.parametrize("kind", ["general", "uniform"])
def test_packets_and_bundles_on_the_zoo_find_the_hits_of_the_per_ray_kernel(gpu, kind, thin, entered):
    """The packet kernel rebuilds its beam and its octant signs inside an instance's space, the bundle kernel its bundle: behind a mirror those signs flip.
    Camera rays of a 96 x 54 frame, 16 samples in flight, through pt_intersect's packets (neighbouring pixels, and shuffled so that packets straddle
    octants) and through the first pass of a batch: every hit record is the per-ray kernel's to the bit, except at exact-t ties."""
    W, Hh, spp = 96, 54, 16
    b = _zoo(kind, thin)
    base = gpu.FLAG_NO_BAKED_INSTANCES if entered else 0
    per_ray = U.make_ctx(gpu, b, W, Hh, flags=base, samples_in_flight=spp)
    packet = U.make_ctx(gpu, b, W, Hh, flags=base | gpu.FLAG_PACKET_INTERSECT, samples_in_flight=spp)
    queued = U.make_ctx(gpu, b, W, Hh, flags=base | gpu.FLAG_QUEUE_PRIMARY_RAYS | gpu.FLAG_NO_PACKETS, samples_in_flight=spp)
    o, d, _ = per_ray.gen_rays(0, W * Hh)
    perm = np.random.default_rng(3).permutation(len(o))
    for name, oo, dd in (("neighbours", o, d), ("shuffled", o[perm], d[perm])):
        got, want = packet.intersect(oo, dd), per_ray.intersect(oo, dd)
        U.assert_hits_of_the_per_ray_kernel(got, want, name)
        assert (got["prim"] >= 0).mean() > 0.3, name
    assert packet.stats()["packet_launches"] > 0 and per_ray.stats()["packet_launches"] == 0
    n = W * Hh * spp
    for sample in (0, spp):
        o1, d1, pixel1, got = per_ray.primary_pass(sample, spp, n)  # (no packet flag: pt_intersect is per ray, the first pass goes through bundles)
        o2, d2, pixel2, want = queued.primary_pass(sample, spp, n)  # k_gen + the per-ray kernel
        assert np.array_equal(pixel1, pixel2)
        assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32)) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))
        U.assert_hits_of_the_per_ray_kernel(got, want, f"first pass, sample {sample}")
        assert (got["prim"] >= 0).mean() > 0.3
        assert len(np.unique(got["inst"][got["prim"] >= 0])) >= 5  # blobs are in view, not the ground alone
    assert per_ray.stats()["bundle_launches"] == 2 and queued.stats()["packet_launches"] == 0 and queued.stats()["bundle_launches"] == 0
    for ctx in (per_ray, packet, queued):
        ctx.close()


# ---- (c) scale ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unit_hits(gpu):
    """{(scene, mode): (closest hits, occlusion verdicts)} of every kernel at unit scale and unit direction length: what the scaled cases below must reproduce
    to the bit.  Made once, ahead of them: a failure here is a failure of the unit-scale launch, and shows as one."""
    out = {}
    for name in ("grid", "mixed"):
        b, o, d, tmax, _, _ = _case(name)
        for mode in MODES:
            ctx = U.make_ctx(gpu, b, 64, 36, flags=U.mode_flags(gpu, mode))
            out[name, mode] = ctx.intersect(o, d), ctx.intersect(o, d, tmax=tmax, any_hit=True)["prim"]
            ctx.close()
    return out


def _same_bits(got, unit, t_factor):
    assert np.array_equal(got["prim"], unit["prim"]) and np.array_equal(got["inst"], unit["inst"]), int((got["prim"] != unit["prim"]).sum())
    for k in ("u", "v"):
        assert np.array_equal(got[k].view(np.uint32), unit[k].view(np.uint32)), k
    assert np.array_equal(got["t"].view(np.uint32), (unit["t"] * np.float32(t_factor)).view(np.uint32))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [-20, -7, 10, 20])
@pytest.mark.parametrize("name", ["grid", "mixed"])
def test_a_change_of_units_changes_nothing_but_the_units(gpu, unit_hits, name, k, mode):
    """scenes.scaled(flat, k) -- the same scene in units 2^k times smaller -- with origins and shadow-ray lengths scaled alike.  (1) The hits, t divided by
    2^k, pass against the UNIT-scale oracle with the unit-scale tolerances (the oracle is exactly equivariant: tests/test_transforms_cpu.py).  (2) They are
    the same kernel's unit-scale hits to the bit: same triangle and instance, same u and v, t times 2^k exactly -- every fp32 add, multiply, FMA,
    reciprocal and comparison commutes with a power of two inside the exponent range; only an absolute constant does not."""
    b, o, d, tmax, want, occ = _case(name)
    s = np.float32(2.0 ** k)
    ctx = U.make_ctx(gpu, scenes.scaled(b.flat, k), 64, 36, flags=U.mode_flags(gpu, mode))
    got = ctx.intersect(o * s, d)
    occ_got = ctx.intersect(o * s, d, tmax=tmax * s, any_hit=True)["prim"]
    if name == "mixed":
        _check_route(ctx, name, mode)
    else:
        U.check_kernel_used(ctx, mode)
    ctx.close()
    in_units = dict(got, t=got["t"] / s)
    _against_the_oracle(b.flat, mode, in_units, want, occ_got, occ, grid=name == "grid")
    unit, unit_occ = unit_hits[name, mode]
    _same_bits(got, unit, s)
    assert np.array_equal(occ_got, unit_occ)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [-12, 12])
@pytest.mark.parametrize("name", ["grid", "mixed"])
def test_the_length_of_the_direction_changes_nothing_but_t(gpu, unit_hits, name, k, mode):
    """Directions times 2^k at unit scene scale: t -- and the length a shadow ray must be given -- times 2^-k, everything else the same bits; against the
    oracle and against the same kernel's hits for unit directions, as above."""
    b, o, d, tmax, want, occ = _case(name)
    s = np.float32(2.0 ** k)
    ctx = U.make_ctx(gpu, b, 64, 36, flags=U.mode_flags(gpu, mode))
    got = ctx.intersect(o, d * s)
    occ_got = ctx.intersect(o, d * s, tmax=tmax / s, any_hit=True)["prim"]
    U.check_kernel_used(ctx, mode)
    ctx.close()
    _against_the_oracle(b.flat, mode, dict(got, t=got["t"] * s), want, occ_got, occ, grid=name == "grid")
    unit, unit_occ = unit_hits[name, mode]
    _same_bits(got, unit, 1 / s)
    assert np.array_equal(occ_got, unit_occ)


# ---- (d) axis-parallel rays in a large scene ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _axis_case():
    """The rotated grid in units 4096 times smaller (coordinates up to 2e4, a node's quantisation step above 4) and 12 000 rays with one or two exactly-zero
    direction components, half of them starting exactly ON a plane of a node's box -- where the slab test meets 0 * (1 / 0)."""
    flat = scenes.scaled(_grid().flat, 12)
    s = 4096.0
    o, d = U.axis_parallel_rays(flat, 12000, 9, (-4 * s, 0.05 * s, -4 * s), (4 * s, 3 * s, 4 * s))
    want = O.intersect_batch(O.BoundScene(flat), o, d, threads=8)
    return flat, o, d, want


@pytest.mark.parametrize("mode", ["baked", "two_level", "packet", "team"])
def test_axis_parallel_rays_in_a_large_scene(gpu, mode):
    """As test_edge_cases (tests/test_gpu_intersect.py) holds the Cornell room: a verdict may differ from the oracle's only where the hit grazes a triangle's
    boundary (a barycentric below 1e-5); every t is finite or +inf, never NaN; a ray that leaves the scene reports prim -1, instance -1, t +inf.  Where both
    sides hit the same triangle, t is the oracle's within what compare_hits grants fp32: 2e-4 relative, 1e-6 absolute in unit-scale units.  (Origins in the
    plane of the translated light quad are left out by gpu_util.axis_parallel_rays and tested on their own below.)"""
    flat, o, d, want = _axis_case()
    ctx = U.make_ctx(gpu, flat, 64, 36, flags=U.mode_flags(gpu, mode))
    got = ctx.intersect(o, d)
    U.check_kernel_used(ctx, mode)
    ctx.close()
    assert not np.isnan(got["t"]).any() and not np.isnan(got["u"]).any() and not np.isnan(got["v"]).any()
    gh, wh = got["prim"] >= 0, want["prim"] >= 0
    assert np.isfinite(got["t"][gh]).all() and (got["t"][gh] > 0).all()
    assert (got["inst"][~gh] == -1).all() and (got["prim"][~gh] == -1).all() and np.isposinf(got["t"][~gh]).all()
    for k in np.flatnonzero(gh != wh):
        h = got if gh[k] else want
        u, v = float(h["u"][k]), float(h["v"][k])
        assert min(abs(u), abs(v), abs(1.0 - u - v)) < 1e-5, (k, u, v)
    both = gh & wh & (got["prim"] == want["prim"]) & (got["inst"] == want["inst"])
    assert both.sum() > 0.3 * len(o) and (gh & wh & ~both).sum() <= 1e-2 * len(o)
    excess = np.abs(got["t"][both] - want["t"][both]) - 2e-4 * np.abs(want["t"][both])
    print(f"axis-parallel rays, {mode}: {int(both.sum())} common hits, worst |dt| - 2e-4 |t| = {excess.max():.3e}, verdicts differ for {int((gh != wh).sum())}")
    assert (excess <= 1e-6 * 4096).all()  # (compare_hits' t_atol in this scene's units: t's absolute error goes with the coordinates' magnitude, not with t)
    assert 0.01 < (~wh).mean() < 0.9  # rays leave the scene, too


@functools.lru_cache(maxsize=None)
def _light_plane_case():
    flat = scenes.scaled(_grid().flat, 12)
    (leaf, axis), = U.flat_translated_leaves(flat)  # the light quad, at y = 4 * 4096
    o, d, kind = U.rays_from_the_plane_of(flat, leaf, axis, 6000, 13)
    return flat, leaf, o, d, kind, O.intersect_batch(O.BoundScene(flat), o, d, threads=8)


@pytest.mark.parametrize("mode", ["baked", "two_level", "packet", "team"])
def test_rays_that_start_in_the_plane_of_a_translated_copied_quad(gpu, mode):
    """The one departure from the reference that include/ptamd.h states at pt_intersect, pinned.  6 000 rays start exactly in the plane y = 4 * 4096 of the
    light quad of the scaled grid -- over it and beside it; leaving upwards, leaving downwards, running in the plane; half of them axis-parallel.  The quad is
    a single leaf, copied to world space in all four modes.  Where the oracle reports the light (it moves the zero component of the instance-space origin to
    -FLT_MIN: a hit at t = FLT_MIN / d.y, or along an in-plane ray), the kernels meet it at t = 0 and report what exact arithmetic reports
    (tests/test_transforms_cpu.py): nothing, prim -1, instance -1, t +inf -- nothing lies above the light.  NOTHING ELSE differs: every other ray passes
    compare_hits with the tolerances of its route, and the kernels never report the light for a ray of this plane."""
    flat, leaf, o, d, kind, want = _light_plane_case()
    ctx = U.make_ctx(gpu, flat, 64, 36, flags=U.mode_flags(gpu, mode))
    got = ctx.intersect(o, d)
    U.check_kernel_used(ctx, mode)
    ctx.close()
    light = want["inst"] == leaf
    assert light.sum() > 0.2 * len(o) and light[kind == 0].any() and light[kind == 2].any() and not light[kind == 1].any()
    assert not np.isnan(got["t"]).any()
    assert (got["prim"][light] == -1).all() and (got["inst"][light] == -1).all() and np.isposinf(got["t"][light]).all()
    assert not (got["inst"] == leaf).any()
    rest = {k: v[~light] for k, v in got.items() if k != "ms"}, {k: v[~light] for k, v in want.items()}
    info = U.compare_hits(flat, *rest, edge_flip_frac=0.0 if U.entered(mode) else 5e-4, t_atol=1e-6 * 4096)
    assert info["flips"] == 0 and info["n"] > 0.2 * len(o)


# ---- (e) zero-area triangles -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _degenerate_case(builder, mirrored):
    b = scenes.degenerate_blob(BUILDERS[builder], mirrored)
    o, d = U.zoo_rays(b, N_RAYS, 43, (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
    tmax = np.random.default_rng(4).uniform(0.05, 4, len(o)).astype(np.float32)
    sc = O.BoundScene(b.flat)
    return b, o, d, tmax, O.intersect_batch(sc, o, d, threads=8), O.intersect_batch(sc, o, d, tmax=tmax, any_hit=True, threads=8)["prim"]


@pytest.mark.parametrize("mode", ["baked", "two_level", "packet", "two_level_packet", "team"])
@pytest.mark.parametrize("placement", ["world", "mirrored"])
@pytest.mark.parametrize("builder", sorted(BUILDERS))
def test_zero_area_triangles_inside_a_mesh(gpu, builder, placement, mode):
    """120 zero-area triangles (a repeated vertex; three collinear vertices) among the 1 280 of a blob, under every builder: as a world-space mesh (identity),
    as a mirrored instance that is entered (two_level*) and as a copy of it (baked, packet, team).  A device leaf holds two triangles and marks an empty slot
    with the all-zero triangle; a leaf of zero-area triangles must not pass for one.  Closest hit and any hit against the oracle; no zero-area triangle is
    ever reported; and after the device has refitted the mesh from its unchanged vertices (pt_refit_vertices, pt_upload_dynamic) every bit is as before."""
    b, o, d, tmax, want, occ = _degenerate_case(builder, placement == "mirrored")
    flat = b.flat
    degenerate = scenes.degenerate_triangles(flat)
    ctx = U.make_ctx(gpu, b, 64, 36, flags=U.mode_flags(gpu, mode))
    got = ctx.intersect(o, d)
    occ_got = ctx.intersect(o, d, tmax=tmax, any_hit=True)["prim"]
    _against_the_oracle(flat, mode, got, want, occ_got, occ)
    assert not degenerate[got["prim"][got["prim"] >= 0]].any()
    U.check_kernel_used(ctx, mode)
    assert (ctx.stats()["entered_instances"] > 0) == U.entered(mode)
    ctx.refit_vertices(b.scene.mesh_offsets(b.mesh)[0], b.mesh.vertices_view())
    ctx.upload_dynamic(b.scene.flatten_dynamic_only()[0])
    again = ctx.intersect(o, d)
    for k in ("t", "u", "v"):
        assert np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)), k
    assert np.array_equal(again["prim"], got["prim"]) and np.array_equal(again["inst"], got["inst"])
    assert np.array_equal(ctx.intersect(o, d, tmax=tmax, any_hit=True)["prim"], occ_got)
    ctx.close()


# ---- (f) shading on the transformed instances -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["copied", "entered"])
@pytest.mark.parametrize("integrator", ["IS", "MIS"])
def test_zoo_room_renders_like_the_oracle(gpu, integrator, route):
    """A mirrored PBR blob, a sheared rough-glass blob under a non-uniformly scaled PBR one and a small rough-glass blob in the Cornell room: shading
    normals, entering / leaving decisions and the normal transform of such instances, path by path against the oracle with the gates of the MIS tests
    (tests/test_gpu_mis.py): 64 x 36, 16 spp, both integrators, instances copied and entered."""
    W, Hh, spp = 64, 36, 16
    b = scenes.zoo_room(W, Hh)
    flags = (gpu.FLAG_INTEGRATOR_MIS if integrator == "MIS" else 0) | (gpu.FLAG_NO_BAKED_INSTANCES if route == "entered" else 0)
    ctx = U.make_ctx(gpu, b, W, Hh, seed=3, samples_in_flight=1, flags=flags)
    ctx.render(spp)
    a, st = ctx.read_accum()[:, :3], ctx.stats()
    ctx.close()
    assert (st["entered_instances"] > 0) == (route == "entered")
    ref, cnt = O.render(U.oracle_scene(b), b.camera, W, Hh, spp, seed=3, threads=8, integrator=O.INTEGRATOR_MIS if integrator == "MIS" else O.INTEGRATOR_IS)
    assert np.isfinite(a).all()
    U.render_gates(a, ref[:, :3], st, cnt, spp, b.camera, W * Hh, MEASURED, name=f"zoo room vs the oracle, {integrator}, {route}")
