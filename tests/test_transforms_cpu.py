"""What tests/test_gpu_transforms.py takes for granted, pinned on the CPU: on scenes with mirrored, sheared, strongly non-uniformly scaled, tiny and huge
instances and with zero-area triangles the oracle (the reference's arithmetic, fp32) finds what a float64 brute-force intersector finds; and the oracle is
exactly equivariant under a change of units by a power of two and under a power-of-two change of the direction's length.  With these the GPU tests may hold
a scaled scene's hits against the unit-scale oracle, and any difference they see belongs to the kernels."""
import functools

import numpy as np
import pytest

import bruteforce as B
import gpu_util as U
import orclib as O
from ptamd import device as D, host as H, scenes

BUILDERS = {"sah": H.BVH_BINNED_SAH, "fast": H.BVH_BINNED_FAST, "sbvh": H.BVH_SPATIAL_SPLIT}
N_BRUTE = 4000
BLOB_LO, BLOB_HI = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)


@functools.lru_cache(maxsize=None)
def _zoo(kind):
    return scenes.transform_zoo(kind)


def _against_float64(flat, o, d, want=None):
    """The caps of the oracle against float64: no hit / miss difference away from a triangle's boundary (smallest float64 barycentric of the disputed
    triangle below 2e-4), boundary-grazing differences for at most 1e-4 of the rays, t within 2e-4 relative for every ray both sides hit."""
    got = O.intersect_batch(O.BoundScene(flat), o, d, threads=8)
    want = B.intersect(flat, o, d) if want is None else want
    assert not np.isnan(got["t"]).any()
    gh, wh = got["prim"] >= 0, want["prim"] >= 0
    flips = np.flatnonzero(gh != wh)
    for k in flips:
        h = got if gh[k] else want
        u, v = B.barycentrics(flat, o[k:k + 1], d[k:k + 1], h["prim"][k:k + 1], h["inst"][k:k + 1])
        assert min(abs(u[0]), abs(v[0]), abs(1 - u[0] - v[0])) < 2e-4, f"ray {k}: hit / miss differs away from any edge (u={u[0]}, v={v[0]})"
    assert len(flips) <= 1e-4 * len(o), len(flips)
    both = gh & wh
    rel = np.abs(got["t"][both] - want["t"][both]) / want["t"][both]
    assert (rel <= 2e-4).all(), f"t differs by {rel.max():.2e} for {int((rel > 2e-4).sum())} rays"
    assert both.mean() > 0.3
    return got, want


@pytest.mark.parametrize("kind", ["general", "uniform", "mixed"])
def test_oracle_finds_what_float64_brute_force_finds_on_the_zoo(kind):
    """... with unit directions, and with directions a thousand times shorter and ten thousand times longer (t is in units of |d|)."""
    b = _zoo(kind)
    o, d = U.zoo_rays(b, N_BRUTE, 41)
    got, want = _against_float64(b.flat, o, d)
    assert len(np.unique(got["inst"][got["prim"] >= 0])) >= len(b.targets) + 1, "every blob and the ground are hit"
    for f in (1e-3, 1e4):
        df = (d * np.float32(f)).astype(np.float32)
        ratio = np.linalg.norm(d.astype(np.float64), axis=1) / np.linalg.norm(df.astype(np.float64), axis=1)
        _against_float64(b.flat, o[:1500], df[:1500], {k: (v[:1500] * ratio[:1500] if k == "t" else v[:1500]) for k, v in want.items()})


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("builder", sorted(BUILDERS))
def test_zero_area_triangles_are_accepted_and_never_hit(builder, mirrored):
    b = scenes.degenerate_blob(BUILDERS[builder], mirrored)
    flat = b.flat
    degenerate = scenes.degenerate_triangles(flat)
    assert 120 <= degenerate.sum() <= 130 and len(flat.triangles) >= 1400  # (an SBVH may reference a triangle from more than one leaf)
    assert np.isfinite(flat.vertices["normal"]).all() and np.isfinite(flat.vertices["vertex"]).all()
    st = b.mesh.stats()
    assert st["all_triangles_referenced"] and st["triangles_inside_leaves"] and st["children_inside_parents"]
    o, d = U.zoo_rays(b, N_BRUTE, 43, BLOB_LO, BLOB_HI)
    got, want = _against_float64(flat, o, d)
    assert not degenerate[got["prim"][got["prim"] >= 0]].any() and not degenerate[want["prim"][want["prim"] >= 0]].any()
    tmax = np.random.default_rng(4).uniform(0.05, 4, len(o)).astype(np.float32)
    occ = O.intersect_batch(O.BoundScene(flat), o, d, tmax=tmax, any_hit=True, threads=8)["prim"]
    clear = np.abs(want["t"] - tmax) > 2e-4 * tmax  # (segments that end within round-off of the first hit are decided by fp32)
    assert np.array_equal(occ[clear] != 0, (want["t"] < tmax)[clear])


def test_oracle_finds_what_float64_finds_for_axis_parallel_rays_in_a_large_scene():
    """The rotated grid in units 4096 times smaller, rays with one or two exactly-zero direction components, half of them starting on a node's plane.  Left out:
    rays with an exactly-zero ORIGIN component -- the reference moves such a component to -FLT_MIN inside an instance (NO_PARALLEL_RAYS, scene.cl:123-137), so
    a ray that starts in the ground's plane y = 0 starts below it by the reference's own definition, and float64 has no say in that."""
    flat = scenes.scaled(scenes.instanced_grid(64, 36, level=3, sky_size=(16, 8), rotate=True).flat, 12)
    s = 4096.0
    o, d = U.axis_parallel_rays(flat, 2400, 9, (-4 * s, 0.05 * s, -4 * s), (4 * s, 3 * s, 4 * s))
    keep = (o != 0).all(1)
    assert 0.6 * len(o) < keep.sum() < len(o)
    _against_float64(flat, o[keep][:1500], d[keep][:1500])


def test_float64_sees_no_hit_where_a_ray_starts_in_the_plane_of_the_light():
    """The one place where the kernels leave the oracle (include/ptamd.h, pt_intersect; pinned on the GPU by tests/test_gpu_transforms.py): rays that start
    exactly in the plane of the translated light quad of the grid, in units 4096 times smaller.  The oracle reports the light for those over the quad that
    leave the plane upwards or run in it -- it moves the zero component of the instance-space origin to -FLT_MIN --; float64 meets the quad at t = 0 and
    reports it for none.  Everywhere else the two agree."""
    flat = scenes.scaled(scenes.instanced_grid(64, 36, level=3, sky_size=(16, 8), rotate=True).flat, 12)
    (leaf, axis), = U.flat_translated_leaves(flat)
    o, d, kind = U.rays_from_the_plane_of(flat, leaf, axis, 600, 13)
    got, want = O.intersect_batch(O.BoundScene(flat), o, d, threads=8), B.intersect(flat, o, d)
    light = got["inst"] == leaf
    assert light.sum() > 0.2 * len(o) and not (want["inst"] == leaf).any()
    assert not light[kind == 1].any() and light[kind == 0].any() and light[kind == 2].any()
    assert (got["t"][light & (kind == 0)] < 1e-30).all()  # FLT_MIN / d.y
    assert (want["prim"][light] == -1).all()  # nothing lies above the light
    assert np.array_equal(got["prim"][~light] >= 0, want["prim"][~light] >= 0)


def _equivariance_scenes():
    return {"grid_rotated": scenes.instanced_grid(64, 36, level=3, sky_size=(16, 8), rotate=True), "zoo_mixed": _zoo("mixed")}


@functools.lru_cache(maxsize=None)
def _unit(name):
    b = _equivariance_scenes()[name]
    if name == "zoo_mixed":
        o, d = U.zoo_rays(b, 20000, 47)
    else:
        o, d = U.random_rays(20000, 47, (-4, 0.05, -4), (4, 3, 4))
    tmax = np.random.default_rng(5).uniform(0.05, 4, len(o)).astype(np.float32)
    sc = O.BoundScene(b.flat)
    return b.flat, o, d, tmax, O.intersect_batch(sc, o, d, threads=8), O.intersect_batch(sc, o, d, tmax=tmax, any_hit=True, threads=8)["prim"]


def _same_hits(got, want, t_factor):
    assert np.array_equal(got["prim"], want["prim"]) and np.array_equal(got["inst"], want["inst"])
    for k in ("u", "v"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert np.array_equal(got["t"].view(np.uint32), (want["t"] * np.float32(t_factor)).view(np.uint32))


@pytest.mark.parametrize("k", [-20, -7, 10, 20])
@pytest.mark.parametrize("name", ["grid_rotated", "zoo_mixed"])
def test_oracle_is_exactly_equivariant_under_a_change_of_units(name, k):
    """scenes.scaled(flat, k) with the rays' origins (and the shadow rays' lengths) scaled alike: the same triangle, instance and u / v bits, t times 2^k
    to the bit."""
    flat, o, d, tmax, want, occ = _unit(name)
    s = np.float32(2.0 ** k)
    sc = O.BoundScene(scenes.scaled(flat, k))
    _same_hits(O.intersect_batch(sc, o * s, d, threads=8), want, s)
    assert (want["prim"] >= 0).mean() > 0.3
    assert np.array_equal(O.intersect_batch(sc, o * s, d, tmax=tmax * s, any_hit=True, threads=8)["prim"], occ)


@pytest.mark.parametrize("k", [-12, 12])
@pytest.mark.parametrize("name", ["grid_rotated", "zoo_mixed"])
def test_oracle_is_exactly_equivariant_under_the_length_of_the_direction(name, k):
    """Directions times 2^k: t (and with it the length a shadow ray is given) times 2^-k, everything else the same bits."""
    flat, o, d, tmax, want, occ = _unit(name)
    s = np.float32(2.0 ** k)
    sc = O.BoundScene(flat)
    _same_hits(O.intersect_batch(sc, o, d * s, threads=8), want, 1 / s)
    assert np.array_equal(O.intersect_batch(sc, o, d * s, tmax=tmax / s, any_hit=True, threads=8)["prim"], occ)


@pytest.mark.parametrize("kind", ["general", "uniform", "mixed"])
@pytest.mark.parametrize("mode", U.MODES)
def test_the_zoo_takes_the_instance_routes_it_was_made_for(kind, mode):
    """The conversion alone (no device): which route the zoo's instances take in each of the nine modes, by the rules of gpu_util.zoo_route."""
    dyn = {key: int(v, 10) for key, v in U.parse_digest(D.debug_convert(_zoo(kind).flat, flags=U.mode_flags(D, mode)))["dynamic"].items()
           if key in ("enteredInstances", "enteredGeneral", "foldedInstances", "generalRoute", "bakedNodes")}
    folded, general = U.zoo_route(kind, mode)
    assert (dyn["foldedInstances"], dyn["generalRoute"]) == (folded, general), dyn
    n = len(_zoo(kind).targets)
    if U.entered(mode):
        assert dyn["enteredInstances"] == n + (2 if mode.startswith("unbaked") else 0) and dyn["bakedNodes"] == 0
        if not mode.endswith("parked"):  # (asked to park, the conversion counts every instance as one for the general way in)
            assert dyn["enteredGeneral"] == {"general": n, "uniform": 0, "mixed": 1}[kind]
    else:
        assert dyn["enteredInstances"] == 0 and dyn["bakedNodes"] > 0


def test_zoo_room_renders_finite_images_with_both_integrators():
    b = scenes.zoo_room()
    sc = U.oracle_scene(b)
    for integrator in (O.INTEGRATOR_IS, O.INTEGRATOR_MIS):
        img, _ = O.render(sc, b.camera, b.width, b.height, 4, seed=3, threads=8, integrator=integrator)
        assert np.isfinite(img).all() and 0.02 < img[:, :3].mean() / 4 < 1.0
    o, d = U.zoo_rays(b, 4000, 3, (-0.9, 0.1, -0.9), (0.9, 1.9, 0.9))
    hit = O.intersect_batch(sc, o, d, threads=8)
    assert len(np.unique(hit["inst"][hit["prim"] >= 0])) == 5  # the room and the four blobs
    _against_float64(b.flat, o[:1000], d[:1000])
