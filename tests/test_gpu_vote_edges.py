"""The step votes of the per-ray kernels (pt_trace.h) at the states where a wrong count or a lane mistaken for idle would show.

A lane without a ray holds kRefIdle in its current reference and every vote of the hot loop is a compare on that reference; the kernel hands out rays once
8 lanes are idle, leaves the hot loop once 16 / 24 / 32 / 48 lanes are parked, and serves 64 entries per packet.  So: queues of 1 ... 4 097 rays around those
counts, and ray patterns that put the lanes of a wave into chosen states -- all the same, all finished at the root, hit and miss lane by lane, one long ray
among 63 that finish at once, rays deep enough to spill the 12-entry LDS stack -- through pt_intersect on a small scene (a level-3 blob over a quad), closest
hit and any hit, over every route the six instantiations of k_trace take: one world-space tree (LEVELS 0), the folded and the parked route (LEVELS 1), the
general route (LEVELS 2).

Expected: the oracle's hits and occlusion verdicts by the comparison of tests/test_gpu_intersect.py (gpu_util.compare_hits: integers exact, t / u / v within
2e-4 relative; occlusion verdicts may differ where a segment ends within round-off of its hit: at most 2 per queue there, here too); the general route equal
to the parked route on the same scene as that file demands it (same triangle and instance, the same t / u / v bits).  pt_intersect fills its result buffers
with sentinels before the launch: an entry no lane wrote comes back as t = NaN or as verdict -1, so every queue entry must have got a result.  (An entry
written twice with the same value cannot be seen through the hook.)"""
import numpy as np
import pytest

import gpu_util as U
import orclib as O
from ptamd import host as H, layout as L, scenes
from test_gpu_intersect import _chain_scene

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 8, 9, 56, 57, 63, 64, 65, 127, 4097)
N = max(SIZES)
PATTERNS = ("identical", "all_miss", "alternating", "one_long", "random")
BLOB_AT, BLOB_SCALE = (0.3, 0.9, -0.2), 0.8


def _scene(turned):
    mesh = scenes.blob_mesh(L.material_diffuse((0.7, 0.3, 0.2)), level=3, seed=3, builder=H.BVH_BINNED_SAH)
    scene = H.Scene()
    mb = scenes._MeshBuilder()
    mb.add_quad((-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3), 0)
    scene.add_node(mb.build([L.material_diffuse((0.6, 0.6, 0.6))], H.BVH_BINNED_SAH))
    q = (float(np.cos(0.4)), 0.0, float(np.sin(0.4)), 0.0) if turned else (1, 0, 0, 0)
    scene.add_node(mesh, location=BLOB_AT, orientation_wxyz=q, scale=(BLOB_SCALE,) * 3)
    return scene.flatten()


def _unit(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


def _rays(pattern):
    """N rays and shadow-ray lengths; a queue of n rays is the first n (so one oracle run per pattern serves every queue size)."""
    rng = np.random.default_rng(PATTERNS.index(pattern) + 40)
    # rays that leave the scene's box at once: from above it, pointing up -- they finish at the root
    miss_o = rng.uniform((-2, 4, -2), (2, 6, 2), (N, 3)).astype(np.float32)
    miss_d = _unit(np.c_[rng.uniform(-0.5, 0.5, N), rng.uniform(0.5, 1, N), rng.uniform(-0.5, 0.5, N)])
    # rays from above aimed at the blob and the ground around it
    hit_o = rng.uniform((-1.5, 2.5, -1.5), (1.5, 3.5, 1.5), (N, 3)).astype(np.float32)
    target = np.asarray(BLOB_AT) + rng.uniform(-0.7, 0.7, (N, 3)) * (1, 0.5, 1)
    hit_d = _unit(target - hit_o)
    tmax = rng.uniform(0.05, 6, N).astype(np.float32)
    k = np.arange(N)
    if pattern == "identical":
        o = np.tile(np.array([[0.35, 3.0, -0.15]], np.float32), (N, 1))
        d = np.tile(_unit([[0.02, -1.0, 0.03]]), (N, 1))
        tmax = np.where(k < N // 2, 10.0, 1.0).astype(np.float32)  # first half occluded by the blob, second half ends above it
    elif pattern == "all_miss":
        o, d = miss_o, miss_d
    elif pattern == "alternating":
        even = (k % 2 == 0)[:, None]
        o, d = np.where(even, hit_o, miss_o), np.where(even, hit_d, miss_d)
    elif pattern == "one_long":
        # one lane in 64 walks the length of the scene just above the ground, through the blob's box, while the other 63 finish at the root
        long_o = np.c_[np.full(N, -2.9), rng.uniform(0.55, 1.2, N), rng.uniform(-0.5, 0.1, N)].astype(np.float32)
        long_d = _unit(np.c_[np.ones(N), rng.uniform(-0.05, 0.02, N), rng.uniform(-0.03, 0.03, N)])
        one = (k % 64 == 37)[:, None] | (k == 0)[:, None]  # (entry 0 too: the queues shorter than 38)
        o, d = np.where(one, long_o, miss_o), np.where(one, long_d, miss_d)
        tmax = np.where(one[:, 0], 10.0, tmax).astype(np.float32)
    else:
        o, d = U.random_rays(N, 23, (-2.5, 0.05, -2.5), (2.5, 2.5, 2.5))
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), tmax


@pytest.fixture(scope="module")
def cases():
    """{turned: (flat, {pattern: (o, d, tmax, oracle closest hits, oracle verdicts)})}: computed once, read by every test below."""
    out = {}
    for turned in (False, True):
        flat = _scene(turned)
        sc = O.BoundScene(flat)
        per = {}
        for p in PATTERNS:
            o, d, tmax = _rays(p)
            per[p] = (o, d, tmax, O.intersect_batch(sc, o, d, threads=8), O.intersect_batch(sc, o, d, tmax=tmax, any_hit=True, threads=8)["prim"])
        out[turned] = (flat, per)
    # what the patterns are for: both outcomes in every mixed pattern, none in the pure ones
    per = out[False][1]
    assert (per["identical"][3]["prim"] >= 0).all() and (per["all_miss"][3]["prim"] < 0).all()
    assert per["identical"][4][:N // 2].all() and not per["identical"][4][N // 2:].any()
    alt = per["alternating"][3]["prim"] >= 0
    assert alt[0::2].mean() > 0.9 and not alt[1::2].any()
    assert (per["one_long"][3]["prim"] >= 0).mean() < 0.05
    return out


def _written(got, any_hit):
    if any_hit:
        return np.isin(got["prim"], (0, 1))
    return ~np.isnan(got["t"])


def _check(ctx, flat, per, edge_flip_frac=0.0, twin=None):
    for p in PATTERNS:
        o, d, tmax, want, want_occ = per[p]
        for n in SIZES:
            got = ctx.intersect(o[:n], d[:n])
            assert _written(got, False).all(), (p, n, "closest hit: entries without a result", np.flatnonzero(~_written(got, False))[:8])
            want_n = {k: v[:n] for k, v in want.items()}
            if ((got["prim"] >= 0) & (want_n["prim"] >= 0)).any():
                info = U.compare_hits(flat, got, want_n, edge_flip_frac=edge_flip_frac)
            else:  # (compare_hits takes means over the rays that hit on both sides: a queue without one is compared here)
                assert np.array_equal(got["prim"] >= 0, want_n["prim"] >= 0), (p, n)
                info = dict(flips=0, edge_flips=0)
            assert info["flips"] == 0, (p, n)
            missed = got["prim"] < 0
            assert np.isinf(got["t"][missed]).all() and (got["prim"][missed] == -1).all() and (got["inst"][missed] == -1).all(), (p, n)
            occ = ctx.intersect(o[:n], d[:n], tmax=tmax[:n], any_hit=True)
            assert _written(occ, True).all(), (p, n, "any hit: entries without a verdict", np.flatnonzero(~_written(occ, True))[:8])
            assert (occ["prim"] != want_occ[:n]).sum() <= 2 + info["edge_flips"], (p, n, np.flatnonzero(occ["prim"] != want_occ[:n])[:8])
            if twin is not None:  # the parked route on the same scene
                ref = twin.intersect(o[:n], d[:n])
                assert np.array_equal(got["prim"], ref["prim"]) and np.array_equal(got["inst"], ref["inst"]), (p, n)
                for k in ("t", "u", "v"):
                    assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (p, n, k)
                assert np.array_equal(occ["prim"], twin.intersect(o[:n], d[:n], tmax=tmax[:n], any_hit=True)["prim"]), (p, n)


@pytest.mark.parametrize("route", ["flat", "folded", "parked"])
def test_votes_on_a_blob_over_a_quad(gpu, cases, route):
    """k_trace<., 0> on the world-space copy, k_trace<., 1> with the blob and the quad folded, and with both parked at their instance references."""
    flat, per = cases[False]
    flags = {"flat": 0, "folded": gpu.FLAG_NO_BAKED_INSTANCES, "parked": gpu.FLAG_NO_BAKED_INSTANCES | gpu.FLAG_PARKED_INSTANCES}[route]
    ctx = gpu.Context(64, 36, flags=flags)
    ctx.upload_scene(flat)
    st = ctx.stats()
    assert (st["entered_instances"], st["folded_instances"], st["general_route"]) == {"flat": (0, 0, 0), "folded": (2, 2, 0), "parked": (2, 0, 0)}[route], st
    # (a world-space copy rounds its triangle edges in another space than the oracle: a ray may change sides of an edge it grazes, as in test_gpu_intersect.py)
    _check(ctx, flat, per, edge_flip_frac=5e-4 if route == "flat" else 0.0)
    assert ctx.stats()["packet_launches"] == 0 and ctx.stats()["team_launches"] == 0
    ctx.close()


def test_votes_on_the_general_route(gpu, cases):
    """k_trace<., 2>: the blob turned (entered through the full transform), the quad through the entry record's short form; against the oracle and, bit for bit,
    against the parked route on the same scene."""
    flat, per = cases[True]
    general = gpu.Context(64, 36, flags=gpu.FLAG_NO_BAKED_INSTANCES)
    general.upload_scene(flat)
    parked = gpu.Context(64, 36, flags=gpu.FLAG_NO_BAKED_INSTANCES | gpu.FLAG_PARKED_INSTANCES)
    parked.upload_scene(flat)
    assert general.stats()["general_route"] == 1 and general.stats()["folded_instances"] == 0 and parked.stats()["general_route"] == 0
    _check(general, flat, per, twin=parked)
    general.close()
    parked.close()


def test_votes_while_lanes_spill_their_stack(gpu):
    """A 100-level chain entered from the far side needs ~100 pending entries (12 in LDS, the rest spilled); from the near side two.  Deep and shallow rays
    lane by lane, and one deep ray among 63 shallow ones, over the same queue sizes: the deep rays find the last triangle, the shallow ones the first."""
    n_tri = 100
    flat, z = _chain_scene(n_tri)
    ctx = gpu.Context(8, 8)
    ctx.upload_scene(flat)
    rng = np.random.default_rng(5)
    xy = rng.uniform(0.05, 0.45, (N, 2)).astype(np.float32)
    k = np.arange(N)
    for name, deep in (("alternating", k % 2 == 0), ("one_deep", (k % 64 == 37) | (k == 0)), ("all_deep", k >= 0)):
        o = np.c_[xy, np.where(deep, 100.0, -100.0)].astype(np.float32)
        d = np.c_[np.zeros((N, 2)), np.where(deep, -1.0, 1.0)].astype(np.float32)
        # shadow rays: the deep ones reach half of the chain (occluded), the shallow ones stop short of it
        tmax = np.where(deep, 95.0, 99.0).astype(np.float32)
        for n in SIZES:
            got = ctx.intersect(o[:n], d[:n])
            assert _written(got, False).all(), (name, n)
            assert np.array_equal(got["prim"], np.where(deep[:n], n_tri - 1, 0)), (name, n)
            want_t = np.where(deep[:n], 100.0 - z[n_tri - 1], 100.0 + z[0])
            assert np.allclose(got["t"], want_t, rtol=1e-5), (name, n)
            occ = ctx.intersect(o[:n], d[:n], tmax=tmax[:n], any_hit=True)
            assert _written(occ, True).all(), (name, n)
            assert np.array_equal(occ["prim"], deep[:n].astype(np.int32)), (name, n)
    assert ctx.stats()["stack_need"] >= n_tri - 4
    ctx.close()
