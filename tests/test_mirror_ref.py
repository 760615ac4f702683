"""Guide reflections as tests/mirror_ref.py restates them (include/ptamd.h, "guide reflections"), on the oracle alone: what any implementation of the
contract has -- nothing to reflect, no change; a planar mirror shows the mirror image of the room; tints multiply in stage order; a bent normal and
stage K end a chain on the mirror --, what single precision costs it, and what guides taken through a mirror wall buy the filter and the history."""
import numpy as np
import pytest

import chain_ref as CH
import denoise_ref as R
import gpu_util as U
import mirror_ref as M
import orclib as O
import temporal_ref as T
from ptamd import host as H, layout as L, scenes
from test_chain_ref import BOX_CENTRE, BOX_HALF, _box_axes, glass_box_room
from test_denoise_ref import pixel_centre_rays

TINT = np.asarray(scenes.CORRIDOR_TINT, np.float32).astype(np.float64)


def mirror_scene(name, width=64, height=36):
    """the four scenes the device is held against (tests/test_gpu_guide_mirror.py)"""
    if name == "mirror_wall":
        return scenes.cornell_mirror_wall(width, height)
    if name == "mirror_corridor":
        return scenes.mirror_corridor(width, height)
    if name == "mirror_blob_room":
        return scenes.mirror_blob_room(width, height)
    return glass_box_room(width, height)


MIRROR_SCENES = ["mirror_wall", "mirror_corridor", "mirror_blob_room", "glass_box"]
# the float32 restatement's own error against float64 (test_float32_follows_the_same_chain): the worst of the four scenes each
FLOAT32_DISTANCE, FLOAT32_NORMAL, FLOAT32_ALBEDO = 5.6e-7, 3.6e-6, 3.4e-8
BLOB_FLIP_CAP = 0.03  # the share of mirror_blob_room's pixels that float32 decision flips may send to another terminal


def on_mirror(flat, prim):
    """the terminal primitive's material is a MIRROR"""
    out = np.zeros(len(prim), bool)
    hit = prim >= 0
    out[hit] = M.is_mirror(flat.materials[flat.triangles["materialIndex"][prim[hit]]])
    return out


def test_reflections_off_is_the_chain():
    b = glass_box_room(32, 32)
    sc = U.oracle_scene(b)
    o, d = pixel_centre_rays(b.camera, 32, 32)
    want = CH.chain(b.flat, sc, o, d, 4)
    got = M.chain(b.flat, sc, o, d, 4, reflections=False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert all(np.array_equal(got[2][k], want[2][k], equal_nan=True) for k in want[2])


@pytest.mark.parametrize("K", [1, 4])
def test_rays_that_never_reflect_get_the_chains_values(K):
    """cornell_box (nothing to follow) and the glass-box room on the rays whose chain meets no total internal reflection: chain_ref's values exactly"""
    for b, everything in ((scenes.cornell_box(32, 32), True), (glass_box_room(32, 32), False)):
        sc = U.oracle_scene(b)
        o, d = pixel_centre_rays(b.camera, 32, 32)
        want_a, want_g, want = CH.chain(b.flat, sc, o, d, K)
        a, g, info = M.chain(b.flat, sc, o, d, K)
        plain = ~info["met"]
        assert plain.all() if everything else plain.sum() > 800
        assert np.array_equal(a[plain], want_a[plain]) and np.array_equal(g[plain], want_g[plain])
        assert np.array_equal(info["prim"][plain], want["prim"][plain]) and np.array_equal(info["depth"][plain], want["depth"][plain])
        assert (info["reflections"][plain] == 0).all() and (info["tint"][plain] == 1).all()


def mirrored_about(flat, z0):
    """the flattened scene (one identity instance) mirrored about the plane z = z0: vertices, normals, node boxes of both levels, lights"""
    v, n, top, l = flat.vertices.copy(), flat.sub_nodes.copy(), flat.top_nodes.copy(), flat.lights.copy()
    v["vertex"][:, 2] = np.float32(2 * z0) - v["vertex"][:, 2]
    v["normal"][:, 2] *= -1
    with np.errstate(over="ignore", invalid="ignore"):
        for nodes in (n, top):
            lo, hi = nodes["min"][:, 2].copy(), nodes["max"][:, 2].copy()
            nodes["min"][:, 2], nodes["max"][:, 2] = np.float32(2 * z0) - hi, np.float32(2 * z0) - lo
    l["vertices"][:, :, 2] = np.float32(2 * z0) - l["vertices"][:, :, 2]
    return H.FlatScene(v, flat.triangles, flat.materials, n, l, top, flat.top_root, flat.num_instances)


def test_a_planar_mirror_shows_the_mirror_image_of_the_room():
    """cornell_mirror_wall, pixel-centre rays whose first hit is the mirror, K = 1: the terminal point is the mirror image (about z = 0.99) of where
    the STRAIGHT ray, carried on behind the mirror plane, hits the room mirrored about that plane -- to 1e-6 --, the terminal primitive is that hit's,
    and dist is the straight distance to that image less the one 1e-4 offset of the reflected segment.  (Distance tolerance 3e-6: three float32 hit
    distances of up to 8 m, half an ulp -- 4.8e-7 -- each, and two origins rounded to float32.)"""
    b = scenes.cornell_mirror_wall(64, 64)
    sc = U.oracle_scene(b)
    o, d = pixel_centre_rays(b.camera, 64, 64)
    a, g, info = M.chain(b.flat, sc, o, d, 1)
    m = info["first_mirror"]
    assert m.sum() > 300 and (info["reflections"][m] == 1).all() and (info["depth"][m] == 1).all() and (info["reflections"][~m] == 0).all()
    first = O.intersect_batch(sc, o[m], d[m], threads=8)
    t0 = first["t"].astype(np.float64)
    assert np.abs(o[m][:, 2] + d[m][:, 2] * t0 - scenes.MIRROR_Z).max() < 1e-6
    behind = U.oracle_scene(mirrored_about(b.flat, scenes.MIRROR_Z))
    o2 = o[m].astype(np.float64) + d[m].astype(np.float64) * (t0 + CH.EPS)[:, None]
    second = O.intersect_batch(behind, o2.astype(np.float32), d[m], threads=8)
    hit = second["prim"] >= 0
    assert np.array_equal(hit, info["prim"][m] >= 0) and hit.sum() > 60 and (~hit).sum() > 60  # (most of what the mirror shows is the room's opening: misses)
    assert np.array_equal(second["prim"][hit], info["prim"][m][hit])
    # where the straight ray meets the plane of that triangle, in float64 (the hit distance of a float32 record is good to 5e-7 at 8 m: too coarse here)
    mirrored = behind.flat
    corner = mirrored.vertices["vertex"][mirrored.triangles["indices"][np.maximum(second["prim"], 0)], :3].astype(np.float64)
    normal = np.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
    o64, d64 = o[m].astype(np.float64), d[m].astype(np.float64)
    image = o64 + d64 * (((corner[:, 0] - o64) * normal).sum(1) / (d64 * normal).sum(1))[:, None]
    want = image * (1, 1, -1) + (0, 0, 2 * scenes.MIRROR_Z)
    # A queue entry is rounded to float32 once (chain_ref): the reflected origin to 6e-8 per component near 1 m, the direction to 3e-8 per component,
    # and a direction error e moves a hit at distance s that meets its surface at the cosine c by s e / c.  1e-6 is asked of the rays whose reflected
    # segment is at most 3 m and meets the terminal at c >= 0.5: 1e-7 + 3 x 5.2e-8 x 2 / 0.5 = 7e-7; a grazing hit on the ceiling amplifies further.
    seg = np.linalg.norm(image - o64, axis=1) - t0
    cos_t = np.abs((d64 * normal).sum(1)) / np.linalg.norm(normal, axis=1)
    steep = hit & (seg <= 3.0) & (cos_t >= 0.5)
    err = np.abs(info["point"][m] - want).max(1)
    print(f"{int(hit.sum())} reflected hits, {int(steep.sum())} of them steep: point error {err[steep].max():.2e} (all hits {err[hit].max():.2e})")
    assert steep.sum() >= 15 and len(np.unique(second["prim"][steep])) >= 2
    assert err[steep].max() < 1e-6
    straight = np.linalg.norm(image - o[m].astype(np.float64), axis=1)
    assert np.abs(g[m][hit, 3] - (straight[hit] - CH.EPS)).max() < 3e-6
    assert (g[m][~hit, 3] == R.SKY_DEPTH).all() and (a[m][~hit, 3] == 0).all()
    # the tint of one reflection: the mirror's base colour on the terminal's albedo; the sky keeps the tint itself
    colour = np.float32(0.9).astype(np.float64)
    mat = b.flat.materials[b.flat.triangles["materialIndex"][second["prim"][hit]]]
    own = np.where((mat["type"] == L.MAT_DIFFUSE)[:, None], mat["colour"][:, :3].astype(np.float64), 1.0)  # (the light deposits (1,1,1))
    assert np.abs(a[m][hit, :3] - colour * own).max() < 1e-12 and np.abs(a[m][~hit, :3] - colour).max() < 1e-12


def test_tints_multiply_and_stage_K_ends_on_a_mirror():
    """mirror_corridor, K = 4: a chain of m reflections that ends on a wall, the floor or the ceiling deposits colour^m (.) that surface's albedo, one that
    leaves through the opening colour^m with hits 0, and the chains still between the mirrors at stage 4 end ON a mirror: colour^4 (.) colour, hits 1"""
    b = scenes.mirror_corridor(64, 36)
    sc = U.oracle_scene(b)
    o, d = pixel_centre_rays(b.camera, 64, 36)
    a, g, info = M.chain(b.flat, sc, o, d, 4)
    mirror = on_mirror(b.flat, info["prim"])
    m = info["reflections"]
    assert info["first_mirror"].all() and np.array_equal(m, info["depth"])
    for count in (1, 2, 3, 4):
        assert ((m == count) & ~mirror & (info["prim"] >= 0)).sum() > 20, count
    wall = ~mirror & (info["prim"] >= 0)
    mat = b.flat.materials[b.flat.triangles["materialIndex"][info["prim"][wall]]]
    albedo = np.where((mat["type"] == L.MAT_DIFFUSE)[:, None], mat["colour"][:, :3].astype(np.float64), 1.0)  # (the light deposits (1,1,1))
    assert np.abs(a[wall, :3] - TINT[None] ** m[wall, None] * albedo).max() < 1e-12 and (a[wall, 3] == 1).all()
    miss = info["prim"] < 0
    assert miss.sum() > 50 and np.abs(a[miss, :3] - TINT[None] ** m[miss, None]).max() < 1e-12 and (a[miss, 3] == 0).all()
    assert mirror.sum() > 100 and (info["depth"][mirror] == 4).all() and (m[mirror] == 4).all()
    assert np.abs(a[mirror, :3] - TINT[None] ** 5).max() < 1e-12 and (a[mirror, 3] == 1).all()
    # every K: the chains that are still between the mirrors end at stage K on a mirror
    for K in (1, 2, 3):
        _, _, i = M.chain(b.flat, sc, o, d, K)
        end = on_mirror(b.flat, i["prim"])
        assert end.sum() > 100 and (i["depth"][end] == K).all()


def test_total_internal_reflection_goes_on():
    """the ray of test_chain_ref (45 degrees into the glass box's front face, 5 cm from its edge), which the chain ends on the side face: with
    reflections it is reflected there and ends on a surface that is not glass, or at stage K"""
    b = glass_box_room(32, 32)
    sc = U.oracle_scene(b)
    front, side = _box_axes()
    face = BOX_CENTRE + front * BOX_HALF[2]
    dg = (-front + side) / np.sqrt(2.0)
    og = face + side * 0.25 - dg * 0.3
    _, g0, off = CH.chain(b.flat, sc, og[None], dg[None], 4)
    assert off["tir"][0] and off["depth"][0] == 1
    a, g, info = M.chain(b.flat, sc, og[None], dg[None], 4)
    assert info["reflections"][0] >= 1 and info["met"][0] and info["depth"][0] >= 2 and not info["tir"][0]
    types = b.flat.materials["type"][b.flat.triangles["materialIndex"][info["prim"][0]]]
    assert info["depth"][0] == 4 or types not in (L.MAT_REFRACTIVE, L.MAT_BASIC_REFRACTIVE)
    assert g[0, 3] > g0[0, 3] and (info["tint"][0] == 1).all()  # further than the side face; glass does not tint
    # K = 1: the side face is met at stage K, where every surface is terminal -- the chain's own deposit
    a1, g1, i1 = M.chain(b.flat, sc, og[None], dg[None], 1)
    assert i1["depth"][0] == 1 and i1["reflections"][0] == 0 and np.array_equal(g1[0], g0[0]) and (a1[0] == 1).all()


def test_a_bent_normal_ends_the_chain_on_the_mirror():
    """mirror_blob_room: near the blob's silhouette the interpolated normal sends the reflection through the surface (G.R <= 1e-4) -- those chains end
    on the blob with its own albedo and no reflection; the others leave on the ray's side of the real normal"""
    b = scenes.mirror_blob_room(64, 36)
    sc = U.oracle_scene(b)
    o, d = pixel_centre_rays(b.camera, 64, 36)
    a, g, info = M.chain(b.flat, sc, o, d, 4)
    first = O.intersect_batch(sc, o, d, threads=8)
    k = np.flatnonzero(info["first_mirror"])
    D = d[k].astype(np.float64)
    _, g1, _ = CH.chain(b.flat, sc, o[k], d[k], 0)  # the first hit's deposited normal
    N = g1[:, :3]
    real = CH._real_normal(b.flat, first["prim"][k].astype(np.int64), first["inst"][k].astype(np.int64), np.float64)
    G = np.where(((real * -D).sum(1) > 0)[:, None], real, -real)
    Rf = D + N * (2 * -(N * D).sum(1))[:, None]
    through = (G * Rf / np.linalg.norm(Rf, axis=1, keepdims=True)).sum(1) <= CH.EPS
    assert through.sum() > 20 and (~through).sum() > 200
    bent = k[through]
    assert (info["depth"][bent] == 0).all() and (info["reflections"][bent] == 0).all() and info["met"][bent].all()
    assert np.array_equal(info["prim"][bent], first["prim"][bent]) and on_mirror(b.flat, info["prim"][bent]).all()
    colour = b.flat.materials["colour"][b.flat.triangles["materialIndex"][info["prim"][bent]], :3].astype(np.float64)
    assert np.array_equal(a[bent, :3], colour) and (a[bent, 3] == 1).all()
    assert (info["reflections"][k[~through]] >= 1).all()
    # the instance is mirrored: its determinant is negative, and the deposited normals still face the ray
    m = b.flat.top_nodes["invTransform"][first["inst"][k][0]].reshape(4, 4)[:3, :3]
    assert np.linalg.det(m.astype(np.float64)) < 0 and ((N * D).sum(1) < 0).all()


@pytest.mark.parametrize("name", MIRROR_SCENES)
def test_float32_follows_the_same_chain(name):
    """The float32 restatement against the float64 one, 64 x 36, pixel-centre rays, K = 4: the same terminal primitive and instance for every pixel of
    mirror_wall, mirror_corridor and glass_box; on mirror_blob_room -- a reflection off a curved, mirrored, non-uniformly scaled body amplifies the
    rounding of the normal, and a neighbouring triangle or the other side of a compare is a different terminal -- 1 pixel of 2304 differs (0.04 %; the cap
    is 3 %).  Measured on the agreeing pixels: distance 1.9e-7 / 5.5e-7 / 1.1e-7 / 1.5e-7 relative, normals 6.0e-8 / 6.0e-8 / 3.5e-6 / 3.0e-8 absolute,
    albedo 1.5e-8 / 3.4e-8 / 2.7e-8 / 0 absolute on mirror_wall / mirror_corridor / mirror_blob_room / glass_box.  FLOAT32_* are the worst of each; the
    bounds asserted are twice those.  These are the figures the device test's looser bound of 8 x refers to."""
    b = mirror_scene(name)
    sc = U.oracle_scene(b)
    o, d = pixel_centre_rays(b.camera, 64, 36)
    a64, g64, i64 = M.chain(b.flat, sc, o, d, 4, b.material_textures)
    a32, g32, i32 = M.chain(b.flat, sc, o, d, 4, b.material_textures, dtype=np.float32)
    assert a32.dtype == np.float32 and g32.dtype == np.float32
    same = (i64["prim"] == i32["prim"]) & (i64["inst"] == i32["inst"])
    hit = same & (i64["prim"] >= 0)
    rel = np.abs(g32[hit, 3] - g64[hit, 3]) / g64[hit, 3]
    dn = np.abs(g32[same, :3] - g64[same, :3]).max()
    da = np.abs(a32[same, :3] - a64[same, :3]).max()
    print(f"{name}: same terminal {same.mean():.5f}, distance rel {rel.max():.2e}, normal abs {dn:.2e}, albedo abs {da:.2e}, "
          f"reflected {(i64['reflections'] > 0).mean():.3f}")
    if name == "mirror_blob_room":
        assert (~same).mean() <= BLOB_FLIP_CAP
    else:
        assert same.all()
    assert rel.max() <= 2 * FLOAT32_DISTANCE and dn <= 2 * FLOAT32_NORMAL and da <= 2 * FLOAT32_ALBEDO
    assert np.array_equal(a32[same, 3], a64[same, 3])
    assert np.array_equal(i32["reflections"][same], i64["reflections"][same]) and np.array_equal(i32["depth"][same], i64["depth"][same])
    assert (i64["reflections"] > 0).mean() > 0.05  # reflections are exercised


# ---- what it buys: the mirror wall, 64 x 64 ----------------------------------------------------------
QW = QH = 64
SPATIAL_R = 0.355  # test_guides_through_the_mirror_make_the_reflection_better: the ratio this restatement measures
TEMPORAL_R = 0.68  # test_a_history_behind_the_mirror_follows_the_virtual_image: likewise


def _reference(b, camera):
    sc = U.oracle_scene(b)
    hi, _ = O.render(sc, camera, QW, QH, 1024, threads=8)
    return sc, U.tonemap(hi[:, :3].reshape(QH, QW, 3), 1024, camera)


def test_guides_through_the_mirror_make_the_reflection_better():
    """Oracle alone, cornell_mirror_wall 64 x 64, seed 1: 4 spp filtered with five iterations under the defaults, tone-mapped RMSE against 1024 spp over
    the pixels whose FIRST hit is the mirror, guides from pixel-centre rays -- first-hit guides against guides through the mirror (K = 4, reflections on).
    The gate is (1 + r) / 2 times the first-hit figure, r = SPATIAL_R the ratio this restatement measured ("no better" is 1 and fails); the pixels
    outside the mirror stay within 1.02 x.
    Measured (440 mirror pixels): first-hit 1.068e-4, through the mirror 3.79e-5, r 0.355; outside the mirror 6.37e-4 -> 6.43e-4, 1.009 x."""
    b = scenes.cornell_mirror_wall(QW, QH)
    sc, ref = _reference(b, b.camera)
    lo, _ = O.render(sc, b.camera, QW, QH, 4, seed=1, threads=8)
    o, d = pixel_centre_rays(b.camera, QW, QH)
    a0, g0, _ = M.chain(b.flat, sc, o, d, 0)
    a4, g4, info = M.chain(b.flat, sc, o, d, 4)
    mirror = info["first_mirror"].reshape(QH, QW)
    assert mirror.sum() > 300 and (~mirror).sum() > 300

    def errors(a, g):
        out = U.tonemap(R.denoise_hdr(lo.reshape(QH, QW, 4), 4, a.reshape(QH, QW, 4), g.reshape(QH, QW, 4), 1, 5), 1, b.camera)
        return U.rmse(out[mirror], ref[mirror]), U.rmse(out[~mirror], ref[~mirror])
    (first_in, first_out), (through_in, through_out) = errors(a0, g0), errors(a4, g4)
    print(f"{int(mirror.sum())} mirror px, first-hit {first_in:.3e}, through the mirror {through_in:.3e}, ratio {through_in / first_in:.3f} "
          f"(r {SPATIAL_R}); outside {first_out:.3e} -> {through_out:.3e}, ratio {through_out / first_out:.4f}")
    assert through_in < (1 + SPATIAL_R) / 2 * first_in
    assert through_out <= 1.02 * first_out


def arc_camera(frame, width, height, frames=12, step_deg=2.0):
    """the cameras of the 12-frame arc: cornell_box's camera turned about the room's middle by `step_deg` per frame; the LAST frame is cornell_box's own"""
    a = np.radians(step_deg * (frame - (frames - 1)))
    return scenes._camera(width, height, (3.9 * np.sin(a), 1.0, -3.9 * np.cos(a)), (0.0, 1.0, 0.0), 40.0)


def test_a_history_behind_the_mirror_follows_the_virtual_image():
    """Oracle alone, cornell_mirror_wall 64 x 64: twelve 1-spp frames on an arc of 2 degrees per frame (first_sample = frame), the UNFILTERED history of
    temporal_ref.accumulate under the defaults, guides from pixel-centre rays of each frame's camera; tone-mapped RMSE of the last history against
    1024 spp from the last camera over the pixels whose first hit is the mirror.  Gates: through the mirror (K = 4) < (1 + r_t) / 2 x first-hit guides,
    r_t = TEMPORAL_R the ratio this restatement measured; the mean history count inside the mirror with reflections is within 25 % of the count
    outside it; with first-hit guides it is ABOVE the count outside: the mirror keeps a history it should lose -- the ghosting the feature removes.
    Measured (440 mirror pixels): first-hit 1.352e-4, history count 10.29 in the mirror against 5.69 outside; through the mirror 9.18e-5, count 4.83
    against 5.58; r_t 0.68.  The arc ENDS on the room's axis, where the mirror shows mostly the dark opening.  That choice matters and is the one the
    figures above were first taken with: on an arc that ends 11 or 22 degrees off the axis, where the mirror shows a lit side wall, the same run gives
    3.21e-4 -> 4.22e-4 (1.32) and 4.39e-4 -> 6.08e-4 (1.38) with the same counts -- after twelve 1-spp frames the RMSE of an unfiltered history is
    mostly variance, and a history that is rightly cut to five frames is noisier than a ghosted one of ten.  The counts are the robust statement."""
    b = scenes.cornell_mirror_wall(QW, QH)
    last = arc_camera(11, QW, QH)
    sc, ref = _reference(b, last)
    frames = []
    for f in range(12):
        cam = arc_camera(f, QW, QH)
        lo, _ = O.render(sc, cam, QW, QH, 1, seed=1, first_sample=f, threads=8)
        frames.append((cam, lo.reshape(QH, QW, 4)) + pixel_centre_rays(cam, QW, QH))
    out = {}
    for K in (0, 4):
        history = None
        for cam, lo, o, d in frames:
            a, g, info = M.chain(b.flat, sc, o, d, K)
            a, g = a.reshape(QH, QW, 4), g.reshape(QH, QW, 4)
            cn, nd, _ = T.accumulate(lo, 1, a, g, 1, cam, history=history)
            history = (cn, nd, cam)
        mirror = info["first_mirror"].reshape(QH, QW)
        albedo = R.prepare(lo, 1, a, g, 1)[1]
        img = U.tonemap(cn[..., :3] * albedo, 1, last)
        out[K] = (U.rmse(img[mirror], ref[mirror]), float(cn[..., 3][mirror].mean()), float(cn[..., 3][~mirror].mean()))
    (e0, in0, out0), (e4, in4, out4) = out[0], out[4]
    print(f"{int(mirror.sum())} mirror px: first-hit RMSE {e0:.3e}, history count {in0:.2f} in the mirror / {out0:.2f} outside; through the mirror "
          f"{e4:.3e}, count {in4:.2f} / {out4:.2f}; ratio {e4 / e0:.3f} (r_t {TEMPORAL_R})")
    assert e4 < (1 + TEMPORAL_R) / 2 * e0
    assert abs(in4 - out4) <= 0.25 * out4
    assert in0 > out0


def test_a_static_camera_keeps_its_histories():
    """no camera motion: the reprojection finds every pixel's own history with either guides -- the counts are those of a plain running mean"""
    b = scenes.cornell_mirror_wall(32, 32)
    sc = U.oracle_scene(b)
    o, d = pixel_centre_rays(b.camera, 32, 32)
    for K in (0, 4):
        a, g, info = M.chain(b.flat, sc, o, d, K)
        history = None
        for f in range(3):
            lo, _ = O.render(sc, b.camera, 32, 32, 1, seed=1, first_sample=f, threads=8)
            cn, nd, _ = T.accumulate(lo.reshape(32, 32, 4), 1, a.reshape(32, 32, 4), g.reshape(32, 32, 4), 1, b.camera, history=history)
            history = (cn, nd, b.camera)
        hit = (a[:, 3] > 0).reshape(32, 32)
        assert np.abs(cn[..., 3][hit] - 3).max() < 1e-6
