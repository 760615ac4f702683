"""The guide chain as tests/chain_ref.py restates it (include/ptamd.h, "guide chain"), on the oracle alone: what any implementation of the contract
has -- no glass, no change; parallel faces give the direction back; a grazing exit is total internal reflection --, what single precision costs it,
and that guides taken through the glass make the filtered image behind the glass better."""
import numpy as np
import pytest

import chain_ref as CH
import denoise_ref as R
import gpu_util as U
import orclib as O
from ptamd import layout as L, scenes
from test_denoise_ref import pixel_centre_rays

GLASS = L.material_basic_refractive(1.5)
BOX_CENTRE, BOX_HALF, BOX_YAW = np.array([-0.35, 0.602, 0.3]), np.array([0.3, 0.6, 0.3]), np.radians(20.0)  # the tall box of scenes.cornell_box


def glass_box_room(width, height):
    return scenes.cornell_box(width, height, box_materials=[L.material_diffuse(scenes.WHITE), GLASS])


def gpu_scene(name, width=64, height=36):
    """the four scenes the device is held against (tests/test_gpu_guide_chain.py)"""
    if name == "glass_box":
        return glass_box_room(width, height)
    if name == "behind_rough_glass":
        return scenes.cornell_behind_glass(width, height, rough=True)
    if name == "zoo_room":
        return scenes.zoo_room(width, height)
    return scenes.glass_first(width, height)


GPU_SCENES = ["glass_box", "behind_rough_glass", "zoo_room", "glass_first"]
FLOAT32_DISTANCE, FLOAT32_NORMAL = 1e-5, 1.9e-5  # the float32 restatement's own error against float64 (test_float32_follows_the_same_chain)


@pytest.mark.parametrize("K", [0, 1, 4])
def test_without_glass_or_with_no_transmissions_the_chain_is_the_first_hit(K):
    """K = 0 on a scene with glass, and any K on cornell_box: guide_deposits' values exactly"""
    for b in ([glass_box_room(32, 32)] if K == 0 else []) + [scenes.cornell_box(32, 32)]:
        sc = U.oracle_scene(b)
        o, d = pixel_centre_rays(b.camera, 32, 32)
        want_a, want_g = R.guide_deposits(b.flat, d, O.intersect_batch(sc, o, d, threads=8))
        a, g, info = CH.chain(b.flat, sc, o, d, K)
        assert np.array_equal(a, want_a) and np.array_equal(g, want_g)
        assert (info["depth"] == 0).all() and not info["tir"].any()


def _box_axes():
    c, s = np.cos(BOX_YAW), np.sin(BOX_YAW)
    return np.array([-s, 0.0, -c]), np.array([c, 0.0, -s])  # outward normals of the box's -z face (towards the camera) and of its +x face


def test_parallel_faces_give_the_direction_back_and_a_grazing_exit_is_reflected():
    b = glass_box_room(32, 32)
    sc = U.oracle_scene(b)
    front, side = _box_axes()
    face = BOX_CENTRE + front * BOX_HALF[2]  # centre of the face towards the camera
    # through the two parallel faces, from straight on to 50 degrees off: the ray leaves parallel to how it came (stage 0 enters, stage 1 leaves,
    # stage 2 ends on a wall or the floor)
    ang = np.radians([0.0, 10.0, 25.0, 50.0])
    d = np.array([-front * np.cos(x) - side * np.sin(x) for x in ang])
    o = face[None] - d * 1.0 + side[None] * 0.1 * np.sin(ang)[:, None]  # (aimed a little to the side so that the exit stays on the back face)
    a, g, info = CH.chain(b.flat, sc, o, d, 4)
    assert (info["depth"] == 2).all() and not info["tir"].any() and (a[:, 3] == 1).all()
    assert np.abs(info["dir"] - d).max() < 1e-6
    # at normal incidence the distance sum is the straight-line distance, less the two offsets of 1e-4 the continuation rays start with
    straight = np.linalg.norm(info["point"][0] - o[0])
    assert abs(g[0, 3] - straight) < 2.5 * CH.EPS, (g[0, 3], straight)
    assert g[0, 3] > 1.0 + 2 * BOX_HALF[2]  # ... and it lies behind the box
    # off the normal the path inside is displaced sideways: longer than the straight line to the same point's depth, never shorter than the chord
    assert (g[1:, 3] > np.linalg.norm(info["point"][1:] - o[1:], axis=1) - 2.5 * CH.EPS).all()
    # K = 1 stops at the back face, on glass: the glass's own deposit (albedo 1, hit), at the distance to that face
    a1, g1, info1 = CH.chain(b.flat, sc, o[:1], d[:1], 1)
    assert info1["depth"][0] == 1 and (a1[0] == 1).all() and abs(g1[0, 3] - (1.0 + 2 * BOX_HALF[2])) < 2 * CH.EPS
    assert np.abs(g1[0, :3] - front).max() < 1e-6  # the back face's normal, turned to face the ray inside the glass

    # entering the front face 45 degrees off, 5 cm from its edge: inside, the ray meets the side face beyond the critical angle
    # (asin(1 / 1.5) = 41.8 degrees; it arrives at 90 - asin(sin 45 / 1.5) = 61.9)
    dg = (-front + side) / np.sqrt(2.0)
    og = face + side * 0.25 - dg * 0.3  # (from inside the room: the left wall is near)
    a, g, info = CH.chain(b.flat, sc, og[None], dg[None], 4)
    assert info["tir"][0] and info["depth"][0] == 1
    assert (a[0] == 1).all()  # the terminal is the glass itself
    assert np.abs(g[0, :3] + side).max() < 1e-6  # the side face's normal, facing the ray: inwards


@pytest.mark.parametrize("name", GPU_SCENES)
def test_float32_follows_the_same_chain(name):
    """The float32 restatement against the float64 one, 64 x 36, pixel-centre rays, K = 4: the same terminal primitive and instance for every pixel.
    Measured on those: distance 8.8e-7 / 2.4e-7 / 9.9e-6 / 1.8e-7 relative and normals 5.0e-8 / 5.2e-8 / 1.9e-5 / 0 absolute on glass_box /
    behind_rough_glass / zoo_room / glass_first -- FLOAT32_DISTANCE and FLOAT32_NORMAL are zoo_room's, the worst: a chain of up to five segments whose
    glass is a sheared instance (its normal transform amplifies the rounding of the interpolated normal, and the refracted direction inherits it).
    The bounds asserted are twice those.  These are the figures the device test's looser bound of 8 x refers to."""
    b = gpu_scene(name)
    sc = U.oracle_scene(b)
    o, d = pixel_centre_rays(b.camera, 64, 36)
    a64, g64, i64 = CH.chain(b.flat, sc, o, d, 4, b.material_textures)
    a32, g32, i32 = CH.chain(b.flat, sc, o, d, 4, b.material_textures, dtype=np.float32)
    assert a32.dtype == np.float32 and g32.dtype == np.float32
    same = (i64["prim"] == i32["prim"]) & (i64["inst"] == i32["inst"])
    hit = same & (i64["prim"] >= 0)
    rel = np.abs(g32[hit, 3] - g64[hit, 3]) / g64[hit, 3]
    dn = np.abs(g32[same, :3] - g64[same, :3]).max()
    print(f"{name}: same terminal {same.mean():.4f}, distance rel {rel.max():.2e}, normal abs {dn:.2e}, through glass {(i64['depth'] > 0).mean():.3f}")
    assert same.all()
    assert rel.max() <= 2 * FLOAT32_DISTANCE and dn <= 2 * FLOAT32_NORMAL
    assert np.array_equal(a32[same, 3], a64[same, 3]) and np.abs(a32[same, :3] - a64[same, :3]).max() <= 1e-6
    assert (i64["depth"] > 0).mean() > 0.02  # the chain is exercised


QUALITY = {
    # scene -> r, the ratio the restatement measures (tone-mapped RMSE over first-hit-glass pixels, guides through glass / first-hit guides)
    "glass_box": 0.88,
    "behind_basic_pane": 0.85,
    "behind_rough_pane": 0.83,
}


def _quality_scene(name):
    if name == "glass_box":
        return glass_box_room(64, 64)
    return scenes.cornell_behind_glass(64, 64, rough=name == "behind_rough_pane")


@pytest.mark.parametrize("name", list(QUALITY))
def test_guides_through_glass_make_the_image_behind_glass_better(name):
    """Oracle alone, 64 x 64: 4 spp filtered with five iterations under the defaults, tone-mapped RMSE against 1024 spp over the pixels whose FIRST hit
    is glass, guides from pixel-centre rays -- first-hit guides against guides through the glass (K = 4).  The gate is (1 + r) / 2 times the first-hit
    figure, r the ratio this restatement measured (QUALITY above; "no better" is ratio 1 and fails); pixels outside the glass stay within 1.005 x.
    Measured:  glass_box  first-hit 6.49e-5, through 5.72e-5, r 0.88 (430 px);  behind_basic_pane  9.82e-5 / 8.34e-5, r 0.85 (1274 px);
    behind_rough_pane  9.84e-5 / 8.13e-5, r 0.83; outside the glass the ratios are 1.0001 / 0.997 / 0.997."""
    b = _quality_scene(name)
    sc = U.oracle_scene(b)
    W = H = 64
    lo, _ = O.render(sc, b.camera, W, H, 4, threads=8)
    hi, _ = O.render(sc, b.camera, W, H, 1024, threads=8)
    ref = U.tonemap(hi[:, :3].reshape(H, W, 3), 1024, b.camera)
    o, d = pixel_centre_rays(b.camera, W, H)
    a0, g0, _ = CH.chain(b.flat, sc, o, d, 0)
    a4, g4, info = CH.chain(b.flat, sc, o, d, 4)
    glass = info["first_glass"].reshape(H, W)
    assert glass.sum() > 300 and (~glass).sum() > 300

    def errors(a, g):
        out = U.tonemap(R.denoise_hdr(lo.reshape(H, W, 4), 4, a.reshape(H, W, 4), g.reshape(H, W, 4), 1, 5), 1, b.camera)
        return U.rmse(out[glass], ref[glass]), U.rmse(out[~glass], ref[~glass])
    (first_in, first_out), (through_in, through_out) = errors(a0, g0), errors(a4, g4)
    r = QUALITY[name]
    print(f"{name}: {int(glass.sum())} glass px, first-hit {first_in:.3e}, through glass {through_in:.3e}, ratio {through_in / first_in:.3f} (r {r}); "
          f"outside {first_out:.3e} -> {through_out:.3e}, ratio {through_out / first_out:.4f}")
    assert through_in < (1 + r) / 2 * first_in
    assert through_out <= 1.005 * first_out
