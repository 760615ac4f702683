"""Instance motion on the device (pt_set_instance_motion, k_guides<true>, k_temporal<true>; include/ptamd.h "instance motion") against its numpy
restatement (tests/motion_ref.py): the motion-aware accumulate on the synthetic moved sphere, the two guide deposits on a scene of mirrored,
sheared and non-uniformly scaled instances, a rendered moving instance, the refusals, the C++ example."""
import math
import os
import subprocess

import numpy as np
import pytest

import gpu_util as U
import motion_ref as M
import temporal_ref as T
from ptamd import device as D, host as H, layout as L, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

_ONE = {}


def one_instance_flat():
    """a scene of one instance (the Cornell box): what a context must hold before a motion can be set on it"""
    if "flat" not in _ONE:
        _ONE["flat"] = scenes.cornell_box(64, 64).flat
    return _ONE["flat"]


def motion_ctx(gpu, width, height):
    """a context on which a motion is set -- every leaf where it was: nothing moves, and the motion kernels are the ones that run"""
    flat = one_instance_flat()
    ctx = U.make_ctx(gpu, flat, width, height)
    ctx.set_instance_motion(flat.top_nodes)
    assert ctx.instance_motion == (True, 0)
    return ctx


def load(ctx, case, motion=True):
    ctx.write_accum(case["accum"], case["spp"])
    ctx.write_guides(case["albedo_hits"], case["normal_depth"], case["gspp"])
    if motion:
        ctx.write_motion_guides(case["motion"], case["prev_normal"])
    ctx.set_camera(case["camera"])
    ctx.write_temporal(case["hist_cn"], case["hist_nd"], case["hist_camera"])


def read(ctx, case):
    cn, nd = ctx.read_temporal()
    return cn.reshape(case["height"], case["width"], 4), nd.reshape(case["height"], case["width"], 4)


# ---------------------------------------------------------------- 1. k_temporal<true> against the restatement
@pytest.mark.parametrize("turn", [False, True])
@pytest.mark.parametrize("width,height", T.SIZES)
def test_accumulate_with_motion_matches_the_restatement(gpu, width, height, turn):
    case = M.make_moved_case("pan", width, height, turn=turn)
    name = f"pan {width}x{height}{', turned' if turn else ''}"
    ctx = motion_ctx(gpu, width, height)
    load(ctx, case)
    ctx.temporal_accumulate()
    cn, nd = read(ctx, case)
    ref, bound = M.bound(case)
    err_rgb = float(np.abs(cn[..., :3].astype(np.float64) - ref[..., :3]).max())
    err_n = float(np.abs(cn[..., 3].astype(np.float64) - ref[..., 3]).max())
    U.record_margin(f"temporal with motion vs restatement: {name}", error_rgb=err_rgb, error_count=err_n, bound=bound)
    print(f"{name}: rgb error {err_rgb:.3e}, count error {err_n:.3e}, bound {bound:.3e}")
    assert err_rgb <= bound and err_n <= bound
    load(ctx, case)  # (the sets flipped: the history goes into what is now the newest one)
    ctx.temporal_accumulate()
    cn2, nd2 = read(ctx, case)
    assert np.array_equal(cn2.view(np.uint32), cn.view(np.uint32)) and np.array_equal(nd2.view(np.uint32), nd.view(np.uint32))
    ctx.close()
    plain = gpu.Context(width, height)
    load(plain, case, motion=False)
    plain.temporal_accumulate()
    pcn, pnd = read(plain, case)
    plain.close()
    sphere = case["sphere"]
    differs = float(np.abs(cn[sphere].astype(np.float64) - pcn[sphere]).max())
    U.record_margin(f"temporal with motion vs the plain kernel on the sphere: {name}", difference=differs, bound=bound)
    assert differs > 10 * bound
    assert np.array_equal(nd.view(np.uint32), pnd.view(np.uint32))  # the set written out holds the CURRENT (n, z) either way
    if (width, height) != (16, 16):  # (14 pixels of sphere there: the normal term rejects most taps either way)
        assert cn[sphere, 3].mean() > 2.0 > pcn[sphere, 3].mean()


# ---------------------------------------------------------------- 2. zero motion is the plain kernel
@pytest.mark.parametrize("pose", ["pan", "history"])
def test_zero_motion_gives_the_plain_kernels_bits(gpu, pose):
    case = M.make_moved_case(pose, 70, 45, zero_motion=True, same_guides=(pose == "history"))
    assert not case["motion"].any() and np.array_equal(case["prev_normal"][..., :3], case["normal_depth"][..., :3])
    ctx = motion_ctx(gpu, 70, 45)
    load(ctx, case)
    ctx.temporal_accumulate()
    cn, nd = read(ctx, case)
    never = gpu.Context(70, 45)
    load(never, case, motion=False)
    never.temporal_accumulate()
    pcn, pnd = read(never, case)
    assert (cn[..., 3] > 1.5).mean() > 0.5  # the history was used
    assert np.array_equal(cn.view(np.uint32), pcn.view(np.uint32)) and np.array_equal(nd.view(np.uint32), pnd.view(np.uint32))
    ctx.close()
    never.close()


# ---------------------------------------------------------------- 3. the guide deposits
def zoo_states():
    """(bundle, flat A, flat B): scenes.zoo_room(64, 36), and the same with scene node 2 (the non-uniformly scaled parent; its sheared child follows)
    moved and turned and node 1 (the mirrored blob) translated.  Nodes 0 (the room) and 4 (the small blob) stay."""
    if "zoo" not in _ONE:
        b = scenes.zoo_room(64, 36)
        a = b.scene.flatten()
        b.scene.set_transform(2, location=(0.4, 0.5, 0.2), orientation_wxyz=scenes._axis_angle((0, 1, 0), 0.35))
        b.scene.set_transform(1, location=(-0.3, 0.55, 0.25))
        _ONE["zoo"] = (b, a, b.scene.flatten())
    return _ONE["zoo"]


def _tiles(width, height, parity, size=16):
    return [(x, y, min(x + size, width), min(y + size, height)) for y in range(0, height, size) for x in range(0, width, size)
            if ((x // size) + (y // size)) % 2 == parity]


@pytest.mark.parametrize("entered", [False, True])
def test_guide_deposits_of_moved_instances(gpu, entered):
    """entered: PT_FLAG_NO_BAKED_INSTANCES -- instances entered at traversal and instances copied to world space must both report the right record"""
    b, flat_a, flat_b = zoo_states()
    w, h, n = b.width, b.height, b.width * b.height
    flags = gpu.FLAG_NO_BAKED_INSTANCES if entered else 0
    leaves = np.flatnonzero(flat_b.top_nodes["isLeaf"] != 0)
    moved_leaf = np.array([not np.array_equal(flat_a.top_nodes["invTransform"][k], flat_b.top_nodes["invTransform"][k]) for k in range(len(flat_b.top_nodes))])
    assert len(flat_a.top_nodes) == len(flat_b.top_nodes) and moved_leaf[leaves].sum() == 3 and (~moved_leaf[leaves]).sum() == 2

    def ctx_on_b(motion=True, **kw):
        c = U.make_ctx(gpu, flat_b, w, h, camera=b.camera, flags=flags, **kw)
        if motion:
            c.set_instance_motion(flat_a.top_nodes)
            assert c.instance_motion == (True, 3)
        return c
    ctx = ctx_on_b()
    o, d, pixel = ctx.gen_rays(0, n)
    hits = ctx.intersect(o, d)  # the per-ray kernel the guide pass runs: the same t bits
    ctx.render_guides(1)
    got_a, got_g = ctx.read_guides()
    got_m, got_pn = ctx.read_motion_guides()
    m, pn, g = got_m[pixel], got_pn[pixel], got_g[pixel]
    want_m, want_pn, extra = M.motion_deposits(flat_b, flat_a.top_nodes, o, d, hits, np.float64)
    want_m32 = M.motion_deposits(flat_b, flat_a.top_nodes, o, d, hits, np.float32)[0]
    assert want_m32.dtype == np.float32
    hit = hits["prim"] >= 0
    moved = hit & moved_leaf[np.where(hit, hits["inst"], 0)]
    assert moved.sum() > 100 and (hit & ~moved).sum() > 100 and (~hit).sum() > 0
    # motion: 8 x what single precision costs the restatement + 1e-6 x the scene's extent
    root = flat_b.top_nodes[flat_b.top_root]
    extent = float(max(np.abs(root["min"][:3]).max(), np.abs(root["max"][:3]).max()))
    bound = 8.0 * float(np.abs(want_m32.astype(np.float64) - want_m).max()) + 1e-6 * extent
    err = float(np.abs(m.astype(np.float64) - want_m).max())
    U.record_margin(f"motion guide vs restatement: zoo_room 64x36, {'entered' if entered else 'copied'}", error=err, bound=bound,
                    largest=float(np.abs(want_m).max()), moved_pixels=int(moved.sum()))
    print(f"motion deposits ({'entered' if entered else 'copied'}): error {err:.3e}, bound {bound:.3e}, largest displacement {np.abs(want_m).max():.3f}")
    assert err <= bound and np.abs(want_m[moved]).max() > 0.05 and np.all(m[:, 3] == 0) and np.all(pn[:, 3] == 0)
    # prev_normal: 1e-5 absolute, the tolerance of the guide normals (tests/test_gpu_guides.py).  Whether N was flipped is the device's decision
    # where N.D is within round-off of zero: there the flip is read off the device's own normal deposit.
    flip_dev = (g[:, :3].astype(np.float64) * extra["normal_unflipped"]).sum(1) < 0
    grazing = hit & (np.abs(extra["n_dot_d"]) < 1e-6)
    assert grazing.mean() < 1e-2
    want_pn[grazing, :3] = np.where(flip_dev[grazing, None], -extra["then_unflipped"][grazing], extra["then_unflipped"][grazing])
    err_n = float(np.abs(pn[:, :3].astype(np.float64) - want_pn[:, :3]).max())
    U.record_margin(f"prev_normal guide vs restatement: zoo_room 64x36, {'entered' if entered else 'copied'}", error=err_n, gate=1e-5,
                    flipped=int((extra["n_dot_d"][hit] > 0).sum()))
    assert err_n <= 1e-5  # (the flipped deposits, a handful at the blobs' silhouettes, are counted in the margin above)
    assert np.abs(pn[moved, :3] - g[moved, :3]).max() > 1e-2  # the turned instances' normals did turn
    # an instance that stayed: exact zeros, and the bits of N; a miss: zero and -D with the bits of normal_depth.xyz
    for mask in (hit & ~moved, ~hit):
        assert np.all(m[mask] == 0)
        assert np.array_equal(pn[mask, :3].view(np.uint32), g[mask, :3].view(np.uint32))
    # the other two sums do not know about the motion
    plain = ctx_on_b(motion=False)
    plain.render_guides(1)
    pa, pg = plain.read_guides()
    assert np.array_equal(pa.view(np.uint32), got_a.view(np.uint32)) and np.array_equal(pg.view(np.uint32), got_g.view(np.uint32))
    assert not any(x.any() for x in plain.read_motion_guides())
    plain.close()
    ctx.close()
    # 2 + 3 samples are 5 samples, and complementary tilings add up to the whole, for the motion sums as well
    whole = ctx_on_b(samples_in_flight=16)
    whole.render_guides(5)
    wm, wpn = whole.read_motion_guides()
    split = ctx_on_b(samples_in_flight=16)
    split.render_guides(2)
    split.render_guides(3)
    sm, spn = split.read_motion_guides()
    assert np.array_equal(sm.view(np.uint32), wm.view(np.uint32)) and np.array_equal(spn.view(np.uint32), wpn.view(np.uint32))
    parts = []
    for parity in (0, 1):
        t = ctx_on_b(samples_in_flight=16)
        t.set_tiles(_tiles(w, h, parity))
        t.render_guides(5)
        parts.append(t.read_motion_guides())
        t.close()
    assert np.array_equal(parts[0][0] + parts[1][0], wm) and np.array_equal(parts[0][1] + parts[1][1], wpn)
    assert (np.abs(parts[0][1][:, :3]).sum(1) == 0).any() and (np.abs(parts[1][1][:, :3]).sum(1) == 0).any()  # each left the other's pixels alone
    whole.close()
    split.close()


# ---------------------------------------------------------------- 4. a rendered moving instance
def _sliding_blob():
    mats = scenes._room_materials()
    mb = scenes._MeshBuilder()
    scenes._room(mb, mats)
    scene = H.Scene()
    scene.add_node(mb.build(mats, H.BVH_BINNED_SAH))
    blob = scenes.blob_mesh(L.material_diffuse((0.8, 0.8, 0.8)), level=3, builder=H.BVH_BINNED_SAH)
    node = scene.add_node(blob, location=(-0.3, 0.6, 0.0), scale=(0.9, 0.9, 0.9))
    return scene, node, scenes._camera(64, 64, (0.0, 1.0, -3.9), (0.0, 1.0, 0.0), 40.0)


def test_a_rendered_moving_instance_keeps_its_history_with_motion(gpu):
    """Twelve 1-spp frames, static camera; the blob slides 0.05 along x and turns 3 degrees about y per frame.  With the motion set every frame the
    blob's pixels keep a history and the filtered last frame is closer (tone-mapped RMSE, over those pixels) to 256 spp than without.  Measured on an
    MI355X (EXPERIMENTS.md, "Instance motion"): mean count 2.74 against 1.71, RMSE 2.58e-4 against 2.79e-4 over 342 pixels; only the orderings are gated."""
    frames = 12
    scene, node, cam = _sliding_blob()
    flats = []
    for f in range(frames):
        scene.set_transform(node, location=(-0.3 + 0.05 * f, 0.6, 0.0), orientation_wxyz=scenes._axis_angle((0, 1, 0), math.radians(3.0 * f)))
        flats.append(scene.flatten() if f == 0 else scene.flatten_dynamic(flats[0])[0])
    blob_leaf = 1  # (leaves of the host library's top level are the scene nodes, in order)
    assert flats[-1].top_nodes["isLeaf"][blob_leaf] and not np.array_equal(flats[0].top_nodes["invTransform"][blob_leaf], flats[-1].top_nodes["invTransform"][blob_leaf])

    def loop(with_motion):
        ctx = U.make_ctx(gpu, flats[0], 64, 64, camera=cam)
        for f in range(frames):
            if f:
                ctx.upload_dynamic(flats[f])
            ctx.set_sample_base(f)
            ctx.clear()
            if with_motion and f:
                ctx.set_instance_motion(flats[f - 1].top_nodes)
                assert ctx.instance_motion == (True, 1)
            ctx.render(1)
            ctx.render_guides(1)
            ctx.temporal_accumulate()
        assert ctx.temporal_frames == frames
        cn, _ = ctx.read_temporal()
        out = ctx.denoise(5, hdr=True, input_temporal=True)[..., :3]
        o, d, pixel = ctx.gen_rays(0, 64 * 64)
        hits = ctx.intersect(o, d)
        blob = np.zeros(64 * 64, bool)
        blob[pixel] = hits["inst"] == blob_leaf
        ctx.close()
        return cn.reshape(64, 64, 4), out, blob.reshape(64, 64)
    cn_a, out_a, blob = loop(True)
    cn_b, out_b, blob_b = loop(False)
    assert np.array_equal(blob, blob_b) and blob.sum() > 150
    ref = U.make_ctx(gpu, flats[-1], 64, 64, camera=cam)
    ref.set_sample_base(1000)
    ref.render(256)
    want = U.tonemap(ref.read_accum()[:, :3].reshape(64, 64, 3), 256, cam)
    ref.close()
    count_a, count_b = float(cn_a[blob, 3].mean()), float(cn_b[blob, 3].mean())
    e_a, e_b = U.rmse(U.tonemap(out_a, 1, cam)[blob], want[blob]), U.rmse(U.tonemap(out_b, 1, cam)[blob], want[blob])
    U.record_margin("rendered moving blob, cornell room 64x64, 12 frames of 1 spp", count_with_motion=count_a, count_without=count_b,
                    rmse_with_motion=e_a, rmse_without=e_b, ratio=e_a / e_b, blob_pixels=int(blob.sum()))
    print(f"moving blob ({blob.sum()} pixels): mean history count {count_a:.2f} with motion, {count_b:.2f} without; tone-mapped RMSE against 256 spp "
          f"{e_a:.3e} with, {e_b:.3e} without, ratio {e_a / e_b:.3f}")
    assert count_a > 2.0 and count_a > count_b
    assert e_a < e_b


# ---------------------------------------------------------------- 5. refusals and lifetimes
def test_refusals_and_lifetimes(gpu):
    INVALID, STATE, UNSUPPORTED = -1, -3, -4
    flat = one_instance_flat()
    top = flat.top_nodes
    assert len(top) == 1
    bare = gpu.Context(16, 16)
    assert bare.instance_motion == (False, 0) and bare.motion_guides_device_ptr(0) == 0
    assert U.status(lambda: bare.set_instance_motion(top)) == STATE  # no dynamic state
    bare.close()
    parity = U.make_ctx(gpu, flat, 16, 16, rng_mode=D.RNG_LFSR113_PARITY)
    assert U.status(lambda: parity.set_instance_motion(top)) == UNSUPPORTED
    parity.close()
    refill = U.make_ctx(gpu, flat, 64, 64, max_active_rays=1024)
    assert U.status(lambda: refill.set_instance_motion(top)) == UNSUPPORTED
    refill.close()

    ctx = U.make_ctx(gpu, flat, 16, 16, camera=scenes.cornell_box(16, 16).camera)
    assert U.status(lambda: ctx.set_instance_motion(np.zeros((2, 16), np.float32))) == INVALID  # not the state's node count
    bad = top["invTransform"].copy()
    bad[0, 0:3] = 0.0
    assert U.status(lambda: ctx.set_instance_motion(bad)) == INVALID  # singular
    bad = top["invTransform"].copy()
    bad[0, 13] = np.nan
    assert U.status(lambda: ctx.set_instance_motion(bad)) == INVALID  # not finite
    assert ctx.instance_motion == (False, 0)  # a refused call is no call
    was = top["invTransform"].copy()
    was[0, 12] += 0.25  # the box was a quarter to the side (in its own space)
    ctx.set_instance_motion(was)
    assert ctx.instance_motion == (True, 1)
    assert ctx.motion_guides_device_ptr(0) and ctx.motion_guides_device_ptr(1) and ctx.motion_guides_device_ptr(0) != ctx.motion_guides_device_ptr(1)
    ctx.set_instance_motion(top)  # (a record array: its invTransform is taken)
    assert ctx.instance_motion == (True, 0)
    ctx.set_instance_motion(was)
    ctx.render_guides(1)
    assert U.status(lambda: ctx.set_instance_motion(was)) == STATE  # guide samples are in: neither set ...
    assert U.status(lambda: ctx.set_instance_motion(None)) == STATE  # ... nor forgotten
    m, pn = ctx.read_motion_guides()
    on_box = m[:, 0] != 0  # every hit moved by -0.25 along x, a miss by nothing
    assert on_box.sum() > 128 and np.allclose(m[on_box, 0], -0.25, rtol=0, atol=1e-6) and not m[:, 1:].any()
    assert np.abs(pn[:, :3]).sum(1).min() > 0.99 and not pn[:, 3].any()
    ctx.clear()  # zeroes the sums, keeps the motion
    assert ctx.instance_motion == (True, 1) and ctx.guide_samples == 0
    assert not any(x.any() for x in ctx.read_motion_guides())
    ctx.set_instance_motion(None)
    assert ctx.instance_motion == (False, 0)
    ctx.set_instance_motion(was)
    ctx.upload_dynamic(flat)  # a tick: the indices were the old state's
    assert ctx.instance_motion == (False, 0)
    # pt_write_guides leaves the motion sums alone
    rng = np.random.default_rng(5)
    wm, wpn = rng.normal(size=(256, 4)).astype(np.float32), rng.normal(size=(256, 4)).astype(np.float32)
    ctx.write_motion_guides(wm, wpn)
    ctx.write_guides(np.ones((256, 4), np.float32), np.ones((256, 4), np.float32), 3)
    m, pn = ctx.read_motion_guides()
    assert np.array_equal(m, wm) and np.array_equal(pn, wpn) and ctx.guide_samples == 3
    ctx.close()


# ---------------------------------------------------------------- 6. the C++ example
def test_cpp_moving_example(gpu, tmp_path):
    """examples/moving_cornell.cpp: three images of one size that differ; over the blob's final screen rectangle the image filtered over the history
    with motion has less high-frequency energy than the one without."""
    paths = [tmp_path / n for n in ("filtered.ppm", "temporal_plain.ppm", "temporal_motion.ppm")]
    r = subprocess.run([os.path.join(ROOT, "examples", "moving_cornell"), "12"] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split() if "=" in kv)
    assert int(fields["frames"]) == 12 and int(fields["spp"]) == 1 and int(fields["temporal_frames"]) == 12 and int(fields["moving"]) == 1
    x0, y0, x1, y1 = (int(v) for v in fields["blob_rect"].split(","))
    alone, without, with_motion = (U.read_ppm(p) for p in paths)
    assert alone.shape == without.shape == with_motion.shape == (256, 256, 3)
    assert not np.array_equal(without, with_motion) and not np.array_equal(alone, with_motion)
    assert 0 <= x0 < x1 <= 256 and 0 <= y0 < y1 <= 256 and (x1 - x0) * (y1 - y0) > 400
    lw, lm = (U.mean_abs_laplacian(x[y0:y1, x0:x1]) for x in (without, with_motion))
    print(f"mean |Laplacian| over the blob's rectangle: over the history without motion {lw:.4f}, with motion {lm:.4f}")
    assert lm < lw
