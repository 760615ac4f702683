"""Vertex motion on the device (pt_set_vertex_motion, k_guides<2>; include/ptamd.h "vertex motion") against its numpy restatement
(tests/vertex_motion_ref.py): the two guide deposits of a refitted mesh over both refit routes, both instance routes and two builders, the cases
where nothing deformed, a pipelined upload, a rendered leaning blob, the refusals, the C++ example."""
import os
import subprocess

import numpy as np
import pytest

import gpu_util as U
import vertex_motion_ref as V
from ptamd import device as D, host as H, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _on_second_state(gpu, room, flat_a, flat_b, route, flags=0, vertex=True, prev_top=None, vertex_first=False, **kw):
    """a context that held flat_a, took the sphere's current shape (flat_b) by `route`, ticked and cleared; then the motions asked for"""
    c = U.make_ctx(gpu, flat_a, room.width, room.height, camera=room.camera, flags=flags, **kw)
    room.refit_on(c, route, flat_b)
    c.clear()
    if vertex and vertex_first:
        c.set_vertex_motion()
    if prev_top is not None:
        c.set_instance_motion(prev_top)
    if vertex and not vertex_first:
        c.set_vertex_motion()
    if vertex:
        assert c.vertex_motion == (True, 1)
    return c


def _changed_triangles(flat_a, flat_b):
    changed = np.any(flat_a.vertices["vertex"] != flat_b.vertices["vertex"], 1) | np.any(flat_a.vertices["normal"] != flat_b.vertices["normal"], 1)
    return changed[flat_b.triangles["indices"]].any(1)


def _check_deposits(name, ctx, flat_now, flat_then, prev_top, thin_lens=False, least=0.02):
    """one guide sample of ctx against the restatement; returns what the callers compare further: (pixel, hits, deformed mask, the four sums)"""
    n = ctx.width * ctx.height
    o, d, pixel = ctx.gen_rays(0, n)
    hits = ctx.intersect(o, d)  # the per-ray kernel the guide pass runs: the same t, u, v bits
    ctx.render_guides(1)
    got_a, got_g = ctx.read_guides()
    got_m, got_pn = ctx.read_motion_guides()
    m, pn, g = got_m[pixel], got_pn[pixel], got_g[pixel]
    want_m, want_pn, extra = V.deposits(flat_now, flat_then, prev_top, o, d, hits, np.float64, thin_lens)
    want_m32 = V.deposits(flat_now, flat_then, prev_top, o, d, hits, np.float32, thin_lens)[0]
    assert want_m32.dtype == np.float32
    hit = hits["prim"] >= 0
    deformed = hit & _changed_triangles(flat_then, flat_now)[np.where(hit, hits["prim"], 0)]
    assert deformed.sum() > 100 and (hit & ~deformed).sum() > 100 and (~hit).sum() > 0  # (tests/test_vertex_motion_cpu.py states this of the scene)
    # motion: 8 x what single precision costs the restatement + 1e-6 x the scene's extent
    bound = 8.0 * float(np.abs(want_m32.astype(np.float64) - want_m).max()) + 1e-6 * V.scene_extent(flat_now)
    err = float(np.abs(m.astype(np.float64) - want_m).max())
    largest = float(np.abs(want_m[deformed, :3]).max())
    U.record_margin(f"vertex motion guide vs restatement: {name}", error=err, bound=bound, largest=largest, deformed_pixels=int(deformed.sum()))
    print(f"{name}: motion error {err:.3e}, bound {bound:.3e}, largest displacement on the blob {largest:.3f}, {deformed.sum()} deformed pixels")
    assert err <= bound and largest > least and np.all(m[:, 3] == 0) and np.all(pn[:, 3] == 0)
    # prev_normal: 1e-5 absolute; where N.D is within round-off of zero the flip is read off the device's own normal deposit
    flip_dev = (g[:, :3].astype(np.float64) * extra["normal_unflipped"]).sum(1) < 0
    grazing = hit & (np.abs(extra["n_dot_d"]) < 1e-6)
    assert grazing.mean() < 1e-2
    want_pn[grazing, :3] = np.where(flip_dev[grazing, None], -extra["then_unflipped"][grazing], extra["then_unflipped"][grazing])
    err_n = float(np.abs(pn[:, :3].astype(np.float64) - want_pn[:, :3]).max())
    U.record_margin(f"vertex motion prev_normal vs restatement: {name}", error=err_n, gate=1e-5, flipped=int((extra["n_dot_d"][hit] > 0).sum()))
    print(f"{name}: prev_normal error {err_n:.3e}")
    assert err_n <= 1e-5
    assert np.abs(pn[deformed, :3] - g[deformed, :3]).max() > 1e-2  # the twisted surface's normals did turn
    return pixel, hits, deformed, (got_a, got_g, got_m, got_pn)


# ---------------------------------------------------------------- 1. deposits against the restatement
@pytest.mark.parametrize("builder", ["BVH_BINNED_SAH", "BVH_SPATIAL_SPLIT"])
@pytest.mark.parametrize("entered", [False, True])
@pytest.mark.parametrize("route", ["host_nodes", "device"])
def test_guide_deposits_of_a_refitted_mesh(gpu, route, entered, builder):
    """state A, the sphere twisted and squashed (frame 1 of test_deforming_mesh_through_refit) for state B, one guide sample with vertex motion set"""
    room = V.DeformingRoom(getattr(H, builder))
    flat_a, flat_b = room.flat0, room.frame(1)
    flags = gpu.FLAG_NO_BAKED_INSTANCES if entered else 0
    name = f"deforming room 64x36, {route}, {'entered' if entered else 'copied'}, {builder}"
    ctx = _on_second_state(gpu, room, flat_a, flat_b, route, flags)
    pixel, hits, deformed, (got_a, got_g, got_m, got_pn) = _check_deposits(name, ctx, flat_b, flat_a, None)
    m, pn, g = got_m[pixel], got_pn[pixel], got_g[pixel]
    assert np.all(_bits(m[~deformed]) == 0)  # the room and the misses: exact zeros ...
    assert _same_bits(pn[~deformed, :3], g[~deformed, :3])  # ... and the bits of normal_depth.xyz
    ctx.close()
    plain = _on_second_state(gpu, room, flat_a, flat_b, route, flags, vertex=False)  # the other two sums do not know about the motion
    assert plain.vertex_motion == (False, 0)
    plain.render_guides(1)
    pa, pg = plain.read_guides()
    assert _same_bits(pa, got_a) and _same_bits(pg, got_g)
    plain.close()


def test_guide_deposits_through_a_thin_lens(gpu):
    room = V.DeformingRoom(thin_lens=True)
    assert room.camera["thinLensEnabled"]
    flat_a, flat_b = room.flat0, room.frame(1)
    ctx = _on_second_state(gpu, room, flat_a, flat_b, "device")
    pixel, hits, deformed, sums = _check_deposits("deforming room 64x36, thin lens", ctx, flat_b, flat_a, None, thin_lens=True)
    assert np.all(_bits(sums[2][pixel][~deformed]) == 0)
    ctx.close()


@pytest.mark.parametrize("route,entered", [("host_nodes", True), ("device", False)])
def test_guide_deposits_of_a_refitted_and_reposed_mesh(gpu, route, entered):
    """the sphere's instance is turned and moved by the same tick, the room shifted: instance motion and vertex motion together, in either order of the
    setters; pixels of the (undeformed, shifted) room are bit-equal to a context with the instance motion alone"""
    room = V.DeformingRoom()
    flat_a = room.flat0
    room.scene.set_transform(room.node, location=(0.15, 0.85, 0.0), orientation_wxyz=scenes._axis_angle((0, 1, 0), 0.4))
    room.scene.set_transform(0, location=(0.03, 0.0, 0.01))
    flat_b = room.frame(1)
    assert not np.array_equal(flat_a.top_nodes["invTransform"][:2], flat_b.top_nodes["invTransform"][:2])
    flags = gpu.FLAG_NO_BAKED_INSTANCES if entered else 0
    ctx = _on_second_state(gpu, room, flat_a, flat_b, route, flags, prev_top=flat_a.top_nodes)
    assert ctx.instance_motion == (True, 2)
    name = f"deforming room 64x36, refitted and re-posed, {route}, {'entered' if entered else 'copied'}"
    pixel, hits, deformed, (got_a, got_g, got_m, got_pn) = _check_deposits(name, ctx, flat_b, flat_a, flat_a.top_nodes)
    ctx.close()
    other = _on_second_state(gpu, room, flat_a, flat_b, route, flags, prev_top=flat_a.top_nodes, vertex_first=True)
    other.render_guides(1)
    om, opn = other.read_motion_guides()
    assert _same_bits(om, got_m) and _same_bits(opn, got_pn)  # the order of the two setters does not matter
    other.close()
    alone = _on_second_state(gpu, room, flat_a, flat_b, route, flags, vertex=False, prev_top=flat_a.top_nodes)
    alone.render_guides(1)
    am, apn = alone.read_motion_guides()
    alone.close()
    still = np.ones(len(got_m), bool)
    still[pixel] = ~deformed
    assert np.abs(am[pixel][(hits["prim"] >= 0) & ~deformed]).max() > 0.005  # the room did move
    assert _same_bits(am[still], got_m[still]) and _same_bits(apn[still], got_pn[still])
    moved = ~still
    assert np.abs(am[moved] - got_m[moved]).max() > 0.02  # ... and on the sphere the deformation comes on top


def _tiles(width, height, parity, size=16):
    return [(x, y, min(x + size, width), min(y + size, height)) for y in range(0, height, size) for x in range(0, width, size)
            if ((x // size) + (y // size)) % 2 == parity]


@pytest.mark.parametrize("route,entered", [("host_nodes", False), ("device", True)])
def test_samples_and_tiles_add_up(gpu, route, entered):
    """2 + 3 samples are 5 samples, and two complementary 16-pixel tilings add up to the whole, bit for bit, with 16 samples in flight"""
    room = V.DeformingRoom()
    flat_a, flat_b = room.flat0, room.frame(1)
    flags = gpu.FLAG_NO_BAKED_INSTANCES if entered else 0
    whole = _on_second_state(gpu, room, flat_a, flat_b, route, flags, samples_in_flight=16)
    whole.render_guides(5)
    wm, wpn = whole.read_motion_guides()
    whole.close()
    assert np.abs(wm).max() > 0.1
    split = _on_second_state(gpu, room, flat_a, flat_b, route, flags, samples_in_flight=16)
    split.render_guides(2)
    split.render_guides(3)
    sm, spn = split.read_motion_guides()
    split.close()
    assert _same_bits(sm, wm) and _same_bits(spn, wpn)
    one = _on_second_state(gpu, room, flat_a, flat_b, route, flags, samples_in_flight=1)
    one.render_guides(5)
    om, opn = one.read_motion_guides()
    one.close()
    assert _same_bits(om, wm) and _same_bits(opn, wpn)  # independent of samples_in_flight
    parts = []
    for parity in (0, 1):
        t = U.make_ctx(gpu, flat_a, room.width, room.height, camera=room.camera, flags=flags, samples_in_flight=16)
        t.set_tiles(_tiles(room.width, room.height, parity))
        room.refit_on(t, route, flat_b)
        t.clear()
        t.set_vertex_motion()
        t.render_guides(5)
        parts.append(t.read_motion_guides())
        t.close()
    assert np.array_equal(parts[0][0] + parts[1][0], wm) and np.array_equal(parts[0][1] + parts[1][1], wpn)
    assert (np.abs(parts[0][1][:, :3]).sum(1) == 0).any() and (np.abs(parts[1][1][:, :3]).sum(1) == 0).any()  # each left the other's pixels alone


# ---------------------------------------------------------------- 2. nothing deformed
@pytest.mark.parametrize("how", ["tick", "same_vertices_host_nodes", "same_vertices_device"])
def test_nothing_deformed_gives_the_bits_without_vertex_motion(gpu, how):
    """a tick without a refit (nothing is copied, deformed == 0), and a refit with the very same vertices (k_guides<2> on a snapshot with the current
    bits, deformed == 1): the four guide sums are those of a context that has an instance motion with every leaf where it was, and the first two
    those of a context without any motion"""
    room = V.DeformingRoom()
    flat = room.flat0

    def second_state(c):
        if how == "tick":
            c.upload_dynamic(flat)
        else:
            room.refit_on(c, how[len("same_vertices_"):], room.shape(room.p0))
        c.clear()
    ctx = U.make_ctx(gpu, flat, room.width, room.height, camera=room.camera)
    second_state(ctx)
    ctx.set_vertex_motion()
    assert ctx.vertex_motion == (True, 0 if how == "tick" else 1) and ctx.instance_motion == (False, 0)
    ctx.render_guides(2)
    got = ctx.read_guides() + ctx.read_motion_guides()
    ctx.close()
    ref = U.make_ctx(gpu, flat, room.width, room.height, camera=room.camera)
    second_state(ref)
    ref.set_instance_motion(flat.top_nodes)
    assert ref.vertex_motion == (False, 0) and ref.instance_motion == (True, 0)
    ref.render_guides(2)
    want = ref.read_guides() + ref.read_motion_guides()
    ref.close()
    for a, b in zip(got, want):
        assert _same_bits(a, b)
    assert not got[2].any() and _same_bits(got[3][:, :3], got[1][:, :3])  # exact zeros, and the bits of the normal sum
    never = U.make_ctx(gpu, flat, room.width, room.height, camera=room.camera)
    second_state(never)
    never.render_guides(2)
    na, ng = never.read_guides()
    never.close()
    assert _same_bits(na, got[0]) and _same_bits(ng, got[1])


# ---------------------------------------------------------------- 3. a pipelined caller
@pytest.mark.parametrize("route", ["host_nodes", "device"])
def test_the_next_upload_may_start_before_the_guide_pass(gpu, route):
    """set_vertex_motion, then the NEXT state's refit and upload_dynamic_async (it overwrites the set that held "then"), then the guide pass: the sums
    are those of a context that rendered its guides first -- the pass reads the snapshot.  After the tick the deposits describe B -> C."""
    room = V.DeformingRoom()
    flat_a, flat_b = room.flat0, room.frame(1)
    first = _on_second_state(gpu, room, flat_a, flat_b, route)
    first.render_guides(2)
    want = first.read_guides() + first.read_motion_guides()
    first.close()
    ctx = _on_second_state(gpu, room, flat_a, flat_b, route)
    flat_c = room.frame(2)
    room.hand_over(ctx, route, flat_c)  # no tick: state B stays active
    ctx.render_guides(2)
    got = ctx.read_guides() + ctx.read_motion_guides()
    for a, b in zip(got, want):
        assert _same_bits(a, b)
    assert np.abs(got[2]).max() > 0.1
    ctx.frame_tick()
    assert ctx.vertex_motion == (False, 0)  # the tick forgets it
    ctx.clear()
    ctx.set_vertex_motion()
    assert ctx.vertex_motion == (True, 1)
    _check_deposits(f"deforming room 64x36, pipelined, {route}: B -> C", ctx, flat_c, flat_b, None)
    ctx.close()


# ---------------------------------------------------------------- 4. a rendered leaning blob
def test_a_rendered_leaning_blob_keeps_its_history_with_vertex_motion(gpu):
    """Twelve 1-spp 64x64 frames, static camera; the sphere leans, p.x = p0.x + 0.04 f (p0.y + 0.5)^2 -- about a pixel per frame at its top --, refitted
    on the device every frame.  With vertex motion set every frame the sphere's pixels keep more history than without, and the filtered last frame is
    closer (tone-mapped RMSE over those pixels) to 256 spp of the last state.  The figures measured on an MI355X are in EXPERIMENTS.md ("Vertex
    motion"); only the orderings are gated."""
    frames = 12
    room = V.DeformingRoom(width=64, height=64, fov=40.0)
    cam = room.camera

    def lean(f):
        p = room.p0.copy()
        p[:, 0] = room.p0[:, 0] + np.float32(0.04 * f) * (room.p0[:, 1] + np.float32(0.5)) ** 2
        return p
    first_vertex, _ = room.scene.mesh_offsets(room.blob)

    def loop(with_motion):
        room.shape(lean(0))
        ctx = U.make_ctx(gpu, room.flat0, 64, 64, camera=cam)
        for f in range(frames):
            if f:
                room.blob.refit(lean(f))
                ctx.refit_vertices(first_vertex, room.blob.vertices_view())
                ctx.upload_dynamic(room.scene.flatten_dynamic_only()[0])
            ctx.set_sample_base(f)
            ctx.clear()
            if with_motion and f:
                ctx.set_vertex_motion()
                assert ctx.vertex_motion == (True, 1)
            ctx.render(1)
            ctx.render_guides(1)
            ctx.temporal_accumulate()
        assert ctx.temporal_frames == frames
        cn, _ = ctx.read_temporal()
        out = ctx.denoise(5, hdr=True, input_temporal=True)[..., :3]
        o, d, pixel = ctx.gen_rays(0, 64 * 64)
        hits = ctx.intersect(o, d)
        blob = np.zeros(64 * 64, bool)
        blob[pixel] = (hits["prim"] >= 0) & (hits["inst"] == V.BLOB_LEAF)
        ctx.close()
        return cn.reshape(64, 64, 4), out, blob.reshape(64, 64)
    cn_a, out_a, blob = loop(True)
    cn_b, out_b, blob_b = loop(False)
    assert np.array_equal(blob, blob_b) and blob.sum() > 150
    ref = U.make_ctx(gpu, room.shape(lean(frames - 1)), 64, 64, camera=cam)
    ref.set_sample_base(1000)
    ref.render(256)
    want = U.tonemap(ref.read_accum()[:, :3].reshape(64, 64, 3), 256, cam)
    ref.close()
    count_a, count_b = float(cn_a[blob, 3].mean()), float(cn_b[blob, 3].mean())
    e_a, e_b = U.rmse(U.tonemap(out_a, 1, cam)[blob], want[blob]), U.rmse(U.tonemap(out_b, 1, cam)[blob], want[blob])
    U.record_margin("rendered leaning blob, cornell room 64x64, 12 frames of 1 spp", count_with_motion=count_a, count_without=count_b,
                    rmse_with_motion=e_a, rmse_without=e_b, ratio=e_a / e_b, blob_pixels=int(blob.sum()))
    print(f"leaning blob ({blob.sum()} pixels): mean history count {count_a:.2f} with vertex motion, {count_b:.2f} without; tone-mapped RMSE against "
          f"256 spp {e_a:.3e} with, {e_b:.3e} without, ratio {e_a / e_b:.3f}")
    assert count_a > count_b
    assert e_a < e_b


# ---------------------------------------------------------------- 5. refusals and lifetimes
def test_refusals_and_lifetimes(gpu):
    STATE, UNSUPPORTED = -3, -4
    room = V.DeformingRoom(width=16, height=16, fov=40.0)
    flat_a, w, h = room.flat0, 16, 16
    bare = gpu.Context(w, h)
    assert bare.vertex_motion == (False, 0)
    assert U.status(lambda: bare.set_vertex_motion()) == STATE  # no dynamic state
    assert U.status(lambda: bare.set_vertex_motion(False)) == STATE
    bare.close()
    parity = U.make_ctx(gpu, flat_a, w, h, rng_mode=D.RNG_LFSR113_PARITY)
    assert U.status(lambda: parity.set_vertex_motion()) == UNSUPPORTED
    parity.close()
    refill = U.make_ctx(gpu, flat_a, 64, 64, max_active_rays=1024)
    assert U.status(lambda: refill.set_vertex_motion()) == UNSUPPORTED
    refill.close()

    ctx = U.make_ctx(gpu, flat_a, w, h, camera=room.camera)
    assert U.status(lambda: ctx.set_vertex_motion()) == STATE  # one state so far: there is no "then"
    ctx.set_vertex_motion(False)  # forgetting what is not set is no error
    flat_b = room.frame(1)
    room.hand_over(ctx, "device", flat_b)
    assert U.status(lambda: ctx.set_vertex_motion()) == STATE  # an upload is pending (and still no previous state)
    ctx.frame_tick()
    ctx.clear()
    flat_c = room.frame(2)
    room.hand_over(ctx, "device", flat_c)
    assert U.status(lambda: ctx.set_vertex_motion()) == STATE  # pending: it is overwriting the set that held state A
    assert ctx.vertex_motion == (False, 0)  # a refused call is no call
    ctx.frame_tick()
    ctx.clear()
    ctx.set_vertex_motion()
    assert ctx.vertex_motion == (True, 1)
    ctx.render_guides(1)
    assert U.status(lambda: ctx.set_vertex_motion()) == STATE  # guide samples are in: neither set ...
    assert U.status(lambda: ctx.set_vertex_motion(False)) == STATE  # ... nor forgotten
    assert ctx.vertex_motion == (True, 1)
    m, pn = ctx.read_motion_guides()
    assert np.abs(m).max() > 0.02 and not m[:, 3].any() and not pn[:, 3].any()
    ctx.clear()  # zeroes the sums, keeps the motion
    assert ctx.vertex_motion == (True, 1) and ctx.guide_samples == 0
    assert not any(x.any() for x in ctx.read_motion_guides())
    ctx.render_guides(1)
    m2, pn2 = ctx.read_motion_guides()
    assert _same_bits(m2, m) and _same_bits(pn2, pn)  # ... and the snapshot with it
    ctx.clear()
    ctx.set_instance_motion(flat_c.top_nodes)
    assert ctx.instance_motion == (True, 0) and ctx.vertex_motion == (True, 1)
    ctx.set_instance_motion(None)  # forgets the instance part alone
    assert ctx.instance_motion == (False, 0) and ctx.vertex_motion == (True, 1)
    ctx.render_guides(1)
    m3, pn3 = ctx.read_motion_guides()
    assert _same_bits(m3, m) and _same_bits(pn3, pn)
    ctx.clear()
    ctx.set_vertex_motion(False)
    assert ctx.vertex_motion == (False, 0)
    ctx.set_vertex_motion()
    ctx.upload_dynamic(flat_c)  # a tick forgets it
    assert ctx.vertex_motion == (False, 0)
    ctx.clear()
    ctx.set_vertex_motion()
    assert ctx.vertex_motion == (True, 0)  # both sets hold the same version now: nothing deformed
    # a previous state on the other static scene (a rebuilt tree) has no vertex motion
    other = scenes.cornell_box(w, h).flat
    ctx.upload_static_async(other)
    ctx.upload_dynamic(other)
    ctx.clear()
    assert U.status(lambda: ctx.set_vertex_motion()) == UNSUPPORTED
    assert ctx.vertex_motion == (False, 0)
    ctx.upload_dynamic(other)  # a second state on the rebuilt scene: vertex motion is back
    ctx.clear()
    ctx.set_vertex_motion()
    assert ctx.vertex_motion == (True, 0)
    ctx.close()


# ---------------------------------------------------------------- 6. the C++ example
def test_cpp_deforming_example(gpu, tmp_path):
    """examples/deforming_cornell.cpp: three images of one size that differ; over the blob's final screen rectangle the image filtered over the
    history with vertex motion has less high-frequency energy than the one without."""
    paths = [tmp_path / n for n in ("filtered.ppm", "temporal_plain.ppm", "temporal_motion.ppm")]
    r = subprocess.run([os.path.join(ROOT, "examples", "deforming_cornell"), "12"] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split() if "=" in kv)
    assert int(fields["frames"]) == 12 and int(fields["spp"]) == 1 and int(fields["temporal_frames"]) == 12 and int(fields["deformed"]) == 1
    x0, y0, x1, y1 = (int(v) for v in fields["blob_rect"].split(","))
    alone, without, with_motion = (U.read_ppm(p) for p in paths)
    assert alone.shape == without.shape == with_motion.shape == (256, 256, 3)
    assert not np.array_equal(without, with_motion) and not np.array_equal(alone, with_motion)
    assert 0 <= x0 < x1 <= 256 and 0 <= y0 < y1 <= 256 and (x1 - x0) * (y1 - y0) > 400
    lw, lm = (U.mean_abs_laplacian(x[y0:y1, x0:x1]) for x in (without, with_motion))
    print(f"mean |Laplacian| over the blob's rectangle: over the history without vertex motion {lw:.4f}, with it {lm:.4f}")
    assert lm < lw
