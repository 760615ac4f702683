"""Rebuilt motion on the device (pt_set_rebuilt_motion, k_gather_then, then k_guides<2>; include/ptamd.h "rebuilt motion"): the gather kernel alone,
an identity map against the refit route, really rebuilt trees against the numpy restatement (tests/rebuilt_motion_ref.py), trees of other triangle
counts, both motions together, a pipelined upload, a rendered leaning blob that is rebuilt every frame, the refusals, the C++ example."""
import os
import subprocess

import numpy as np
import pytest

import gpu_util as U
import rebuilt_motion_ref as RB
import vertex_motion_ref as V
from ptamd import device as D, host as H, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NONE = RB.NONE


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _adopt_rebuilt(ctx, flat):
    """a rebuilt scene and its dynamic state, adopted"""
    ctx.upload_static_async(flat)
    ctx.upload_dynamic_async(flat)
    ctx.frame_tick()


def _on_rebuilt_state(gpu, room, flat_a, flat_b, prev_triangle, flags=0, rebuilt=True, prev_top=None, rebuilt_first=False, tiles=None, **kw):
    """a context that held flat_a, adopted the rebuilt flat_b and cleared; then the motions asked for"""
    c = U.make_ctx(gpu, flat_a, room.width, room.height, camera=room.camera, flags=flags, **kw)
    if tiles is not None:
        c.set_tiles(tiles)
    _adopt_rebuilt(c, flat_b)
    c.clear()
    if rebuilt and rebuilt_first:
        c.set_rebuilt_motion(prev_triangle)
    if prev_top is not None:
        c.set_instance_motion(prev_top)
    if rebuilt and not rebuilt_first:
        c.set_rebuilt_motion(prev_triangle)
    if rebuilt:
        assert c.rebuilt_motion == (True, int((np.asarray(prev_triangle) != NONE).sum())) and c.vertex_motion == (True, 1)
    return c


def _changed_triangles(flat_now, flat_then, prev_triangle):
    """per triangle of flat_now: its geometry then (through the map; its own where there is none) differs from its geometry now"""
    then = RB._Then(flat_now, flat_then, prev_triangle)
    a, b = then.vertices[then.triangles["indices"]], flat_now.vertices[flat_now.triangles["indices"]]
    return (np.any(a["vertex"] != b["vertex"], -1) | np.any(a["normal"] != b["normal"], -1)).any(1)


def _check_deposits(name, ctx, flat_now, flat_then, prev_triangle, prev_top, least=0.02):
    """test_gpu_vertex_motion._check_deposits, restated for a map: one guide sample of ctx against the restatement, the same gates; returns
    (pixel, hits, deformed mask, the four sums)"""
    n = ctx.width * ctx.height
    o, d, pixel = ctx.gen_rays(0, n)
    hits = ctx.intersect(o, d)  # the per-ray kernel the guide pass runs: the same t, u, v bits
    ctx.render_guides(1)
    got_a, got_g = ctx.read_guides()
    got_m, got_pn = ctx.read_motion_guides()
    m, pn, g = got_m[pixel], got_pn[pixel], got_g[pixel]
    want_m, want_pn, extra = RB.deposits_rebuilt(flat_now, flat_then, prev_triangle, prev_top, o, d, hits, np.float64)
    want_m32 = RB.deposits_rebuilt(flat_now, flat_then, prev_triangle, prev_top, o, d, hits, np.float32)[0]
    assert want_m32.dtype == np.float32
    hit = hits["prim"] >= 0
    deformed = hit & _changed_triangles(flat_now, flat_then, prev_triangle)[np.where(hit, hits["prim"], 0)]
    assert deformed.sum() > 100 and (hit & ~deformed).sum() > 100 and (~hit).sum() > 0
    bound = 8.0 * float(np.abs(want_m32.astype(np.float64) - want_m).max()) + 1e-6 * V.scene_extent(flat_now)
    err = float(np.abs(m.astype(np.float64) - want_m).max())
    largest = float(np.abs(want_m[deformed, :3]).max())
    U.record_margin(f"rebuilt motion guide vs restatement: {name}", error=err, bound=bound, largest=largest, deformed_pixels=int(deformed.sum()))
    print(f"{name}: motion error {err:.3e}, bound {bound:.3e}, largest displacement on the blob {largest:.3f}, {deformed.sum()} deformed pixels")
    assert err <= bound and largest > least and np.all(m[:, 3] == 0) and np.all(pn[:, 3] == 0)
    flip_dev = (g[:, :3].astype(np.float64) * extra["normal_unflipped"]).sum(1) < 0
    grazing = hit & (np.abs(extra["n_dot_d"]) < 1e-6)
    assert grazing.mean() < 1e-2
    want_pn[grazing, :3] = np.where(flip_dev[grazing, None], -extra["then_unflipped"][grazing], extra["then_unflipped"][grazing])
    err_n = float(np.abs(pn[:, :3].astype(np.float64) - want_pn[:, :3]).max())
    U.record_margin(f"rebuilt motion prev_normal vs restatement: {name}", error=err_n, gate=1e-5, flipped=int((extra["n_dot_d"][hit] > 0).sum()))
    print(f"{name}: prev_normal error {err_n:.3e}")
    assert err_n <= 1e-5
    assert np.abs(pn[deformed, :3] - g[deformed, :3]).max() > 1e-2  # the twisted surface's normals did turn
    return pixel, hits, deformed, (got_a, got_g, got_m, got_pn)


# ---------------------------------------------------------------- 1. the gather kernel alone
def _records(n, seed):
    """n 128-byte records of distinct bit patterns, NaN payloads, infinities and denormals among them"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 2 ** 32, (n, 32), dtype=np.uint64).astype(np.uint32)
    r[:, 0] = np.arange(n, dtype=np.uint32) + np.uint32(seed << 20)  # distinct whatever the draw
    r[:, 5] = np.uint32(0x7FC00000) | (np.arange(n, dtype=np.uint32) & np.uint32(0x3FFFFF))  # quiet NaNs with a payload
    r[:, 9] = np.uint32(0xFF800001) + np.arange(n, dtype=np.uint32)  # signalling NaNs
    r[:, 13], r[:, 17], r[:, 31] = 0x7F800000, 0x00000001, 0x80000000
    return r


@pytest.fixture(scope="module")
def gather_ctx(gpu):
    c = gpu.Context(16, 16)
    yield c
    c.close()


@pytest.mark.parametrize("n_now", [1, 7, 8, 9, 63, 65, 511, 513])
def test_the_gather_kernel_copies_bits(gather_ctx, n_now):
    """part of a record group (8 lanes a record), of a wave (8 records) and of a block (32 records); fewer and more records then than now"""
    now = _records(n_now, 1)
    idx = np.arange(n_now, dtype=np.uint32)
    for n_then in sorted({max(n_now // 2, 1), n_now, n_now + 37}):
        then = _records(n_then, 2)
        maps = {"identity": idx % n_then, "reversed": (n_then - 1 - idx % n_then), "none": np.full(n_now, NONE, np.uint32),
                "one index": np.full(n_now, n_then - 1, np.uint32), "alternating": np.where(idx % 2 == 0, NONE, (idx * 7) % n_then)}
        for name, m in maps.items():
            m = m.astype(np.uint32)
            got = gather_ctx.debug_gather_records(then, now, m)
            want = np.where((m == NONE)[:, None], now, then[np.minimum(m, n_then - 1)])  # fancy indexing
            assert np.array_equal(want, RB.gather(then, now, m))
            assert np.array_equal(got, want), (name, n_now, n_then)


def test_the_gather_kernel_guards_its_index(gather_ctx):
    """an index that is not below n_then never becomes an address: the current record comes out (the C ABI refuses such a map before the kernel sees it)"""
    now, then = _records(65, 3), _records(9, 4)
    m = np.arange(65, dtype=np.uint32)
    m[60:] = [9, 10, 0x7FFFFFFF, 0xFFFFFFFE, NONE]
    got = gather_ctx.debug_gather_records(then, now, m)
    assert np.array_equal(got[:9], then) and np.array_equal(got[9:], now[9:])
    assert np.array_equal(gather_ctx.debug_gather_records(np.zeros((0, 32), np.uint32), now, np.zeros(65, np.uint32)), now)  # no record then


# ---------------------------------------------------------------- 2. the same tree, renumbered by nobody
@pytest.mark.parametrize("entered", [False, True])
def test_an_identity_map_is_the_refit_route(gpu, entered):
    """state B holds the refitted arrays of frame 1, handed over as a rebuilt scene with an identity map: the four sums of a context that refitted"""
    room = V.DeformingRoom()
    flat_a, flat_b = room.flat0, room.frame(1)
    flags = gpu.FLAG_NO_BAKED_INSTANCES if entered else 0
    ctx = _on_rebuilt_state(gpu, room, flat_a, flat_b, np.arange(len(flat_b.triangles), dtype=np.uint32), flags)
    ctx.render_guides(2)
    got = ctx.read_guides() + ctx.read_motion_guides()
    ctx.close()
    twin = U.make_ctx(gpu, flat_a, room.width, room.height, camera=room.camera, flags=flags)
    room.refit_on(twin, "device", flat_b)
    twin.clear()
    twin.set_vertex_motion()
    assert twin.vertex_motion == (True, 1) and twin.rebuilt_motion == (False, 0)
    twin.render_guides(2)
    want = twin.read_guides() + twin.read_motion_guides()
    twin.close()
    assert np.abs(want[2]).max() > 0.1
    for a, b in zip(got, want):
        assert _same_bits(a, b)


# ---------------------------------------------------------------- 3. a really rebuilt tree
@pytest.mark.parametrize("builder", ["BVH_BINNED_FAST", "BVH_SPATIAL_SPLIT"])
@pytest.mark.parametrize("entered", [False, True])
def test_guide_deposits_of_a_rebuilt_mesh(gpu, entered, builder):
    """state A, then the sphere twisted and squashed and built from scratch for state B; the map from H.triangle_history"""
    room = RB.RebuiltRoom(getattr(H, builder))
    (flat_a, org_a), (flat_b, org_b) = room.twisted(0), room.twisted(1)
    pmap = H.triangle_history(org_b, org_a)
    assert not np.array_equal(pmap, np.arange(len(pmap)))  # renumbered
    if builder == "BVH_SPATIAL_SPLIT":
        assert len(flat_a.triangles) != len(flat_b.triangles)  # (the chords are split otherwise)
    flags = gpu.FLAG_NO_BAKED_INSTANCES if entered else 0
    name = f"rebuilt room 64x36, {'entered' if entered else 'copied'}, {builder}"
    ctx = _on_rebuilt_state(gpu, room, flat_a, flat_b, pmap, flags)
    pixel, hits, deformed, (got_a, got_g, got_m, got_pn) = _check_deposits(name, ctx, flat_b, flat_a, pmap, None)
    m, pn, g = got_m[pixel], got_pn[pixel], got_g[pixel]
    assert np.all(_bits(m[~deformed]) == 0)  # the room and the misses: exact zeros ...
    assert _same_bits(pn[~deformed, :3], g[~deformed, :3])  # ... and the bits of normal_depth.xyz
    ctx.close()
    plain = _on_rebuilt_state(gpu, room, flat_a, flat_b, pmap, flags, rebuilt=False)  # the other two sums do not know about the motion
    assert plain.rebuilt_motion == (False, 0) and plain.vertex_motion == (False, 0)
    plain.render_guides(1)
    pa, pg = plain.read_guides()
    assert _same_bits(pa, got_a) and _same_bits(pg, got_g)
    plain.close()


# ---------------------------------------------------------------- 4. counts that differ
@pytest.mark.parametrize("direction", ["triangles_go", "triangles_come"])
def test_trees_of_other_triangle_counts(gpu, direction):
    """frame 1 without the sphere's last 200 input triangles, and the reverse: a pixel whose triangle has no predecessor deposits exact zeros and the
    bits of N; the others go against the restatement"""
    room = RB.RebuiltRoom()
    n_in = len(room.faces)
    if direction == "triangles_go":
        (flat_a, org_a), (flat_b, org_b) = room.twisted(0), room.twisted(1, triangles=n_in - 200)
    else:
        (flat_a, org_a), (flat_b, org_b) = room.twisted(0, triangles=n_in - 200), room.twisted(1)
    assert len(flat_a.triangles) != len(flat_b.triangles)
    pmap = H.triangle_history(org_b, org_a)
    new = pmap == NONE
    assert new.any() == (direction == "triangles_come")
    ctx = _on_rebuilt_state(gpu, room, flat_a, flat_b, pmap)
    assert ctx.rebuilt_motion == (True, int((~new).sum()))
    pixel, hits, deformed, (got_a, got_g, got_m, got_pn) = _check_deposits(f"rebuilt room 64x36, {direction}", ctx, flat_b, flat_a, pmap, None)
    ctx.close()
    m, pn, g = got_m[pixel], got_pn[pixel], got_g[pixel]
    assert np.all(_bits(m[~deformed]) == 0) and _same_bits(pn[~deformed, :3], g[~deformed, :3])
    if direction == "triangles_come":
        fresh = (hits["prim"] >= 0) & new[np.where(hits["prim"] >= 0, hits["prim"], 0)]
        assert fresh.sum() > 20 and not (fresh & deformed).any()  # (no predecessor: among the undeformed, exact zeros and the bits of N above)
        print(f"{direction}: {fresh.sum()} pixels on triangles without a predecessor")


# ---------------------------------------------------------------- 5. with set_instance_motion; sums and tiles
def _tiles(width, height, parity, size=16):
    return [(x, y, min(x + size, width), min(y + size, height)) for y in range(0, height, size) for x in range(0, width, size)
            if ((x // size) + (y // size)) % 2 == parity]


def test_a_rebuilt_and_reposed_mesh_and_sums_and_tiles(gpu):
    """the sphere is turned and moved and the room shifted by the tick that adopts the rebuilt tree: both motions, in either order of the setters; one
    and one guide samples are two; two complementary tilings add up"""
    room = RB.RebuiltRoom()
    flat_a, org_a = room.twisted(0)
    flat_b, org_b = room.twisted(1, location=(0.15, 0.85, 0.0), orientation_wxyz=scenes._axis_angle((0, 1, 0), 0.4), walls_at=(0.03, 0.0, 0.01))
    assert len(flat_a.top_nodes) == len(flat_b.top_nodes) and not np.array_equal(flat_a.top_nodes["invTransform"][:2], flat_b.top_nodes["invTransform"][:2])
    pmap = H.triangle_history(org_b, org_a)
    prev = flat_a.top_nodes
    ctx = _on_rebuilt_state(gpu, room, flat_a, flat_b, pmap, prev_top=prev)
    assert ctx.instance_motion == (True, 2)
    _, _, _, (_, _, one_m, one_pn) = _check_deposits("rebuilt room 64x36, rebuilt and re-posed", ctx, flat_b, flat_a, pmap, prev)
    ctx.render_guides(1)  # one and one ...
    whole = ctx.read_guides() + ctx.read_motion_guides()
    ctx.close()
    other = _on_rebuilt_state(gpu, room, flat_a, flat_b, pmap, prev_top=prev, rebuilt_first=True, samples_in_flight=16)
    other.render_guides(2)  # ... are two, whatever the order of the setters and the samples in flight
    got = other.read_guides() + other.read_motion_guides()
    other.close()
    for a, b in zip(got, whole):
        assert _same_bits(a, b)
    assert not _same_bits(whole[2], one_m)
    parts = []
    for parity in (0, 1):
        t = _on_rebuilt_state(gpu, room, flat_a, flat_b, pmap, prev_top=prev, tiles=_tiles(room.width, room.height, parity))
        t.render_guides(2)
        parts.append(t.read_motion_guides())
        t.close()
    assert np.array_equal(parts[0][0] + parts[1][0], whole[2]) and np.array_equal(parts[0][1] + parts[1][1], whole[3])
    assert (np.abs(parts[0][1][:, :3]).sum(1) == 0).any() and (np.abs(parts[1][1][:, :3]).sum(1) == 0).any()  # each left the other's pixels alone


# ---------------------------------------------------------------- 6. a pipelined caller
def test_the_next_rebuild_may_start_before_the_guide_pass(gpu):
    """set_rebuilt_motion, then the NEXT rebuilt scene's uploads (they overwrite the set that held "then"), then the guide pass: the sums of a context
    that rendered its guides first.  After the tick the deposits describe B -> C."""
    room = RB.RebuiltRoom()
    (flat_a, org_a), (flat_b, org_b), (flat_c, org_c) = room.twisted(0), room.twisted(1), room.twisted(2)
    ab, bc = H.triangle_history(org_b, org_a), H.triangle_history(org_c, org_b)
    first = _on_rebuilt_state(gpu, room, flat_a, flat_b, ab)
    first.render_guides(2)
    want = first.read_guides() + first.read_motion_guides()
    first.close()
    ctx = _on_rebuilt_state(gpu, room, flat_a, flat_b, ab)
    ctx.upload_static_async(flat_c)
    ctx.upload_dynamic_async(flat_c)  # no tick: state B stays active
    ctx.render_guides(2)
    got = ctx.read_guides() + ctx.read_motion_guides()
    for a, b in zip(got, want):
        assert _same_bits(a, b)
    assert np.abs(got[2]).max() > 0.1
    ctx.frame_tick()
    assert ctx.rebuilt_motion == (False, 0) and ctx.vertex_motion == (False, 0)  # the tick forgets it
    ctx.clear()
    ctx.set_rebuilt_motion(bc)
    _check_deposits("rebuilt room 64x36, pipelined: B -> C", ctx, flat_c, flat_b, bc, None)
    ctx.close()


# ---------------------------------------------------------------- 7. a rendered leaning blob, rebuilt every frame
def test_a_rendered_leaning_blob_keeps_its_history_when_it_is_rebuilt(gpu):
    """The loop of test_a_rendered_leaning_blob_keeps_its_history_with_vertex_motion -- twelve 1-spp 64x64 frames, static camera, the sphere leaning by
    p.x = p0.x + 0.04 f (p0.y + 0.5)^2 -- with a NEW mesh and tree per frame (upload_static_async).  With the map of H.triangle_history set every frame
    the sphere's pixels keep more history than without, and the filtered last frame is closer (tone-mapped RMSE over those pixels) to 256 spp of the
    last state.  Only the orderings are gated; the figures, and the refit route's from the same run, are recorded (EXPERIMENTS.md, "Rebuilt motion")."""
    frames = 12
    room = RB.RebuiltRoom(width=64, height=64, fov=40.0)
    refit_room = V.DeformingRoom(width=64, height=64, fov=40.0)
    cam = room.camera
    assert cam.tobytes() == refit_room.camera.tobytes()

    def lean(f):
        p = room.p0.copy()
        p[:, 0] = room.p0[:, 0] + np.float32(0.04 * f) * (room.p0[:, 1] + np.float32(0.5)) ** 2
        return p

    def finish(ctx):
        assert ctx.temporal_frames == frames
        cn, _ = ctx.read_temporal()
        out = ctx.denoise(5, hdr=True, input_temporal=True)[..., :3]
        o, d, pixel = ctx.gen_rays(0, 64 * 64)
        hits = ctx.intersect(o, d)
        blob = np.zeros(64 * 64, bool)
        blob[pixel] = (hits["prim"] >= 0) & (hits["inst"] == V.BLOB_LEAF)
        ctx.close()
        return cn.reshape(64, 64, 4), out, blob.reshape(64, 64)

    def frame(ctx, f, motion):
        ctx.set_sample_base(f)
        ctx.clear()
        if f:
            motion()
        ctx.render(1)
        ctx.render_guides(1)
        ctx.temporal_accumulate()

    def rebuilt_loop(with_motion):
        flat, org = room.frame(lean(0))
        ctx = U.make_ctx(gpu, flat, 64, 64, camera=cam)
        for f in range(frames):
            if f:
                then = org
                flat, org = room.frame(lean(f))
                _adopt_rebuilt(ctx, flat)
            frame(ctx, f, lambda: with_motion and ctx.set_rebuilt_motion(H.triangle_history(org, then)))
            assert ctx.rebuilt_motion[0] == bool(with_motion and f)
        return finish(ctx), flat

    def refit_loop(with_motion):
        first_vertex, _ = refit_room.scene.mesh_offsets(refit_room.blob)
        ctx = U.make_ctx(gpu, refit_room.shape(lean(0)), 64, 64, camera=cam)
        for f in range(frames):
            if f:
                refit_room.blob.refit(lean(f))
                ctx.refit_vertices(first_vertex, refit_room.blob.vertices_view())
                ctx.upload_dynamic(refit_room.scene.flatten_dynamic_only()[0])
            frame(ctx, f, lambda: with_motion and ctx.set_vertex_motion())
        return finish(ctx)
    (cn_a, out_a, blob), last = rebuilt_loop(True)
    (cn_b, out_b, blob_b), _ = rebuilt_loop(False)
    assert np.array_equal(blob, blob_b) and blob.sum() > 150
    ref = U.make_ctx(gpu, last, 64, 64, camera=cam)
    ref.set_sample_base(1000)
    ref.render(256)
    want = U.tonemap(ref.read_accum()[:, :3].reshape(64, 64, 3), 256, cam)
    ref.close()

    def figures(cn, out, over):
        return float(cn[over, 3].mean()), U.rmse(U.tonemap(out, 1, cam)[over], want[over])
    (count_a, e_a), (count_b, e_b) = figures(cn_a, out_a, blob), figures(cn_b, out_b, blob)
    rcn_a, rout_a, rblob = refit_loop(True)  # beside them, not gated: the refit route over the same shapes (its own tree, its own silhouette pixels)
    rcn_b, rout_b, _ = refit_loop(False)
    (rcount_a, re_a), (rcount_b, re_b) = figures(rcn_a, rout_a, rblob), figures(rcn_b, rout_b, rblob)
    U.record_margin("rendered leaning blob rebuilt every frame, cornell room 64x64, 12 frames of 1 spp", count_with_motion=count_a, count_without=count_b,
                    rmse_with_motion=e_a, rmse_without=e_b, ratio=e_a / e_b, blob_pixels=int(blob.sum()), refit_count_with_motion=rcount_a,
                    refit_count_without=rcount_b, refit_rmse_with_motion=re_a, refit_rmse_without=re_b, refit_blob_pixels=int(rblob.sum()))
    print(f"leaning blob rebuilt every frame ({blob.sum()} pixels): mean history count {count_a:.2f} with rebuilt motion, {count_b:.2f} without; tone-mapped "
          f"RMSE against 256 spp {e_a:.3e} with, {e_b:.3e} without, ratio {e_a / e_b:.3f}; the refit route: count {rcount_a:.2f} / {rcount_b:.2f}, "
          f"RMSE {re_a:.3e} / {re_b:.3e} over {rblob.sum()} pixels")
    assert count_a > count_b
    assert e_a < e_b


# ---------------------------------------------------------------- 8. refusals and lifetimes
def test_refusals_and_lifetimes(gpu):
    INVALID, STATE, UNSUPPORTED = -1, -3, -4
    start = D.live_resources()
    room = RB.RebuiltRoom(width=16, height=16, fov=40.0)
    (flat_a, org_a), (flat_b, org_b), (flat_c, org_c) = room.twisted(0), room.twisted(1), room.twisted(2, triangles=len(room.faces) - 200)
    ab, bc = H.triangle_history(org_b, org_a), H.triangle_history(org_c, org_b)
    w = h = 16
    bare = gpu.Context(w, h)
    assert bare.rebuilt_motion == (False, 0)
    assert U.status(lambda: bare.set_rebuilt_motion(ab)) == STATE  # no dynamic state
    assert U.status(lambda: bare.set_rebuilt_motion(None)) == STATE
    bare.close()
    parity = U.make_ctx(gpu, flat_a, w, h, rng_mode=D.RNG_LFSR113_PARITY)
    assert U.status(lambda: parity.set_rebuilt_motion(ab)) == UNSUPPORTED
    parity.close()
    refill = U.make_ctx(gpu, flat_a, 64, 64, max_active_rays=1024)
    assert U.status(lambda: refill.set_rebuilt_motion(ab)) == UNSUPPORTED
    refill.close()

    ctx = U.make_ctx(gpu, flat_a, w, h, camera=room.camera)
    assert U.status(lambda: ctx.set_rebuilt_motion(np.arange(len(flat_a.triangles), dtype=np.uint32))) == STATE  # one state so far: there is no "then"
    ctx.set_rebuilt_motion(None)  # forgetting what is not set is no error
    ctx.upload_static_async(flat_b)
    ctx.upload_dynamic_async(flat_b)
    assert U.status(lambda: ctx.set_rebuilt_motion(ab)) == STATE  # an upload is pending
    ctx.frame_tick()
    ctx.clear()

    def untouched():
        assert ctx.rebuilt_motion == (False, 0) and ctx.vertex_motion == (False, 0)
    assert U.status(lambda: ctx.set_vertex_motion()) == UNSUPPORTED  # a rebuilt state has no vertex motion of that kind, as before
    untouched()
    assert U.status(lambda: ctx.set_rebuilt_motion(ab[:-1])) == INVALID  # not the active state's triangle count
    assert U.status(lambda: ctx.set_rebuilt_motion(np.r_[ab, ab[:1]])) == INVALID
    bad = ab.copy()
    bad[5], bad[7] = len(flat_a.triangles), NONE - 1
    with pytest.raises(D.PtError, match=r"\(-1\).*entry 5 names triangle " + str(len(flat_a.triangles))):  # the first offending index
        ctx.set_rebuilt_motion(bad)
    untouched()
    ctx.set_guide_chain(1)
    assert U.status(lambda: ctx.set_rebuilt_motion(ab)) == UNSUPPORTED  # motion deposits along a chain are not supported
    ctx.set_rebuilt_motion(None)  # (forgetting is)
    ctx.set_guide_chain(0)
    untouched()
    ctx.render_guides(1)
    plain = ctx.read_guides()
    assert U.status(lambda: ctx.set_rebuilt_motion(ab)) == STATE  # guide samples are in: neither set ...
    assert U.status(lambda: ctx.set_rebuilt_motion(None)) == STATE  # ... nor forgotten
    untouched()
    assert all(_same_bits(a, b) for a, b in zip(ctx.read_guides(), plain))
    ctx.clear()
    ctx.set_rebuilt_motion(ab)
    assert ctx.rebuilt_motion == (True, len(ab)) and ctx.vertex_motion == (True, 1)
    ctx.render_guides(1)
    assert all(_same_bits(a, b) for a, b in zip(ctx.read_guides(), plain))  # the first two sums do not know
    m, pn = ctx.read_motion_guides()
    assert np.abs(m).max() > 0.02 and not m[:, 3].any() and not pn[:, 3].any()
    assert U.status(lambda: ctx.set_rebuilt_motion(bad)) == STATE and ctx.rebuilt_motion == (True, len(ab))
    ctx.clear()  # zeroes the sums, keeps the motion
    assert ctx.rebuilt_motion == (True, len(ab)) and ctx.guide_samples == 0
    assert not any(x.any() for x in ctx.read_motion_guides())
    assert U.status(lambda: ctx.set_rebuilt_motion(bad)) == INVALID and ctx.rebuilt_motion == (True, len(ab))  # a refused call changes nothing ...
    ctx.render_guides(1)
    m2, pn2 = ctx.read_motion_guides()
    assert _same_bits(m2, m) and _same_bits(pn2, pn)  # ... the snapshot included
    ctx.clear()
    ctx.set_vertex_motion(False)  # either call forgets it
    assert ctx.rebuilt_motion == (False, 0) and ctx.vertex_motion == (False, 0)
    ctx.set_rebuilt_motion(ab)
    ctx.set_rebuilt_motion(None)
    assert ctx.rebuilt_motion == (False, 0) and ctx.vertex_motion == (False, 0)
    ctx.set_rebuilt_motion(ab)
    _adopt_rebuilt(ctx, flat_c)  # a tick forgets it
    assert ctx.rebuilt_motion == (False, 0) and ctx.vertex_motion == (False, 0)
    ctx.clear()
    assert U.status(lambda: ctx.set_rebuilt_motion(ab)) == INVALID  # the map of another state
    ctx.set_rebuilt_motion(bc)  # a smaller state after a larger one: the buffers stay
    assert ctx.rebuilt_motion == (True, len(bc))
    ctx.upload_dynamic(flat_c)  # a second state on the same tree: the plain vertex motion is back, and takes the place of the rebuilt one
    ctx.clear()
    ctx.set_rebuilt_motion(np.arange(len(flat_c.triangles), dtype=np.uint32))
    assert ctx.rebuilt_motion == (True, len(flat_c.triangles))
    ctx.set_vertex_motion()
    assert ctx.vertex_motion == (True, 0) and ctx.rebuilt_motion == (False, 0)
    ctx.close()
    assert D.live_resources() == start


# ---------------------------------------------------------------- 9. the C++ example
def test_cpp_rebuilt_example(gpu):
    """examples/rebuilt_cornell.cpp at a small size: RayTracer::setRebuiltMotion over rebuildGeometry / frameTick; it gates both orderings itself"""
    r = subprocess.run([os.path.join(ROOT, "examples", "rebuilt_cornell"), "8", "96", "128"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split() if "=" in kv)
    assert int(fields["frames"]) == 8 and int(fields["followed"]) > 0 and int(fields["followed_without"]) == 0
    assert float(fields["count_with_motion"]) > float(fields["count_without"]) and float(fields["rmse_with_motion"]) < float(fields["rmse_without"])
