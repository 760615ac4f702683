"""Queues smaller than a batch (pt_config.ext_queue_fraction / shadow_queue_fraction, round 6; the reference keeps one slot per entry in every queue,
src/raytracer.cpp:760-787): the second extension queue and the shadow queue only hold what a batch's first pass emits; the library measures that (a probe batch,
then the counters of every batch) and cuts batches to what fits.  The image never depends on it; a wrong guess is reported, not rendered."""
import functools

import numpy as np
import pytest

import gpu_util as U
import orclib as O
from ptamd import scenes

pytestmark = pytest.mark.gpu

# fractions of sampled pixels within tolerance of the oracle as measured on the MI355X (profiles/round6/parity_margins_queue_fractions.json): gpu_util.fraction_gate holds
# every such comparison against 0.98 x its entry here (and never below the legacy gate)
MEASURED = {
    'later passes fit the shadow queue, glass_first, 2 bounces, fractions 0.9 / 0.3: sampled pixels within 1e-3 of the oracle': 1.0000,
    'small queues, closed_room, fractions 0.3 / 0.62: sampled pixels within 1e-3 of the oracle': 1.0000,
    'small queues, closed_room, fractions 0.9 / 0.3: sampled pixels within 1e-3 of the oracle': 1.0000,
    'small queues, entered, fractions 0.3 / 0.62: sampled pixels within 1e-3 of the oracle': 0.9997,
    'small queues, entered, fractions 0.9 / 0.3: sampled pixels within 1e-3 of the oracle': 0.9997,
    'small queues, glass_first, fractions 0.3 / 0.62: sampled pixels within 1e-3 of the oracle': 1.0000,
    'small queues, glass_first, fractions 0.9 / 0.3: sampled pixels within 1e-3 of the oracle': 1.0000,
    'small queues, open_sky, fractions 0.3 / 0.62: sampled pixels within 1e-3 of the oracle': 0.9997,
    'small queues, open_sky, fractions 0.9 / 0.3: sampled pixels within 1e-3 of the oracle': 0.9997,
    'small queues, thin_lens, fractions 0.3 / 0.62: sampled pixels within 1e-3 of the oracle': 0.9993,
    'small queues, thin_lens, fractions 0.9 / 0.3: sampled pixels within 1e-3 of the oracle': 0.9993,
    'textured room after a texture swap: sampled pixels within 1e-3 of the oracle': 1.0000,
}
W, HH, N, SPP = 160, 90, 64, 16 + 3 * 64  # (the probe batch of 16, then whole batches)
PAIRS = {"bench": None, "reversed": (0.9, 0.3)}  # (ext_queue_fraction, shadow_queue_fraction); "bench": bench.py's headline pair; "reversed": shadow queue the smaller


def _render(gpu, b, W, Hh, spp, in_flight, seed=9, **kw):
    ctx = U.make_ctx(gpu, b, W, Hh, seed=seed, samples_in_flight=in_flight, **kw)
    ctx.render(spp)
    a, st = ctx.read_accum()[:, :3].copy(), ctx.stats()
    ctx.close()
    return a, st


@pytest.mark.parametrize("scene", ["open_sky", "closed_room", "thin_lens"])
def test_smaller_queues_render_the_same_image(gpu, scene):
    """open_sky: config 4's kind of scene (a quarter of the paths go on, fewer than half spawn a shadow ray): the fractions fit, batches stay whole after the
    probe.  closed_room: nearly every path goes on -- the same fractions force SMALLER batches, nothing else.  thin_lens: the first queue keeps all its planes."""
    W, Hh, n, spp = 160, 90, 64, 16 + 3 * 64  # (the probe batch of 16, then whole batches: the statistics name the LAST batch)
    if scene == "closed_room":
        b = scenes.cornell_box(W, Hh)
    else:
        b = scenes.instanced_grid(W, Hh, level=3, sky_size=(32, 16), thin_lens=scene == "thin_lens")
    want, st0 = _render(gpu, b, W, Hh, spp, n)
    got, st1 = _render(gpu, b, W, Hh, spp, n, ext_queue_fraction=0.45, shadow_queue_fraction=0.6)
    assert st0["probe_batches"] == 0 and st0["first_pass_ext_ratio"] == 0
    assert st1["probe_batches"] == 1 and 0 < st1["first_pass_ext_ratio"] <= 1 and 0 < st1["first_pass_shadow_ratio"] <= 1
    for k in ("rays_generated", "rays_extension", "rays_shadow", "shade_hits", "deposits"):
        assert st0[k] == st1[k], (k, st0[k], st1[k])  # the same paths, whatever the batches
    assert np.allclose(got, want, rtol=2e-5, atol=2e-5 * want.max())  # (planes are folded in another order: sums differ by round-off)
    if scene == "closed_room":
        assert st1["first_pass_ext_ratio"] > 0.6 and st1["batch_samples"] < n, st1  # what goes on does not fit 0.45 of a whole batch: smaller batches
    else:
        assert st1["first_pass_ext_ratio"] < 0.42 and st1["first_pass_shadow_ratio"] < 0.57 and st1["batch_samples"] == n, st1


def test_a_new_camera_or_scene_state_is_probed_again(gpu):
    W, Hh, n = 160, 90, 64
    b = scenes.instanced_grid(W, Hh, level=3, sky_size=(32, 16))
    ctx = U.make_ctx(gpu, b, W, Hh, seed=2, samples_in_flight=n, ext_queue_fraction=0.5, shadow_queue_fraction=0.6)
    ctx.render(2 * n)
    r_sky = ctx.stats()["first_pass_ext_ratio"]
    assert ctx.stats()["probe_batches"] == 1
    ctx.render(n)
    assert ctx.stats()["probe_batches"] == 1  # same epoch: the counters of the earlier batches serve
    down = scenes._camera(W, Hh, (0.0, 6.0, 0.1), (0.0, 0.0, 0.0), 40.0)  # straight down at the meshes and the ground
    ctx.set_camera(down)
    ctx.clear()
    ctx.render(2 * n)
    st = ctx.stats()
    assert st["probe_batches"] == 2 and abs(st["first_pass_ext_ratio"] - r_sky) > 0.1, (st, r_sky)  # another view, another ratio: measured again, not inherited
    want, _ = _render(gpu, scenes.SceneBundle(b.scene, down, W, Hh, sky=b.sky), W, Hh, 2 * n, n, seed=2)
    assert np.allclose(ctx.read_accum()[:, :3], want, rtol=2e-5, atol=2e-5 * want.max())
    ctx.upload_dynamic(b.flat)  # a frame tick (the same state again): a new epoch all the same
    ctx.render(n)
    assert ctx.stats()["probe_batches"] == 3
    ctx.close()


def test_a_batch_that_outgrows_its_queues_is_reported_not_rendered(gpu, monkeypatch):
    """The guard behind the guess: PTAMD_DEBUG_BATCH_SCALE makes the library cut its batches three times too large for the closed room; the rays beyond the queues'
    ends are dropped ON THE DEVICE (no write past the end), the batch reports it, pt_synchronize and the image reads fail until pt_clear."""
    W, Hh, n = 160, 90, 64
    b = scenes.cornell_box(W, Hh)
    monkeypatch.setenv("PTAMD_DEBUG_BATCH_SCALE", "3.0")
    ctx = U.make_ctx(gpu, b, W, Hh, seed=3, samples_in_flight=n, ext_queue_fraction=0.3, shadow_queue_fraction=0.3)
    ctx.render(4 * n, sync=False)
    with pytest.raises(gpu.PtError, match="more rays than its queues hold"):
        ctx.synchronize()
    with pytest.raises(gpu.PtError, match="more rays than its queues hold"):
        ctx.read_accum()
    with pytest.raises(gpu.PtError, match="more rays than its queues hold"):
        ctx.render(n)
    monkeypatch.delenv("PTAMD_DEBUG_BATCH_SCALE")
    probes = ctx.stats()["probe_batches"]
    assert probes == 1
    ctx.clear()
    ctx.render(2 * n)  # batches that fit again: the context is as good as new
    assert ctx.stats()["probe_batches"] == probes + 1  # the ratios learned from counts that were cut at the queues' ends are not kept: probed again
    want, _ = _render(gpu, b, W, Hh, 2 * n, n, seed=3)
    assert np.allclose(ctx.read_accum()[:, :3], want, rtol=2e-5, atol=2e-5 * want.max())
    ctx.close()


def test_few_samples_in_flight_and_short_renders_with_smaller_queues(gpu):
    """The corners of the batch sizing: 32 samples in flight (the fractions are floored at what the 16-sample probe batch may emit), renders of fewer than 16
    samples (no bundles: whole camera rays are queued -- they fit the floor), a render that ends in a short batch."""
    W, Hh = 160, 90
    b = scenes.instanced_grid(W, Hh, level=3, sky_size=(32, 16))
    for n, spps in ((32, (32, 64)), (64, (5, 16 + 64 + 7)), (16, (48,))):
        want_ctx = U.make_ctx(gpu, b, W, Hh, seed=5, samples_in_flight=n)
        ctx = U.make_ctx(gpu, b, W, Hh, seed=5, samples_in_flight=n, ext_queue_fraction=0.3, shadow_queue_fraction=0.62)
        for spp in spps:
            ctx.render(spp)
            want_ctx.render(spp)
        a, w = ctx.read_accum()[:, :3], want_ctx.read_accum()[:, :3]
        assert np.allclose(a, w, rtol=2e-5, atol=2e-5 * w.max()), n
        for k in ("rays_generated", "rays_extension", "rays_shadow"):
            assert ctx.stats()[k] == want_ctx.stats()[k], (n, k)
        ctx.close()
        want_ctx.close()


def _fractions(pair):
    if PAIRS[pair] is None:
        import bench
        return bench.EXT_QUEUE_FRACTION, bench.SHADOW_QUEUE_FRACTION
    return PAIRS[pair]


@functools.lru_cache(maxsize=None)
def _bundle(scene):
    if scene == "closed_room":
        return scenes.cornell_box(W, HH)
    if scene == "glass_first":
        return scenes.glass_first(W, HH)
    return scenes.instanced_grid(W, HH, level=3, sky_size=(32, 16), thin_lens=scene == "thin_lens")


@functools.lru_cache(maxsize=None)
def _oracle(scene, spp, max_bounces=0, n_pixels=3000, seed=9):
    """the oracle's values of `n_pixels` sampled pixels, path by path (the same counter PRNG as the device)"""
    b = _bundle(scene)
    px = np.random.default_rng(7).choice(W * HH, n_pixels, replace=False).astype(np.uint32)
    ref, _ = O.render(U.oracle_scene(b), b.camera, W, HH, spp, seed=seed, max_bounces=max_bounces, pixels=px, threads=16)
    return px, ref[px, :3]


_FULL = {}


def _full_queues(gpu, scene, flags):
    """the image and counters of the context with queues as large as the batch (rounds 1-5)"""
    if (scene, flags) not in _FULL:
        _FULL[(scene, flags)] = _render(gpu, _bundle(scene), W, HH, SPP, N, flags=flags)
    return _FULL[(scene, flags)]


def _oracle_gates(name, got, scene, spp, camera, max_bounces=0, **extra):
    px, want = _oracle(scene, spp, max_bounces)
    U.image_margins(f"{name}, {spp} spp", got[px], want, spp, camera, 1e-3, 1e-3, **extra)
    close = np.isclose(got[px], want, rtol=1e-3, atol=1e-3 * want.max()).all(axis=1)
    U.fraction_gate(f"{name}: sampled pixels within 1e-3 of the oracle", close, MEASURED, legacy=0.97)


COUNTERS = ("rays_generated", "rays_extension", "rays_shadow", "shade_hits", "deposits")


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("scene", ["open_sky", "closed_room", "thin_lens", "entered", "glass_first"])
def test_small_queues_against_the_oracle(gpu, scene, pair):
    """Queues smaller than a batch held against the oracle itself, not only against the full-queue context (a bug the two share would pass that).  `bench`:
    the fractions bench.py times; `reversed`: a shadow queue smaller than the extension queue.  glass_first: camera rays that hit glass send no shadow ray, the
    walls behind it do -- a later pass emits more shadow rays than the first, which the sizing must see (with the reversed pair, a batch sized by the first pass
    alone would overrun the shadow queue)."""
    fe, fs = _fractions(pair)
    flags = gpu.FLAG_NO_BAKED_INSTANCES if scene == "entered" else 0
    b = _bundle("open_sky" if scene == "entered" else scene)
    want, st0 = _full_queues(gpu, "open_sky" if scene == "entered" else scene, flags)
    ctx = U.make_ctx(gpu, b, W, HH, seed=9, samples_in_flight=N, flags=flags, ext_queue_fraction=fe, shadow_queue_fraction=fs)
    ctx.render(SPP)
    got, st = ctx.read_accum()[:, :3].copy(), ctx.stats()
    ctx.close()
    assert st["probe_batches"] == 1 and 0 < st["first_pass_ext_ratio"] <= 1 and 0 <= st["first_pass_shadow_ratio"] <= 1, st
    for k in COUNTERS:
        assert st0[k] == st[k], (k, st0[k], st[k])  # the same paths, whatever the batches
    assert np.allclose(got, want, rtol=2e-5, atol=2e-5 * want.max())
    if scene == "glass_first":
        assert st["first_pass_shadow_ratio"] < 0.05, st  # the pane fills the view: the first pass sends (next to) no shadow ray
        assert st["batch_samples"] < N, st  # ... the second one sends one for most paths: neither pair holds a whole batch's
    _oracle_gates(f"small queues, {scene}, fractions {fe} / {fs}", got, "open_sky" if scene == "entered" else scene, SPP, b.camera,
                  ext_queue_fraction=fe, shadow_queue_fraction=fs, batch_samples=st["batch_samples"],
                  first_pass_ext_ratio=st["first_pass_ext_ratio"], first_pass_shadow_ratio=st["first_pass_shadow_ratio"])


def _first_pass_batch(owned, planes, fe, ratio_ext):
    """The batch ensureQueues + safeBatch + pt_render's cut would allow if only what the FIRST pass emits were known (csrc/pt_schedule.h, csrc/ptamd.hip), for a
    scene whose first pass sends no shadow ray: the extension queue alone limits it."""
    cap = (owned * planes + 63) & ~63
    cap_ext = min(cap, ((int(cap * float(np.float32(fe))) + 63) & ~63) + 64)
    cap_ext = max(cap_ext, min(cap, (16 * owned + 63) & ~63))
    room = cap_ext - min(65536.0, cap_ext / 64.0)
    batch = int(max(1.0, min(float(planes), room / (ratio_ext * 1.03 * owned))))
    batch = max(batch, min(16, planes))
    g = 256
    while g > 1 and batch < g:
        g >>= 1
    return batch - batch % g


def test_later_passes_fit_the_shadow_queue(gpu, monkeypatch):
    """A shadow queue smaller than the extension queue (0.9 / 0.3) on glass_first with two bounces: pass 0 (the pane) emits no shadow ray, pass 1 (the walls) one
    for nearly every path.  Sized by pass 0 alone, a batch of 32 would emit ~32 samples' worth of shadow rays into a queue of ~19: the batch is sized by the
    busiest pass instead, and a batch that outgrows the queue in a later pass all the same is cut there on the device and reported."""
    fe, fs, bounces = 0.9, 0.3, 2
    b = _bundle("glass_first")
    # the CPU oracle: with two bounces only passes 0 and 1 emit, and pass 0 sends no shadow ray -- every shadow ray is pass 1's
    _, cnt = O.render(U.oracle_scene(b), b.camera, W, HH, 4, seed=9, max_bounces=bounces, threads=16)
    later = cnt["raysShadow"] / cnt["raysGenerated"]
    assert later > fs + 0.3, cnt
    want, st0 = _render(gpu, b, W, HH, SPP, N, max_bounces=bounces)
    ctx = U.make_ctx(gpu, b, W, HH, seed=9, samples_in_flight=N, max_bounces=bounces, ext_queue_fraction=fe, shadow_queue_fraction=fs)
    ctx.render(SPP)  # (synchronises: a reported overflow raises here)
    got, st = ctx.read_accum()[:, :3].copy(), ctx.stats()
    ctx.close()
    assert st["first_pass_shadow_ratio"] < 0.05, st
    first_only = _first_pass_batch(W * HH, N, fe, st["first_pass_ext_ratio"])
    assert st["batch_samples"] < first_only, (st, first_only)  # the sizing sees pass 1's shadow rays (32 by pass 0 alone, 16 with them)
    assert st["batch_samples"] * later * 1.03 <= fs * N, (st, later)
    for k in COUNTERS:
        assert st0[k] == st[k], (k, st0[k], st[k])
    assert np.allclose(got, want, rtol=2e-5, atol=2e-5 * want.max())
    _oracle_gates(f"later passes fit the shadow queue, glass_first, {bounces} bounces, fractions {fe} / {fs}", got, "glass_first", SPP, b.camera,
                  max_bounces=bounces, batch_samples=st["batch_samples"], later_pass_shadow_ratio=later)
    # batches twice what fits (32: pass 0's extension rays fit, pass 1's shadow rays do not): cut on the device, reported, never returned as an image
    monkeypatch.setenv("PTAMD_DEBUG_BATCH_SCALE", "2.0")
    ctx = U.make_ctx(gpu, b, W, HH, seed=9, samples_in_flight=N, max_bounces=bounces, ext_queue_fraction=fe, shadow_queue_fraction=fs)
    ctx.render(4 * N, sync=False)
    with pytest.raises(gpu.PtError, match="more rays than its queues hold"):
        ctx.synchronize()
    with pytest.raises(gpu.PtError, match="more rays than its queues hold"):
        ctx.read_accum()
    monkeypatch.delenv("PTAMD_DEBUG_BATCH_SCALE")
    probes = ctx.stats()["probe_batches"]
    ctx.clear()
    ctx.render(SPP)
    assert ctx.stats()["probe_batches"] == probes + 1  # the ratios learned from cut counts are dropped with the overflow
    assert np.allclose(ctx.read_accum()[:, :3], want, rtol=2e-5, atol=2e-5 * want.max())
    ctx.close()


def _textured_room(tex):
    """config 1's room with every wall, the floor and the ceiling diffuse through the material texture, seen from its opening; the sky behind the walls"""
    from ptamd import host as H, layout as L
    mats = scenes._room_materials() + [L.material_diffuse((0, 0, 0), texture_id=0)]
    mb = scenes._MeshBuilder()
    scenes._room(mb, mats)
    mb.m = [m if m == 3 else 4 for m in mb.m]  # (3: the light)
    scene = H.Scene()
    scene.add_node(mb.build(mats, H.BVH_BINNED_SAH))
    cam = scenes._camera(W, HH, (0.0, 1.0, -0.9), (0.0, 1.0, 1.0), 60.0)
    return scenes.SceneBundle(scene, cam, W, HH, sky=scenes.procedural_sky(32, 16), material_textures=tex, name="textured_room")


def test_a_texture_upload_is_probed_again(gpu):
    """What goes on after a hit depends on the textures: an alpha-0 texel lets the path through (survives always), a dark solid one ends most.  Ratios learned
    with a dark solid albedo map (~10 % go on) must not size the batches after an alpha-holed map (~46 %) is uploaded: the upload starts a new epoch."""
    fe = 0.3
    solid = scenes.checker_texture(64, a=(0.15, 0.15, 0.15, 1.0), b=(0.05, 0.05, 0.05, 1.0))[None]
    holed = scenes.checker_texture(64, a=(0.15, 0.15, 0.15, 1.0), b=(0.05, 0.05, 0.05, 0.0))[None]  # every other checker square alpha 0
    b = _textured_room(solid)
    ctx = U.make_ctx(gpu, b, W, HH, seed=4, samples_in_flight=N, ext_queue_fraction=fe)
    ctx.render(2 * N)
    st = ctx.stats()
    r_solid = st["first_pass_ext_ratio"]
    assert st["probe_batches"] == 1 and r_solid < 0.2, st
    ctx.upload_texture(0, holed)
    ctx.clear()
    ctx.reset_stats()
    ctx.render(SPP)  # (synchronises: with the ratios of the solid map its batches of 64 would overflow the extension queue)
    st = ctx.stats()
    assert st["probe_batches"] == 2 and st["first_pass_ext_ratio"] - r_solid > 0.1, (st, r_solid)
    assert st["batch_samples"] < N, st
    got = ctx.read_accum()[:, :3].copy()
    fresh_b = _textured_room(holed)
    want, st0 = _render(gpu, fresh_b, W, HH, SPP, N, seed=4)
    for k in COUNTERS:
        assert st0[k] == st[k], (k, st0[k], st[k])
    assert np.allclose(got, want, rtol=2e-5, atol=2e-5 * want.max())
    px = np.random.default_rng(3).choice(W * HH, 3000, replace=False).astype(np.uint32)
    ref, _ = O.render(U.oracle_scene(fresh_b), fresh_b.camera, W, HH, SPP, seed=4, pixels=px, threads=16)
    U.image_margins(f"textured room after a texture swap, {SPP} spp", got[px], ref[px, :3], SPP, fresh_b.camera, 1e-3, 1e-3,
                    first_pass_ext_ratio_before=r_solid, first_pass_ext_ratio_after=st["first_pass_ext_ratio"])
    close = np.isclose(got[px], ref[px, :3], rtol=1e-3, atol=1e-3 * ref[px, :3].max()).all(axis=1)
    U.fraction_gate("textured room after a texture swap: sampled pixels within 1e-3 of the oracle", close, MEASURED, legacy=0.97)
    # a sky upload is a new epoch too
    ctx.upload_texture(1, scenes.procedural_sky(32, 16, brightness=2.0))
    ctx.render(N)
    assert ctx.stats()["probe_batches"] == 3
    ctx.close()


def test_tiles_and_camera_switches_with_small_queues(gpu):
    """The bench fractions on a context that owns two of eight interleaved tile sets (bench.tile_rects: what the ranks of an 8-GPU job own), on a re-tiled
    context, and across pinhole -> thin lens -> pinhole on one context (the first queue's planes are sized for a pinhole's bundles: re-made for the lens)."""
    import bench
    fe, fs = bench.EXT_QUEUE_FRACTION, bench.SHADOW_QUEUE_FRACTION
    b = _bundle("open_sky")
    whole, _ = _full_queues(gpu, "open_sky", 0)
    whole = whole.reshape(HH, W, 3)

    def mask_of(rects):
        m = np.zeros((HH, W), bool)
        for x0, y0, x1, y1 in rects:
            m[y0:y1, x0:x1] = True
        return m

    def check_tiles(ctx, rects):
        a = ctx.read_accum()[:, :3].reshape(HH, W, 3)
        m = mask_of(rects)
        assert m.any() and not m.all()
        assert np.allclose(a[m], whole[m], rtol=2e-5, atol=2e-5 * whole.max())
        assert not a[~m].any(), "pixels the context does not own stay zero"

    ctxs = []
    for rank in (0, 5):
        rects = bench.tile_rects(W, HH, rank, 8)
        ctx = U.make_ctx(gpu, b, W, HH, seed=9, samples_in_flight=N, ext_queue_fraction=fe, shadow_queue_fraction=fs)
        ctx.set_tiles(rects)
        ctx.render(SPP)
        assert ctx.stats()["probe_batches"] == 1
        check_tiles(ctx, rects)
        ctxs.append(ctx)
    # re-tiled: rank 0's context takes rank 3's tiles -- new queues, a new probe, the right pixels
    ctx = ctxs[0]
    rects = bench.tile_rects(W, HH, 3, 8)
    ctx.set_tiles(rects)
    ctx.clear()
    ctx.render(SPP)
    assert ctx.stats()["probe_batches"] == 2
    check_tiles(ctx, rects)
    for c in ctxs:
        c.close()
    # camera switches on one context, each render against a fresh context's image
    lens = _bundle("thin_lens")
    ctx = U.make_ctx(gpu, b, W, HH, seed=9, samples_in_flight=N, ext_queue_fraction=fe, shadow_queue_fraction=fs)
    for k, bb in enumerate((b, lens, b)):
        ctx.set_camera(bb.camera)
        ctx.clear()
        ctx.render(SPP)  # ("the first queue was sized for camera rays queued as directions only" would raise here)
        st = ctx.stats()
        assert st["probe_batches"] == k + 1, st
        want, _ = _full_queues(gpu, "thin_lens" if bb is lens else "open_sky", 0)
        got = ctx.read_accum()[:, :3]
        assert np.allclose(got, want, rtol=2e-5, atol=2e-5 * want.max()), k
    ctx.close()
