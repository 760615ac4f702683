"""Adaptive sampling on the device (pt_set_adaptive, pt_render_adaptive, k_adaptive_eval; include/ptamd.h "adaptive sampling") against its numpy
restatement (tests/adaptive_ref.py): planted states through write_adaptive, the halves as the plain renders they are, a masked round as the tiled
render it is, a run to completion on a room surrounded by black sky, the gain at equal budget, the refusals and the lifetime."""
import numpy as np
import pytest

import adaptive_ref as R
import gpu_util as U
import orclib as O
from ptamd import device as D, scenes

pytestmark = pytest.mark.gpu
INVALID, STATE, UNSUPPORTED = -1, -3, -4
W = H = 64


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def midpoint_threshold(block_error):
    """halfway between the two middle values of the sorted block errors, which must differ by more than 1e-3 relative: no block may be excused"""
    e = np.sort(np.asarray(block_error, np.float64))
    if len(e) == 1:
        return float(e[0]) * 0.5
    lo, hi = e[len(e) // 2 - 1], e[len(e) // 2]
    assert hi - lo > 1e-3 * hi, (lo, hi)
    return float(0.5 * (lo + hi))


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (8, 8), (9, 9), (70, 45), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_planted_states_match_the_restatement(gpu, shape):
    """error and block_error within 1e-4 relative + 1e-7 (a dozen float32 operations and a 64-term sum cost under 1e-5); nonfinite exact; a second
    evaluation with the same bits; the flags of every block further than 1e-3 relative from the threshold; the accumulator with the bits of A + B
    where n == S, within 1e-6 relative elsewhere, 0 where n == 0."""
    w, h = shape
    A, B, counts, special = R.planted(w, h, 11)
    MIN, MAX = 4, 16
    ref = R.evaluate(A, B, counts, w, h, 0.0, MIN, MAX)
    thr = midpoint_threshold(ref["block_error"])
    ref = R.evaluate(A, B, counts, w, h, thr, MIN, MAX)
    ctx = gpu.Context(w, h)
    ctx.set_adaptive(threshold=thr, min_samples=MIN, round_samples=2, max_samples=MAX)
    assert ctx.adaptive is True and ctx.adaptive_device_ptr(0) == 0
    ctx.write_adaptive(A, B, counts)
    assert all(ctx.adaptive_device_ptr(k) != 0 for k in range(4)) and ctx.adaptive_device_ptr(4) == 0
    got, st, accum = ctx.read_adaptive(), ctx.adaptive_stats, ctx.read_accum()
    assert ctx.samples_per_pixel == ref["spp"] == st["max_count"]
    assert np.array_equal(got["counts"], counts) and np.array_equal(bits(got["A"]), bits(A)) and np.array_equal(bits(got["B"]), bits(B))
    err = np.abs(got["error"].astype(np.float64) - ref["error"])
    berr = np.abs(got["block_error"].astype(np.float64) - ref["block_error"])
    print(f"{w}x{h}: error off by {err.max():.3e}, block error by {berr.max():.3e} (largest {ref['block_error'].max():.3e}), threshold {thr:.4e}, "
          f"nonfinite {st['nonfinite']}, active {st['active_blocks']} of {st['blocks']}")
    assert (err <= 1e-4 * np.abs(ref["error"]) + 1e-7).all()
    assert (berr <= 1e-4 * np.abs(ref["block_error"]) + 1e-7).all()
    assert (got["error"][special] == 0).all() if len(special) else True
    assert st["nonfinite"] == ref["nonfinite"] == len(special)
    assert st["blocks"] == len(ref["flags"]) and st["samples_total"] == ref["samples_total"] and st["min_count"] == ref["min_count"]
    assert st["max_block_error"] == float(got["block_error"].max())
    # flags: the next round renders exactly the flagged blocks, so the stats' count is the flags' -- every block is further than 1e-3 from the threshold
    assert (np.abs(ref["block_error"].astype(np.float64) - thr) > 1e-3 * thr).all()
    assert st["active_blocks"] == ref["active_blocks"]
    device_flags = R.active_set(ref["block_counts"], got["block_error"], thr, MIN, MAX)
    assert np.array_equal(device_flags, ref["flags"])
    # the published accumulator
    S, n = ref["spp"], counts
    finite = np.isfinite(A[:, :3]).all(axis=1) & np.isfinite(B[:, :3]).all(axis=1)
    full = (n == S) & finite
    assert np.array_equal(bits(accum[full, :3]), bits((A[full, :3] + B[full, :3]).astype(np.float32)))
    part = (n != S) & (n > 0) & finite
    assert np.allclose(accum[part, :3], ref["accum"][part, :3], rtol=1e-6, atol=0)
    assert (accum[n == 0] == 0).all() and (accum[:, 3] == 0).all()
    assert finite.all() or not np.isfinite(accum[~finite, :3]).all()
    # a second evaluation (the same parameters set again re-evaluate the flags): the same bits
    ctx.set_adaptive(threshold=thr, min_samples=MIN, round_samples=2, max_samples=MAX)
    again = ctx.read_adaptive()
    for k in ("error", "block_error"):
        assert np.array_equal(bits(again[k]), bits(got[k])), k
    assert ctx.adaptive_stats == st and np.array_equal(bits(ctx.read_accum()[finite]), bits(accum[finite]))
    ctx.close()


@pytest.fixture(scope="module")
def cornell():
    return scenes.cornell_box(W, H)


def first_round(gpu, cornell):
    ctx = U.make_ctx(gpu, cornell, W, H)
    ctx.set_adaptive(threshold=0.0, min_samples=8, round_samples=8, max_samples=16)
    st = ctx.render_adaptive(1)
    assert st["rounds"] == 1 and ctx.samples_per_pixel == 8
    return ctx


def test_halves_are_plain_renders(gpu, cornell):
    ctx = first_round(gpu, cornell)
    got = ctx.read_adaptive()
    off = U.make_ctx(gpu, cornell, W, H)
    off.render(4)
    assert np.array_equal(bits(got["A"]), bits(off.read_accum()))
    off.clear()
    off.set_sample_base(4)
    off.render(4)
    assert np.array_equal(bits(got["B"]), bits(off.read_accum()))
    accum = ctx.read_accum()
    assert np.array_equal(bits(accum[:, :3]), bits((got["A"][:, :3] + got["B"][:, :3]).astype(np.float32))) and (accum[:, 3] == 0).all()
    assert (got["counts"] == 8).all()
    st = ctx.adaptive_stats
    assert (st["min_count"], st["max_count"], st["samples_total"], st["active_blocks"]) == (8, 8, 8 * W * H, st["blocks"])
    assert ctx.stats()["rays_generated"] == 8 * W * H  # pt_stats counts the rays as pt_render counts them
    ctx.close(), off.close()


def test_a_masked_round_is_a_tiled_render(gpu, cornell):
    ctx = first_round(gpu, cornell)
    before = ctx.read_adaptive()
    thr = midpoint_threshold(before["block_error"])
    ctx.set_adaptive(threshold=thr, min_samples=8, round_samples=8, max_samples=16)
    active = ~(before["block_error"] < np.float32(thr))
    assert ctx.adaptive_stats["active_blocks"] == int(active.sum()) and 0 < active.sum() < len(active)
    st = ctx.render_adaptive(1)
    assert st["rounds"] == 2 and ctx.samples_per_pixel == 16 and st["active_blocks"] == 0
    after = ctx.read_adaptive()
    mask = active[R.block_of_pixel(W, H)]
    rects = R.block_rects(W, H, active)
    off = U.make_ctx(gpu, cornell, W, H)
    for half, spp in (("A", 8), ("B", 12)):
        off.set_tiles([])
        off.write_accum(before[half], spp)
        off.set_tiles(rects)
        off.render(4)
        want = off.read_accum()
        assert np.array_equal(bits(after[half][mask]), bits(want[mask])), half
        assert np.array_equal(bits(after[half][~mask]), bits(before[half][~mask])), half
    assert (after["counts"][mask] == 16).all() and (after["counts"][~mask] == 8).all()
    accum = ctx.read_accum()
    idle = ((before["A"][~mask, :3] + before["B"][~mask, :3]) * np.float32(2)).astype(np.float32)
    assert np.allclose(accum[~mask, :3], idle, rtol=1e-6, atol=0)
    assert np.array_equal(bits(accum[mask, :3]), bits((after["A"][mask, :3] + after["B"][mask, :3]).astype(np.float32)))
    assert st["samples_total"] == int(after["counts"].astype(np.uint64).sum()) and st["min_count"] == 8
    ctx.close(), off.close()


FAR_MIN, FAR_ROUND, FAR_MAX, FAR_THRESHOLD = 16, 16, 128, 0.02


@pytest.fixture(scope="module")
def far(gpu, cornell):
    """the Cornell room from far enough back that black sky surrounds it, and its sky-only blocks: every pixel of the block and all its neighbours
    saw no surface in four guide samples (the jitter of a sample stays inside its pixel)"""
    camera = scenes._camera(W, H, (0.0, 1.0, -9.0), (0.0, 1.0, 0.0), 40.0)
    ctx = U.make_ctx(gpu, cornell, W, H, camera=camera)
    ctx.render_guides(4)
    hits = ctx.read_guides()[0][:, 3].reshape(H, W)
    guides = ctx.read_guides()
    ctx.close()
    padded = np.pad(hits, 1, mode="edge")
    near = sum(padded[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    sky = np.bincount(R.block_of_pixel(W, H), weights=(near.ravel() > 0), minlength=64) == 0
    assert sky.sum() >= len(sky) // 4 and (~sky).sum() >= 4, int(sky.sum())
    return {"camera": camera, "sky": sky, "guides": guides}


def far_run(gpu, cornell, far, threshold=FAR_THRESHOLD, max_samples=FAR_MAX):
    ctx = U.make_ctx(gpu, cornell, W, H, camera=far["camera"])
    ctx.set_adaptive(threshold=threshold, min_samples=FAR_MIN, round_samples=FAR_ROUND, max_samples=max_samples)
    return ctx, ctx.render_adaptive(0)


def test_to_completion(gpu, cornell, far):
    ctx, st = far_run(gpu, cornell, far)
    got = ctx.read_adaptive()
    S = ctx.samples_per_pixel
    block_counts = got["counts"][R.lanes(W, H)[:, 0]]
    print(f"to completion: {st}, sky-only blocks {int(far['sky'].sum())}, counts {np.unique(block_counts, return_counts=True)}")
    assert st["active_blocks"] == 0 or st["max_count"] == FAR_MAX
    assert st["max_count"] == S == int(got["counts"].max())
    assert (block_counts[far["sky"]] == FAR_MIN).all()
    assert st["samples_total"] < W * H * st["max_count"] and st["samples_total"] == int(got["counts"].astype(np.uint64).sum())
    assert (got["counts"] == block_counts[R.block_of_pixel(W, H)]).all() and (got["counts"] % 2 == 0).all() and block_counts.min() >= FAR_MIN
    flags = R.active_set(block_counts, got["block_error"], FAR_THRESHOLD, FAR_MIN, FAR_MAX)
    stopped = ~flags & (block_counts < FAR_MAX)
    assert stopped.any() and (got["block_error"][stopped] < np.float32(FAR_THRESHOLD)).all()
    assert int(flags.sum()) == st["active_blocks"]
    accum = ctx.read_accum()
    want = O.accumulate("oracle", accum, U.oracle_scene(cornell).kernel_data(far["camera"], W, H), W, H, S)
    assert np.allclose(ctx.resolve(), want, atol=2e-5)
    mean = (got["A"][:, :3].astype(np.float64) + got["B"][:, :3]) / np.maximum(got["counts"], 1)[:, None]
    assert np.allclose(accum[:, :3] / np.float32(S), mean, rtol=2e-6, atol=0)  # each pixel's mean radiance times pt_samples_per_pixel
    # the whole frame is owned again: the guide pass covers every pixel, with the bits of a context that never had the mode on
    ctx.render_guides(4)
    for a, b in zip(ctx.read_guides(), far["guides"]):
        assert np.array_equal(bits(a), bits(b))
    assert np.isfinite(ctx.denoise(iterations=3)).all()
    ctx.close()


def test_gain_at_equal_budget(gpu, cornell, far):
    """tone-mapped RMSE against 4096 spp of other random numbers, pooled over the quarter of blocks whose reference halves differ most: adaptive
    below a uniform render of the same samples_total.  Gate < 1; the ratio is on the record."""
    halves = []
    for k in range(2):
        ref = U.make_ctx(gpu, cornell, W, H, camera=far["camera"])
        ref.set_sample_base(1000000 + 2048 * k)
        ref.render(2048)
        halves.append(ref.read_accum())
        ref.close()
    n = np.full(W * H, 4096, np.uint32)
    e, _ = R.pixel_error(halves[0], halves[1], n)
    Eb = R.block_error(e, W, H)[1]
    hard = np.zeros(64, bool)
    hard[np.argsort(Eb)[-16:]] = True
    mask = hard[R.block_of_pixel(W, H)]
    want = U.tonemap((halves[0][:, :3].astype(np.float64) + halves[1][:, :3]), 4096, far["camera"])
    ctx, st = far_run(gpu, cornell, far, max_samples=256)
    S = ctx.samples_per_pixel
    adaptive = U.tonemap(ctx.read_accum()[:, :3].astype(np.float64), S, far["camera"])
    counts = ctx.read_adaptive()["counts"]
    ctx.close()
    spp = int(round(st["samples_total"] / (W * H) / 2.0)) * 2
    uni = U.make_ctx(gpu, cornell, W, H, camera=far["camera"])
    uni.render(spp)
    uniform = U.tonemap(uni.read_accum()[:, :3].astype(np.float64), spp, far["camera"])
    uni.close()
    ea, eu = U.rmse(adaptive[mask], want[mask]), U.rmse(uniform[mask], want[mask])
    U.record_margin("adaptive sampling: equal-budget RMSE, hardest quarter of blocks", adaptive=ea, uniform=eu, ratio=ea / eu, uniform_spp=spp,
                    samples_total=st["samples_total"], hard_mean_count=float(counts[mask].mean()), gate=1.0)
    print(f"gain: adaptive {ea:.4e}, uniform {eu:.4e} at {spp} spp, ratio {ea / eu:.3f}; hard blocks hold {counts[mask].mean():.1f} samples; {st}")
    assert counts[mask].mean() > spp
    assert ea / eu < 1.0


def test_refusals_and_lifetime(gpu, cornell):
    baseline = D.live_resources()
    w = h = 32
    small = scenes.cornell_box(w, h)
    for kw in ({"rng_mode": D.RNG_LFSR113_PARITY}, {"max_active_rays": 512}):  # parity / refill mode, as pt_render_guides
        c = gpu.Context(w, h, **kw)
        assert U.status(lambda: c.set_adaptive(threshold=0.1)) == UNSUPPORTED and c.adaptive is False
        c.close()
    off = U.make_ctx(gpu, small, w, h)
    for call in (lambda: off.render_adaptive(1), lambda: off.adaptive_stats, off.read_adaptive, lambda: off.adaptive_params,
                 lambda: off.write_adaptive(np.zeros((w * h, 4)), np.zeros((w * h, 4)), np.zeros(w * h))):
        assert U.status(call) == STATE  # mode off
    off.set_tiles([(0, 0, 16, 16)])
    assert U.status(lambda: off.set_adaptive(threshold=0.1)) == UNSUPPORTED and off.adaptive is False  # tiles are set
    off.set_tiles([])
    off.render(4)
    never = off.read_accum()
    assert U.status(lambda: off.set_adaptive(threshold=0.1)) == STATE and off.adaptive is False  # samples in: pt_clear first
    off.close()

    ctx = U.make_ctx(gpu, small, w, h)
    prm = dict(threshold=0.05, min_samples=4, round_samples=4, max_samples=8)
    ctx.set_adaptive(**prm)
    assert ctx.adaptive_params == (float(np.float32(0.05)), 4, 4, 8)
    ctx.render_adaptive(1)
    state = ctx.read_adaptive()

    def untouched():
        now = ctx.read_adaptive()
        return ctx.adaptive is True and ctx.adaptive_params == (float(np.float32(0.05)), 4, 4, 8) and ctx.samples_per_pixel == 4 and all(
            np.array_equal(bits(now[k]) if now[k].dtype == np.float32 else now[k], bits(state[k]) if state[k].dtype == np.float32 else state[k]) for k in state)

    bad = [dict(min_samples=3), dict(round_samples=5), dict(max_samples=9), dict(min_samples=16, max_samples=8), dict(max_samples=(1 << 20) + 2),
           dict(threshold=-0.1), dict(threshold=float("nan")), dict(threshold=float("inf"))]
    for kw in bad:
        assert U.status(lambda: ctx.set_adaptive(**{**prm, **kw})) == INVALID, kw
        assert untouched(), kw
    assert U.status(lambda: ctx.set_tiles([(0, 0, 16, 16)])) == UNSUPPORTED and untouched()
    assert U.status(lambda: ctx.render(1)) == STATE and untouched()
    assert U.status(lambda: ctx.write_accum(never, 4)) == STATE and untouched()
    assert U.status(lambda: ctx.set_adaptive(False)) == STATE and untouched()  # samples in: pt_clear first
    counts = state["counts"].copy()
    for change in (lambda c: c.__setitem__(0, 2), lambda c: c.__setitem__(slice(None), 3), lambda c: c.__setitem__(slice(None), 10)):
        wrong = counts.copy()
        change(wrong)  # not constant over a block; odd; above max_samples
        assert U.status(lambda: ctx.write_adaptive(state["A"], state["B"], wrong)) == INVALID and untouched()
    ctx.set_tiles([])  # the whole frame: allowed, and what the context owns anyway
    assert untouched()

    ctx.clear()
    zero = ctx.read_adaptive()
    assert ctx.adaptive is True and ctx.samples_per_pixel == 0 and ctx.adaptive_stats["rounds"] == 0 and not any(v.any() for v in zero.values())
    ctx.set_adaptive(False)
    assert ctx.adaptive is False
    ctx.render(4)
    assert np.array_equal(bits(ctx.read_accum()), bits(never))  # the bits of a context that never had the mode on
    ctx.close()
    assert D.live_resources() == baseline
