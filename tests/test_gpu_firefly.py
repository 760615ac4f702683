"""The firefly clamp on the device (pt_set_firefly_clamp, k_firefly, k_temporal<., ., ., true>, k_denoise_prepare<., true>; include/ptamd.h "firefly
clamp") against its numpy restatement (tests/firefly_ref.py): the plane and its counters on planted inputs through write_accum / write_guides, the
bits the consumers owe a context with the mode off, the NaN that no longer reaches the history, the refusals, and a rendered room with a mirror blob."""
import os
import subprocess

import numpy as np
import pytest

import firefly_ref as F
import firefly_scan as S
import gpu_util as U
from ptamd import device as D, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, STATE, UNSUPPORTED = -1, -3, -4


def load(ctx, case, history=False):
    ctx.write_accum(case["accum"], case["spp"])
    ctx.write_guides(case["albedo_hits"], case["normal_depth"], case["gspp"])
    ctx.set_camera(case["camera"])
    if history:
        ctx.write_temporal(case["hist_cn"], case["hist_nd"], case["hist_camera"])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def counts_agree(counts, case, **prm):
    """the device's counters against the float64 restatement's: `nonfinite` exact, `clamped` give or take the pixels within 1e-4 of their cap"""
    ref = F.run_case(case, **prm)
    return counts[1] == ref["counts"][1] and abs(counts[0] - ref["counts"][0]) <= len(F.near(case, ref, **prm))


@pytest.mark.parametrize("name,kw,prm", F.CASES, ids=[n for n, _, _ in F.CASES])
def test_plane_matches_the_restatement(gpu, name, kw, prm):
    """plane within 8 x what float32 costs the restatement on that input + 1e-6 x the largest output; `nonfinite` exact, `clamped` within the number of
    pixels that sit within 1e-4 of their cap; a second evaluation with the same bits; every unclamped pixel with the bits a mode-off context gives d (the
    first frame of a history is (d, 1)).  16 x 16 is smaller than the 32 x 8 tile, 70 x 45 no multiple of it, 150 x 83 several tiles each way, 5 x 3
    narrower than the window, 2 x 1 has one neighbour, 1 x 1 none."""
    case = F.make_case(**kw)
    h, w = case["height"], case["width"]
    ctx = gpu.Context(w, h)
    ctx.set_firefly_clamp(**prm)
    assert ctx.firefly_clamp is True and ctx.firefly_device_ptr == 0
    load(ctx, case)
    plane, counts = ctx.read_firefly()
    assert ctx.firefly_device_ptr != 0 and ctx.firefly_counts == counts
    ref, bound = F.bounds(case, **prm)
    near = F.near(case, ref, **prm)
    err = float(np.abs(plane.reshape(h, w, 4).astype(np.float64) - ref["plane"]).max())
    U.record_margin(f"firefly plane vs restatement: {name}", error=err, bound=bound, clamped=counts[0], nonfinite=counts[1], near=len(near))
    print(f"{name}: error {err:.3e}, bound {bound:.3e}, counts {counts} (restatement {ref['counts']}), near {len(near)}")
    assert np.isfinite(plane).all()
    assert err <= bound
    assert counts[1] == ref["counts"][1] and abs(counts[0] - ref["counts"][0]) <= len(near)
    s = plane[:, 3]
    assert counts == (int(((s < 1) & (s > 0)).sum()), int((s == 0).sum()))
    again, counts_again = ctx.read_firefly()
    assert np.array_equal(bits(again), bits(plane)) and counts_again == counts
    off = gpu.Context(w, h)
    load(off, case)
    off.temporal_accumulate()
    d = off.read_temporal()[0]
    off.close()
    unclamped = s == 1
    assert unclamped.any() and np.array_equal(bits(plane)[unclamped, :3], bits(d)[unclamped, :3])
    ctx.close()


@pytest.mark.parametrize("modes", [False, True], ids=["plain", "variance+response"])
@pytest.mark.parametrize("size", [(16, 16), (70, 45)], ids=["16x16", "70x45"])
def test_where_nothing_clamps_the_history_has_the_bits_of_the_mode_off(gpu, size, modes):
    """a smooth ramp, counts (0, 0): colour_count and normal_depth, the variance plane and the fast history of k_temporal<., ., ., true> have the bits
    of a context with the mode off -- a first frame, then an accumulate over it under a panned camera"""
    w, h = size
    first, second = F.make_smooth_case(w, h, "history"), F.make_smooth_case(w, h, "pan")
    second["accum"] = (second["accum"] * np.float32(1.25)).astype(np.float32)
    assert F.run_case(second, np.float32)["counts"] == (0, 0)
    on, off = gpu.Context(w, h), gpu.Context(w, h)
    on.set_firefly_clamp()
    for ctx in (on, off):
        if modes:
            ctx.set_temporal_variance()
            ctx.set_temporal_response()
    for case in (first, second):
        for ctx in (on, off):
            load(ctx, case)
            ctx.temporal_accumulate()
        assert on.firefly_counts == (0, 0)
        for a, b in zip(on.read_temporal(), off.read_temporal()):
            assert np.array_equal(bits(a), bits(b))
        if modes:
            assert np.array_equal(bits(on.read_temporal_variance()), bits(off.read_temporal_variance()))
            assert np.array_equal(bits(on.read_temporal_fast()), bits(off.read_temporal_fast()))
    assert on.temporal_frames == 2 and on.read_temporal()[0][:, 3].max() > 1
    on.close(), off.close()


@pytest.mark.parametrize("prm", F.PARAMS, ids=["defaults", "rank 3 scale 2"])
def test_accumulate_over_spikes_matches_the_restatement(gpu, prm):
    """70 x 45 with every planted feature over a written history: colour_count within the bound of temporal_ref.accumulate fed the restated plane;
    normal_depth with the bits of a context with the mode off"""
    case = F.make_case(70, 45)
    ctx, off = gpu.Context(70, 45), gpu.Context(70, 45)
    ctx.set_firefly_clamp(**prm)
    for c in (ctx, off):
        load(c, case, history=True)
        c.temporal_accumulate()
    (cn, nd), (_, nd_off) = ctx.read_temporal(), off.read_temporal()
    ref, bound = F.temporal_bound(case, **prm)
    err = float(np.abs(cn.reshape(45, 70, 4).astype(np.float64) - ref).max())
    U.record_margin(f"firefly accumulate vs restatement: {prm}", error=err, bound=bound)
    print(f"{prm}: error {err:.3e}, bound {bound:.3e}, counts {ctx.firefly_counts}")
    assert err <= bound
    assert counts_agree(ctx.firefly_counts, case, **prm)
    assert np.array_equal(bits(nd), bits(nd_off))
    ctx.close(), off.close()


@pytest.mark.parametrize("history", [False, True], ids=["first frame", "over a history"])
def test_a_nan_pixel_does_not_reach_the_history(gpu, history):
    """the planted NaN and Inf: with the mode on colour_count is finite everywhere -- and stays so through a second accumulate --, the same inputs
    with the mode off are not.  The accumulator itself keeps them either way."""
    case = F.make_case(70, 45)
    for clamp in (True, False):
        ctx = gpu.Context(70, 45)
        if clamp:
            ctx.set_firefly_clamp()
        load(ctx, case, history=history)
        for _ in range(2):
            ctx.temporal_accumulate()
            assert np.isfinite(ctx.read_temporal()[0]).all() == clamp
        if clamp:
            assert ctx.firefly_counts[1] == 2
            assert np.array_equal(bits(ctx.read_accum()), bits(case["accum"]).reshape(-1, 4))
        ctx.close()


@pytest.mark.parametrize("size,prm", [((70, 45), {}), ((70, 45), dict(rank=3, scale=2.0)), ((150, 83), {})], ids=["70x45", "70x45 rank 3 scale 2", "150x83"])
def test_the_filter_starts_from_the_plane(gpu, size, prm):
    """denoise, 5 iterations, HDR, accumulator input: within denoise_ref's bound of the restated plane filtered; the mode off differs (the spikes)"""
    w, h = size
    case = F.make_case(w, h)
    ctx = gpu.Context(w, h)
    ctx.set_firefly_clamp(**prm)
    load(ctx, case)
    out = ctx.denoise(5, hdr=True)[..., :3]
    ref, bound = F.filter_bound(case, 5, **prm)
    err = float(np.abs(out.astype(np.float64) - ref).max())
    U.record_margin(f"firefly filter vs restatement: {w}x{h} {prm}", error=err, bound=bound)
    print(f"{w}x{h} {prm}: error {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(out).all() and err <= bound
    assert counts_agree(ctx.firefly_counts, case, **prm)
    ctx.set_firefly_clamp(False)
    assert not np.array_equal(bits(ctx.denoise(5, hdr=True)[..., :3]), bits(out))
    ctx.close()


def test_zero_iterations_and_the_temporal_inputs_are_the_mode_offs(gpu):
    """iterations == 0 over the accumulator stays pt_resolve's image / the mean bit for bit; the temporal input reads the history, not the plane; resolve
    and the accumulator are untouched"""
    case = F.make_case(70, 45)
    on, off = gpu.Context(70, 45), gpu.Context(70, 45)
    on.set_firefly_clamp()
    for ctx in (on, off):
        load(ctx, case, history=True)
    for hdr in (True, False):
        assert np.array_equal(bits(on.denoise(0, hdr=hdr)), bits(off.denoise(0, hdr=hdr)))
        assert np.array_equal(bits(on.denoise(3, hdr=hdr, input_temporal=True)), bits(off.denoise(3, hdr=hdr, input_temporal=True)))
    assert np.array_equal(bits(on.resolve()), bits(off.resolve()))
    assert np.array_equal(bits(on.read_accum()), bits(off.read_accum()))
    on.close(), off.close()


def test_refusals_and_what_they_leave_alone(gpu):
    case = F.make_case(16, 16)
    ctx = gpu.Context(16, 16)
    assert ctx.firefly_clamp is False and ctx.firefly_device_ptr == 0
    assert U.status(ctx.read_firefly) == STATE  # the mode is off
    assert U.status(lambda: ctx.firefly_counts) == STATE  # nothing was evaluated
    for bad in (dict(rank=5), dict(scale=-1.0), dict(scale=0.5), dict(scale=0.999), dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=-float("inf"))):
        assert U.status(lambda: ctx.set_firefly_clamp(**bad)) == INVALID, bad
        assert ctx.firefly_clamp is False
    ctx.set_firefly_clamp(rank=3, scale=2.0)
    assert U.status(ctx.read_firefly) == STATE  # no colour samples
    ctx.write_accum(case["accum"], case["spp"])
    assert U.status(ctx.read_firefly) == STATE  # no guide samples
    assert ctx.firefly_device_ptr == 0
    load(ctx, case)
    ctx.set_tiles([(0, 0, 8, 16)])
    assert U.status(ctx.read_firefly) == UNSUPPORTED
    ctx.set_tiles([])
    assert U.status(lambda: ctx.firefly_counts) == STATE
    plane, counts = ctx.read_firefly()
    assert U.status(lambda: ctx.set_firefly_clamp(rank=7)) == INVALID and U.status(lambda: ctx.set_firefly_clamp(scale=0.25)) == INVALID
    assert ctx.firefly_clamp is True
    again, counts_again = ctx.read_firefly()  # the parameters that were set are still in force
    assert np.array_equal(bits(again), bits(plane)) and counts_again == counts and counts_agree(counts, case, rank=3, scale=2.0)
    ctx.set_firefly_clamp(rank=1, scale=1.5)  # the mode may change at any time, with a history or without
    ctx.temporal_accumulate()
    assert ctx.temporal_frames == 1 and counts_agree(ctx.firefly_counts, case, rank=1, scale=1.5)
    assert ctx.firefly_counts != counts
    ctx.set_firefly_clamp(False)
    assert ctx.firefly_clamp is False and ctx.firefly_device_ptr == 0
    assert U.status(ctx.read_firefly) == STATE
    ctx.temporal_accumulate()  # the plain kernel again
    assert not np.isfinite(ctx.read_temporal()[0]).all()
    ctx.close()
    for kw in (dict(rng_mode=D.RNG_LFSR113_PARITY), dict(max_active_rays=1024)):
        other = gpu.Context(64, 64, **kw)
        assert U.status(other.set_firefly_clamp) == UNSUPPORTED
        assert other.firefly_clamp is False
        other.close()


def test_the_buffers_go_with_the_context(gpu):
    """a context that never calls the setter allocates nothing for the stage; with the mode on the plane and the counters are two allocations more, made
    at the first evaluation and gone with the context: pt_debug_live_resources returns to its baseline"""
    case = F.make_case(16, 16)
    base = gpu.live_resources()
    counts = []
    for clamp in (False, True):
        ctx = gpu.Context(16, 16)
        load(ctx, case)
        before = gpu.live_resources()[0]
        if clamp:
            ctx.set_firefly_clamp()
            assert gpu.live_resources()[0] == before  # the setter allocates nothing
        ctx.temporal_accumulate()
        ctx.denoise(2, hdr=True)
        ctx.temporal_accumulate()
        counts.append(gpu.live_resources()[0])
        ctx.close()
        assert gpu.live_resources() == base
    assert counts[1] == counts[0] + 2


# ---------------------------------------------------------------- end to end
def test_a_rendered_room_with_a_mirror_blob(gpu):
    """mirror_blob_room at 64 x 36, 1 spp, four sample bases, guides through the chain with reflections (K = 4, four guide samples), five iterations of
    the filter over the accumulator, tone-mapped RMSE against the oracle's 1024 spp: the on / off ratio pooled over the bases as a sum of squared errors
    is at most (1 + r_cpu) / 2, r_cpu = firefly_ref.R_CPU the restatement's own figure on the oracle's renders (tests/test_firefly_ref.py) -- halfway
    between that and no gain: the device draws other noise than the oracle, and a single base moves between 0.69 and 0.73 there."""
    w, h = 64, 36
    b = scenes.mirror_blob_room(w, h)
    _, want = S.reference(b, w, h, 1024)
    ctx = U.make_ctx(gpu, b, w, h)
    ctx.set_guide_chain(4)
    ctx.set_guide_reflections()
    sums = {True: 0.0, False: 0.0}
    clamped = []
    for base in (0, 1000, 2000, 3000):
        ctx.set_sample_base(base)
        ctx.clear()
        ctx.render(1)
        ctx.render_guides(4)
        for clamp in (False, True):
            ctx.set_firefly_clamp(clamp)
            image = ctx.denoise(5, hdr=True)[..., :3]
            sums[clamp] += U.rmse(U.tonemap(image.astype(np.float64), 1, b.camera), want) ** 2
        clamped.append(ctx.firefly_counts[0])
    ctx.close()
    ratio = float(np.sqrt(sums[True] / sums[False]))
    U.record_margin("firefly clamp, mirror_blob_room 64x36, 1 spp, four bases", rmse_off=float(np.sqrt(sums[False] / 4)), rmse_on=float(np.sqrt(sums[True] / 4)),
                    ratio=ratio, gate=(1 + F.R_CPU) / 2, clamped=clamped)
    print(f"pooled RMSE off {np.sqrt(sums[False] / 4):.3e}, on {np.sqrt(sums[True] / 4):.3e}, ratio {ratio:.3f} (gate {(1 + F.R_CPU) / 2:.3f}), clamped {clamped}")
    assert ratio <= (1 + F.R_CPU) / 2


def test_cpp_firefly_example(gpu):
    """examples/firefly_cornell.cpp: the C++ class, the Cornell room with a mirror blob, 12 frames of 1 spp through history and filter with the clamp
    off and on against its own 256 spp"""
    r = subprocess.run([os.path.join(ROOT, "examples", "firefly_cornell")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    fields = dict(kv.split("=") for line in r.stdout.splitlines() for kv in line.split() if "=" in kv)
    off, on = float(fields["rmse_off"]), float(fields["rmse_on"])
    U.record_margin("firefly_cornell, 12 frames of 1 spp", rmse_off=off, rmse_on=on, clamped=int(fields["clamped"]), luminance_kept=float(fields["luminance_kept"]))
    assert on <= off
    assert int(fields["clamped"]) > 0 and 0.5 < float(fields["luminance_kept"]) <= 1.0
