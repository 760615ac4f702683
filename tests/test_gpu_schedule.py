"""The launch schedule (csrc/pt_schedule.h): which kernels a batch launches, counted.  One small context per row of CONFIGS; between them the rows reach
every instantiation of the kernel tables and every field of the batch plan."""
import numpy as np
import pytest

import gpu_util as U
from ptamd import device as D, layout as L, scenes

pytestmark = pytest.mark.gpu

COUNTERS = ("gen_launches", "packet_launches", "bundle_launches", "team_launches")
UNSUPPORTED = -4  # PT_ERR_UNSUPPORTED
TL, PARKED, QUEUED = D.FLAG_TWO_LEVEL_ONLY, D.FLAG_PARKED_INSTANCES, D.FLAG_QUEUE_PRIMARY_RAYS


def _cornell(glass=False):
    boxes = [L.material_refractive(0.9, 1.5, (1.0, 0.6, 0.6), 5.0), L.material_diffuse(scenes.WHITE)] if glass else None
    return scenes.cornell_box(32, 32, box_materials=boxes)  # 1 024 pixels, no instance references, a tree the team kernel's stack holds


def _zoo(kind, thin=False):
    return scenes.transform_zoo(kind, thin_lens=thin)  # 96 x 54; its blobs stay instance references under FLAG_TWO_LEVEL_ONLY


# Expected (gen, packet, bundle, team) launches, read off pt_schedule.h.  A batch of the fixed schedule is 4 bounces (max_bounces 0) of one extension pass, one
# shade launch and one shadow pass.  Its first pass: a batch of >= 16 samples per pixel is coherent -- the bundle kernel generates and walks the camera rays
# (packet + 1, bundle + 1, no k_gen), the packet kernel walks them where FLAG_QUEUE_PRIMARY_RAYS has k_gen queue them (gen + 1, packet + 1), the per-ray kernel
# with FLAG_NO_PACKETS (gen + 1); a smaller batch is k_gen + the per-ray kernel.  Every other pass goes through the per-ray kernel, or the team kernel -- scenes
# without instance references, never in parity mode -- in two cases: both first passes of a batch of ONE sample in flight (team + 2), and any pass of a batch whose
# entry count equals that of the batch the last pass-counter report came from (render() synchronises, so the report of call k is there in call k + 1; every pass
# of these frames holds fewer rays than the machine has teams): the 8 passes of a 1-spp frame, the 7 that are not the bundle kernel's of a coherent batch, all 8
# with FLAG_NO_PACKETS.  samples_in_flight 48 rounds down to 32 planes; render(48) is a batch of 32 and one of 16, neither of which meets a report of its size.
# ext_queue_fraction 0.5 at 32 planes: queues of 16 448 entries, so render(32) is a probe batch of 16, waited for, and a batch of 16 that meets its report.
# The refill loop (parity mode, max_active_rays) launches k_gen once per pass that has free slots and pixels left: once per sample where the queue holds the
# frame; with 256 slots for 1 024 pixels it depends on how many paths end per pass (the figure below is the parent commit's, and deterministic).
# `primary`: (batch, what ctx.primary_pass(0, batch, ...) adds) or the status it refuses with.  The hook issues the first pass of pt_render's batch through the
# same plan: the same k_gen / packet / bundle launches.  It never counts a team launch: teamLaunch asks for the entries of the batch being enqueued, which only
# pt_render sets -- the camera rays of a 1-spp frame go through the per-ray kernel there (same hits, pt_team.h), where pt_render's first pass adds team + 1.
CONFIGS = {
    # id: (scene, context arguments, spp of each render call, counters after each call, primary)
    "frames": (_cornell, dict(samples_in_flight=1), [1, 1], [(1, 0, 0, 2), (2, 0, 0, 10)], (1, (1, 0, 0, 0))),
    "frames_parked": (lambda: _zoo("uniform"), dict(samples_in_flight=1, flags=TL | PARKED), [1, 1], [(1, 0, 0, 0), (2, 0, 0, 0)], (1, (1, 0, 0, 0))),
    "batch16": (_cornell, dict(samples_in_flight=16, flags=D.FLAG_PACKET_INTERSECT), [16, 16], [(0, 1, 1, 0), (0, 2, 2, 7)], (16, (0, 1, 1, 0))),
    "split48": (_cornell, dict(samples_in_flight=48), [48], [(0, 2, 2, 0)], (32, (0, 1, 1, 0))),
    "no_packets": (_cornell, dict(samples_in_flight=16, flags=D.FLAG_NO_PACKETS), [16, 16], [(1, 0, 0, 0), (2, 0, 0, 8)], (16, (1, 0, 0, 0))),
    "queued": (_cornell, dict(samples_in_flight=16, flags=QUEUED), [16], [(1, 1, 0, 0)], (16, (1, 1, 0, 0))),
    "mis": (_cornell, dict(samples_in_flight=16, flags=D.FLAG_INTEGRATOR_MIS), [16], [(0, 1, 1, 0)], (16, (0, 1, 1, 0))),
    "bins": (lambda: _cornell(glass=True), dict(samples_in_flight=16, flags=D.FLAG_MATERIAL_BINS), [16], [(0, 1, 1, 0)], (16, (0, 1, 1, 0))),
    "small_queues": (_cornell, dict(samples_in_flight=32, ext_queue_fraction=0.5), [32], [(0, 2, 2, 7)], UNSUPPORTED),
    "parity": (_cornell, dict(rng_mode=D.RNG_LFSR113_PARITY), [2], [(2, 0, 0, 0)], UNSUPPORTED),
    "parity_mis": (_cornell, dict(rng_mode=D.RNG_LFSR113_PARITY, flags=D.FLAG_INTEGRATOR_MIS), [2], [(2, 0, 0, 0)], UNSUPPORTED),
    "refill": (_cornell, dict(max_active_rays=256), [1], [(8, 0, 0, 0)], UNSUPPORTED),
    "two_level": (lambda: _zoo("uniform"), dict(samples_in_flight=16, flags=TL | D.FLAG_PACKET_INTERSECT), [16], [(0, 1, 1, 0)], (16, (0, 1, 1, 0))),
    "two_level_queued": (lambda: _zoo("uniform"), dict(samples_in_flight=16, flags=TL | QUEUED), [16], [(1, 1, 0, 0)], (16, (1, 1, 0, 0))),
    "lens": (lambda: _zoo("uniform", thin=True), dict(samples_in_flight=16), [16], [(0, 1, 1, 0)], (16, (0, 1, 1, 0))),
    "lens_general": (lambda: _zoo("general", thin=True), dict(samples_in_flight=16, flags=TL), [16], [(0, 1, 1, 0)], (16, (0, 1, 1, 0))),
}


def counters(ctx):
    st = ctx.stats()
    return tuple(int(st[k]) for k in COUNTERS)


def make(gpu, name):
    scene, kw, calls, want, primary = CONFIGS[name]
    b = scene()
    return b, U.make_ctx(gpu, b, b.width, b.height, seed=5, **kw), calls, want, primary


@pytest.mark.parametrize("name", list(CONFIGS))
def test_each_batch_launches_the_kernels_its_plan_names(gpu, name):
    """Exact launch counts after every render call, and what pt_primary_pass adds to them (or the refusal of a context it does not serve); contexts with
    FLAG_PACKET_INTERSECT also send a closest-hit and an any-hit pt_intersect through the packet kernels.  Every image is complete (no NaN, light arrived)."""
    b, ctx, calls, want, primary = make(gpu, name)
    for spp, expected in zip(calls, want):
        ctx.render(spp)
        got = counters(ctx)
        print(name, "after render", spp, dict(zip(COUNTERS, got)))
        assert got == expected, (name, spp, got, expected)
    a = ctx.read_accum()[:, :3]
    assert np.isfinite(a).all() and a.mean() > 0
    assert ctx.samples_per_pixel == sum(calls)
    before = counters(ctx)
    if primary == UNSUPPORTED:
        assert U.status(lambda: ctx.primary_pass(0, 1, b.width * b.height)) == UNSUPPORTED
        assert counters(ctx) == before
    else:
        batch, added = primary
        _, _, _, hits = ctx.primary_pass(0, batch, b.width * b.height * batch)
        got = tuple(x - y for x, y in zip(counters(ctx), before))
        print(name, "primary_pass adds", dict(zip(COUNTERS, got)))
        assert got == added, (name, got, added)
        assert (hits["prim"] >= 0).mean() > 0.3
    # the scenes are what the rows are for: instance references in the tree (the two-level instantiations; parity mode always enters its instances, the
    # room's one included), the general route (k_trace<., 2>)
    st = ctx.stats()
    entered = ("frames_parked", "two_level", "two_level_queued", "lens_general", "parity", "parity_mis")
    assert (st["entered_instances"] > 0) == (name in entered), st["entered_instances"]
    assert (st["general_route"] == 1) == (name == "lens_general")
    if CONFIGS[name][1].get("flags", 0) & D.FLAG_PACKET_INTERSECT:
        o, d, _ = ctx.gen_rays(0, b.width * b.height)
        before = counters(ctx)
        closest, occluded = ctx.intersect(o, d), ctx.intersect(o, d, tmax=np.full(len(o), 1e30, np.float32), any_hit=True)
        assert counters(ctx) == (before[0], before[1] + 2, before[2], before[3])
        assert np.isin(occluded["prim"], (0, 1)).all() and (occluded["prim"] == (closest["prim"] >= 0)).mean() > 0.99  # (any hit reports 0 / 1)
    ctx.close()
