"""Which refusal wins where two or more hold at once, for the entry points whose checks are shared helpers in the C-ABI shell (csrc/ptamd.hip): the
frame stages (pt_denoise, pt_temporal_accumulate, pt_read_firefly), the setters and transfers of the two temporal modes and the three motion
setters.  The other GPU tests pin each refusal's code one condition at a time; the order within an entry point is part of the contract as well, and
nothing else holds it.  Every row: an entry point, a context in which several refusal conditions hold, the code returned and a piece of the message in
pt_last_error that names the refusal that fired.  16 x 16 on the Cornell room; the one launch on a scene is a single guide sample."""
import re

import numpy as np
import pytest

from ptamd import device as D, scenes

pytestmark = pytest.mark.gpu
W = H = 16
OK, INVALID, STATE, UNSUPPORTED = 0, -1, -3, -4


@pytest.fixture(scope="module")
def room():
    return scenes.cornell_box(W, H)


# ---------------------------------------------------------------- context states (each row gets a context of its own)
def bare(gpu, room):
    """whole frame, no scene, no camera, no samples, every mode off, no history"""
    return gpu.Context(W, H)


def tiled(gpu, room):
    ctx = bare(gpu, room)
    ctx.set_tiles([(0, 0, 8, 8)])
    return ctx


def tiled_clamping(gpu, room):
    ctx = tiled(gpu, room)
    ctx.set_firefly_clamp()
    return ctx


def sampled(gpu, room):
    """colour and guide samples, no history, the variance off"""
    ctx = bare(gpu, room)
    ctx.write_accum(np.ones((W * H, 4), np.float32), 1)
    ctx.write_guides(np.ones((W * H, 4), np.float32), np.ones((W * H, 4), np.float32), 1)
    return ctx


def with_history(gpu, room):
    ctx = bare(gpu, room)
    ctx.write_temporal(np.ones((W * H, 4), np.float32), np.ones((W * H, 4), np.float32), room.camera)
    assert ctx.temporal_frames == 1
    return ctx


def parity(gpu, room):
    return gpu.Context(W, H, rng_mode=D.RNG_LFSR113_PARITY)


def chained(gpu, room):
    """a scene whose only dynamic state is active, a guide chain set, no guide samples"""
    ctx = gpu.Context(W, H)
    ctx.upload_scene(room.flat)
    ctx.set_camera(room.camera)
    ctx.set_guide_chain(2)
    return ctx


def chained_with_guides(gpu, room):
    ctx = chained(gpu, room)
    ctx.render_guides(1)
    assert ctx.guide_samples == 1
    return ctx


A_MAP = np.zeros(1, np.uint32)  # (a map that is there: what it holds is never looked at in these rows)

ROWS = [
    # the frame stages: parameters, then tiles, then (the history alone) the camera, then the samples, then what needs them
    ("denoise: bad input, no samples", bare, lambda c, r: c.denoise(input=99), STATE, "no colour samples yet"),
    ("denoise: tiles, no samples", tiled, lambda c, r: c.denoise(), UNSUPPORTED, "tiles are set -- the filter needs"),
    ("denoise: guided, variance off, no history", sampled, lambda c, r: c.denoise(input=D.DENOISE_INPUT_TEMPORAL_VARIANCE), STATE,
     "while the temporal variance is off"),
    ("temporal_accumulate: max_history 4097, tiles", tiled, lambda c, r: c.temporal_accumulate(max_history=4097), INVALID, "max_history = 4097"),
    ("temporal_accumulate: tiles, no camera", tiled, lambda c, r: c.temporal_accumulate(), UNSUPPORTED, "tiles are set -- the history is reprojected"),
    ("temporal_accumulate: no camera, no samples", bare, lambda c, r: c.temporal_accumulate(), STATE, "no camera yet"),
    ("read_firefly: mode off, tiles", tiled, lambda c, r: c.read_firefly(), STATE, "the firefly clamp is off"),
    ("read_firefly: tiles, no samples", tiled_clamping, lambda c, r: c.read_firefly(), UNSUPPORTED, "tiles are set -- the clamp needs"),
    # the temporal modes: schedule, then parameters, then the history
    ("set_temporal_variance: bad parameter, history", with_history, lambda c, r: c.set_temporal_variance(sigma_variance=-1.0), INVALID,
     "pt_set_temporal_variance: negative or non-finite parameter"),
    ("set_temporal_response: bad parameter, history", with_history, lambda c, r: c.set_temporal_response(sigma_response=float("nan")), INVALID,
     "pt_set_temporal_response: negative or non-finite parameter"),
    ("set_temporal_variance: parity, bad parameter", parity, lambda c, r: c.set_temporal_variance(relative_floor=-1.0), UNSUPPORTED,
     "pt_set_temporal_variance: the fixed schedule"),
    ("set_temporal_response: parity, bad parameter", parity, lambda c, r: c.set_temporal_response(fast_history=5000), UNSUPPORTED,
     "pt_set_temporal_response: the fixed schedule"),
    ("read_temporal_variance: mode off, no history", bare, lambda c, r: c.read_temporal_variance(), STATE, "the temporal variance is off (pt_set_temporal_variance)"),
    ("read_temporal_fast: mode off, no history", bare, lambda c, r: c.read_temporal_fast(), STATE, "the temporal response is off (pt_set_temporal_response)"),
    # the motion setters: schedule, state, guide samples; forgetting returns before the guide chain is looked at; the chain before everything else
    ("set_instance_motion: forget, chain", chained, lambda c, r: c.set_instance_motion(None), OK, ""),
    ("set_vertex_motion: forget, chain", chained, lambda c, r: c.set_vertex_motion(False), OK, ""),
    ("set_rebuilt_motion: forget, chain", chained, lambda c, r: c.set_rebuilt_motion(None), OK, ""),
    ("set_instance_motion: guide samples, chain", chained_with_guides, lambda c, r: c.set_instance_motion(r.flat.top_nodes), STATE,
     "pt_set_instance_motion: 1 guide samples are in the sums already"),
    ("set_vertex_motion: guide samples, chain", chained_with_guides, lambda c, r: c.set_vertex_motion(), STATE,
     "pt_set_vertex_motion: 1 guide samples are in the sums already"),
    ("set_rebuilt_motion: guide samples, chain", chained_with_guides, lambda c, r: c.set_rebuilt_motion(A_MAP), STATE,
     "pt_set_rebuilt_motion: 1 guide samples are in the sums already"),
    ("set_vertex_motion: chain, no previous state", chained, lambda c, r: c.set_vertex_motion(), UNSUPPORTED, "pt_set_vertex_motion: a guide chain is set"),
    ("set_rebuilt_motion: chain, no previous state", chained, lambda c, r: c.set_rebuilt_motion(A_MAP), UNSUPPORTED, "pt_set_rebuilt_motion: a guide chain is set"),
    ("set_instance_motion: wrong n_top, chain", chained, lambda c, r: c.set_instance_motion(np.zeros((len(r.flat.top_nodes) + 1, 16), np.float32)),
     UNSUPPORTED, "pt_set_instance_motion: a guide chain is set"),
]


@pytest.mark.parametrize("name,state,call,code,says", ROWS, ids=[row[0] for row in ROWS])
def test_the_refusal_that_wins(gpu, room, name, state, call, code, says):
    ctx = state(gpu, room)
    try:
        if code == OK:
            call(ctx, room)
            return
        with pytest.raises(D.PtError) as e:
            call(ctx, room)
        m = re.search(r"failed \((-?\d+)\): (.*)", str(e.value), re.S)
        assert m, str(e.value)
        print(f"{name}: {m.group(1)} {m.group(2)}")
        assert int(m.group(1)) == code and says in m.group(2)
    finally:
        ctx.close()
