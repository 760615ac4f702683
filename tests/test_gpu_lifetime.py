"""Who frees what (csrc/pt_context.h): every device allocation, pinned allocation, event and stream the library makes is owned by a member of the
context or by a local of the hook that made it.  pt_debug_live_resources counts what is alive in the process; here the counts come back to where they
stood -- after a context that went through every entry point with buffers of its own, on a caller's stream, after calls that refuse, and with a
second context alive that must not notice the first one going."""
import gc

import numpy as np
import pytest
import torch

from ptamd import device as D, scenes

pytestmark = pytest.mark.gpu

W, H, RAYS = 32, 24, 64


@pytest.fixture(scope="module")
def room():
    b = scenes.cornell_box(W, H)
    b.flat  # flattened once, shared
    return b


def _live():
    gc.collect()  # (a context another test dropped without close() goes now, not in the middle of a case)
    return D.live_resources()


def _ctx(room, **kw):
    c = D.Context(W, H, **kw)
    c.upload_scene(room.flat)
    c.set_camera(room.camera)
    return c


def _a_few_hits(ctx):
    o, d, pixel = ctx.gen_rays(0, RAYS)
    hits = ctx.intersect(o, d)
    sel = np.flatnonzero(hits["prim"] >= 0)[:5]
    assert len(sel) == 5
    return o, d, pixel, hits, sel


def _shade(ctx, o, d, pixel, hits, sel, prim=None):
    n = len(sel)
    return ctx.shade_batch(o[sel], d[sel], np.ones((n, 3), np.float32), pixel[sel], np.zeros(n, np.uint32), np.zeros(n, np.uint32), hits["t"][sel],
                           hits["u"][sel], hits["v"][sel], hits["prim"][sel] if prim is None else prim, hits["inst"][sel])


def _tour(room):
    flat = room.flat
    ctx = _ctx(room)
    during = D.live_resources()
    ctx.render(2)
    ctx.render_guides(1)
    ctx.refit_vertices(0, flat.vertices)
    ctx.upload_dynamic(flat)  # a second state, of another version of the static arrays: "then" exists, and the snapshot of its records is taken
    ctx.clear()
    ctx.set_instance_motion(flat.top_nodes)
    ctx.set_vertex_motion()
    assert ctx.vertex_motion == (True, 1)
    ctx.render(2)
    ctx.render_guides(1)
    ctx.temporal_accumulate()
    ctx.temporal_accumulate()
    assert np.isfinite(ctx.denoise(iterations=2)).all()
    assert np.isfinite(ctx.resolve()).all()
    ctx.update_geometry(flat)
    ctx.refit_vertices(0, flat.vertices)
    ctx.upload_dynamic(flat)
    ctx.upload_static_async(flat)
    ctx.upload_dynamic_async(flat)
    ctx.frame_tick()
    o, d, pixel, hits, sel = _a_few_hits(ctx)
    occluded = ctx.intersect(o, d, tmax=np.full(RAYS, 1e30, np.float32), any_hit=True)
    assert np.array_equal(occluded["prim"] == 1, hits["prim"] >= 0)
    po, pd, ppixel, phits = ctx.primary_pass(0, 1, W * H)
    assert (phits["prim"] >= 0).any()
    assert np.isfinite(_shade(ctx, o, d, pixel, hits, sel)["radiance"]).all()
    a = np.linspace(0.5, 4.0, RAYS).astype(np.float32)
    assert np.allclose(ctx.debug_math_probe(a, a[::-1])["sqrt"], np.sqrt(a))
    ctx.profile_kernels(True)
    ctx.render(1)
    busiest = D.live_resources()
    ctx.close()
    return during, busiest


def test_a_context_that_went_everywhere_leaves_nothing(gpu, room):
    base = _live()
    for _ in range(2):  # a second context neither inherits nor disturbs anything
        during, busiest = _tour(room)
        assert all(d > b for d, b in zip(during, base)), (base, during)  # (the counters do count: a context holds something of every kind)
        assert all(x >= d for x, d in zip(busiest, during)), (during, busiest)
        assert D.live_resources() == base, (base, during, busiest)


def test_the_callers_stream_outlives_the_context(gpu, room):
    base = _live()
    s = torch.cuda.Stream()
    ctx = _ctx(room)
    streams = D.live_resources()[3]
    ctx.set_stream(s.cuda_stream)
    assert D.live_resources()[3] == streams - 1  # the context's own render stream went; the caller's is not counted
    ctx.render(2)
    assert ctx.read_accum()[:, :3].sum() > 0
    ctx.close()
    assert D.live_resources() == base
    with torch.cuda.stream(s):
        x = torch.full((4096,), 3.0, device="cuda") * 2.0
    s.synchronize()
    assert float(x.sum()) == 4096 * 6.0


def test_refusals_leave_nothing_behind(gpu, room, monkeypatch):
    base = _live()
    o = np.zeros((RAYS, 3), np.float32)
    d = np.tile(np.float32([0, 0, 1]), (RAYS, 1))
    hits0 = dict(t=np.ones(RAYS, np.float32), u=np.zeros(RAYS, np.float32), v=np.zeros(RAYS, np.float32), prim=np.zeros(RAYS, np.int32),
                 inst=np.zeros(RAYS, np.int32))
    empty = D.Context(W, H)
    before = D.live_resources()
    with pytest.raises(D.PtError, match="upload the scene first"):
        empty.intersect(o, d)
    assert D.live_resources() == before
    with pytest.raises(D.PtError, match="upload the scene first"):
        _shade(empty, o, d, np.zeros(RAYS, np.uint32), hits0, np.arange(5))
    assert D.live_resources() == before
    empty.close()
    assert D.live_resources() == base

    ctx = _ctx(room)
    ctx.render(1)
    ro, rd, pixel, hits, sel = _a_few_hits(ctx)
    before = D.live_resources()
    with pytest.raises(D.PtError, match="invalid prim/inst"):
        _shade(ctx, ro, rd, pixel, hits, sel, prim=np.full(5, len(room.flat.triangles) + 5, np.int32))
    assert D.live_resources() == before
    with pytest.raises(D.PtError, match="no guide samples yet"):
        ctx.denoise(iterations=2)
    assert D.live_resources() == before
    monkeypatch.setenv("PTAMD_OFFSET_LIMIT", "1")
    with pytest.raises(D.PtError, match="more than 4 GB of either"):
        ctx.upload_dynamic(room.flat)
    monkeypatch.delenv("PTAMD_OFFSET_LIMIT")
    assert D.live_resources() == before
    ctx.render(1)  # ... and the context goes on
    ctx.close()
    assert D.live_resources() == base


def test_a_second_context_does_not_notice_the_first_one_going(gpu, room):
    base = _live()
    first, second = _ctx(room), _ctx(room)
    first.render(2)
    second.render(2)
    want = second.read_accum().copy()
    assert want[:, :3].sum() > 0
    both = D.live_resources()
    first.close()
    left = D.live_resources()
    assert all(b < l < t for b, l, t in zip(base, left, both)), (base, left, both)
    second.clear()
    second.render(2)
    assert second.read_accum().tobytes() == want.tobytes()
    second.close()
    assert D.live_resources() == base
