#!/usr/bin/env python3
"""Device time of pt_temporal_accumulate at 1280 x 720 and 1920 x 1080, one JSON line (EXPERIMENTS.md).
Not part of bench.py.     usage: python tools/temporal_timing.py [--calls 25] [--batch 20] [--scene cornell|blob] [--motion] [--variance] [--response] [--firefly]

temporal_ms.static / .panned: median device ms of ONE pt_temporal_accumulate, measured between two events on the stream the context renders on
around `batch` calls in a row (one call is tens of microseconds: a pair of events around a single launch would time the events).  static: the camera
of the history is the current one (every pixel finds its four taps around its own position); panned: the camera alternates between two poses 1.5
degrees apart about the room's centre, so every call reprojects.  frame_ms: the same measurement of pt_render(1), the 1-spp frame the history serves.
floor_bytes: what a call must move -- three 16-byte reads of the current frame, two 16-byte writes and the history's two images read once (neighbours
share their taps): 7 x 16 = 112 bytes per pixel; fraction_of_copy: that traffic per second against pt_debug_copy_bandwidth.
--response: the same two figures with pt_set_temporal_response on -- one call is then k_temporal<., ., true> and k_temporal_response behind it, and the
floor 152 + 44 bytes per pixel (the two kernels' shares come from a kernel trace of this script).
--firefly: the same two figures with pt_set_firefly_clamp on -- one call is then a 8-byte memset, k_firefly (32 bytes read, 16 written per pixel) and
k_temporal<., ., ., true> (one 16-byte read of the current frame in place of two: 96 bytes) --, each as median / min / max over the calls next to the
plain kernel's own median / min / max in the same process: the spread of the plain figures is the margin the two are told apart by."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "opencl-path-tracer_amd"), ROOT]

FLOOR_BYTES_PER_PIXEL = 7 * 16
MOTION_FLOOR_BYTES_PER_PIXEL = 9 * 16  # --motion: the two motion sums are read as well
# --response: k_temporal<., ., true> reads the fast image once more and writes it and the luminance pairs (16 + 16 + 8 = 40 bytes more: 152);
# k_temporal_response reads the luminance pairs, colour_count and the fast image and writes s (8 + 16 + 16 + 4 = 44 bytes; 16 more where it stores)
RESPONSE_EXTRA_BYTES_PER_PIXEL, RESPONSE_MIX_BYTES_PER_PIXEL = 40, 44
VARIANCE_EXTRA_BYTES_PER_PIXEL = 8  # --variance: the history's variance plane read once, the new one written (4 bytes each): 120 and 152
FIREFLY_BYTES_PER_PIXEL = 48 + 6 * 16  # --firefly: k_firefly's 32 + 16, and a k_temporal that reads the plane in place of the accumulator and the albedo sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--scene", default="cornell")
    ap.add_argument("--motion", action="store_true", help="also time k_temporal<true> (instance motion set), next to the plain kernel")
    ap.add_argument("--variance", action="store_true", help="also time k_temporal<., true> (pt_set_temporal_variance), next to the plain kernel")
    ap.add_argument("--response", action="store_true", help="also time k_temporal<., ., true> + k_temporal_response (pt_set_temporal_response), next to the plain kernel")
    ap.add_argument("--firefly", action="store_true", help="also time k_firefly + k_temporal<., ., ., true> (pt_set_firefly_clamp), next to the plain kernel, with min / max")
    args = ap.parse_args()
    import torch
    from ptamd import device as D, scenes

    out = {"calls": args.calls, "batch": args.batch, "scene": args.scene, "floor_bytes_per_pixel": FLOOR_BYTES_PER_PIXEL, "sizes": {}}
    stream = torch.cuda.Stream()
    for width, height in ((1280, 720), (1920, 1080)):
        b = scenes.cornell_box(width, height) if args.scene == "cornell" else scenes.blob_room(width, height, level=5)
        ctx = D.Context(width, height, samples_in_flight=1)
        ctx.upload_scene(b.flat, sky=b.sky, material_textures=b.material_textures)
        ctx.set_camera(b.camera)
        ctx.set_stream(stream.cuda_stream)
        t = math.radians(1.5)
        turned = scenes._camera(width, height, (-3.9 * math.sin(t), 1.0, -3.9 * math.cos(t)), (0.0, 1.0, 0.0), 40.0)

        def timed(fn, per=1, spread=False):
            ms = []
            for k in range(args.warmup + args.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for i in range(per):
                    fn(i)
                e1.record(stream)
                ctx.synchronize()
                if k >= args.warmup:
                    ms.append(e0.elapsed_time(e1) / per)
            if spread:
                return {"median": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5)}
            return statistics.median(ms)

        frame = timed(lambda i: ctx.render(1, sync=False))
        ctx.clear()
        ctx.render(1)
        ctx.render_guides(1)
        ctx.temporal_reset()
        ctx.temporal_accumulate()
        static = timed(lambda i: ctx.temporal_accumulate(sync=False), args.batch)

        def panned_call(i):
            ctx.set_camera(turned if i % 2 else b.camera)  # (host side only: the accumulator and the guides stay what they are)
            ctx.temporal_accumulate(sync=False)
        panned = timed(panned_call, args.batch)
        cn, _ = ctx.read_temporal()
        floor = FLOOR_BYTES_PER_PIXEL * width * height
        copy = ctx.copy_bandwidth(1 << 28, 5)
        out["sizes"][f"{width}x{height}"] = {
            "frame_ms": round(frame, 4), "temporal_ms": {"static": round(static, 5), "panned": round(panned, 5)}, "floor_bytes": floor,
            "gbps": {"static": round(floor / static / 1e6, 1), "panned": round(floor / panned / 1e6, 1)}, "copy_gbps": round(copy, 1),
            "fraction_of_copy": {"static": round(floor / static / 1e6 / copy, 3), "panned": round(floor / panned / 1e6 / copy, 3)},
            "mean_history_count_panned": round(float(cn[:, 3].mean()), 2)}
        if args.variance:
            # k_temporal<false, true> in the same process, against the same copy rate and the plain kernel above: one more 4-byte plane read and written
            ctx.set_camera(b.camera)
            ctx.temporal_reset()
            ctx.set_temporal_variance()
            ctx.temporal_accumulate()
            v_static = timed(lambda i: ctx.temporal_accumulate(sync=False), args.batch)
            v_panned = timed(panned_call, args.batch)
            v_floor = (FLOOR_BYTES_PER_PIXEL + VARIANCE_EXTRA_BYTES_PER_PIXEL) * width * height
            out["sizes"][f"{width}x{height}"]["variance"] = {
                "temporal_ms": {"static": round(v_static, 5), "panned": round(v_panned, 5)}, "floor_bytes": v_floor,
                "ratio_to_plain": {"static": round(v_static / static, 3), "panned": round(v_panned / panned, 3)},
                "fraction_of_copy": {"static": round(v_floor / v_static / 1e6 / copy, 3), "panned": round(v_floor / v_panned / 1e6 / copy, 3)}}
            ctx.temporal_reset()
            ctx.set_temporal_variance(False)
            ctx.temporal_accumulate()
        if args.response:
            # k_temporal<false, false, true> and k_temporal_response behind it, in the same process and the same batches as the plain kernel, against the same
            # copy rate: one call is the two launches.  The accumulator stays what it is, so s is 0 almost everywhere and the mix stores next to nothing: the
            # floor is the one without the store.  (The two kernels' shares: a kernel trace of this script.)
            ctx.set_camera(b.camera)
            ctx.temporal_reset()
            ctx.set_temporal_response()
            ctx.temporal_accumulate()
            r_static = timed(lambda i: ctx.temporal_accumulate(sync=False), args.batch)
            r_panned = timed(panned_call, args.batch)
            r_floor = (FLOOR_BYTES_PER_PIXEL + RESPONSE_EXTRA_BYTES_PER_PIXEL + RESPONSE_MIX_BYTES_PER_PIXEL) * width * height
            out["sizes"][f"{width}x{height}"]["response"] = {
                "temporal_ms": {"static": round(r_static, 5), "panned": round(r_panned, 5)}, "floor_bytes": r_floor,
                "ratio_to_plain": {"static": round(r_static / static, 3), "panned": round(r_panned / panned, 3)},
                "mean_mix_factor_panned": round(float(ctx.read_temporal_response().mean()), 5),
                "fraction_of_copy": {"static": round(r_floor / r_static / 1e6 / copy, 3), "panned": round(r_floor / r_panned / 1e6 / copy, 3)}}
            ctx.temporal_reset()
            ctx.set_temporal_response(False)
            ctx.temporal_accumulate()
        if args.firefly:
            # the memset, k_firefly and k_temporal<false, false, false, true> in the same process and the same batches as the plain kernel, which is timed
            # again right before: median / min / max of both
            ctx.set_camera(b.camera)
            ctx.temporal_reset()
            ctx.temporal_accumulate()
            off = {"static": timed(lambda i: ctx.temporal_accumulate(sync=False), args.batch, spread=True), "panned": timed(panned_call, args.batch, spread=True)}
            if not hasattr(ctx, "set_firefly_clamp"):  # a build from before the mode: the plain figures and their spread, to hold the mode off against
                out["sizes"][f"{width}x{height}"]["firefly"] = {"plain_ms": off}
                ctx.close()
                continue
            ctx.set_firefly_clamp()
            ctx.temporal_accumulate()
            on = {"static": timed(lambda i: ctx.temporal_accumulate(sync=False), args.batch, spread=True), "panned": timed(panned_call, args.batch, spread=True)}
            f_floor = FIREFLY_BYTES_PER_PIXEL * width * height
            out["sizes"][f"{width}x{height}"]["firefly"] = {
                "plain_ms": off, "temporal_ms": on, "floor_bytes": f_floor, "counts": list(ctx.firefly_counts),
                "ratio_to_plain": {k: round(on[k]["median"] / off[k]["median"], 3) for k in on},
                "fraction_of_copy": {k: round(f_floor / on[k]["median"] / 1e6 / copy, 3) for k in on}}
            ctx.set_firefly_clamp(False)
            ctx.set_camera(b.camera)
        if args.motion:
            # k_temporal<true> in the same process, against the same copy rate: every instance was a millimetre to the side, so every pixel of it carries
            # a displacement; two more 16-byte reads per pixel, 9 x 16 = 144 bytes
            was = b.flat.top_nodes["invTransform"].copy()
            was[:, 12] += 1e-3
            ctx.set_camera(b.camera)
            ctx.clear()
            ctx.set_instance_motion(was)
            is_set, moving = ctx.instance_motion
            assert is_set and moving == int((b.flat.top_nodes["isLeaf"] != 0).sum())
            ctx.render(1)
            ctx.render_guides(1)
            m_static = timed(lambda i: ctx.temporal_accumulate(sync=False), args.batch)
            m_panned = timed(panned_call, args.batch)
            m_floor = MOTION_FLOOR_BYTES_PER_PIXEL * width * height
            out["sizes"][f"{width}x{height}"]["motion"] = {
                "temporal_ms": {"static": round(m_static, 5), "panned": round(m_panned, 5)}, "floor_bytes": m_floor, "moving_instances": moving,
                "expected_ms": {"static": round(static * MOTION_FLOOR_BYTES_PER_PIXEL / FLOOR_BYTES_PER_PIXEL, 5),
                                "panned": round(panned * MOTION_FLOOR_BYTES_PER_PIXEL / FLOOR_BYTES_PER_PIXEL, 5)},
                "fraction_of_copy": {"static": round(m_floor / m_static / 1e6 / copy, 3), "panned": round(m_floor / m_panned / 1e6 / copy, 3)}}
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
