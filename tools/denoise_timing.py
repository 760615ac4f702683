#!/usr/bin/env python3
"""Device time of the guide pass and of the a-trous denoiser at 1280 x 720 and 1920 x 1080, one JSON line (EXPERIMENTS.md).
Not part of bench.py.     usage: python tools/denoise_timing.py [--calls 25] [--scene cornell|blob] [--variance] [--firefly]

denoise_ms[N]: median `ms_out` of pt_denoise with N iterations (hipEvents around the filter's kernels); their differences say what each
iteration costs.  guides_ms: median device ms of pt_render_guides(1), between two events on the stream the context renders on.  frame_ms: the
same for pt_render(1), the frame the two serve.  bytes: what the filter must move (prepare: 3 reads + 2 writes, every iteration 2 reads + 1
write of a float4 image); fraction_of_copy: that traffic per second against pt_debug_copy_bandwidth.
--variance: the same six medians for PT_DENOISE_INPUT_TEMPORAL (k_atrous over the history) and PT_DENOISE_INPUT_TEMPORAL_VARIANCE (k_atrous<., true>) in the
same process, and per iteration -- the difference of two consecutive medians -- the ratio of the second to the first.
--firefly: median / min / max of pt_denoise with 1 and 5 iterations over the accumulator with pt_set_firefly_clamp off and on in the same process (on: a
memset and k_firefly before a prepare that reads the plane): the spread of the mode-off figures is the margin the two are told apart by."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "opencl-path-tracer_amd"), ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scene", default="cornell")
    ap.add_argument("--variance", action="store_true", help="also time the variance-guided filter against the plain one over the same history")
    ap.add_argument("--firefly", action="store_true", help="also time the filter over the accumulator with the firefly clamp on, next to the mode off, with min / max")
    args = ap.parse_args()
    import torch
    from ptamd import device as D, scenes

    out = {"calls": args.calls, "scene": args.scene, "sizes": {}}
    stream = torch.cuda.Stream()
    for width, height in ((1280, 720), (1920, 1080)):
        b = scenes.cornell_box(width, height) if args.scene == "cornell" else scenes.blob_room(width, height, level=5)
        ctx = D.Context(width, height, samples_in_flight=1)
        ctx.upload_scene(b.flat, sky=b.sky, material_textures=b.material_textures)
        ctx.set_camera(b.camera)
        ctx.set_stream(stream.cuda_stream)

        def timed(fn):
            ms = []
            for k in range(args.warmup + args.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                ctx.synchronize()
                if k >= args.warmup:
                    ms.append(e0.elapsed_time(e1))
            return statistics.median(ms)

        frame = timed(lambda: ctx.render(1, sync=False))
        guides = timed(lambda: ctx.render_guides(1, sync=False))
        den = {}
        for n in range(1, 7):
            ms = [ctx.denoise(n, with_ms=True)[1] for _ in range(args.warmup + args.calls)][args.warmup:]
            den[n] = statistics.median(ms)
        pixels = width * height
        moved = (5 * 16 + 5 * 3 * 16) * pixels
        copy = ctx.copy_bandwidth(1 << 28, 5)
        out["sizes"][f"{width}x{height}"] = {
            "frame_ms": round(frame, 4), "guides_ms": round(guides, 4), "denoise_ms": {str(k): round(v, 4) for k, v in den.items()},
            "bytes_5_iterations": moved, "gbps_5_iterations": round(moved / den[5] / 1e6, 1), "copy_gbps": round(copy, 1),
            "fraction_of_copy": round(moved / den[5] / 1e6 / copy, 3)}
        if args.firefly:
            per = {}
            have = hasattr(ctx, "set_firefly_clamp")  # (a build from before the mode: the mode-off figures and their spread alone)
            for name, clamp in (("off", False), ("on", True), ("off_again", False)) if have else (("off", False),):
                if have:
                    ctx.set_firefly_clamp(clamp)
                per[name] = {}
                for n in (1, 5):
                    ms = [ctx.denoise(n, with_ms=True)[1] for _ in range(args.warmup + args.calls)][args.warmup:]
                    per[name][str(n)] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
                if clamp:
                    per["counts"] = list(ctx.firefly_counts)
            if have:
                per["on_minus_off_ms"] = {n: round(per["on"][n]["median"] - per["off"][n]["median"], 4) for n in ("1", "5")}
            out["sizes"][f"{width}x{height}"]["firefly"] = per
        if args.variance:
            ctx.clear()
            ctx.render(1)
            ctx.render_guides(1)
            ctx.temporal_reset()
            ctx.set_temporal_variance()
            for f in range(4):  # a history with counts and a variance plane that are not trivial
                ctx.temporal_accumulate()
            per = {}
            for name, which in (("plain", D.DENOISE_INPUT_TEMPORAL), ("guided", D.DENOISE_INPUT_TEMPORAL_VARIANCE)):
                per[name] = {}
                for n in range(1, 7):
                    ms = [ctx.denoise(n, with_ms=True, input=which)[1] for _ in range(args.warmup + args.calls)][args.warmup:]
                    per[name][n] = statistics.median(ms)
            step = {name: {1: per[name][1]} | {n: per[name][n] - per[name][n - 1] for n in range(2, 7)} for name in per}  # (1: prepare included)
            out["sizes"][f"{width}x{height}"]["variance"] = {
                "denoise_ms": {name: {str(k): round(v, 4) for k, v in per[name].items()} for name in per},
                "iteration_ms": {name: {str(2 ** (k - 1)): round(v, 4) for k, v in step[name].items()} for name in per},
                "ratio_by_step": {str(2 ** (k - 1)): round(step["guided"][k] / step["plain"][k], 3) for k in range(1, 7)}}
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
