#!/usr/bin/env python3
"""What adaptive sampling buys and what its bookkeeping costs, at 1280 x 720 and 1920 x 1080 on cornell_box and blob_room: one JSON line
(EXPERIMENTS.md, "Adaptive sampling").  Not part of bench.py.
    usage: python tools/adaptive_timing.py [--max 1024] [--min 128] [--round 128] [--thresholds 0.02,0.01,0.005] [--reference 4096] [--scenes cornell,blob] [--sizes 1280x720,1920x1080]

Per scene and size: `uniform`, pt_render(max) -- wall ms, the device ms pt_stats reports for the call, rays (extension + shadow) from pt_stats; per threshold
pt_render_adaptive(0) -- wall ms, rays, samples_total, rounds, blocks still active, and from pt_debug_adaptive_timing the device ms inside the evaluate /
publish launch (with the bytes it must move: 60 per pixel, against pt_debug_copy_bandwidth) and the host ms spent changing the
pixel list (the list, its upload, every queue released and allocated again), with how often.  With --reference N > 0: the tone-mapped RMSE against N samples per pixel of other random numbers, pooled over the quarter of 8 x 8 blocks
whose reference halves differ most, for the uniform render and every adaptive one, and `uniform_ms_at_equal_error`: the uniform wall time scaled by
(uniform error / adaptive error)^2 -- an extrapolation along error ~ 1 / sqrt(spp), not a measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "opencl-path-tracer_amd"), os.path.join(ROOT, "tests"), ROOT]


def tonemap(rgb, spp, camera):
    ev = np.log2(float(camera["relativeAperture"]) ** 2 / float(camera["shutterTime"]) * 100 / float(camera["ISO"]))
    lum = rgb / spp / (1.2 * 2.0 ** ev)
    return lum / (1 + lum)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max", type=int, default=1024)
    ap.add_argument("--min", type=int, default=128)
    ap.add_argument("--round", type=int, default=128)
    ap.add_argument("--thresholds", default="0.02,0.01,0.005")
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--scenes", default="cornell,blob")
    ap.add_argument("--sizes", default="1280x720,1920x1080")
    args = ap.parse_args()
    from ptamd import device as D, scenes
    import adaptive_ref as R

    out = {"max_samples": args.max, "min_samples": args.min, "round_samples": args.round, "reference_spp": args.reference, "runs": {}}
    for scene in args.scenes.split(","):
        for size in args.sizes.split(","):
            width, height = (int(v) for v in size.split("x"))
            b = scenes.cornell_box(width, height) if scene == "cornell" else scenes.blob_room(width, height, level=5)

            def context():
                ctx = D.Context(width, height)
                ctx.upload_scene(b.flat, sky=b.sky, material_textures=b.material_textures)
                ctx.set_camera(b.camera)
                return ctx

            def rays(ctx):
                st = ctx.stats()
                return int(st["rays_extension"] + st["rays_shadow"])

            res = {}
            want = mask = None
            if args.reference > 0:
                halves = []
                for k in range(2):
                    ctx = context()
                    ctx.set_sample_base((1 << 24) + k * (args.reference // 2))
                    ctx.render(args.reference // 2)
                    halves.append(ctx.read_accum()[:, :3])
                    ctx.close()
                e, _ = R.pixel_error(halves[0], halves[1], np.full(width * height, args.reference, np.uint32))
                Eb = R.block_error(e, width, height)[1]
                hard = np.zeros(len(Eb), bool)
                hard[np.argsort(Eb)[-(len(Eb) // 4):]] = True
                mask = hard[R.block_of_pixel(width, height)]
                want = tonemap(halves[0][mask].astype(np.float64) + halves[1][mask], args.reference, b.camera)

            def error(ctx):
                if want is None:
                    return None
                got = tonemap(ctx.read_accum()[mask, :3].astype(np.float64), ctx.samples_per_pixel, b.camera)
                return float(np.sqrt(np.mean((got - want) ** 2)))

            ctx = context()
            ctx.render(16)  # (queues allocated, ratios learned, kernels loaded: not what is being timed)
            ctx.clear()
            r0, t0 = rays(ctx), time.perf_counter()
            ctx.render(args.max)
            wall = (time.perf_counter() - t0) * 1e3
            uniform = {"wall_ms": round(wall, 2), "rays": rays(ctx) - r0, "samples_total": width * height * args.max, "pooled_error": error(ctx)}
            copy = ctx.copy_bandwidth(1 << 28, 5)
            ctx.close()
            res["uniform"] = uniform
            res["copy_gbps"] = round(copy, 1)
            for thr in (float(t) for t in args.thresholds.split(",")):
                ctx = context()
                ctx.render(16)
                ctx.clear()
                ctx.set_adaptive(threshold=thr, min_samples=args.min, round_samples=args.round, max_samples=args.max)
                r0, t0 = rays(ctx), time.perf_counter()
                st = ctx.render_adaptive(0)
                wall = (time.perf_counter() - t0) * 1e3
                eval_ms, evals, list_ms, lists = ctx.adaptive_timing
                per_eval = eval_ms / max(evals, 1)
                moved = 60 * width * height
                a = {"wall_ms": round(wall, 2), "rays": rays(ctx) - r0, "samples_total": int(st["samples_total"]), "rounds": int(st["rounds"]),
                     "share_of_uniform": round(st["samples_total"] / (width * height * args.max), 4), "active_blocks": int(st["active_blocks"]),
                     "eval_ms_total": round(eval_ms, 4), "eval_ms_per_round": round(per_eval, 4), "eval_bytes": moved,
                     "eval_gbps": round(moved / per_eval / 1e6, 1) if per_eval > 0 else None,
                     "eval_fraction_of_copy": round(moved / per_eval / 1e6 / copy, 3) if per_eval > 0 else None,
                     "list_ms_total": round(list_ms, 2), "list_changes": int(lists), "list_ms_per_change": round(list_ms / max(lists, 1), 2),
                     "pooled_error": error(ctx)}
                if a["pooled_error"] and uniform["pooled_error"]:
                    a["uniform_ms_at_equal_error"] = round(uniform["wall_ms"] * (uniform["pooled_error"] / a["pooled_error"]) ** 2, 2)
                ctx.close()
                res[f"threshold_{thr:g}"] = a
            out["runs"][f"{scene}_{size}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
