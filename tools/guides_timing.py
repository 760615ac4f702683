#!/usr/bin/env python3
"""Device time of pt_render_guides(4) at 1920 x 1080 on the blob room after a refit of its blob, one JSON line (EXPERIMENTS.md, "Vertex motion"):
without motion (k_guides<0>), with an instance motion set (k_guides<1>) and with instance and vertex motion (k_guides<2>).  Not part of bench.py.
     usage: python tools/guides_timing.py [--calls 15] [--warmup 3] [--level 6] [--samples 4]

Each figure is the median over `calls` of the time between two events on the stream the context renders on, around ONE pt_render_guides(samples):
the camera rays, the closest-hit pass and k_guides, `samples` times.  The three cases run in one process on the same scene state -- the blob leaning
0.05 at its top against the state before --, so the first two, which are the kernels of before, are the yardstick of the third."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "opencl-path-tracer_amd"), ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--samples", type=int, default=4)
    args = ap.parse_args()
    import numpy as np
    import torch
    from ptamd import device as D, scenes

    width, height = 1920, 1080
    b = scenes.blob_room(width, height, level=args.level)
    blob = b.scene._meshes[1]
    flat = b.flat
    ctx = D.Context(width, height)
    ctx.upload_scene(flat, sky=b.sky, material_textures=b.material_textures)
    ctx.set_camera(b.camera)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    # the next state: the blob leans (refitted on the device), every instance was a millimetre to the side
    p = blob.vertices_view()["vertex"][:, :3].copy()
    p[:, 0] += 0.05 * (p[:, 1] + 0.5) ** 2
    blob.refit(p)
    first_vertex, _ = b.scene.mesh_offsets(blob)
    ctx.refit_vertices(first_vertex, blob.vertices_view())
    dyn = b.scene.flatten_dynamic_only()[0]
    ctx.upload_dynamic(dyn)
    was = dyn.top_nodes["invTransform"].copy()
    was[:, 12] += 1e-3

    def timed():
        ms = []
        for k in range(args.warmup + args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.render_guides(args.samples, sync=False)
            e1.record(stream)
            ctx.synchronize()
            if k >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    out = {"width": width, "height": height, "triangles": int(len(flat.triangles)), "samples": args.samples, "calls": args.calls}
    ctx.clear()
    out["no_motion"] = timed()
    ctx.clear()
    ctx.set_instance_motion(was)
    out["instance_motion"] = timed()
    ctx.clear()
    ctx.set_vertex_motion()
    assert ctx.instance_motion[0] and ctx.vertex_motion == (True, 1)
    out["instance_and_vertex_motion"] = timed()
    m, _ = ctx.read_motion_guides()
    out["largest_motion_sum"] = round(float(np.abs(m).max()), 4)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
