#!/usr/bin/env python3
"""Device time of pt_render_guides(4) at 1920 x 1080 on the blob room after a refit of its blob, one JSON line (EXPERIMENTS.md, "Vertex motion"):
without motion (k_guides<0>), with an instance motion set (k_guides<1>) and with instance and vertex motion (k_guides<2>).  Not part of bench.py.
     usage: python tools/guides_timing.py [--calls 15] [--warmup 3] [--level 6] [--samples 4] [--chain K [--reflections] [--scene S]] [--rebuilt]

Each figure is the median over `calls` of the time between two events on the stream the context renders on, around ONE pt_render_guides(samples):
the camera rays, the closest-hit pass and k_guides, `samples` times.  The three cases run in one process on the same scene state -- the blob leaning
0.05 at its top against the state before --, so the first two, which are the kernels of before, are the yardstick of the third.

--chain K (EXPERIMENTS.md, "Guide chain"): the blob room with a GLASS blob (BASIC_REFRACTIVE, index 1.5) instead, no motion: pt_render_guides(samples) with
pt_set_guide_chain(K) -- K = 0 makes the launches of a library without the chain, and never calls the setter, so that PTAMD_LIB may name such a library --
next to the 1-spp frame the guides serve (pt_clear + pt_render(1), timed the same way) and the share of guide entries that go through glass.

--reflections (EXPERIMENTS.md, "Guide reflections"; with --chain K): pt_set_guide_reflections(1) as well, and --scene names what the chain runs over:
glass_blob (the default: the reflecting kernel over glass), mirror_blob (the blob room with a polished metal blob) or mirror_wall (cornell_mirror_wall).
Without --reflections the setter is never called, and a scene without glass then runs the chain-off kernels whatever K.

--rebuilt (EXPERIMENTS.md, "Rebuilt motion"): the device work of ONE pt_set_rebuilt_motion -- the map's upload, k_gather_then, the per-instance tables --
between two events on the render stream, on the blob room with a 20 480-triangle blob and on the benchmark scene (scenes.instanced_grid: the ~1M
instanced triangles are its shading records times its instances; the records are what the call moves), the map a seeded random permutation.  Beside it,
from a second context on the same scene, ONE pt_set_vertex_motion(1) after a refit: the device-to-device copy of the same number of records, which is
how the same buffer was filled before there was a map.  The two calls alternate, `calls` times each after `warmup`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "opencl-path-tracer_amd"), ROOT]


def chain_timing(args, D, L, scenes, torch, np, width, height):
    if args.scene == "mirror_wall":
        b = scenes.cornell_mirror_wall(width, height)
    else:
        blob = L.material_pbr_metal((0.95, 0.8, 0.5), 1.0) if args.scene == "mirror_blob" else L.material_basic_refractive(1.5)
        b = scenes.blob_room(width, height, material=blob, level=args.level)
    ctx = D.Context(width, height)
    ctx.upload_scene(b.flat, sky=b.sky, material_textures=b.material_textures)
    ctx.set_camera(b.camera)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    if args.chain:
        ctx.set_guide_chain(args.chain)
    if args.reflections:
        ctx.set_guide_reflections(True)

    def timed(work):
        ms = []
        for k in range(args.warmup + args.calls):
            ctx.clear()
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            work()
            e1.record(stream)
            ctx.synchronize()
            if k >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    out = {"width": width, "height": height, "triangles": int(len(b.flat.triangles)), "samples": args.samples, "calls": args.calls, "chain": args.chain,
           "scene": args.scene, "reflections": bool(args.reflections)}
    out["render_guides"] = timed(lambda: ctx.render_guides(args.samples, sync=False))
    out["frame_1spp"] = timed(lambda: ctx.render(1, sync=False))
    ctx.clear()
    ctx.render_guides(1)
    a, g = ctx.read_guides()
    out["mean_distance"] = round(float(g[:, 3][a[:, 3] > 0].mean()), 4)  # (moves behind the blob with the chain on)
    if args.chain:
        ctx.debug_guide_chain_terminals(True)
        ctx.clear()
        ctx.render_guides(1)
        stage = ctx.read_guide_chain_terminals()[:, 2]
        out["entries_per_stage"] = np.bincount(stage[stage >= 0], minlength=args.chain + 1).tolist()  # (all zero: the chain-off kernels ran)
    ctx.close()
    print(json.dumps(out))


def rebuilt_timing(args, D, H, scenes, torch, np):
    out = {"calls": args.calls, "warmup": args.warmup}
    for name, bundle in (("blob_20k", scenes.blob_room(256, 256, level=5, builder=H.BVH_BINNED_FAST)), ("bench_scene", scenes.instanced_grid(256, 256, level=args.level))):
        flat, n = bundle.flat, len(bundle.flat.triangles)
        ctxs, streams = [], []
        for _ in range(2):
            c = D.Context(256, 256)
            c.upload_scene(flat, sky=bundle.sky, material_textures=bundle.material_textures)
            c.set_camera(bundle.camera)
            streams.append(torch.cuda.Stream())
            c.set_stream(streams[-1].cuda_stream)
            ctxs.append(c)
        rebuilt, refitted = ctxs
        rebuilt.upload_static_async(flat)  # the same arrays as a rebuilt scene: the other static set, the other dynamic set
        rebuilt.upload_dynamic(flat)
        mesh = bundle.scene._meshes[-1]
        first_vertex, _ = bundle.scene.mesh_offsets(mesh)
        refitted.refit_vertices(first_vertex, mesh.vertices_view())  # the same vertices: another version of the static arrays, so the records are copied
        refitted.upload_dynamic(bundle.scene.flatten_dynamic_only()[0])
        perm = np.random.default_rng(7).permutation(n).astype(np.uint32)
        ms = {"set_rebuilt_motion": [], "set_vertex_motion": []}
        for k in range(args.warmup + args.calls):
            for key, c, s, call in (("set_vertex_motion", refitted, streams[1], lambda: refitted.set_vertex_motion()),
                                    ("set_rebuilt_motion", rebuilt, streams[0], lambda: rebuilt.set_rebuilt_motion(perm))):
                c.clear()
                c.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                call()
                e1.record(s)
                c.synchronize()
                if k >= args.warmup:
                    ms[key].append(e0.elapsed_time(e1))
        assert rebuilt.rebuilt_motion == (True, n) and refitted.vertex_motion == (True, 1)
        r = {key: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for key, v in ms.items()}
        r["records"], r["record_bytes_moved"] = n, n * 256
        r["ratio_of_medians"] = round(r["set_rebuilt_motion"]["median_ms"] / r["set_vertex_motion"]["median_ms"], 3)
        out[name] = r
        for c in ctxs:
            c.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--chain", type=int, default=None, help="time the guide chain with this many transmissions on the glass blob room instead")
    ap.add_argument("--reflections", action="store_true", help="with --chain: pt_set_guide_reflections(1) as well")
    ap.add_argument("--scene", choices=["glass_blob", "mirror_blob", "mirror_wall"], default="glass_blob", help="with --chain: what the chain runs over")
    ap.add_argument("--rebuilt", action="store_true", help="time pt_set_rebuilt_motion beside pt_set_vertex_motion's device-to-device copy instead")
    args = ap.parse_args()
    import numpy as np
    import torch
    from ptamd import device as D, host as H, layout as L, scenes

    width, height = 1920, 1080
    if args.rebuilt:
        return rebuilt_timing(args, D, H, scenes, torch, np)
    if args.chain is not None:
        return chain_timing(args, D, L, scenes, torch, np, width, height)
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
