"""The scan that chooses the firefly clamp's defaults (include/ptamd.h, PT_FIREFLY_DEFAULT_*), on the oracle alone: five rooms at 1 and 4 spp, two
sample bases each, every (rank, scale) of the grid; the quantity is the tone-mapped RMSE against a converged render after five a-trous iterations
(tests/denoise_ref.py, defaults), clamp on over clamp off.  Guides from pixel-centre rays through the guide chain with reflections (K = 4), as the
mirror tests take them."""
import numpy as np

import denoise_ref as R
import firefly_ref as F
import gpu_util as U
import mirror_ref as M
import orclib as O
from ptamd import scenes
from test_denoise_ref import pixel_centre_rays

ROOMS = [("cornell_box", scenes.cornell_box, 64, 64, 256), ("cornell_mirror_wall", scenes.cornell_mirror_wall, 64, 64, 1024),
         ("cornell_behind_glass", scenes.cornell_behind_glass, 64, 64, 1024), ("mirror_blob_room", scenes.mirror_blob_room, 64, 36, 1024),
         ("zoo_room", scenes.zoo_room, 64, 36, 1024)]
RANKS, SCALES = (1, 2, 3, 4), (1.5, 2.0, 3.0, 4.0, 8.0)
PAIRS = [(r, s) for r in RANKS for s in SCALES]
SPPS, BASES = (1, 4), (0, 1000)
REFERENCE_BASE = 100000  # the converged render's first sample: none of the frames' samples is in it
ITERATIONS = 5


def reference(bundle, width, height, spp):
    sc = U.oracle_scene(bundle)
    hi, _ = O.render(sc, bundle.camera, width, height, spp, first_sample=REFERENCE_BASE, threads=8)
    return sc, U.tonemap(hi[:, :3].reshape(height, width, 3), spp, bundle.camera)


def scan(rooms=ROOMS, pairs=PAIRS, spps=SPPS, bases=BASES):
    """{(room, spp, base): dict(off=rmse, on={pair: rmse}, kept={pair: luminance kept}, unfiltered={pair: ratio before the filter})}"""
    out = {}
    for name, make, w, h, ref_spp in rooms:
        b = make(w, h)
        sc, ref = reference(b, w, h, ref_spp)
        o, d = pixel_centre_rays(b.camera, w, h)
        a, g, _ = M.chain(b.flat, sc, o, d, 4)
        a, g = a.reshape(h, w, 4), g.reshape(h, w, 4)
        for spp in spps:
            for base in bases:
                lo, _ = O.render(sc, b.camera, w, h, spp, seed=1, first_sample=base, threads=8)
                lo = lo.reshape(h, w, 4)
                d0, albedo, n, z = R.prepare(lo, spp, a, g, 1)
                image = lambda dd, filt: U.tonemap((R.atrous(dd, n, z, ITERATIONS) if filt else dd) * albedo, 1, b.camera)
                run = dict(off=U.rmse(image(d0, True), ref), on={}, kept={}, unfiltered={})
                raw = U.rmse(image(d0, False), ref)
                dd, lum, finite = F.demodulated(lo, spp, a, 1)
                for pair in pairs:
                    plane = F.clamp_plane(dd, lum, finite, *pair)[0][..., :3]
                    run["on"][pair] = U.rmse(image(plane, True), ref)
                    run["unfiltered"][pair] = U.rmse(image(plane, False), ref) / raw
                    run["kept"][pair] = float(R.luminance(plane * albedo).sum() / R.luminance(d0 * albedo).sum())
                out[(name, spp, base)] = run
    return out


def worst_ratio(result, pair):
    return max(run["on"][pair] / run["off"] for run in result.values())


def choose(result, pairs=PAIRS):
    """(pair, whether it qualifies): the smallest worst-case on / off ratio among the pairs whose ratio is <= 1.00 on every run; if none qualifies, the
    smallest worst case of all"""
    worst = {pair: worst_ratio(result, pair) for pair in pairs}
    good = [p for p in pairs if worst[p] <= 1.0]
    return min(good or pairs, key=lambda p: worst[p]), bool(good)


def pooled(result, room, spp, pair):
    """the on / off ratio of one room at one spp, pooled over its bases as a sum of squared errors"""
    runs = [run for (name, s, _), run in result.items() if name == room and s == spp]
    return float(np.sqrt(sum(run["on"][pair] ** 2 for run in runs) / sum(run["off"] ** 2 for run in runs)))
