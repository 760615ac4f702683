"""Writes tests/golden/render_stats.npz: the reference's side of tests/render_stats.py -- per scene, K groups of n samples per pixel of the reference's own
kernels (oracle/_ref, run through oracle/orclib.py), each reduced to 72 block means of the luminance and the three whole-image channel means.  Data only.

Per scene n starts at render_stats.N_START and doubles until both conditions hold (the levels never move):
  * the standard error of a difference of two whole-image means of K groups is at most 0.5 % of the mean;
  * control: the reference's first K / 2 groups against its last K / 2 pass the three statistics the tests apply.
What was measured is stored beside the groups (NAME/se, NAME/control = [min block p, signed mean of block t, whole-image p, min channel p]).

    python tests/golden/make_render_stats.py        (needs oracle/_ref: the reference tree at build time)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (os.path.join(ROOT, "opencl-path-tracer_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import orclib as O  # noqa: E402
import render_stats as R  # noqa: E402


def main():
    O.build()
    assert O.have_ref(), "oracle/_ref is not built: the reference tree is needed to (re)generate this fixture"
    builders = R.scene_builders()
    out = {"K": np.int32(R.K)}
    for name in R.SCENES:
        bundle = builders[name]()
        n = R.N_START
        while True:
            groups = R.reference_groups(bundle, R.K, n)
            se = R.relative_se_of_difference(groups)
            c = R.compare(groups[:R.K // 2], groups[R.K // 2:])
            ok = se <= R.SE_LIMIT and all(R.verdict(c).values())
            print(f"{name}: n = {n}, se of a difference {100 * se:.3f} %, control: min block p {c['block_p_min']:.3e} (max |t| {c['block_t_max']:.2f}), "
                  f"signed {c['signed']:+.2f}, image p {c['image_p']:.3f}, channels min p {c['channel_p_min']:.3f} -> {'ok' if ok else 'double n'}")
            if ok:
                break
            n *= 2
            assert n <= 1024, "the conditions are not met by any affordable n: look at the scene, not at the levels"
        out[name + "/groups"] = groups
        out[name + "/n"] = np.int32(n)
        out[name + "/se"] = np.float64(se)
        out[name + "/control"] = np.array([c["block_p_min"], c["signed"], c["image_p"], c["channel_p_min"]], np.float64)
    path = os.path.join(HERE, "render_stats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
