"""Production renders of the device library against the reference's own kernels, statistically (tests/render_stats.py; the reference's side is the fixture
tests/golden/render_stats.npz).  A default context -- default schedule, packets and bundles, copied instances, counter PRNG -- renders K groups of n
samples per pixel, once as sample ranges of one seed (pt_clear + pt_set_sample_base(g * n) + pt_render(n): how a frame loop decorrelates its frames) and
once with K seeds; either way the groups must lie in the reference's distribution."""
import numpy as np
import pytest

import gpu_util as U
import render_stats as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def builders():
    return R.scene_builders()


def _sample_ranges(gpu, bundle, n, seed=1):
    ctx = U.make_ctx(gpu, bundle, R.W, R.H, seed=seed)
    out = []
    for g in range(R.K):
        ctx.clear()
        ctx.set_sample_base(g * n)
        ctx.render(n)
        out.append(R.reduce_group(ctx.read_accum(), n))
    assert ctx.sample_base == (R.K - 1) * n
    ctx.close()
    return np.array(out)


def _seeds(gpu, bundle, n):
    out = []
    for g in range(R.K):
        ctx = U.make_ctx(gpu, bundle, R.W, R.H, seed=1000 + g)
        ctx.render(n)
        out.append(R.reduce_group(ctx.read_accum(), n))
        ctx.close()
    return np.array(out)


@pytest.mark.parametrize("scene", R.SCENES)
def test_sample_ranges_of_one_seed_lie_in_the_references_distribution(gpu, builders, scene):
    f = R.fixture()[scene]
    got = _sample_ranges(gpu, builders[scene](), f["n"])
    R.assert_same_distribution(f"device, sample ranges, {scene}", got, f["groups"])
    c = R.compare(got * 1.03, f["groups"])  # sensitivity: a 3 % bias of the same groups is seen
    assert not R.verdict(c)["image"], (scene, c["image_p"])


@pytest.mark.parametrize("scene", R.SCENES)
def test_distinct_seeds_lie_in_the_references_distribution(gpu, builders, scene):
    f = R.fixture()[scene]
    got = _seeds(gpu, builders[scene](), f["n"])
    R.assert_same_distribution(f"device, {R.K} seeds, {scene}", got, f["groups"])
