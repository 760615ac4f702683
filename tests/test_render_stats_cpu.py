"""Counter-mode renders of the oracle against the reference's own kernels, statistically (tests/render_stats.py): the fixture of the reference's side meets
the conditions it was generated under and regenerates to the same bits where oracle/_ref is built; the oracle's production-mode groups lie in the
reference's distribution, block by block, in the blocks' common lean and in the whole-image mean; a 3 % bias does not."""
import numpy as np
import pytest

import orclib as O
import render_stats as R


@pytest.fixture(scope="module")
def builders():
    return R.scene_builders()


@pytest.fixture(scope="module")
def oracle_side(builders):
    cache = {}

    def groups(scene):
        if scene not in cache:
            cache[scene] = R.oracle_groups(builders[scene](), R.K, R.fixture()[scene]["n"], seed=1)
        return cache[scene]
    return groups


def test_fixture_meets_the_conditions_it_was_generated_under():
    g = R.gates()
    for scene in R.SCENES:
        f = R.fixture()[scene]
        assert f["groups"].shape == (R.K, R.BLOCKS + 3) and f["groups"].dtype == np.float32 and f["n"] >= R.N_START
        assert np.isfinite(f["groups"]).all() and f["groups"][:, R.BLOCKS:].min() > 0
        se = R.relative_se_of_difference(f["groups"])
        assert se == f["se"] and se <= R.SE_LIMIT, (scene, se)
        c = R.compare(f["groups"][:R.K // 2], f["groups"][R.K // 2:])  # control: the reference against itself passes what the tests apply
        assert np.allclose([c["block_p_min"], c["signed"], c["image_p"], c["channel_p_min"]], f["control"], rtol=1e-9), scene
        assert all(R.verdict(c).values()), (scene, c["block_p_min"], c["signed"], c["image_p"])
        print(f"{scene}: n = {f['n']}, se {100 * se:.3f} %, control min block p {c['block_p_min']:.2e} (gate {g['block_p']:.2e}), signed {c['signed']:+.2f}, "
              f"image p {c['image_p']:.3f}")


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built (reference tree absent)")
@pytest.mark.parametrize("scene", R.SCENES)
def test_fixture_regenerates_to_the_same_bits(builders, scene):
    f = R.fixture()[scene]
    got = R.reference_groups(builders[scene](), 2, f["n"])
    assert np.array_equal(got.view(np.uint32), f["groups"][:2].view(np.uint32))


@pytest.mark.parametrize("scene", R.SCENES)
def test_counter_mode_renders_lie_in_the_references_distribution(oracle_side, scene):
    R.assert_same_distribution(f"oracle counter mode, {scene}", oracle_side(scene), R.fixture()[scene]["groups"])


@pytest.mark.parametrize("scene", R.SCENES)
def test_a_three_percent_bias_is_seen(oracle_side, scene):
    c = R.compare(oracle_side(scene) * 1.03, R.fixture()[scene]["groups"])
    assert not R.verdict(c)["image"] and c["image_p"] < R.gates()["image_p"], (scene, c["image_p"])
