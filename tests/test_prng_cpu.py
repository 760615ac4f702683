"""The production PRNG (csrc/pt_math.h: counterKey, counterHash, Rng::u01) on the CPU: the numpy restatement of tests/prng_ref.py is the oracle's generator
bit for bit, the construction has the structure its comments claim, a battery of statistics over the index sets the tracer uses accepts it (and an
independent generator) and rejects each of five plausible slips, and no stage of any integrator draws more than the 16 numbers it owns."""
import itertools

import numpy as np
import pytest

import orclib as O
import prng_ref as P
from prng_ref import EDGE, edge_keys
from ptamd import scenes


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_restatement_is_the_oracle_bit_for_bit():
    lib = O.oracle()
    rng = np.random.default_rng(7)
    rand = rng.integers(0, 1 << 32, (3000, 3), dtype=np.uint32)
    rd, rk = rng.integers(0, 17, 3000), rng.integers(0, 16, 3000)
    want = np.array([lib.orc_counter_u01(int(p), int(s), int(d), int(k), int(sd)) for (p, s, sd), d, k in zip(rand, rd, rk)], np.float32)
    assert np.array_equal(_bits(P.u01(rand[:, 0], rand[:, 1], rand[:, 2], rd, rk)), _bits(want))
    keys = edge_keys()
    depth, dim = np.arange(17, dtype=np.uint32)[None, :, None], np.arange(16, dtype=np.uint32)[None, None, :]
    got = P.u01(keys[:, 0, None, None], keys[:, 1, None, None], keys[:, 2, None, None], depth, dim)
    want = np.array([[[lib.orc_counter_u01(int(p), int(s), d, k, int(sd)) for k in range(16)] for d in range(17)] for p, s, sd in keys], np.float32)
    assert got.shape == want.shape == (125, 17, 16)
    assert np.array_equal(_bits(got), _bits(want))
    assert 0.0 <= got.min() and got.max() < 1.0


def test_mix32_and_the_hash_round_trip_through_their_inverses():
    rng = np.random.default_rng(8)
    x = np.concatenate([rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint32), np.array(EDGE + [0xFF, 0x100, 0xFFFFFF00, 0x7FFFFFFF], np.uint32)])
    assert np.array_equal(P.mix32_inverse(P.mix32(x)), x) and np.array_equal(P.mix32(P.mix32_inverse(x)), x)
    k1 = np.concatenate([rng.integers(0, 1 << 32, len(x) - 9, dtype=np.uint32), np.array(EDGE + EDGE[:4], np.uint32)])
    assert np.array_equal(P.counter_hash_inverse(P.counter_hash(x, k1), k1), x) and np.array_equal(P.counter_hash(P.counter_hash_inverse(x, k1), k1), x)


def test_gamma_is_odd_for_every_edge_key():
    keys = edge_keys()
    _, _, gamma = P.counter_key(keys[:, 0], keys[:, 1], keys[:, 2])
    assert np.all(gamma & 1 == 1)


def test_stream_names_of_a_full_hd_64_sample_set_are_distinct():
    """The name of a stream is (k0, k1); k0 is a function of the pixel (and the seed), k1 of the sample.  The 1920 x 1080 k0 are distinct and the 64 k1 are
    distinct, hence so are the 1920 x 1080 x 64 pairs -- for two seeds, and for sample ranges a base apart."""
    pixels = np.arange(1920 * 1080, dtype=np.uint32)
    for seed in (1, 0xFFFFFFFF):
        k0, _, _ = P.counter_key(pixels, 0, seed)
        assert len(np.unique(k0)) == len(pixels)
    for base in (0, 64, (1 << 32) - 32):  # (the last range wraps)
        _, k1, _ = P.counter_key(0, np.arange(64, dtype=np.uint32) + np.uint32(base), 1)
        assert len(np.unique(k1)) == 64
    # ... and the 64-bit names themselves, on a part small enough to sort: 2^15 pixels x 64 samples
    k0, k1, _ = P.counter_key(pixels[: 1 << 15, None], np.arange(64, dtype=np.uint32)[None, :], 1)
    names = (k0.astype(np.uint64) << np.uint64(32)) | k1.astype(np.uint64)
    assert len(np.unique(names)) == names.size == 1 << 21


def test_u01_is_strictly_below_one():
    u = P.to_u01(np.array([0xFFFFFFFF, 0xFFFFFF00, 0, 0xFF, 0x100], np.uint32))
    top = np.float32(1.0) - np.float32(2.0 ** -24)
    assert u[0] == u[1] == top and top < 1.0
    assert u[2] == u[3] == 0.0 and u[4] == np.float32(2.0 ** -24)


def test_random_integer_never_exceeds_j():
    top = np.float32(1.0) - np.float32(2.0 ** -24)
    for n in (1, 2, 3, 7, 1000, 10 ** 6, (1 << 24) - 1, 1 << 24, (1 << 24) + 2):
        r = P.random_integer(0, n - 1, np.array([0.0, 2.0 ** -24, 0.5, top], np.float32))
        assert r[0] == 0 and r.min() >= 0 and r.max() <= n - 1, (n, r)
        if n <= 1 << 24:  # the largest draw selects the last entry (at 2^24, (float)n * top = n - 1 exactly; beyond, 24-bit draws skip entries)
            assert r[3] == n - 1, (n, r)
    assert P.random_integer(3, 9, np.float32([0.0, top])).tolist() == [3, 9]


# ---- the battery ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verdicts():
    gens = {"shipped": P.shipped, "philox": P.philox_control()}
    gens.update({name: g for name, (g, _) in P.VARIANTS.items()})
    out = {name: P.judge(P.battery(g)) for name, g in gens.items()}
    for name, v in out.items():
        outside = {k: round(x[0], 1) for k, x in v.items() if not x[3]}
        print(f"{name}: {len(v)} statistics, outside their interval: {outside}")
    return out


def _report(v):
    return {k: x[:3] for k, x in v.items() if not x[3]}


def test_battery_accepts_the_shipped_generator(verdicts):
    v = verdicts["shipped"]
    assert len(v) >= 26
    for name, (value, lo, hi, inside) in v.items():
        print(f"{name:55s} {value:12.2f}  in [{lo:.2f}, {hi:.2f}]")
    assert all(x[3] for x in v.values()), _report(v)


def test_battery_accepts_an_independent_generator(verdicts):
    """Philox draws truncated to 24 bits behind the same signature: the thresholds are those of the statistics, not of our generator"""
    v = verdicts["philox"]
    assert all(x[3] for x in v.values()), _report(v)


@pytest.mark.parametrize("variant", sorted(P.VARIANTS))
def test_battery_rejects_a_slipped_generator(verdicts, variant):
    v, named = verdicts[variant], P.VARIANTS[variant][1]
    assert not v[named][3], (variant, named, v[named])


def test_thresholds_are_quantiles_at_the_family_level():
    """Bonferroni over the battery: each statistic's interval leaves level / n outside, half on either side"""
    r = P.battery(P.philox_control(3))
    j = P.judge(r)
    each = P.FAMILY_LEVEL / len(r)
    for name, (value, dist) in r.items():
        lo, hi = j[name][1], j[name][2]
        assert dist.cdf(lo) <= each / 2 + 1e-12 or dist.cdf(lo - 1) < each / 2 <= dist.cdf(lo), name  # (continuous | the integer quantile of the Poisson)
        assert dist.sf(hi) <= each / 2 + 1e-12, name


# ---- the stage budget -------------------------------------------------------------------------------------------------------------------------------------
def test_no_stage_draws_more_than_its_sixteen_numbers():
    """ctr = depth * 16 + dim + 1: a stage that made a 17th draw would read the next depth's first.  The oracle counts the draws of every stage (camera ray
    with and without the thin lens, shade with light sample and continuation) and keeps the most; every material of the oracle-vs-reference scenes and the
    diffuse box, both integrators, both ways to pick a light."""
    import test_oracle_vs_ref as T
    lib = O.oracle()
    cases = dict(T.CASES, cornell=lambda: scenes.cornell_box(48, 27))
    assert "instanced_thin_lens" in cases
    lib.orc_counter_stage_draws_reset()
    assert lib.orc_counter_stage_draws_max() == 0
    worst = {}
    for name in sorted(cases):
        b = cases[name]()
        sky = b.sky if b.sky is not None else np.full((1, 4, 8, 4), 0.7, np.float32)
        sc = O.BoundScene(b.flat, sky=sky, material_textures=b.material_textures)
        for integrator, lights in itertools.product((O.INTEGRATOR_IS, O.INTEGRATOR_MIS), (O.LIGHTS_UNIFORM, O.LIGHTS_SOLID_ANGLE)):
            lib.orc_counter_stage_draws_reset()
            acc, cnt = O.render(sc, b.camera, 48, 27, 4, seed=2, threads=4, integrator=integrator, light_sampling=lights)
            assert cnt["raysGenerated"] == 48 * 27 * 4 and np.isfinite(acc).all()
            worst[(name, integrator, lights)] = lib.orc_counter_stage_draws_max()
    mark = max(worst.values())
    print("most draws by one stage:", mark, worst)
    assert mark >= 4, "the mark counts (a thin-lens camera ray alone draws four numbers)"
    assert mark <= P.STAGE_SLOTS, mark
    lib.orc_counter_stage_draws_reset()
    assert lib.orc_counter_stage_draws_max() == 0
