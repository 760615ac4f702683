"""The fast division / square-root / normalize helpers of k_shade (csrc/pt_math.h) against the plain operators as the same build compiles them
(Context.debug_math_probe), bit for bit over the helpers' contract, and two small renders through the new paths against the oracle.

The contract: the same bits whenever every operand and every result is a normal float, +-0, +-inf or NaN.  The generators below emit only such
inputs -- decided from the inputs alone, in float64 with a binade of margin at either end -- so no output is ever masked after the fact."""
import itertools

import numpy as np
import pytest

import gpu_util as U
import orclib as O
from ptamd import scenes

pytestmark = pytest.mark.gpu

N_PAIRS = 1 << 20
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
ROOT_LOW = (-126.0, -96.001)  # log2 of the x that sqrtf rescales before the hardware root (x < 2^-96)


def _log_uniform(rng, n, lo=-126.0, hi=126.0):
    """n floats of either sign with magnitudes log-uniform over [2^lo, 2^hi] (float32: normal by construction)"""
    m = np.exp2(rng.uniform(lo, hi, n))
    m = np.clip(m, 2.0 ** lo, 2.0 ** hi).astype(np.float32)
    return np.where(rng.integers(0, 2, n) == 1, -m, m).astype(np.float32)


def _quotient_normal(a, b):
    """|a / b| a normal float with a binade to spare at either end (float64: exact enough to decide that from the inputs)"""
    q = np.abs(a.astype(np.float64)) / np.abs(b.astype(np.float64))
    return (q >= 2.0 ** -125) & (q <= 2.0 ** 126)


def _vector_in_contract(a, b):
    """normalize((a, b, a + b)): the squared length a normal float or an overflow to +inf (never denormal), and every component over the length zero or
    a normal float.  The length itself then lies in [2^-62, 2^64]: its reciprocal is normal."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    s64 = (a + b).astype(np.float64)  # the third component as the kernel forms it (float32 sum)
    d = a64 * a64 + b64 * b64 + s64 * s64
    ok = d >= 2.0 ** -124
    # the kernel's float32 products: a square below the normal range may be flushed or kept, identically in both forms -- but keep the sum well clear of it
    ln = np.sqrt(d)
    for c in (a64, b64, s64):
        q = np.abs(c) / ln
        ok &= (q == 0.0) | (q >= 2.0 ** -125) | (d > 2.0 ** 127)  # (an overflowed length is +inf in both forms: every component becomes 0)
    ok &= ~((d > 2.0 ** 127) & (d < 2.0 ** 129))  # not near the overflow threshold of the float32 sum, where the two roundings of d could part
    return ok


@pytest.fixture(scope="module")
def probe(gpu):
    """One launch over everything the tests below look at: the seeded pairs, the low-root inputs, the special values."""
    rng = np.random.default_rng(20241)
    a, b = _log_uniform(rng, 2 * N_PAIRS), _log_uniform(rng, 2 * N_PAIRS)
    keep = np.flatnonzero(_quotient_normal(a, b))[:N_PAIRS]
    assert len(keep) == N_PAIRS  # (about three quarters of the draws have a normal quotient)
    a, b = a[keep], b[keep]
    # roots of [2^-126, 2^-96): paired with normal denominators (up to 2^40 times as large) that keep the quotient normal
    ra = np.abs(_log_uniform(rng, 1 << 16, *ROOT_LOW))
    rb = (ra * np.exp2(rng.uniform(0, 40, len(ra))).astype(np.float32)).astype(np.float32)
    rb = np.where(rng.integers(0, 2, len(ra)) == 1, -rb, rb).astype(np.float32)
    # every pairing of +-0, +-inf, NaN; and each of them against normal floats of both signs, either way round
    sa, sb = (np.array(x, np.float32) for x in zip(*itertools.product(SPECIALS, SPECIALS)))
    nrm = np.array([1.0, -3.0, 2.0 ** -126, -2.0 ** 126, 1.5 * 2.0 ** 100, -1.25 * 2.0 ** -100], np.float32)
    ma, mb = (np.array(x, np.float32) for x in zip(*itertools.product(SPECIALS, nrm)))
    A = np.concatenate([a, ra, sa, ma, mb])
    B = np.concatenate([b, rb, sb, mb, ma])
    ctx = gpu.Context(16, 16)
    out = ctx.debug_math_probe(A, B)
    ctx.close()
    n0, n1 = len(a), len(a) + len(ra)
    return {"a": A, "b": B, "out": out, "pairs": slice(0, n0), "low_roots": slice(n0, n1), "specials": slice(n1, len(A))}


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _assert_same_bits(what, plain, fast, a, b):
    bad = np.flatnonzero((_bits(plain) != _bits(fast)).reshape(len(a), -1).any(axis=1))
    print(f"{what}: {len(a)} inputs, {len(bad)} differ")
    assert len(bad) == 0, (what, len(bad), [(float(a[i]), float(b[i]), plain[i].tolist(), fast[i].tolist()) for i in bad[:5]])


def test_generator_covers_the_contract(probe):
    a, b = probe["a"][probe["pairs"]], probe["b"][probe["pairs"]]
    tiny = np.float32(2.0 ** -126)
    assert np.all(np.abs(a) >= tiny) and np.all(np.abs(b) >= tiny) and np.all(np.abs(a) <= 2.0 ** 126) and np.all(np.abs(b) <= 2.0 ** 126)
    ea, eb = np.log2(np.abs(a.astype(np.float64))), np.log2(np.abs(b.astype(np.float64)))
    assert ea.min() < -120 and ea.max() > 120 and eb.min() < -120 and eb.max() > 120  # the whole range of magnitudes
    assert (ea - eb).min() < -120 and (ea - eb).max() > 120  # quotients up to both ends of the normal range
    for s in (a, b):
        assert 0.45 < float((s < 0).mean()) < 0.55  # both signs
    assert int((np.abs(a) < 2.0 ** -96).sum()) > 1000  # low roots among the pairs too
    assert float(_vector_in_contract(a, b).mean()) > 0.4


def test_division_is_bit_identical_over_the_contract(probe):
    s = probe["pairs"]
    _assert_same_bits("a / b vs fastDiv, seeded pairs", probe["out"]["div"][s], probe["out"]["fast_div"][s], probe["a"][s], probe["b"][s])
    q = probe["out"]["div"][s].astype(np.float64)
    want = probe["a"][s].astype(np.float64) / probe["b"][s].astype(np.float64)
    assert np.all(np.abs(q - want) <= 2.0 ** -21 * np.abs(want))  # and it is the quotient (the probe's planes are not mixed up): well inside 2.5 ulp


def test_square_root_is_bit_identical_over_the_contract(probe):
    s = probe["pairs"]
    _assert_same_bits("sqrtf vs fastSqrt, seeded pairs", probe["out"]["sqrt"][s], probe["out"]["fast_sqrt"][s], probe["a"][s], probe["b"][s])
    r = probe["out"]["sqrt"][s].astype(np.float64)
    want = np.sqrt(np.abs(probe["a"][s].astype(np.float64)))
    assert np.all(np.abs(r - want) <= 2.0 ** -21 * want)


def test_square_root_below_the_rescaling_threshold(probe):
    """x in [2^-126, 2^-96): sqrtf multiplies these by 2^32 before the hardware root and the result by 2^-16; the bare instruction must agree."""
    s = probe["low_roots"]
    x = np.abs(probe["a"][s])
    assert np.all(x >= np.float32(2.0 ** -126)) and np.all(x < np.float32(2.0 ** -96)) and len(x) == 1 << 16
    _assert_same_bits("sqrtf vs fastSqrt, x < 2^-96", probe["out"]["sqrt"][s], probe["out"]["fast_sqrt"][s], probe["a"][s], probe["b"][s])
    _assert_same_bits("a / b vs fastDiv, a < 2^-96", probe["out"]["div"][s], probe["out"]["fast_div"][s], probe["a"][s], probe["b"][s])
    want = np.sqrt(x.astype(np.float64))
    assert np.all(np.abs(probe["out"]["fast_sqrt"][s].astype(np.float64) - want) <= 2.0 ** -21 * want)


def test_special_values_are_bit_identical(probe):
    s = probe["specials"]
    a, b, out = probe["a"][s], probe["b"][s], probe["out"]
    assert len(a) == 25 + 2 * 30
    _assert_same_bits("a / b vs fastDiv, +-0 / +-inf / NaN", out["div"][s], out["fast_div"][s], a, b)
    _assert_same_bits("sqrtf vs fastSqrt, +-0 / +-inf / NaN", out["sqrt"][s], out["fast_sqrt"][s], a, b)
    _assert_same_bits("normalize vs fastNormalize, pairings of +-0 / +-inf / NaN", out["normalize"][s][:25], out["fast_normalize"][s][:25], a[:25], b[:25])
    with np.errstate(all="ignore"):
        want = a.astype(np.float64) / b.astype(np.float64)
    got = out["fast_div"][s].astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want) & (np.isinf(want) | (want == 0))
    assert np.array_equal(got[fin], want[fin]) and np.array_equal(np.signbit(got[fin]), np.signbit(want[fin]))


def test_normalize_is_bit_identical_over_the_contract(probe):
    s = probe["pairs"]
    a, b = probe["a"][s], probe["b"][s]
    m = _vector_in_contract(a, b)
    assert m.sum() > 400000
    _assert_same_bits("normalize vs fastNormalize of (a, b, a + b), seeded pairs", probe["out"]["normalize"][s][m], probe["out"]["fast_normalize"][s][m], a[m], b[m])
    v = np.stack([a, b, a + b], 1).astype(np.float64)[m]
    ln = np.linalg.norm(v, axis=1)
    finite = ln < 2.0 ** 63  # (beyond: the float32 squared length is +inf and every component 0, in both forms)
    got = probe["out"]["fast_normalize"][s][m].astype(np.float64)
    assert np.all(np.abs(got[finite] - v[finite] / ln[finite, None]) <= 2.0 ** -20)


RENDERS = {
    "mixed_material_room": lambda: scenes.mixed_material_room(96, 54, level=2),  # five material types: both refractive ones among them
    "instanced_grid": lambda: scenes.instanced_grid(96, 54, level=2),  # sky (the miss branch) and an emissive quad
}


@pytest.mark.parametrize("case", sorted(RENDERS))
def test_render_through_the_fast_paths_matches_the_oracle(gpu, case):
    """A smoke check of the new paths at the gates of test_gpu_render.test_production_render_matches_oracle: counter PRNG on both sides, so the images agree
    path by path except where fp32 round-off flips a branch -- mean bias < 1e-3, ray counts within 0.1 %, > 97 % of the pixels within 1e-3, tone-mapped
    RMSE < 1e-3."""
    b = RENDERS[case]()
    spp = 8
    ctx = U.make_ctx(gpu, b, 96, 54, seed=3, samples_in_flight=1)
    ctx.render(spp)
    a = ctx.read_accum()[:, :3]
    st = ctx.stats()
    ctx.close()
    ref, cnt = O.render(U.oracle_scene(b), b.camera, 96, 54, spp, seed=3, threads=8)
    ref = ref[:, :3]
    assert st["rays_generated"] == cnt["raysGenerated"] == 96 * 54 * spp
    for k, ck in (("rays_extension", "raysExtension"), ("rays_shadow", "raysShadow"), ("shade_hits", "shadeHits")):
        assert abs(st[k] - cnt[ck]) <= 1e-3 * cnt[ck] + 2, (k, st[k], cnt[ck])
    U.image_margins(f"fast shading arithmetic vs the oracle path by path, {case}, 96x54, 8 spp", a, ref, spp, b.camera, 1e-3, 1e-3)
    close = np.isclose(a, ref, rtol=1e-3, atol=1e-3 * ref.max()).all(axis=1)
    U.fraction_gate(f"fast shading arithmetic vs the oracle path by path, {case}, 96x54, 8 spp: pixels within 1e-3", close, None, legacy=0.97)
