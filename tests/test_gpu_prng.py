"""The production PRNG as the device library compiles it (Context.debug_rng_probe: rngCounter, Rng::u01, Rng::randomInteger of csrc/pt_math.h) against the
numpy restatement of tests/prng_ref.py, bit for bit -- the restatement tests/test_prng_cpu.py holds to the oracle and to the statistics."""
import itertools

import numpy as np
import pytest

import prng_ref as P
from prng_ref import EDGE, edge_keys

pytestmark = pytest.mark.gpu

H_EXTREMES = [0, 0xFF, 0x100, 0xFFFFFF00, 0xFFFFFFFF]  # hash words at either end of u01: 0, 0, 2^-24, 1 - 2^-24, 1 - 2^-24
RANGES = [(0, n - 1) for n in (1, 2, 3, 7, 1000, (1 << 24) - 1, 1 << 24, (1 << 24) + 2, 10 ** 6)] + [(3, 9), (-4, 4)]
DEPTHS = 17


@pytest.fixture(scope="module")
def probe(gpu):
    """One launch over everything the tests below look at"""
    rng = np.random.default_rng(31)
    keys = np.concatenate([edge_keys(), rng.integers(0, 1 << 32, (64, 3), dtype=np.uint32)])
    keyed = np.zeros((len(keys) * DEPTHS, 8), np.uint32)
    keyed[:, 1:4] = np.repeat(keys, DEPTHS, axis=0)
    keyed[:, 4] = np.tile(np.arange(DEPTHS, dtype=np.uint32), len(keys))
    k1s = np.concatenate([np.array(EDGE, np.uint32), rng.integers(0, 1 << 32, 11, dtype=np.uint32)])
    rows = []
    for (h, k1), (i, j) in itertools.product(itertools.product(H_EXTREMES, k1s), RANGES):
        gamma = int(rng.integers(0, 1 << 32, dtype=np.uint32)) | 1
        rows.append([1, int(P.counter_hash_inverse(h, k1)[0]), gamma, int(k1), i & 0xFFFFFFFF, j & 0xFFFFFFFF, h, 0])
    raw = np.array(rows, np.uint32)
    entries = np.concatenate([keyed, raw])
    ctx = gpu.Context(16, 16)
    out = ctx.debug_rng_probe(entries)
    ctx.close()
    return {"keyed": keyed, "raw": raw, "out_keyed": out[:len(keyed)], "out_raw": out[len(keyed):]}


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_keyed_draws_are_the_restatement_bit_for_bit(probe):
    k, out = probe["keyed"], probe["out_keyed"]
    assert len(k) >= 125 * DEPTHS and set(k[:, 4].tolist()) == set(range(DEPTHS))
    want = P.u01(k[:, 1, None], k[:, 2, None], k[:, 3, None], k[:, 4, None], np.arange(20, dtype=np.uint32)[None, :])
    bad = np.flatnonzero((_bits(want) != out).any(axis=1))
    assert len(bad) == 0, (len(bad), [(k[i, 1:5].tolist(), out[i].tolist(), _bits(want)[i].tolist()) for i in bad[:3]])
    u = out.view(np.float32)
    assert 0.0 <= u.min() and u.max() < 1.0
    assert len(np.unique(out[:, :16])) > 0.99 * out[:, :16].size  # (draws, not a constant)


def test_draws_past_the_sixteenth_are_the_next_depths_first(probe):
    """The overlap the stage budget (tests/test_prng_cpu.py) guards against, as a fact of the device generator: draw 16 + k of depth d is draw k of depth d + 1"""
    k, out = probe["keyed"], probe["out_keyed"]
    this = np.flatnonzero(k[:, 4] < DEPTHS - 1)
    assert np.array_equal(k[this + 1, 1:4], k[this, 1:4]) and np.array_equal(k[this + 1, 4], k[this, 4] + 1)
    assert np.array_equal(out[this, 16:20], out[this + 1, 0:4])
    assert not np.array_equal(out[this, 12:16], out[this + 1, 0:4])


def test_raw_states_at_the_ends_of_the_hash_range(probe):
    raw, out = probe["raw"], probe["out_raw"]
    h = raw[:, 6]
    assert np.array_equal(P.counter_hash(raw[:, 1], raw[:, 3]), h), "the states are preimages of the extreme hash words"
    assert np.array_equal(out[:, 0], _bits(P.to_u01(h)))
    u = out[:, 0].view(np.float32)
    top = np.float32(1.0) - np.float32(2.0 ** -24)
    assert np.all(u[h >= 0xFFFFFF00] == top) and np.all(u[h <= 0xFF] == 0.0) and np.all(u[h == 0x100] == np.float32(2.0 ** -24)) and u.max() < 1.0
    # the draw after randomInteger: the state moved on by gamma, once
    assert np.array_equal(out[:, 2], _bits(P.to_u01(P.counter_hash(raw[:, 1] + raw[:, 2], raw[:, 3]))))
    assert not out[:, 3:].any()


def test_random_integer_stays_inside_its_range_at_the_extremes(probe):
    """RandomInteger(0, n - 1) picks the light: an index past the table is a read out of bounds.  (float)n * u rounds up to n at the top of the range for
    n >= 2^24; the clamp holds it."""
    raw, out = probe["raw"], probe["out_raw"]
    i, j, r = raw[:, 4].view(np.int32).astype(np.int64), raw[:, 5].view(np.int32).astype(np.int64), out[:, 1].view(np.int32).astype(np.int64)
    assert {(int(a), int(b)) for a, b in zip(i, j)} == set(RANGES)
    assert np.all(r >= i) and np.all(r <= j), [(int(a), int(b), int(c)) for a, b, c in zip(i, j, r) if not a <= c <= b][:5]
    assert np.array_equal(r, P.random_integer(i, j, out[:, 0].view(np.float32)))
    h = raw[:, 6]
    assert np.all(r[h <= 0xFF] == i[h <= 0xFF])
    small = (h >= 0xFFFFFF00) & (j - i + 1 <= 1 << 24)
    assert small.any() and np.all(r[small] == j[small])
