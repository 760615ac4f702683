"""The production (counter) PRNG of csrc/pt_math.h restated in vectorised uint32 numpy, its inverse, deliberately slipped variants of it, and the battery
of statistics tests/test_prng_cpu.py holds it to.  Everything broadcasts over arrays; nothing here needs a GPU or the oracle.

A *generator* below is a callable gen(pixel, sample, seed, depth, dim) -> uint32 array of 24-bit draws (u01 = draw * 2^-24), broadcast over its arguments.
The battery only ever asks for draws through that signature, over the index sets the tracer uses, so the same code judges the shipped generator, the
slipped variants and an independent control (Philox)."""
import numpy as np
from scipy import stats as S

M1, M2 = 0x21F0AAAD, 0x735A2D97
M1_INV, M2_INV = pow(M1, -1, 1 << 32), pow(M2, -1, 1 << 32)
PHI, C_SAMPLE, C_GAMMA = 0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35
STAGE_SLOTS = 16  # ctr = depth * 16 + dim + 1
EDGE = [0, 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1]


def edge_keys():
    """every (pixel, sample, seed) of EDGE^3"""
    return np.array([(p, s, sd) for p in EDGE for s in EDGE for sd in EDGE], np.uint32)


def _u32(x):
    return np.atleast_1d(np.asarray(x)).astype(np.uint32)


def _mul(x, m):
    return (x.astype(np.uint64) * np.uint64(m)).astype(np.uint32)  # (uint64 product, truncated: no overflow warnings)


def mix32(x):
    x = _u32(x)
    x = x ^ (x >> np.uint32(16))
    x = _mul(x, M1)
    x = x ^ (x >> np.uint32(15))
    x = _mul(x, M2)
    x = x ^ (x >> np.uint32(15))
    return x


def _unshift15(x):
    return x ^ (x >> np.uint32(15)) ^ (x >> np.uint32(30))  # y = x ^ x >> 15  =>  x = y ^ y >> 15 ^ y >> 30


def mix32_inverse(y):
    x = _u32(y)
    x = _unshift15(x)
    x = _mul(x, M2_INV)
    x = _unshift15(x)
    x = _mul(x, M1_INV)
    x = x ^ (x >> np.uint32(16))
    return x


def counter_key(pixel, sample, seed):
    """(k0, k1, gamma) as counterKey makes them"""
    pixel, sample, seed = np.broadcast_arrays(_u32(pixel), _u32(sample), _u32(seed))
    k0 = mix32(pixel ^ mix32(seed ^ np.uint32(PHI)))
    k1 = mix32(sample ^ np.uint32(C_SAMPLE))
    gamma = mix32(k0 ^ k1 ^ np.uint32(C_GAMMA)) | np.uint32(1)
    return k0, k1, gamma


def counter_hash(weyl, k1):
    x, k1 = np.broadcast_arrays(_u32(weyl), _u32(k1))
    x = x ^ (x >> np.uint32(16))
    x = _mul(x, M1)
    x = x ^ k1
    x = x ^ (x >> np.uint32(15))
    x = _mul(x, M2)
    x = x ^ (x >> np.uint32(15))
    return x


def counter_hash_inverse(h, k1):
    """the weyl word that counter_hash(., k1) maps to h: every step is a bijection of the 32-bit words"""
    x, k1 = np.broadcast_arrays(_u32(h), _u32(k1))
    x = _unshift15(x)
    x = _mul(x, M2_INV)
    x = _unshift15(x)
    x = x ^ k1
    x = _mul(x, M1_INV)
    x = x ^ (x >> np.uint32(16))
    return x


def weyl_word(k0, gamma, depth, dim):
    ctr = _u32(depth) * np.uint32(STAGE_SLOTS) + _u32(dim) + np.uint32(1)
    return k0 + ctr * gamma  # (uint32 arrays wrap)


def hash_word(pixel, sample, seed, depth, dim):
    k0, k1, gamma = counter_key(pixel, sample, seed)
    return counter_hash(weyl_word(k0, gamma, depth, dim), k1)


def to_u01(h):
    """Rng::u01: (float)(h >> 8) * 2^-24, exact in float32"""
    return (_u32(h) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def u01(pixel, sample, seed, depth, dim):
    return to_u01(hash_word(pixel, sample, seed, depth, dim))


def random_integer(i, j, u):
    """Rng::randomInteger(i, j) of counter mode given its draw u: i + (int)((float)(j - i + 1) * u) in float32, clamped to j"""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    n = (j - i + 1).astype(np.int32).astype(np.float32)
    r = i + (n * np.asarray(u, np.float32)).astype(np.int32).astype(np.int64)
    return np.minimum(r, j).astype(np.int32)


# ---- generators ---------------------------------------------------------------------------------------------------------------------------------------
def shipped(pixel, sample, seed, depth, dim):
    return hash_word(pixel, sample, seed, depth, dim) >> np.uint32(8)


def _variant(name):
    def gen(pixel, sample, seed, depth, dim):
        pixel, sample, seed = _u32(pixel), _u32(sample), _u32(seed)
        if name == "sample_not_keyed":
            sample = sample * np.uint32(0)
        if name == "seed_not_keyed":
            seed = seed * np.uint32(0)
        if name == "pixel_xor_sample_one_word":
            pixel, sample = pixel ^ sample, sample * np.uint32(0)
        k0, k1, gamma = counter_key(pixel, sample, seed)
        if name == "stride_8":
            w = k0 + (_u32(depth) * np.uint32(8) + _u32(dim) + np.uint32(1)) * gamma
        else:
            w = weyl_word(k0, gamma, depth, dim)
        h = np.broadcast_arrays(w, k1)[0] if name == "no_finaliser" else counter_hash(w, k1)
        return h >> np.uint32(8)
    gen.draws_per_stage = 10 if name == "stride_8" else STAGE_SLOTS
    return gen


shipped.draws_per_stage = STAGE_SLOTS
# the slips of the issue, and the statistic each one is caught by (tests/test_prng_cpu.py requires exactly that one among the failures)
VARIANTS = {
    "no_finaliser": (_variant("no_finaliser"), "cells d0 dims 0,1,2"),  # u from the Weyl word: u0 - 2 u1 + u2 = 0 (mod 1)
    "sample_not_keyed": (_variant("sample_not_keyed"), "1-D samples of one pixel"),
    "seed_not_keyed": (_variant("seed_not_keyed"), "1-D seeds"),
    "pixel_xor_sample_one_word": (_variant("pixel_xor_sample_one_word"), "pairs (pixel, sample) | (sample, pixel)"),
    "stride_8": (_variant("stride_8"), "equal draws within a path"),  # draws 8, 9 of a stage are draws 0, 1 of the next
}


def philox_control(key=20260):
    """An independent generator behind the same signature: fresh Philox words, truncated to 24 bits, for whatever index set is asked for"""
    rng = np.random.Generator(np.random.Philox(key=key))

    def gen(pixel, sample, seed, depth, dim):
        shape = np.broadcast_shapes(*(np.shape(np.atleast_1d(a)) for a in (pixel, sample, seed, depth, dim)))
        return rng.integers(0, 1 << 32, size=shape, dtype=np.uint32) >> np.uint32(8)
    gen.draws_per_stage = STAGE_SLOTS
    return gen


# ---- statistics: each returns (value, distribution) with the distribution a frozen scipy.stats one -------------------------------------------------------
def chi2_cells(cols, bits):
    """Pearson chi-square of the cells the top `bits` bits of each column of 24-bit draws name"""
    idx = np.zeros(cols[0].size, np.int64)
    for c in cols:
        idx = (idx << bits) | (c.ravel().astype(np.int64) >> (24 - bits))
    cells = 1 << (bits * len(cols))
    n = idx.size
    assert n <= 1 << 18 and n / cells >= 16, "at most 2^18 draws per statistic, and cells full enough for the chi-square law"
    counts = np.bincount(idx, minlength=cells)
    e = n / cells
    return float(((counts - e) ** 2).sum() / e), S.chi2(cells - 1)


def correlation(x, y):
    """sqrt(N) r of two columns of draws: standard normal for independent columns (N = 2^18)"""
    x, y = x.ravel().astype(np.float64), y.ravel().astype(np.float64)
    assert x.size <= 1 << 18
    r = np.corrcoef(x, y)[0, 1] if x.std() > 0 and y.std() > 0 else 1.0
    return float(r * np.sqrt(x.size)), S.norm()


def variance_of_means(f, var_f):
    """f: (P, N) values of an integrand with variance var_f; (P - 1) * var(per-pixel mean) / (var_f / N) is chi-square with P - 1 degrees of freedom"""
    P, N = f.shape
    assert P * N <= 1 << 18
    m = f.astype(np.float64).mean(axis=1)
    return float((P - 1) * m.var(ddof=1) / (var_f / N)), S.chi2(P - 1)


def equal_draws_in_paths(draws):
    """draws: (P, D) 24-bit draws, one row per path.  Pairs of equal draws within a row: Poisson with mean P * D (D - 1) / 2 * 2^-24 for independent draws"""
    P, D = draws.shape
    s = np.sort(draws, axis=1)
    # a run of k equal values holds k (k - 1) / 2 pairs; runs longer than 2 are out of the question at these sizes, so adjacent equalities count pairs
    pairs = int((s[:, 1:] == s[:, :-1]).sum())
    return float(pairs), S.poisson(P * D * (D - 1) / 2 / 2.0 ** 24)


W_IMAGE = 1920


def battery(gen):
    """{name: (value, distribution)} over the index sets the tracer uses.  Inputs are fixed: the result is a function of `gen` alone."""
    out = {}
    p16 = np.arange(1 << 16, dtype=np.uint32)
    b = np.arange(1 << 16, dtype=np.uint32)  # the first 1024 blocks of 8 x 8 pixels of a 1920-wide image, block after block
    blocks = ((b >> 6) // (W_IMAGE // 8) * 8 + ((b & 63) >> 3)) * W_IMAGE + (b >> 6) % (W_IMAGE // 8) * 8 + (b & 7)
    out["1-D pixels, row order"] = chi2_cells([gen(p16, 0, 1, 0, 0)], 8)
    out["1-D pixels, 8x8-block order"] = chi2_cells([gen(blocks, 0, 1, 0, 0)], 8)
    out["1-D samples of one pixel"] = chi2_cells([gen(12345, p16, 1, 1, 0)], 8)
    out["1-D seeds"] = chi2_cells([gen(777, 3, p16, 0, 0)], 8)
    # the draws one stage consumes together, 4096 pixels (a 64 x 64 corner of the image) x 64 samples
    px = (np.arange(64, dtype=np.uint32)[:, None] * W_IMAGE + np.arange(64, dtype=np.uint32)[None, :]).ravel()[:, None]
    sm = np.arange(64, dtype=np.uint32)[None, :]
    for d in (0, 1, 2):
        u = [gen(px, sm, 1, d, k) for k in (0, 1, 2)]
        out[f"cells d{d} dims 0,1"] = chi2_cells(u[0:2], 6)
        out[f"cells d{d} dims 1,2"] = chi2_cells(u[1:3], 6)
        out[f"cells d{d} dims 0,1,2"] = chi2_cells(u, 4)
    p18 = np.arange(1 << 18, dtype=np.uint32)
    out["pairs pixel p | p+1"] = chi2_cells([gen(p18, 5, 1, 0, 0), gen(p18 + 1, 5, 1, 0, 0)], 6)
    out["pairs pixel p | p+W"] = chi2_cells([gen(p18, 5, 1, 0, 1), gen(p18 + W_IMAGE, 5, 1, 0, 1)], 6)
    q = (np.arange(1 << 10, dtype=np.uint32) * 1873)[:, None]  # 1024 pixels spread over the image
    s8 = np.arange(1 << 8, dtype=np.uint32)[None, :]
    out["pairs sample s | s+1"] = chi2_cells([gen(q, s8, 1, 1, 0), gen(q, s8 + 1, 1, 1, 0)], 6)
    out["pairs sample s | s+64"] = chi2_cells([gen(q, s8, 1, 1, 1), gen(q, s8 + 64, 1, 1, 1)], 6)
    out["pairs sample s | s+1024 (a sample base apart)"] = chi2_cells([gen(q, s8, 1, 0, 0), gen(q, s8 + 1024, 1, 0, 0)], 6)
    pd_, sd, dd = px[:, :, None], np.arange(4, dtype=np.uint32)[None, :, None], np.arange(16, dtype=np.uint32)[None, None, :]
    out["pairs depth d | d+1, equal dim"] = chi2_cells([gen(pd_, sd, 1, dd, 2), gen(pd_, sd, 1, dd + 1, 2)], 6)
    out["pairs seed | seed+1"] = chi2_cells([gen(px, 0, sm + 1, 0, 0), gen(px, 0, sm + 2, 0, 0)], 6)
    a = np.arange(512, dtype=np.uint32)
    out["pairs (pixel, sample) | (sample, pixel)"] = chi2_cells([gen(a[:, None], a[None, :] + 512, 1, 0, 0), gen(a[None, :] + 512, a[:, None], 1, 0, 0)], 6)
    # serial correlation over the samples of a pixel, pooled over 256 pixels
    r = (np.arange(1 << 8, dtype=np.uint32) * 7919)[:, None]
    s10 = np.arange(1 << 10, dtype=np.uint32)[None, :]
    seq = gen(r, s10, 1, 0, 0)
    out["lag-1 correlation over samples"] = correlation(seq[:, :-1], seq[:, 1:])
    out["lag-2 correlation over samples"] = correlation(seq[:, :-2], seq[:, 2:])
    # Monte-Carlo variance of two integrands over the 1024 samples of each of 256 pixels (the first 256 of a row: what a fold of pixel and sample into one
    # word would give one and the same sample set)
    r0 = np.arange(1 << 8, dtype=np.uint32)[:, None]
    u1 = gen(r0, s10, 1, 1, 0).astype(np.float64) * 2.0 ** -24
    u2 = gen(r0, s10, 1, 1, 1).astype(np.float64) * 2.0 ** -24
    out["variance of means of u1*u2"] = variance_of_means(u1 * u2, 7.0 / 144.0)
    out["variance of means of [u1+u2<1]"] = variance_of_means((u1 + u2 < 1.0).astype(np.float64), 0.25)
    # every draw a path can make: 17 depths x the draws of a stage, 960 paths
    n = gen.draws_per_stage
    pp = (np.arange(960, dtype=np.uint32) * 2161)[:, None, None]
    path = gen(pp, 9, 1, np.arange(17, dtype=np.uint32)[None, :, None], np.arange(n, dtype=np.uint32)[None, None, :]).reshape(960, 17 * n)
    out["equal draws within a path"] = equal_draws_in_paths(path)
    return out


FAMILY_LEVEL = 1e-3


def judge(results, level=FAMILY_LEVEL):
    """{name: (value, lo, hi, inside)}: two-sided quantiles of each statistic's own distribution at level / len(results) each (Bonferroni: the chance that an
    ideal generator leaves any interval is at most `level`)"""
    each = level / len(results)
    out = {}
    for name, (v, dist) in results.items():
        lo, hi = dist.ppf(each / 2), dist.isf(each / 2)
        out[name] = (v, float(lo), float(hi), bool(lo <= v <= hi))
    return out
