"""A numpy restatement of the bookkeeping of adaptive sampling (include/ptamd.h, "adaptive sampling"): the active set, the evaluation and the published
accumulator in float32 with the stated operation order, and a round driver over a samples(pixel_mask, first_index, count) callback, so that the whole
loop runs on synthetic noise with no renderer.  The block sum is done twice: in float32 in the order of the kernel's butterfly, and in float64, which
bounds what the order of the reduction costs."""
import numpy as np

F = np.float32
DEFAULT_MIN, DEFAULT_ROUND, DEFAULT_MAX = 64, 64, 1024


def blocks_of(W, H):
    return (W + 7) // 8, (H + 7) // 8


def block_of_pixel(W, H):
    """(H * W,) index of the 8 x 8 block of every pixel, blocks in row-major order"""
    bx, _ = blocks_of(W, H)
    y, x = np.divmod(np.arange(W * H), W)
    return (y // 8) * bx + x // 8


def block_sizes(W, H):
    """n_b: pixels of every block (blocks on the right and bottom edges hold fewer than 64)"""
    return np.bincount(block_of_pixel(W, H), minlength=np.prod(blocks_of(W, H)))


def lanes(W, H):
    """(blocks, 64) pixel index of lane l of every block's wave -- pixel (8 bx + l % 8, 8 by + l // 8) -- or -1 outside the image"""
    bx, by = blocks_of(W, H)
    b = np.arange(bx * by)[:, None]
    l = np.arange(64)[None, :]
    x, y = (b % bx) * 8 + l % 8, (b // bx) * 8 + l // 8
    return np.where((x < W) & (y < H), y * W + x, -1)


def block_rects(W, H, active):
    """the (x0, y0, x1, y1) rects of the active blocks in block-row-major order: what a round hands to the body of pt_set_tiles"""
    bx, _ = blocks_of(W, H)
    return [((b % bx) * 8, (b // bx) * 8, min((b % bx) * 8 + 8, W), min((b // bx) * 8 + 8, H)) for b in np.flatnonzero(active)]


def pixel_list(W, H, active):
    """the owned pixels of a round in list order: block after block, each row-major"""
    ln = lanes(W, H)[np.asarray(active, bool)].ravel()
    return ln[ln >= 0]


def active_set(block_counts, block_error, threshold, min_samples, max_samples):
    """step 2: a pure function of the state and the parameters; the compare is strict, so threshold == 0 never stops a block by its error"""
    c = np.asarray(block_counts)
    return (c < min_samples) | ((c < max_samples) & ~(np.asarray(block_error, F) < F(threshold)))


def pixel_error(A, B, counts):
    """step 4 per pixel: (e, nonfinite mask) in float32 and in the stated order; n == 0 gives 0, a non-finite e gives 0 and is flagged"""
    A, B = np.asarray(A, F)[:, :3], np.asarray(B, F)[:, :3]
    n = np.asarray(counts).astype(F)
    with np.errstate(all="ignore"):
        hn = (n / F(2))[:, None]
        mA, mB = A / hn, B / hn
        m = (A + B) / n[:, None]
        num = np.abs(mA[:, 0] - mB[:, 0]) + np.abs(mA[:, 1] - mB[:, 1]) + np.abs(mA[:, 2] - mB[:, 2])
        msum = m[:, 0] + m[:, 1] + m[:, 2]
        den = F(2) * np.sqrt(np.where(msum > 0, msum, F(0)).astype(F) + F(1e-3))  # max(x, 0) as fmaxf: a NaN gives 0
        e = (num / den).astype(F)
    sampled = np.asarray(counts) > 0
    bad = sampled & ~np.isfinite(e)
    return np.where(sampled & ~bad, e, F(0)).astype(F), bad


def block_error(e, W, H):
    """(E_b in float32 with the butterfly's order of additions, E_b with the sum in float64)"""
    ln = lanes(W, H)
    v = np.where(ln >= 0, np.asarray(e, F)[np.maximum(ln, 0)], F(0)).astype(F)
    exact = v.astype(np.float64).sum(axis=1)
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, idx ^ m]).astype(F)
    nb = block_sizes(W, H)
    return (v[:, 0] / nb.astype(F)).astype(F), exact / nb


def publish(A, B, counts, S):
    """step 5: (A + B) * (S / n) in float32, the scale exactly 1 where n == S, 0 where n == 0; .w = 0"""
    A, B = np.asarray(A, F), np.asarray(B, F)
    n = np.asarray(counts)
    with np.errstate(all="ignore"):
        scale = np.where(n == S, F(1), F(S) / n.astype(F)).astype(F)
        out = ((A[:, :3] + B[:, :3]).astype(F) * scale[:, None]).astype(F)
    out[n == 0] = 0
    return np.concatenate([out, np.zeros((len(out), 1), F)], axis=1)


def evaluate(A, B, counts, W, H, threshold, min_samples, max_samples):
    """steps 4 and 5 on a state as it stands (pt_write_adaptive; the end of a round once the counts are up to date)"""
    counts = np.asarray(counts, np.uint32)
    e, bad = pixel_error(A, B, counts)
    Eb, Eb64 = block_error(e, W, H)
    block_counts = counts[lanes(W, H)[:, 0]]
    S = int(counts.max()) if counts.size else 0
    flags = active_set(block_counts, Eb, threshold, min_samples, max_samples)
    return {"error": e, "block_error": Eb, "block_error64": Eb64, "block_counts": block_counts, "flags": flags, "nonfinite": int(bad.sum()),
            "active_blocks": int(flags.sum()), "samples_total": int(counts.astype(np.uint64).sum()), "min_count": int(block_counts.min()), "max_count": S,
            "max_block_error": float(Eb.max()), "accum": publish(A, B, counts, S), "spp": S}


class State:
    """the adaptive state of a W x H image with no samples: halves, counts, the flags of step 2 (every block: a count of 0 is below min_samples)"""

    def __init__(self, W, H, threshold=0.0, min_samples=DEFAULT_MIN, round_samples=DEFAULT_ROUND, max_samples=DEFAULT_MAX):
        assert min_samples % 2 == 0 and round_samples % 2 == 0 and max_samples % 2 == 0 and 2 <= min_samples <= max_samples and round_samples >= 2
        self.W, self.H = W, H
        self.threshold, self.min_samples, self.round_samples, self.max_samples = threshold, min_samples, round_samples, max_samples
        self.A, self.B = np.zeros((W * H, 4), F), np.zeros((W * H, 4), F)
        self.counts = np.zeros(W * H, np.uint32)
        self.spp, self.rounds = 0, 0
        self.last = evaluate(self.A, self.B, self.counts, W, H, threshold, min_samples, max_samples)

    @property
    def flags(self):
        return self.last["flags"]

    def round(self, samples):
        """one round; samples(mask, first, count) -> (W * H, 3) sums of `count` samples with indices first .. first + count - 1 (rows outside the mask
        are ignored).  False when there was nothing to do."""
        S = self.spp
        active = self.flags
        if S >= self.max_samples or not active.any():
            return False
        h = min(self.min_samples if S == 0 else self.round_samples, self.max_samples - S) // 2
        mask = active[block_of_pixel(self.W, self.H)]
        for half, first in ((self.A, S), (self.B, S + h)):
            half[mask, :3] = (half[mask, :3] + np.asarray(samples(mask, first, h), F)[mask]).astype(F)
        self.counts[mask] += np.uint32(2 * h)
        self.spp = S + 2 * h
        self.rounds += 1
        self.last = evaluate(self.A, self.B, self.counts, self.W, self.H, self.threshold, self.min_samples, self.max_samples)
        assert self.last["spp"] == self.spp  # the most-sampled pixel always holds S
        return True

    def run(self, samples, rounds=0, after_round=None):
        r = 0
        while (rounds == 0 or r < rounds) and self.round(samples):
            r += 1
            if after_round:
                after_round(self)
        return self.last


class LognormalNoise:
    """The noise model of tests/test_adaptive_ref.py: grey lognormal samples of mean `mean`, per-pixel sigma, drawn per (pixel, sample index) -- the
    same index gives the same sample whoever asks, so a uniform and an adaptive run share their streams."""

    def __init__(self, sigma, max_samples, seed, mean=0.5):
        self.sigma = np.asarray(sigma, np.float64).ravel()
        z = np.random.default_rng(seed).standard_normal((len(self.sigma), max_samples))
        mu = np.log(mean) - 0.5 * self.sigma ** 2
        self.table = np.exp(mu[:, None] + self.sigma[:, None] * z)  # float64; a sum of a round's samples is rounded once, as a render's fold is not -- irrelevant here

    def __call__(self, mask, first, count):
        s = self.table[:, first:first + count].sum(axis=1).astype(F)
        return np.repeat(s[:, None], 3, axis=1)


def cubic_sigma(W, H, sigma_max):
    """sigma_max (x / W)^3 per column, and 0 in the left quarter"""
    x = np.arange(W, dtype=np.float64)
    return np.tile(np.where(x < W / 4, 0.0, sigma_max * (x / W) ** 3), H)


def planted(W_, H_, seed, with_specials=True):
    """a random state: halves of a few units, counts of several even values over the blocks, one n == 0 block, one NaN and one Inf where there is room"""
    rng = np.random.default_rng(seed)
    n, nb = W_ * H_, int(np.prod(blocks_of(W_, H_)))
    bc = rng.choice([2, 4, 8, 12], nb).astype(np.uint32)
    if nb > 1 and with_specials:
        bc[rng.integers(nb)] = 0
    counts = bc[block_of_pixel(W_, H_)]
    A = np.zeros((n, 4), np.float32)
    B = np.zeros((n, 4), np.float32)
    A[:, :3] = rng.uniform(0.0, 2.0, (n, 3)) * counts[:, None] / 2
    B[:, :3] = rng.uniform(0.0, 2.0, (n, 3)) * counts[:, None] / 2
    special = []
    if with_specials and n >= 15:
        live = np.flatnonzero(counts > 0)
        special = list(rng.choice(live, 2, replace=False))
        A[special[0], 1] = np.nan
        B[special[1], 0] = np.inf
    return A, B, counts, special
