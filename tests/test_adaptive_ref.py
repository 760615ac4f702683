"""The bookkeeping of adaptive sampling on synthetic noise, through its numpy restatement (tests/adaptive_ref.py): no renderer, no GPU.

The noise model: grey lognormal samples of mean 0.5 on 64 x 64, sigma 0 in the left quarter and 2 (x / W)^3 to the right of it; min = round = 16, max =
256, threshold 0.02.  Measured with this generator, seeds 1-3: the zero-variance quarter holds exactly 16 samples, samples_total is 0.551-0.560 of the
uniform budget, 29-31 of the 64 blocks reach max.  Equal budget, pooled over eight seeds and the quarter of blocks with the largest sigma: adaptive /
uniform RMSE 0.806 (uniform 144 spp against 256: an oracle that knew the variances would reach sqrt(144 / 256) = 0.75), EXPERIMENTS.md."""
import numpy as np
import pytest

import adaptive_ref as R

W = H = 64
MIN, ROUND, MAX, THRESHOLD, SIGMA_MAX = 16, 16, 256, 0.02, 2.0
SIGMA = R.cubic_sigma(W, H, SIGMA_MAX)


def adaptive_run(seed, threshold=THRESHOLD, after_round=None):
    st = R.State(W, H, threshold, MIN, ROUND, MAX)
    st.run(R.LognormalNoise(SIGMA, MAX, seed), after_round=after_round)
    return st


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_noise_model_run(seed):
    st = adaptive_run(seed)
    counts = st.counts.reshape(H, W)
    assert (counts[:, : W // 4] == MIN).all()  # zero variance: E_b == 0 < threshold at the first judgement
    share = st.last["samples_total"] / (W * H * MAX)
    at_max = int((st.last["block_counts"] == MAX).sum())
    print(f"seed {seed}: share {share:.4f}, blocks at max {at_max}, rounds {st.rounds}")
    assert 0.5 < share < 0.6  # the issue's own runs of this model: 0.55-0.56
    assert 16 <= at_max <= 48  # the left quarter never, the quarter with sigma > 0.8 always
    assert (counts[:, -8:] == MAX).all()
    assert st.last["active_blocks"] == 0 and st.spp == MAX


def test_invariants_after_every_round():
    seen = {"rounds": 0}
    prev = {}

    def check(st):
        last, bc = st.last, st.last["block_counts"]
        per_block = st.counts[np.maximum(R.lanes(W, H), 0)]
        assert (per_block == bc[:, None]).all()  # constant per block
        assert (st.counts % 2 == 0).all() and st.counts.min() >= MIN and st.counts.max() <= MAX
        assert int(st.counts.astype(np.uint64).sum()) == last["samples_total"]
        assert last["max_count"] == st.spp == int(st.counts.max())
        if prev:  # blocks that were inactive keep the bits of A and B
            idle = ~prev["flags"][R.block_of_pixel(W, H)]
            assert idle.any()
            assert np.array_equal(st.A[idle].view(np.uint32), prev["A"][idle].view(np.uint32))
            assert np.array_equal(st.B[idle].view(np.uint32), prev["B"][idle].view(np.uint32))
            assert (st.counts[idle] == prev["counts"][idle]).all()
        prev.update(flags=last["flags"].copy(), A=st.A.copy(), B=st.B.copy(), counts=st.counts.copy())
        seen["rounds"] += 1

    st = adaptive_run(1, after_round=check)
    assert seen["rounds"] == st.rounds == MAX // ROUND


def test_threshold_zero_is_uniform_sampling():
    st = adaptive_run(2, threshold=0.0)
    assert (st.counts == MAX).all() and st.rounds == MAX // ROUND
    noise = R.LognormalNoise(SIGMA, MAX, 2)
    # the same samples in the same halves: A holds the first half of every round, B the second, each added round after round in float32
    A = np.zeros(W * H, np.float32)
    for first in range(0, MAX, ROUND):
        A = (A + noise(None, first, ROUND // 2)[:, 0]).astype(np.float32)
    assert np.array_equal(st.A[:, 0], A)
    assert np.array_equal(st.last["accum"][:, :3], (st.A[:, :3] + st.B[:, :3]).astype(np.float32))  # n == S everywhere: the bits of A + B


def test_zero_variance_blocks_stop_at_min_samples_with_zero_error():
    st = R.State(W, H, 1e-30, MIN, ROUND, MAX)  # the smallest threshold still stops them: E_b is exactly 0
    st.run(R.LognormalNoise(SIGMA, MAX, 3))
    quarter = (np.arange(W * H) % W) < W // 4
    blocks = np.unique(R.block_of_pixel(W, H)[quarter])
    assert (st.last["block_error"][blocks] == 0).all() and (st.last["block_error64"][blocks] == 0).all()
    assert (st.counts[quarter] == MIN).all() and (st.counts[~quarter] == MAX).all()


def test_equal_budget_gain():
    """adaptive against a uniform run of the same total budget (rounded to a multiple of 16), RMSE against the true mean pooled over the quarter of
    blocks with the largest sigma and over eight seeds.  Gate: strictly below; expected near sqrt(uniform spp / max) = 0.75."""
    hard = (np.arange(W * H) % W) >= 3 * W // 4
    sq = {"adaptive": 0.0, "uniform": 0.0}
    spps = []
    for seed in range(1, 9):
        st = adaptive_run(seed)
        spp = int(round(st.last["samples_total"] / (W * H) / 16.0)) * 16
        spps.append(spp)
        noise = R.LognormalNoise(SIGMA, MAX, seed)
        uniform = noise(None, 0, spp)[:, 0].astype(np.float64) / spp
        mean = (st.A[:, 0].astype(np.float64) + st.B[:, 0]) / st.counts
        sq["adaptive"] += float(((mean[hard] - 0.5) ** 2).sum())
        sq["uniform"] += float(((uniform[hard] - 0.5) ** 2).sum())
    ratio = (sq["adaptive"] / sq["uniform"]) ** 0.5
    print(f"equal budget: uniform spp {spps}, adaptive / uniform RMSE {ratio:.3f}")
    assert ratio < 1.0


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (8, 8), (9, 9), (70, 45)])
def test_edge_shapes(shape):
    W_, H_ = shape
    nb = R.block_sizes(W_, H_)
    bx, by = R.blocks_of(W_, H_)
    assert nb.sum() == W_ * H_ and len(nb) == bx * by
    if shape == (9, 9):
        assert list(nb) == [64, 8, 8, 1]  # four blocks, three partial
    ln = R.lanes(W_, H_)
    inside = ln[ln >= 0]
    assert sorted(inside) == list(range(W_ * H_))  # every pixel is one lane of one block
    assert (R.block_of_pixel(W_, H_)[np.maximum(ln, 0)] == np.arange(bx * by)[:, None])[ln >= 0].all()
    assert list(R.pixel_list(W_, H_, np.ones(bx * by, bool))) == list(inside)
    A, B, counts, _ = R.planted(W_, H_, 5, with_specials=False)
    if bx * by > 1:
        counts[R.block_of_pixel(W_, H_) == 0] = 0
    ev = R.evaluate(A, B, counts, W_, H_, 0.1, 4, 12)
    assert np.allclose(ev["block_error"], ev["block_error64"], rtol=1e-5, atol=1e-9)  # what the order of a 64-term float32 sum costs
    e = ev["error"]
    for b in range(bx * by):  # the block mean over n_b pixels, not over 64
        assert ev["block_error64"][b] == pytest.approx(e[R.block_of_pixel(W_, H_) == b].astype(np.float64).mean(), rel=1e-12, abs=1e-300)
    S = ev["spp"]
    assert (ev["accum"][counts == 0] == 0).all() and (ev["error"][counts == 0] == 0).all()
    full = counts == S
    assert np.array_equal(ev["accum"][full, :3], (A[full, :3] + B[full, :3]).astype(np.float32))
    assert (ev["accum"][:, 3] == 0).all()
    assert (ev["flags"] == ((ev["block_counts"] < 4) | ((ev["block_counts"] < 12) & ~(ev["block_error"] < np.float32(0.1))))).all()


def test_planted_nan_and_inf():
    A, B, counts, special = R.planted(64, 64, 9)
    ev = R.evaluate(A, B, counts, 64, 64, 10.0, 2, 12)  # a threshold every finite block is under
    assert ev["nonfinite"] == 2 and (ev["error"][special] == 0).all()
    assert np.isfinite(ev["block_error"]).all() and np.isfinite(ev["error"]).all()
    stopped = ev["block_counts"] >= 2
    assert not ev["flags"][stopped].any()  # the blocks with the NaN and the Inf stop like their neighbours
    assert ev["flags"][ev["block_counts"] == 0].all()
    clean_A, clean_B = A.copy(), B.copy()
    clean_A[special[0], 1], clean_B[special[1], 0] = 0.5, 0.5
    clean = R.evaluate(clean_A, clean_B, counts, 64, 64, 10.0, 2, 12)
    others = np.ones(64 * 64, bool)
    others[special] = False
    assert np.array_equal(ev["error"][others], clean["error"][others]) and clean["nonfinite"] == 0
