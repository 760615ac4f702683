"""The numpy restatement of pt_temporal_accumulate (tests/temporal_ref.py) on the CPU: conditions on the synthetic inputs, so that the device
tests (tests/test_gpu_temporal.py) cannot pass on an empty branch, and properties of the arithmetic itself."""
import numpy as np
import pytest

import temporal_ref as T


@pytest.mark.parametrize("width,height", T.SIZES)
def test_share_of_pixels_that_find_their_history(width, height):
    """Wsum >= 1e-12 for most pixels of a small pan, for a good part but not all of a large move, for none when the camera turned away."""
    share = {}
    for pose in ("pan", "big", "turn"):
        wsum = T.run_case(T.make_case(pose, width, height), np.float64)[2]
        share[pose] = float((wsum >= 1e-12).mean())
    print(f"{width}x{height}: share of pixels with a history {share}")
    assert share["pan"] >= 0.7
    assert 0.2 <= share["big"] <= 0.9
    assert share["turn"] == 0.0


@pytest.mark.parametrize("width,height", T.SIZES)
def test_same_camera_same_guides_is_the_plain_blend(width, height):
    """every N_h >= 1, history guides equal to the current ones, camera unchanged: d_out = h + (d - h) / min(N_h + 1, max) with h = d_h(p)"""
    case = T.make_case("history", width, height, all_counted=True, same_guides=True)
    out, nd, wsum = T.run_case(case, np.float64)
    d = T.R.prepare(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], np.float64)[0]
    h, n_h = case["hist_cn"][..., :3].astype(np.float64), case["hist_cn"][..., 3].astype(np.float64)
    n_out = np.minimum(n_h + 1.0, T.MAX_HISTORY)
    want = h + (d - h) / n_out[..., None]
    # round-off: the history's guides are stored as float32 (2^-24 relative on z is e_z = 1.2e-6, on n.n_h e_n = 64 x 1.2e-7), so a weight is
    # 1 - O(1e-5), a count of up to 40 is good to 1e-3 and the blend to 1e-4 of its value
    assert np.allclose(wsum, 1.0, rtol=0, atol=1e-4)
    assert np.allclose(out[..., 3], n_out, rtol=0, atol=1e-3)
    assert np.allclose(out[..., :3], want, rtol=1e-4, atol=1e-6 * float(np.abs(want).max()))


def test_constant_input_gives_the_running_mean_until_max_history():
    width, height, max_history = 16, 16, 5
    case = T.make_case("history", width, height, same_guides=True)
    frames = [T.make_case("history", width, height, seed=100 + k)["accum"] for k in range(8)]
    hist, mean = None, None
    for k, accum in enumerate(frames):
        out, nd, _ = T.accumulate(accum, case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], case["camera"], hist,
                                  max_history=max_history)
        d = T.R.prepare(accum, case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], np.float64)[0]
        count = min(k + 1, max_history)
        mean = d if mean is None else mean + (d - mean) / count  # the running mean, exponential once the count is capped
        assert np.allclose(out[..., 3], count, rtol=0, atol=1e-6), k
        assert np.allclose(out[..., :3], mean, rtol=1e-7, atol=1e-7 * float(np.abs(mean).max())), k
        hist = (out, nd, case["camera"])
    # and with the SAME frame every time the mean is that frame
    hist = None
    for k in range(4):
        out, nd, _ = T.accumulate(frames[0], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], case["camera"], hist)
        hist = (out, nd, case["camera"])
    d0 = T.R.prepare(frames[0], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], np.float64)[0]
    assert np.allclose(out[..., :3], d0, rtol=1e-9, atol=1e-9 * float(d0.max())) and np.allclose(out[..., 3], 4.0, atol=1e-6)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [-7, 3, 20])
def test_scaling_all_colours_by_a_power_of_two_scales_the_output_exactly(dtype, k):
    case = T.make_case("pan", 70, 45)
    out, nd, wsum = T.run_case(case, dtype)
    scaled = dict(case)
    scaled["accum"] = case["accum"] * np.float32(2.0 ** k)
    scaled["hist_cn"] = case["hist_cn"].copy()
    scaled["hist_cn"][..., :3] *= np.float32(2.0 ** k)
    out2, nd2, wsum2 = T.run_case(scaled, dtype)
    assert np.array_equal(out2[..., :3], out[..., :3] * dtype(2.0 ** k))
    assert np.array_equal(out2[..., 3], out[..., 3]) and np.array_equal(nd2, nd) and np.array_equal(wsum2, wsum)


def test_no_history_is_the_current_frame():
    case = T.make_case("pan", 70, 45)
    out, nd, wsum = T.run_case(case, np.float64, history=False)
    d, _, n, z = T.R.prepare(case["accum"], case["spp"], case["albedo_hits"], case["normal_depth"], case["gspp"], np.float64)
    assert np.array_equal(out[..., :3], d) and np.all(out[..., 3] == 1.0) and not wsum.any()
    assert np.array_equal(nd[..., :3], n) and np.array_equal(nd[..., 3], z)
    turn = T.run_case(T.make_case("turn", 70, 45), np.float64)
    d = T.R.prepare(*(T.make_case("turn", 70, 45)[k] for k in ("accum", "spp", "albedo_hits", "normal_depth", "gspp")), np.float64)[0]
    assert np.array_equal(turn[0][..., :3], d) and np.all(turn[0][..., 3] == 1.0)


def test_float32_restatement_stays_in_float32_and_close():
    case = T.make_case("big", 70, 45)
    ref64, b = T.bound(case)
    out32 = T.run_case(case, np.float32)[0]
    assert out32.dtype == np.float32
    diff = float(np.abs(out32.astype(np.float64) - ref64).max())
    print(f"float32 against float64: {diff:.3e}, bound {b:.3e}")
    assert 0 < diff < 1e-2
