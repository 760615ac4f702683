"""numpy restatement of the temporal luminance variance (pt_set_temporal_variance; include/ptamd.h, "temporal variance"): the plane that
pt_temporal_accumulate keeps beside the history, and the variance-guided a-trous filter of PT_DENOISE_INPUT_TEMPORAL_VARIANCE.  Parameterised by
dtype like temporal_ref and denoise_ref, on which it is built: float64 is the reference the device is held against, float32 measures what single
precision costs the same arithmetic on the same input."""
import numpy as np

import denoise_ref as R
import temporal_ref as T

from denoise_ref import FULL_HISTORY, RELATIVE_FLOOR, SIGMA_VARIANCE, history_weight  # noqa: F401 (the defaults of pt_variance_params, and s(p))


def accumulate(*args, **kw):
    """One pt_temporal_accumulate with the variance mode on: temporal_ref.accumulate, whose history carries the variance plane as a fourth element
    and whose third result is the new plane"""
    return T.accumulate(*args, variance=True, **kw)


def initial_variance(variance, count):
    """V_0 = v / N, the variance of the history's MEAN (N below 1 taken as 1)"""
    return variance / np.maximum(count, count.dtype.type(1))


def atrous(d, V, count, n, z, iterations, k_normal=0.0, sigma_depth=0.0, sigma_lum=0.0, sigma_variance=0.0, relative_floor=0.0, full_history=0.0):
    """denoise_ref.atrous with its variance term on.  Returns (d (H, W, 3), V (H, W)) after `iterations` passes."""
    return R.atrous(d, n, z, iterations, k_normal, sigma_depth, sigma_lum, (V, count, sigma_variance, relative_floor, full_history))


def denoise_hdr(hist_cn, variance, albedo_hits, normal_depth, gspp, iterations, dtype=np.float64, **params):
    """the PT_DENOISE_HDR output (H, W, 3) of PT_DENOISE_INPUT_TEMPORAL_VARIANCE: the history's d filtered under the current guides, times the
    current albedo"""
    dt = dtype
    hist_cn, variance = np.asarray(hist_cn).astype(dt), np.asarray(variance).astype(dt)
    H, W = variance.shape
    _, a, n, z = R.prepare(np.zeros((H, W, 4), dt), 1, albedo_hits, normal_depth, gspp, dt)
    d, count = hist_cn[..., :3], hist_cn[..., 3]
    if iterations == 0:
        return d * a
    return atrous(d, initial_variance(variance, count), count, n, z, iterations, **params)[0] * a
