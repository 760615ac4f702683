"""ctypes binding of the HIP C-ABI (include/ptamd.h).  There is no CPU fallback: if libptamd.so
is missing or no HIP device is present, construction fails loudly."""
import ctypes as C
import os
import numpy as np
from . import layout as L

_HERE = os.path.dirname(os.path.abspath(__file__))
DEVICE_LIB_PATH = os.environ.get("PTAMD_LIB") or os.path.join(_HERE, "..", "csrc", "libptamd.so")  # PTAMD_LIB: tuning builds

RNG_COUNTER, RNG_LFSR113_PARITY = 0, 1
TEX_RGBA32F, TEX_BGRA8_UNORM = 0, 1
FLAG_ROWMAJOR_PIXELS = 1
FLAG_NO_BAKED_INSTANCES = 2  # every instance stays two-level
FLAG_TWO_LEVEL_ONLY = 4  # only single-leaf instances are copied to world space
FLAG_NO_PACKETS = 8  # primary rays through the per-ray kernel too
FLAG_PACKET_INTERSECT = 16  # the pt_intersect hook uses the packet kernel where the scene allows it
FLAG_INTEGRATOR_MIS = 32  # neeMisShading instead of neeIsShading
FLAG_COMPARE_SHADING = 64  # the reference's COMPARE_SHADING build: MIS on the left half of the image, IS on the right, same view
FLAG_SOLID_ANGLE_LIGHTS = 128  # NEE picks lights by weightedRandomPointOnLight
FLAG_MATERIAL_BINS = 512  # k_shade walks its tiles in material order (scenes with several material types; measured slower: opt-in)
FLAG_PARKED_INSTANCES = 4096  # entered instances always take the general (parked) route; default: translation + uniform scale is walked through entry nodes
FLAG_TEAM_INTERSECT = 8192  # the pt_intersect hook runs the team kernel (four lanes per ray) where the scene allows it
FLAG_QUEUE_PRIMARY_RAYS = 256  # k_gen writes the primary rays even where the packet kernel could regenerate them


class Config(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_active_rays", C.c_uint32),
                ("max_bounces", C.c_uint32), ("rng_mode", C.c_uint32), ("seed", C.c_uint32), ("device", C.c_int32),
                ("flags", C.c_uint32), ("samples_in_flight", C.c_uint32), ("ext_queue_fraction", C.c_float), ("shadow_queue_fraction", C.c_float)]


class Rect(C.Structure):
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("rays_extension", C.c_uint64), ("rays_shadow", C.c_uint64), ("rays_generated", C.c_uint64),
                ("shade_hits", C.c_uint64), ("deposits", C.c_uint64), ("samples", C.c_uint64),
                ("ms_last_render", C.c_double), ("ms_intersect", C.c_double), ("ms_shade", C.c_double),
                ("ms_shadow", C.c_double), ("ms_gen", C.c_double), ("packet_launches", C.c_uint64), ("ms_packet", C.c_double),
                ("deposits_shadow", C.c_uint64), ("gen_launches", C.c_uint64), ("bundle_launches", C.c_uint64),
                ("stack_need", C.c_uint32), ("folded_instances", C.c_uint32), ("team_launches", C.c_uint64),
                ("entered_instances", C.c_uint32), ("batch_samples", C.c_uint32), ("first_pass_ext_ratio", C.c_float), ("first_pass_shadow_ratio", C.c_float), ("probe_batches", C.c_uint32), ("general_route", C.c_uint32)]


class RaysSoA(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax")]


class HitsSoA(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("t", "u", "v", "prim", "inst")]


class ShadeBatchIO(C.Structure):
    _fields_ = ([("n", C.c_uint32)]
                + [(n, C.c_void_p) for n in ("ox", "oy", "oz", "dx", "dy", "dz", "thr_r", "thr_g", "thr_b", "pixel",
                                             "flags", "bounce", "t", "u", "v", "prim", "inst")]
                + [("sample", C.c_uint32)]
                + [(n, C.c_void_p) for n in ("radiance", "out_alive", "nox", "noy", "noz", "ndx", "ndy", "ndz",
                                             "nthr_r", "nthr_g", "nthr_b", "nflags", "shadow_alive", "sox", "soy",
                                             "soz", "sdx", "sdy", "sdz", "slen", "sc_r", "sc_g", "sc_b",
                                             "in_pdf", "npdf")])


DENOISE_TONEMAPPED, DENOISE_HDR = 0, 1
GUIDE_SKY_DEPTH = 1e6
GUIDE_CHAIN_MAX = 4  # PT_GUIDE_CHAIN_MAX
NO_PREVIOUS_TRIANGLE = 0xFFFFFFFF  # PT_NO_PREVIOUS_TRIANGLE


class DenoiseParams(C.Structure):
    """pt_denoise_params (32 bytes); a filter parameter of 0 selects the default documented in include/ptamd.h"""
    _fields_ = [("iterations", C.c_uint32), ("output", C.c_uint32), ("k_normal", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_lum", C.c_float), ("input", C.c_uint32), ("_reserved", C.c_uint32 * 2)]


DENOISE_INPUT_ACCUM, DENOISE_INPUT_TEMPORAL = 0, 1


class TemporalParams(C.Structure):
    """pt_temporal_params (32 bytes); a parameter of 0 selects the default documented in include/ptamd.h"""
    _fields_ = [("max_history", C.c_uint32), ("k_normal", C.c_float), ("sigma_depth", C.c_float), ("_reserved", C.c_uint32 * 5)]


DENOISE_INPUT_TEMPORAL_VARIANCE = 2


class VarianceParams(C.Structure):
    """pt_variance_params (32 bytes); a parameter of 0 selects the default documented in include/ptamd.h"""
    _fields_ = [("sigma_variance", C.c_float), ("relative_floor", C.c_float), ("full_history", C.c_float), ("_reserved", C.c_uint32 * 5)]


class ResponseParams(C.Structure):
    """pt_response_params (32 bytes); a parameter of 0 selects the default documented in include/ptamd.h"""
    _fields_ = [("fast_history", C.c_uint32), ("sigma_response", C.c_float), ("relative_floor", C.c_float), ("_reserved", C.c_uint32 * 5)]


class FireflyParams(C.Structure):
    """pt_firefly_params (32 bytes); a parameter of 0 selects the default documented in include/ptamd.h"""
    _fields_ = [("rank", C.c_uint32), ("scale", C.c_float), ("_reserved", C.c_uint32 * 6)]


FIREFLY_RADIUS, FIREFLY_MAX_RANK = 2, 4  # PT_FIREFLY_RADIUS, PT_FIREFLY_MAX_RANK


class AdaptiveParams(C.Structure):
    """pt_adaptive_params (32 bytes); a sample count of 0 selects the default documented in include/ptamd.h, threshold 0 never stops a block by its error"""
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_uint32), ("round_samples", C.c_uint32), ("max_samples", C.c_uint32), ("_reserved", C.c_uint32 * 4)]


class AdaptiveStats(C.Structure):
    """pt_adaptive_stats (56 bytes)"""
    _fields_ = [("rounds", C.c_uint32), ("blocks", C.c_uint32), ("active_blocks", C.c_uint32), ("nonfinite", C.c_uint32), ("min_count", C.c_uint32),
                ("max_count", C.c_uint32), ("samples_total", C.c_uint64), ("max_block_error", C.c_float), ("_reserved", C.c_uint32 * 5)]


EXPORTS = ["pt_create", "pt_destroy", "pt_last_error", "pt_set_stream", "pt_upload_static", "pt_upload_static_async", "pt_upload_dynamic",
           "pt_upload_dynamic_async", "pt_frame_tick", "pt_update_geometry", "pt_refit_vertices",
           "pt_upload_texture_array", "pt_set_camera", "pt_set_tiles", "pt_set_accum_buffer", "pt_clear", "pt_render",
           "pt_synchronize", "pt_resolve", "pt_resolve_device", "pt_resolve_device_ptr", "pt_read_accum", "pt_write_accum", "pt_accum_device_ptr",
           "pt_samples_per_pixel", "pt_render_guides", "pt_guide_samples", "pt_read_guides", "pt_write_guides", "pt_guides_device_ptr",
           "pt_set_guide_chain", "pt_guide_chain", "pt_debug_guide_chain_terminals", "pt_debug_read_guide_chain_terminals",
           "pt_set_guide_reflections", "pt_guide_reflections",
           "pt_denoise", "pt_denoise_device", "pt_set_sample_base", "pt_sample_base", "pt_temporal_accumulate", "pt_temporal_reset",
           "pt_temporal_frames", "pt_read_temporal", "pt_write_temporal", "pt_temporal_device_ptr", "pt_set_instance_motion", "pt_instance_motion",
           "pt_read_motion_guides", "pt_write_motion_guides", "pt_motion_guides_device_ptr", "pt_debug_motion_records",
           "pt_set_vertex_motion", "pt_vertex_motion", "pt_debug_vertex_motion_rows",
           "pt_set_rebuilt_motion", "pt_rebuilt_motion", "pt_debug_gather_records", "pt_set_temporal_variance", "pt_temporal_variance",
           "pt_read_temporal_variance", "pt_write_temporal_variance", "pt_temporal_variance_device_ptr",
           "pt_set_temporal_response", "pt_temporal_response", "pt_read_temporal_fast", "pt_write_temporal_fast", "pt_read_temporal_response",
           "pt_temporal_fast_device_ptr", "pt_set_firefly_clamp", "pt_firefly_clamp", "pt_read_firefly", "pt_firefly_counts", "pt_firefly_device_ptr",
           "pt_set_adaptive", "pt_adaptive", "pt_adaptive_params_get", "pt_render_adaptive", "pt_adaptive_stats_get", "pt_read_adaptive", "pt_write_adaptive",
           "pt_adaptive_device_ptr", "pt_debug_adaptive_timing",
           "pt_stats_get", "pt_stats_reset", "pt_profile_kernels", "pt_reduce_accum",
           "pt_intersect", "pt_gen_rays", "pt_primary_pass", "pt_shade_batch", "pt_debug_quantise_node", "pt_debug_convert", "pt_debug_copy_bandwidth", "pt_debug_math_probe", "pt_debug_rng_probe", "pt_debug_live_resources",
           "pt_version"]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(DEVICE_LIB_PATH):
            raise RuntimeError(f"{DEVICE_LIB_PATH} missing: the HIP extension was not built "
                               "(run __graft_entry__.build()); there is no CPU fallback")
        try:
            # torch ships its own libamdhip64; two HIP runtimes in one process do not both see the GPU.
            # Importing torch first makes libptamd.so bind to the runtime torch has already loaded.
            import torch  # noqa: F401
        except ImportError:
            pass
        l = C.CDLL(DEVICE_LIB_PATH)
        l.pt_last_error.restype = C.c_char_p
        l.pt_last_error.argtypes = [C.c_void_p]
        l.pt_version.restype = C.c_char_p
        l.pt_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
        l.pt_destroy.argtypes = [C.c_void_p]
        l.pt_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_upload_static.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_uint32, C.c_void_p, C.c_uint32]
        l.pt_upload_static_async.argtypes = l.pt_upload_static.argtypes
        l.pt_upload_dynamic.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
        l.pt_upload_dynamic_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
        l.pt_frame_tick.argtypes = [C.c_void_p]
        l.pt_update_geometry.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        l.pt_refit_vertices.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        l.pt_upload_texture_array.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        l.pt_set_camera.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_set_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        l.pt_set_accum_buffer.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_clear.argtypes = [C.c_void_p]
        l.pt_render.argtypes = [C.c_void_p, C.c_uint32]
        l.pt_synchronize.argtypes = [C.c_void_p]
        l.pt_resolve.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_resolve_device.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_resolve_device_ptr.restype = C.c_void_p
        l.pt_resolve_device_ptr.argtypes = [C.c_void_p]
        l.pt_read_accum.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_write_accum.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        l.pt_accum_device_ptr.restype = C.c_void_p
        l.pt_accum_device_ptr.argtypes = [C.c_void_p]
        l.pt_samples_per_pixel.restype = C.c_uint32
        l.pt_samples_per_pixel.argtypes = [C.c_void_p]
        l.pt_render_guides.argtypes = [C.c_void_p, C.c_uint32]
        l.pt_guide_samples.restype = C.c_uint32
        l.pt_guide_samples.argtypes = [C.c_void_p]
        l.pt_read_guides.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_write_guides.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        l.pt_guides_device_ptr.restype = C.c_void_p
        l.pt_guides_device_ptr.argtypes = [C.c_void_p, C.c_int]
        l.pt_set_guide_chain.argtypes = [C.c_void_p, C.c_uint32]
        l.pt_guide_chain.restype = C.c_uint32
        l.pt_guide_chain.argtypes = [C.c_void_p]
        l.pt_debug_guide_chain_terminals.argtypes = [C.c_void_p, C.c_int]
        l.pt_debug_read_guide_chain_terminals.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_set_guide_reflections.argtypes = [C.c_void_p, C.c_int]
        l.pt_guide_reflections.restype = C.c_int
        l.pt_guide_reflections.argtypes = [C.c_void_p]
        l.pt_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p, C.POINTER(C.c_float)]
        l.pt_denoise_device.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p]
        l.pt_set_sample_base.argtypes = [C.c_void_p, C.c_uint32]
        l.pt_sample_base.restype = C.c_uint32
        l.pt_sample_base.argtypes = [C.c_void_p]
        l.pt_temporal_accumulate.argtypes = [C.c_void_p, C.POINTER(TemporalParams)]
        l.pt_temporal_reset.argtypes = [C.c_void_p]
        l.pt_temporal_frames.restype = C.c_uint32
        l.pt_temporal_frames.argtypes = [C.c_void_p]
        l.pt_read_temporal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_write_temporal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_temporal_device_ptr.restype = C.c_void_p
        l.pt_temporal_device_ptr.argtypes = [C.c_void_p, C.c_int]
        l.pt_set_instance_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        l.pt_instance_motion.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        l.pt_read_motion_guides.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_write_motion_guides.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_motion_guides_device_ptr.restype = C.c_void_p
        l.pt_motion_guides_device_ptr.argtypes = [C.c_void_p, C.c_int]
        l.pt_debug_motion_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        l.pt_set_vertex_motion.argtypes = [C.c_void_p, C.c_int]
        l.pt_vertex_motion.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        l.pt_debug_vertex_motion_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        l.pt_set_rebuilt_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        l.pt_rebuilt_motion.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        l.pt_debug_gather_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        l.pt_set_temporal_variance.argtypes = [C.c_void_p, C.POINTER(VarianceParams)]
        l.pt_temporal_variance.argtypes = [C.c_void_p]
        l.pt_read_temporal_variance.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_write_temporal_variance.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_temporal_variance_device_ptr.restype = C.c_void_p
        l.pt_temporal_variance_device_ptr.argtypes = [C.c_void_p]
        l.pt_set_temporal_response.argtypes = [C.c_void_p, C.POINTER(ResponseParams)]
        l.pt_temporal_response.argtypes = [C.c_void_p]
        l.pt_read_temporal_fast.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_write_temporal_fast.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_read_temporal_response.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_temporal_fast_device_ptr.restype = C.c_void_p
        l.pt_temporal_fast_device_ptr.argtypes = [C.c_void_p]
        l.pt_set_firefly_clamp.argtypes = [C.c_void_p, C.POINTER(FireflyParams)]
        l.pt_firefly_clamp.argtypes = [C.c_void_p]
        l.pt_read_firefly.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        l.pt_firefly_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        l.pt_firefly_device_ptr.restype = C.c_void_p
        l.pt_firefly_device_ptr.argtypes = [C.c_void_p]
        l.pt_set_adaptive.argtypes = [C.c_void_p, C.POINTER(AdaptiveParams)]
        l.pt_adaptive.argtypes = [C.c_void_p]
        l.pt_adaptive_params_get.argtypes = [C.c_void_p, C.POINTER(AdaptiveParams)]
        l.pt_render_adaptive.argtypes = [C.c_void_p, C.c_uint32]
        l.pt_adaptive_stats_get.argtypes = [C.c_void_p, C.POINTER(AdaptiveStats)]
        l.pt_read_adaptive.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        l.pt_write_adaptive.argtypes = [C.c_void_p] + [C.c_void_p] * 3
        l.pt_adaptive_device_ptr.restype = C.c_void_p
        l.pt_adaptive_device_ptr.argtypes = [C.c_void_p, C.c_int]
        l.pt_debug_adaptive_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        l.pt_stats_get.argtypes = [C.c_void_p, C.POINTER(Stats)]
        l.pt_stats_reset.argtypes = [C.c_void_p]
        l.pt_profile_kernels.argtypes = [C.c_void_p, C.c_int]
        l.pt_reduce_accum.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        l.pt_intersect.argtypes = [C.c_void_p, C.POINTER(RaysSoA), C.c_uint32, C.c_int, C.POINTER(HitsSoA), C.c_uint32,
                                   C.POINTER(C.c_float)]
        l.pt_gen_rays.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 7
        l.pt_primary_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8
        l.pt_shade_batch.argtypes = [C.c_void_p, C.POINTER(ShadeBatchIO)]
        l.pt_debug_convert.argtypes = [C.POINTER(Config)] + [C.c_void_p, C.c_uint32] * 6 + [C.c_uint32, C.c_void_p, C.c_size_t]
        _lib = l
    return _lib


class PtError(RuntimeError):
    pass


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def live_resources():
    """pt_debug_live_resources: (device allocations, pinned allocations, events, streams the library created) alive in this process -- no device needed."""
    out = (C.c_uint32 * 4)()
    lib().pt_debug_live_resources.argtypes = [C.POINTER(C.c_uint32)]
    rc = lib().pt_debug_live_resources(out)
    if rc != 0:
        raise PtError(f"pt_debug_live_resources failed ({rc})")
    return tuple(out)


def debug_convert(flat, flags=0, rng_mode=RNG_COUNTER):
    """pt_debug_convert: the line of digests of what pt_upload_static (records made on the host) and pt_upload_dynamic make of `flat` -- no device needed."""
    cfg = Config(64, 64, 0, 0, rng_mode, 1, 0, flags, 0, 0.0, 0.0)
    line = C.create_string_buffer(2048)
    rc = lib().pt_debug_convert(C.byref(cfg), _p(flat.vertices), len(flat.vertices), _p(flat.triangles), len(flat.triangles), _p(flat.materials),
                                len(flat.materials), _p(flat.sub_nodes), len(flat.sub_nodes), _p(flat.lights), len(flat.lights), _p(flat.top_nodes),
                                len(flat.top_nodes), flat.top_root, line, len(line))
    if rc != 0:
        raise PtError(f"pt_debug_convert failed ({rc}): {lib().pt_last_error(None).decode()}")
    return line.value.decode()


MOTION_RECORD_BYTES = 96  # three float4 rows (A | t) of P - I, then the three rows of the previous invTransform


def _inv_transforms(prev):
    """(n, 16) float32 from an (n, 16) array or a top_nodes record array (its invTransform)"""
    prev = np.asarray(prev)
    if prev.dtype.names and "invTransform" in prev.dtype.names:
        prev = prev["invTransform"]
    return np.ascontiguousarray(prev, np.float32).reshape(-1, 16)


def debug_motion_records(prev_inv, cur_inv):
    """pt_debug_motion_records: the (n, 6, 4) float32 records pt_set_instance_motion makes of n (previous, current) invTransforms -- no device needed."""
    p, c = _inv_transforms(prev_inv), _inv_transforms(cur_inv)
    assert p.shape == c.shape
    out = np.zeros((len(p), 6, 4), np.float32)
    rc = lib().pt_debug_motion_records(_p(p), _p(c), len(p), _p(out))
    if rc != 0:
        raise PtError(f"pt_debug_motion_records failed ({rc}): {lib().pt_last_error(None).decode()}")
    return out


def debug_vertex_motion_rows(inv):
    """pt_debug_vertex_motion_rows: the (n, 3, 4) float32 rows pt_set_vertex_motion makes of n invTransforms -- the linear part of each one's inverse,
    w = 0 -- no device needed."""
    m = _inv_transforms(inv)
    out = np.zeros((len(m), 3, 4), np.float32)
    rc = lib().pt_debug_vertex_motion_rows(_p(m), len(m), _p(out))
    if rc != 0:
        raise PtError(f"pt_debug_vertex_motion_rows failed ({rc}): {lib().pt_last_error(None).decode()}")
    return out


def _denoise_input(input_temporal, input):
    if input is not None:
        return int(input)
    return DENOISE_INPUT_TEMPORAL if input_temporal else DENOISE_INPUT_ACCUM


class Context:
    """One render context on one GPU (mirrors what RayTracer owns, reference src/raytracer.h:54-106)."""

    def __init__(self, width, height, max_active_rays=0, max_bounces=0, rng_mode=RNG_COUNTER, seed=1, device=0,
                 flags=0, samples_in_flight=0, ext_queue_fraction=0.0, shadow_queue_fraction=0.0):
        self._h = C.c_void_p()
        self.width, self.height = width, height
        cfg = Config(width, height, max_active_rays, max_bounces, rng_mode, seed, device, flags, samples_in_flight, ext_queue_fraction, shadow_queue_fraction)
        rc = lib().pt_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise PtError(f"pt_create failed ({rc}): {lib().pt_last_error(None).decode()}")

    def _chk(self, rc, what):
        if rc != 0:
            raise PtError(f"{what} failed ({rc}): {lib().pt_last_error(self._h).decode()}")

    def close(self):
        if self._h:
            lib().pt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- scene
    def upload_scene(self, flat, sky=None, material_textures=None):
        self._chk(lib().pt_upload_static(self._h, _p(flat.vertices), len(flat.vertices), _p(flat.triangles),
                                         len(flat.triangles), _p(flat.materials), len(flat.materials),
                                         _p(flat.sub_nodes), len(flat.sub_nodes)), "pt_upload_static")
        self.upload_dynamic(flat)
        if sky is not None:
            self.upload_texture(1, sky)
        if material_textures is not None:
            self.upload_texture(0, material_textures)

    def upload_static_async(self, flat):
        """A rebuilt scene, converted and copied beside the one that is rendering (the render stream is not synchronised); follow with
        upload_dynamic_async(flat) and frame_tick(), which adopts both."""
        self._chk(lib().pt_upload_static_async(self._h, _p(flat.vertices), len(flat.vertices), _p(flat.triangles), len(flat.triangles),
                                               _p(flat.materials), len(flat.materials), _p(flat.sub_nodes), len(flat.sub_nodes)), "pt_upload_static_async")

    def upload_dynamic(self, flat):
        self._chk(lib().pt_upload_dynamic(self._h, _p(flat.lights), len(flat.lights), _p(flat.top_nodes),
                                          len(flat.top_nodes), flat.top_root), "pt_upload_dynamic")

    def upload_dynamic_async(self, flat):
        """Convert the next dynamic state and start copying it into the inactive device buffers; frame_tick() adopts it."""
        self._chk(lib().pt_upload_dynamic_async(self._h, _p(flat.lights), len(flat.lights), _p(flat.top_nodes),
                                                len(flat.top_nodes), flat.top_root), "pt_upload_dynamic_async")

    def frame_tick(self):
        self._chk(lib().pt_frame_tick(self._h), "pt_frame_tick")

    def update_geometry(self, flat):
        """Refitted geometry (same topology): new vertices and sub-BVH boxes; follow with upload_dynamic(_async) / frame_tick."""
        self._chk(lib().pt_update_geometry(self._h, _p(flat.vertices), len(flat.vertices), _p(flat.sub_nodes), len(flat.sub_nodes)),
                  "pt_update_geometry")

    def refit_vertices(self, first_vertex, vertices):
        """A deformed mesh, refitted on the device: its vertex records (L.VERTEX) replace [first_vertex, ...) of the uploaded array; every box
        of the device's trees is recomputed there.  Follow with upload_dynamic(_async) / frame_tick."""
        v = np.ascontiguousarray(vertices, L.VERTEX)
        self._chk(lib().pt_refit_vertices(self._h, first_vertex, _p(v), len(v)), "pt_refit_vertices")

    def upload_texture(self, kind, arr):
        """[layers][h][w][4]: float32 r g b a (PT_TEX_RGBA32F) or uint8 b g r a (PT_TEX_BGRA8_UNORM, the reference's material
        array format); rows bottom-up."""
        arr = np.asarray(arr)
        fmt = TEX_BGRA8_UNORM if arr.dtype == np.uint8 else TEX_RGBA32F
        arr = np.ascontiguousarray(arr, np.uint8 if fmt == TEX_BGRA8_UNORM else np.float32)
        assert arr.ndim == 4 and arr.shape[3] == 4
        self._chk(lib().pt_upload_texture_array(self._h, kind, arr.shape[2], arr.shape[1], arr.shape[0], fmt, _p(arr)),
                  "pt_upload_texture_array")

    def set_camera(self, camera):
        cam = np.ascontiguousarray(np.asarray(camera, L.CAMERA).reshape(1))
        self._chk(lib().pt_set_camera(self._h, _p(cam)), "pt_set_camera")

    def set_tiles(self, rects):
        arr = (Rect * max(len(rects), 1))(*[Rect(*r) for r in rects])
        self._chk(lib().pt_set_tiles(self._h, arr if rects else None, len(rects)), "pt_set_tiles")

    def set_stream(self, stream_handle):
        """Enqueue everything on a caller-owned HIP stream.  A handle of 0 is the legacy default stream -- what
        torch.cuda.current_stream().cuda_stream is unless a torch.cuda.Stream is current -- which the C-ABI cannot tell from
        "no stream" (NULL = the context's own stream): refuse it instead of silently losing the ordering."""
        if not stream_handle:
            raise PtError("set_stream(0): the legacy default stream cannot be selected; make a torch.cuda.Stream current "
                          "and pass its handle (own_stream() returns to the context's own stream)")
        self._chk(lib().pt_set_stream(self._h, C.c_void_p(stream_handle)), "pt_set_stream")

    def own_stream(self):
        self._chk(lib().pt_set_stream(self._h, None), "pt_set_stream")

    def set_accum_buffer(self, device_ptr):
        self._chk(lib().pt_set_accum_buffer(self._h, C.c_void_p(device_ptr)), "pt_set_accum_buffer")

    # ---- render
    def clear(self):
        self._chk(lib().pt_clear(self._h), "pt_clear")

    def render(self, spp=1, sync=True):
        self._chk(lib().pt_render(self._h, spp), "pt_render")
        if sync:
            self.synchronize()

    def synchronize(self):
        self._chk(lib().pt_synchronize(self._h), "pt_synchronize")

    def read_accum(self):
        out = np.zeros((self.height * self.width, 4), np.float32)
        self._chk(lib().pt_read_accum(self._h, _p(out)), "pt_read_accum")
        return out

    def write_accum(self, accum, spp):
        a = np.ascontiguousarray(accum, np.float32)
        self._chk(lib().pt_write_accum(self._h, _p(a), spp), "pt_write_accum")

    def resolve(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._chk(lib().pt_resolve(self._h, _p(out)), "pt_resolve")
        return out

    def resolve_device(self, device_ptr=None):
        """accumulate kernel into device memory (None: a buffer owned by the context); asynchronous."""
        self._chk(lib().pt_resolve_device(self._h, C.c_void_p(device_ptr) if device_ptr else None), "pt_resolve_device")

    @property
    def resolve_device_ptr(self):
        """Device address of the image resolve_device(None) writes (0 before the first such call)."""
        return lib().pt_resolve_device_ptr(self._h) or 0

    @property
    def samples_per_pixel(self):
        return int(lib().pt_samples_per_pixel(self._h))

    @property
    def accum_device_ptr(self):
        return lib().pt_accum_device_ptr(self._h)

    # ---- first-hit guide buffers and the a-trous denoiser
    def render_guides(self, spp=1, sync=True):
        """`spp` more guide samples (albedo, world-space normal, hit distance, coverage of the camera rays' first hits)."""
        self._chk(lib().pt_render_guides(self._h, spp), "pt_render_guides")
        if sync:
            self.synchronize()

    @property
    def guide_samples(self):
        return int(lib().pt_guide_samples(self._h))

    def read_guides(self):
        """(albedo_hits, normal_depth): two (width*height, 4) arrays of sums over the guide samples"""
        a = np.zeros((self.height * self.width, 4), np.float32)
        g = np.zeros((self.height * self.width, 4), np.float32)
        self._chk(lib().pt_read_guides(self._h, _p(a), _p(g)), "pt_read_guides")
        return a, g

    def write_guides(self, albedo_hits, normal_depth, spp):
        a = np.ascontiguousarray(albedo_hits, np.float32)
        g = np.ascontiguousarray(normal_depth, np.float32)
        assert a.size == g.size == self.width * self.height * 4
        self._chk(lib().pt_write_guides(self._h, _p(a), _p(g), spp), "pt_write_guides")

    def guides_device_ptr(self, which):
        """Device address of the albedo_hits (0) / normal_depth (1) image (0 before the first guide call)."""
        return lib().pt_guides_device_ptr(self._h, which) or 0

    def set_guide_chain(self, max_transmissions):
        """pt_set_guide_chain: guide rays follow up to `max_transmissions` refractions to the first surface that is not glass (0, the default: off).
        Right after clear(): a change is refused once guide samples are in."""
        self._chk(lib().pt_set_guide_chain(self._h, max_transmissions), "pt_set_guide_chain")

    @property
    def guide_chain(self):
        return int(lib().pt_guide_chain(self._h))

    def set_guide_reflections(self, enable=True):
        """pt_set_guide_reflections: the guide chain also follows mirrors (PBR metal of smoothness > 0.94) and total internal reflection, and the
        terminal's albedo is tinted by the mirrors on the way.  Inert without set_guide_chain(K > 0).  Right after clear(), like set_guide_chain."""
        self._chk(lib().pt_set_guide_reflections(self._h, 1 if enable else 0), "pt_set_guide_reflections")

    @property
    def guide_reflections(self):
        return bool(lib().pt_guide_reflections(self._h))

    def debug_guide_chain_terminals(self, enable=True):
        """test hook: chain passes record where each pixel's chain ended (read_guide_chain_terminals)"""
        self._chk(lib().pt_debug_guide_chain_terminals(self._h, 1 if enable else 0), "pt_debug_guide_chain_terminals")

    def read_guide_chain_terminals(self):
        """(width*height, 4) int32 of the last guide sample: primitive, top-level leaf, stage, 1 = total internal reflection (with guide reflections
        on: the number of reflections the chain followed); -1s: a miss / never written"""
        out = np.zeros((self.height * self.width, 4), np.int32)
        self._chk(lib().pt_debug_read_guide_chain_terminals(self._h, _p(out)), "pt_debug_read_guide_chain_terminals")
        return out

    def denoise(self, iterations=5, hdr=False, k_normal=0.0, sigma_depth=0.0, sigma_lum=0.0, with_ms=False, input_temporal=False, input=None):
        """The edge-avoiding a-trous filter over the accumulator under the guides: (height, width, 4) tone-mapped like resolve(), or linear
        mean radiance (hdr=True); with_ms: also the device ms of the filter's kernels; input_temporal: the filter starts from the temporal
        history (temporal_accumulate) instead of the accumulator; input: one of DENOISE_INPUT_* (DENOISE_INPUT_TEMPORAL_VARIANCE: the history
        under its luminance variance, set_temporal_variance), which overrides input_temporal."""
        prm = DenoiseParams(iterations, DENOISE_HDR if hdr else DENOISE_TONEMAPPED, k_normal, sigma_depth, sigma_lum,
                            _denoise_input(input_temporal, input))
        out = np.zeros((self.height, self.width, 4), np.float32)
        ms = C.c_float(0)
        self._chk(lib().pt_denoise(self._h, C.byref(prm), _p(out), C.byref(ms)), "pt_denoise")
        return (out, float(ms.value)) if with_ms else out

    def denoise_device(self, iterations=5, hdr=False, k_normal=0.0, sigma_depth=0.0, sigma_lum=0.0, device_ptr=None, input_temporal=False, input=None):
        """The same into device memory (None: the context-owned image, resolve_device_ptr); asynchronous."""
        prm = DenoiseParams(iterations, DENOISE_HDR if hdr else DENOISE_TONEMAPPED, k_normal, sigma_depth, sigma_lum,
                            _denoise_input(input_temporal, input))
        self._chk(lib().pt_denoise_device(self._h, C.byref(prm), C.c_void_p(device_ptr) if device_ptr else None), "pt_denoise_device")

    # ---- sample base and temporal history
    def set_sample_base(self, base):
        """render / render_guides trace the sample indices base + samples_per_pixel ... (a frame loop that clears every frame sets its frame number)."""
        self._chk(lib().pt_set_sample_base(self._h, base), "pt_set_sample_base")

    @property
    def sample_base(self):
        return int(lib().pt_sample_base(self._h))

    def temporal_accumulate(self, max_history=0, k_normal=0.0, sigma_depth=0.0, sync=True):
        """Reproject the history into the current camera and blend the current frame (accumulator + guides) into it."""
        prm = TemporalParams(max_history, k_normal, sigma_depth)
        self._chk(lib().pt_temporal_accumulate(self._h, C.byref(prm)), "pt_temporal_accumulate")
        if sync:
            self.synchronize()

    def temporal_reset(self):
        self._chk(lib().pt_temporal_reset(self._h), "pt_temporal_reset")

    @property
    def temporal_frames(self):
        return int(lib().pt_temporal_frames(self._h))

    def read_temporal(self):
        """(colour_count, normal_depth) of the newest history set: two (width*height, 4) arrays, (d.rgb, N) and (n.xyz, z)"""
        cn = np.zeros((self.height * self.width, 4), np.float32)
        nd = np.zeros((self.height * self.width, 4), np.float32)
        self._chk(lib().pt_read_temporal(self._h, _p(cn), _p(nd)), "pt_read_temporal")
        return cn, nd

    def write_temporal(self, colour_count, normal_depth, camera):
        """Install a history (a checkpoint, a test input) and the camera it was made under."""
        cn = np.ascontiguousarray(colour_count, np.float32)
        nd = np.ascontiguousarray(normal_depth, np.float32)
        assert cn.size == nd.size == self.width * self.height * 4
        cam = np.ascontiguousarray(np.asarray(camera, L.CAMERA).reshape(1))
        self._chk(lib().pt_write_temporal(self._h, _p(cn), _p(nd), _p(cam)), "pt_write_temporal")

    def temporal_device_ptr(self, which):
        """Device address of the colour_count (0) / normal_depth (1) image of the newest set (0 before the first temporal call)."""
        return lib().pt_temporal_device_ptr(self._h, which) or 0

    # ---- temporal variance
    def set_temporal_variance(self, on=True, sigma_variance=0.0, relative_floor=0.0, full_history=0.0):
        """Keep the luminance variance of every pixel's history beside it (temporal_accumulate) for denoise(input=DENOISE_INPUT_TEMPORAL_VARIANCE);
        False forgets it.  Only while there is no history: right after temporal_reset()."""
        prm = VarianceParams(sigma_variance, relative_floor, full_history)
        self._chk(lib().pt_set_temporal_variance(self._h, C.byref(prm) if on else None), "pt_set_temporal_variance")

    @property
    def temporal_variance(self):
        return bool(lib().pt_temporal_variance(self._h))

    def read_temporal_variance(self):
        """the variance plane of the newest history set: (width*height,) float32"""
        out = np.zeros(self.height * self.width, np.float32)
        self._chk(lib().pt_read_temporal_variance(self._h, _p(out)), "pt_read_temporal_variance")
        return out

    def write_temporal_variance(self, variance):
        """Install the variance plane of the newest set (after write_temporal, which zeroes it)."""
        v = np.ascontiguousarray(variance, np.float32)
        assert v.size == self.width * self.height
        self._chk(lib().pt_write_temporal_variance(self._h, _p(v)), "pt_write_temporal_variance")

    @property
    def temporal_variance_device_ptr(self):
        """Device address of the newest set's variance plane (0 while the mode is off or nothing is allocated yet)."""
        return lib().pt_temporal_variance_device_ptr(self._h) or 0

    # ---- temporal response
    def set_temporal_response(self, on=True, fast_history=0, sigma_response=0.0, relative_floor=0.0):
        """Keep a short, fast history beside the long one (temporal_accumulate) and fall back to it where the two disagree over a 7 x 7 window by more
        than the fast one's noise explains: a lighting change.  False forgets it.  Only while there is no history: right after temporal_reset()."""
        prm = ResponseParams(fast_history, sigma_response, relative_floor)
        self._chk(lib().pt_set_temporal_response(self._h, C.byref(prm) if on else None), "pt_set_temporal_response")

    @property
    def temporal_response(self):
        return bool(lib().pt_temporal_response(self._h))

    def read_temporal_fast(self):
        """the fast history (d_f.rgb, N_f) of the newest set: (width*height, 4) float32"""
        out = np.zeros((self.height * self.width, 4), np.float32)
        self._chk(lib().pt_read_temporal_fast(self._h, _p(out)), "pt_read_temporal_fast")
        return out

    def write_temporal_fast(self, colour_count):
        """Install the fast history of the newest set (after write_temporal, which zeroes it)."""
        f = np.ascontiguousarray(colour_count, np.float32)
        assert f.size == self.width * self.height * 4
        self._chk(lib().pt_write_temporal_fast(self._h, _p(f)), "pt_write_temporal_fast")

    def read_temporal_response(self):
        """the mix factor s of the last temporal_accumulate: (width*height,) float32"""
        out = np.zeros(self.height * self.width, np.float32)
        self._chk(lib().pt_read_temporal_response(self._h, _p(out)), "pt_read_temporal_response")
        return out

    @property
    def temporal_fast_device_ptr(self):
        """Device address of the newest set's fast image (0 while the mode is off or nothing is allocated yet)."""
        return lib().pt_temporal_fast_device_ptr(self._h) or 0

    # ---- firefly clamp
    def set_firefly_clamp(self, enable=True, rank=0, scale=0.0):
        """Bound every pixel's demodulated colour by `scale` x the `rank`-th largest luminance of its 5 x 5 neighbours before temporal_accumulate and
        denoise (accumulator input, iterations > 0) see it; the accumulator, render and resolve are untouched.  False turns it off.  At any time."""
        prm = FireflyParams(rank, scale)
        self._chk(lib().pt_set_firefly_clamp(self._h, C.byref(prm) if enable else None), "pt_set_firefly_clamp")

    @property
    def firefly_clamp(self):
        return bool(lib().pt_firefly_clamp(self._h))

    def read_firefly(self):
        """Evaluates the stage on the current accumulator and guides: ((width*height, 4) float32 plane (d_out.rgb, s), (clamped, nonfinite))"""
        out = np.zeros((self.height * self.width, 4), np.float32)
        counts = (C.c_uint32 * 2)()
        self._chk(lib().pt_read_firefly(self._h, _p(out), counts), "pt_read_firefly")
        return out, (int(counts[0]), int(counts[1]))

    @property
    def firefly_counts(self):
        """(clamped, nonfinite) of the last evaluation, whichever call made it"""
        counts = (C.c_uint32 * 2)()
        self._chk(lib().pt_firefly_counts(self._h, counts), "pt_firefly_counts")
        return int(counts[0]), int(counts[1])

    @property
    def firefly_device_ptr(self):
        """Device address of the clamped plane (0 while the mode is off or before the first evaluation)."""
        return lib().pt_firefly_device_ptr(self._h) or 0

    # ---- adaptive sampling
    def set_adaptive(self, enable=True, threshold=0.0, min_samples=0, round_samples=0, max_samples=0):
        """Converging renders in rounds that stop the 8 x 8 blocks whose two half images agree to within `threshold` (0: never by error -- uniform
        sampling to max_samples).  The sample counts are even; 0 selects 64, 64 and 1024.  False turns the mode off.  The mode changes only right after
        clear(); with the mode on the parameters may change at any time, which re-evaluates the flags."""
        prm = AdaptiveParams(threshold, min_samples, round_samples, max_samples)
        self._chk(lib().pt_set_adaptive(self._h, C.byref(prm) if enable else None), "pt_set_adaptive")

    @property
    def adaptive(self):
        return bool(lib().pt_adaptive(self._h))

    @property
    def adaptive_params(self):
        """(threshold, min_samples, round_samples, max_samples) in force, defaults resolved"""
        prm = AdaptiveParams()
        self._chk(lib().pt_adaptive_params_get(self._h, C.byref(prm)), "pt_adaptive_params_get")
        return float(prm.threshold), int(prm.min_samples), int(prm.round_samples), int(prm.max_samples)

    def render_adaptive(self, rounds=0):
        """Up to `rounds` rounds (0: until no block is active or every pixel holds max_samples); returns adaptive_stats."""
        self._chk(lib().pt_render_adaptive(self._h, rounds), "pt_render_adaptive")
        return self.adaptive_stats

    @property
    def adaptive_stats(self):
        st = AdaptiveStats()
        self._chk(lib().pt_adaptive_stats_get(self._h, C.byref(st)), "pt_adaptive_stats_get")
        return {k: getattr(st, k) for k, _ in AdaptiveStats._fields_ if not k.startswith("_")}

    def read_adaptive(self):
        """dict: A, B (width*height, 4) float32 sums; counts (width*height,) uint32; error (width*height,) float32; block_error (blocks,) float32"""
        n, nb = self.width * self.height, ((self.width + 7) // 8) * ((self.height + 7) // 8)
        out = {"A": np.zeros((n, 4), np.float32), "B": np.zeros((n, 4), np.float32), "counts": np.zeros(n, np.uint32),
               "error": np.zeros(n, np.float32), "block_error": np.zeros(nb, np.float32)}
        self._chk(lib().pt_read_adaptive(self._h, _p(out["A"]), _p(out["B"]), _p(out["counts"]), _p(out["error"]), _p(out["block_error"])), "pt_read_adaptive")
        return out

    def write_adaptive(self, A, B, counts):
        """Restore the two halves and the counts (constant per 8 x 8 block, even, <= max_samples): evaluates and publishes; samples_per_pixel = max count."""
        n = self.width * self.height
        A = np.ascontiguousarray(A, np.float32).reshape(n, 4)
        B = np.ascontiguousarray(B, np.float32).reshape(n, 4)
        counts = np.ascontiguousarray(counts, np.uint32).reshape(n)
        self._chk(lib().pt_write_adaptive(self._h, _p(A), _p(B), _p(counts)), "pt_write_adaptive")

    def adaptive_device_ptr(self, which):
        """Device address of A (0), B (1), counts (2), error (3); 0 before the state is allocated."""
        return lib().pt_adaptive_device_ptr(self._h, which) or 0

    @property
    def adaptive_timing(self):
        """pt_debug_adaptive_timing: (device ms in evaluations, evaluations, host ms changing the pixel list, list changes), sums since creation"""
        out = (C.c_double * 4)()
        self._chk(lib().pt_debug_adaptive_timing(self._h, out), "pt_debug_adaptive_timing")
        return tuple(out)

    # ---- instance motion
    def set_instance_motion(self, prev):
        """The invTransform every top-level node of the active state had when the newest history was made: an (n_top, 16) float32 array, a top_nodes
        record array (its invTransform is taken), or None to forget the motion.  Right after clear(): refused once guide samples are in."""
        if prev is None:
            self._chk(lib().pt_set_instance_motion(self._h, None, 0), "pt_set_instance_motion")
            return
        m = _inv_transforms(prev)
        self._chk(lib().pt_set_instance_motion(self._h, _p(m), len(m)), "pt_set_instance_motion")

    @property
    def instance_motion(self):
        """(set, moving): whether a motion is set, and how many leaves' previous transform differs from the current one in any bit"""
        moving = C.c_uint32(0)
        return bool(lib().pt_instance_motion(self._h, C.byref(moving))), int(moving.value)

    def read_motion_guides(self):
        """(motion, prev_normal): two (width*height, 4) arrays of sums over the guide samples"""
        m = np.zeros((self.height * self.width, 4), np.float32)
        pn = np.zeros((self.height * self.width, 4), np.float32)
        self._chk(lib().pt_read_motion_guides(self._h, _p(m), _p(pn)), "pt_read_motion_guides")
        return m, pn

    def write_motion_guides(self, motion, prev_normal):
        m = np.ascontiguousarray(motion, np.float32)
        pn = np.ascontiguousarray(prev_normal, np.float32)
        assert m.size == pn.size == self.width * self.height * 4
        self._chk(lib().pt_write_motion_guides(self._h, _p(m), _p(pn)), "pt_write_motion_guides")

    def motion_guides_device_ptr(self, which):
        """Device address of the motion (0) / prev_normal (1) image (0 before they are allocated)."""
        return lib().pt_motion_guides_device_ptr(self._h, which) or 0

    # ---- vertex motion
    def set_vertex_motion(self, on=True):
        """Take the geometry of the previous dynamic state (the one before the last frame_tick) as where the refitted meshes were when the newest
        history was made; False forgets it.  Right after clear(), like set_instance_motion."""
        self._chk(lib().pt_set_vertex_motion(self._h, 1 if on else 0), "pt_set_vertex_motion")

    @property
    def vertex_motion(self):
        """(set, deformed): whether a vertex motion is set, and 1 when a refit came between the previous state and the active one (else 0)"""
        deformed = C.c_uint32(0)
        return bool(lib().pt_vertex_motion(self._h, C.byref(deformed))), int(deformed.value)

    # ---- rebuilt motion
    def set_rebuilt_motion(self, prev_triangle):
        """The vertex motion of a state whose tree was REBUILT since the previous one (upload_static_async): prev_triangle[i] is the index triangle i of
        the active state had in the previous dynamic state's triangle array, NO_PREVIOUS_TRIANGLE where it is new (host.triangle_history makes such a
        map).  None forgets the motion.  Right after clear(), like set_vertex_motion, whose state it sets."""
        if prev_triangle is None:
            self._chk(lib().pt_set_rebuilt_motion(self._h, None, 0), "pt_set_rebuilt_motion")
            return
        m = np.ascontiguousarray(prev_triangle, np.uint32)
        if m.ndim != 1:
            raise ValueError("set_rebuilt_motion: the map is one-dimensional, an entry per triangle of the active state")
        self._chk(lib().pt_set_rebuilt_motion(self._h, _p(m), len(m)), "pt_set_rebuilt_motion")

    @property
    def rebuilt_motion(self):
        """(set, followed): whether a rebuilt motion is set, and how many entries of its map name a previous triangle"""
        followed = C.c_uint32(0)
        return bool(lib().pt_rebuilt_motion(self._h, C.byref(followed))), int(followed.value)

    def debug_gather_records(self, then, now, prev_triangle):
        """k_gather_then on the device (pt_debug_gather_records): then (n_then, 32) and now (n_now, 32) uint32 -- 128-byte records --, prev_triangle
        (n_now) uint32; returns the (n_now, 32) uint32 records out[i] = then[prev_triangle[i]] where that entry is below n_then, else now[i]."""
        then = np.ascontiguousarray(then, np.uint32).reshape(-1, 32)
        now = np.ascontiguousarray(now, np.uint32).reshape(-1, 32)
        m = np.ascontiguousarray(prev_triangle, np.uint32)
        if m.shape != (len(now),):
            raise ValueError("debug_gather_records: one map entry per current record")
        out = np.zeros_like(now)
        self._chk(lib().pt_debug_gather_records(self._h, _p(then) if len(then) else None, len(then), _p(now), len(now), _p(m), _p(out)),
                  "pt_debug_gather_records")
        return out

    def stats(self):
        s = Stats()
        self._chk(lib().pt_stats_get(self._h, C.byref(s)), "pt_stats_get")
        return {n: getattr(s, n) for n, _ in s._fields_}

    def copy_bandwidth(self, nbytes=1 << 30, repeat=5):
        """GB/s (read + written) of a float4 grid-stride device copy: the achievable-HBM yardstick of this box."""
        lib().pt_debug_copy_bandwidth.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_float)]
        g = C.c_float(0)
        self._chk(lib().pt_debug_copy_bandwidth(self._h, nbytes, repeat, C.byref(g)), "pt_debug_copy_bandwidth")
        return float(g.value)

    def debug_math_probe(self, a, b):
        """The fast division / square-root helpers of k_shade next to the plain operators, on the device (pt_debug_math_probe): a dict of float32
        arrays div, fast_div, sqrt, fast_sqrt (n) and normalize, fast_normalize (n, 3) of the vectors (a, b, a + b)."""
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        if a.shape != b.shape or a.ndim != 1:
            raise ValueError("debug_math_probe: a and b must be one-dimensional and of one length")
        out = np.zeros((10, len(a)), np.float32)
        lib().pt_debug_math_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        self._chk(lib().pt_debug_math_probe(self._h, _p(a), _p(b), len(a), _p(out)), "pt_debug_math_probe")
        return {"div": out[0], "fast_div": out[1], "sqrt": out[2], "fast_sqrt": out[3],
                "normalize": np.ascontiguousarray(out[4:7].T), "fast_normalize": np.ascontiguousarray(out[7:10].T)}

    def debug_rng_probe(self, entries):
        """The production PRNG (csrc/pt_math.h) on the device (pt_debug_rng_probe).  entries: (n, 8) uint32 -- [0, pixel, sample, seed, depth, ...] for 20
        successive draws of that stage's generator, [1, weyl, gamma, k1, i, j, ...] for one draw of a raw state and the integer in [i, j] it selects.
        Returns (n, 20) uint32: the float bits of the draws (keyed), or [draw bits, integer, bits of the following draw, 0 ...] (raw)."""
        entries = np.ascontiguousarray(entries, np.uint32)
        if entries.ndim != 2 or entries.shape[1] != 8 or len(entries) == 0:
            raise ValueError("debug_rng_probe: entries must be a non-empty (n, 8) uint32 array")
        out = np.zeros((len(entries), 20), np.uint32)
        lib().pt_debug_rng_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        self._chk(lib().pt_debug_rng_probe(self._h, _p(entries), len(entries), _p(out)), "pt_debug_rng_probe")
        return out

    def reset_stats(self):
        self._chk(lib().pt_stats_reset(self._h), "pt_stats_reset")

    def profile_kernels(self, enable=True):
        self._chk(lib().pt_profile_kernels(self._h, int(enable)), "pt_profile_kernels")

    # ---- kernel-granular hooks
    def intersect(self, o, d, tmax=None, any_hit=False, repeat=1):
        o = np.ascontiguousarray(o, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        n = len(o)
        cols = [np.ascontiguousarray(o[:, k]) for k in range(3)] + [np.ascontiguousarray(d[:, k]) for k in range(3)]
        tm = np.ascontiguousarray(tmax, np.float32) if tmax is not None else np.full(n, np.inf, np.float32)
        rays = RaysSoA(*[_p(c).value for c in cols], _p(tm).value)
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        prim, inst = np.zeros(n, np.int32), np.zeros(n, np.int32)
        hits = HitsSoA(_p(t).value, _p(u).value, _p(v).value, _p(prim).value, _p(inst).value)
        ms = C.c_float(0)
        self._chk(lib().pt_intersect(self._h, C.byref(rays), n, int(any_hit), C.byref(hits), repeat, C.byref(ms)),
                  "pt_intersect")
        return dict(t=t, u=u, v=v, prim=prim, inst=inst, ms=ms.value)

    def gen_rays(self, sample, n):
        arrs = [np.zeros(n, np.float32) for _ in range(6)]
        pixel = np.zeros(n, np.uint32)
        self._chk(lib().pt_gen_rays(self._h, sample, n, *[_p(a) for a in arrs], _p(pixel)), "pt_gen_rays")
        return np.stack(arrs[:3], 1), np.stack(arrs[3:], 1), pixel

    def primary_pass(self, sample, batch, n):
        """first pass of one batch as pt_render issues it: (o, d, pixel, hits) in queue order"""
        arrs = [np.zeros(n, np.float32) for _ in range(6)]
        pixel = np.zeros(n, np.uint32)
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        prim, inst = np.zeros(n, np.int32), np.zeros(n, np.int32)
        hits = HitsSoA(_p(t).value, _p(u).value, _p(v).value, _p(prim).value, _p(inst).value)
        self._chk(lib().pt_primary_pass(self._h, sample, batch, n, *[_p(a) for a in arrs], _p(pixel), C.byref(hits)), "pt_primary_pass")
        return np.stack(arrs[:3], 1), np.stack(arrs[3:], 1), pixel, dict(t=t, u=u, v=v, prim=prim, inst=inst)

    def shade_batch(self, o, d, thr, pixel, flags, bounce, t, u, v, prim, inst, sample=0, in_pdf=None):
        """in_pdf: the density with which the previous bounce sampled each ray (None: 0); out["npdf"]: the density k_shade wrote for the next bounce"""
        n = len(o)
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        u32 = lambda a: np.ascontiguousarray(a, np.uint32)
        o, d, thr = f32(o), f32(d), f32(thr)
        ins = [f32(o[:, 0]), f32(o[:, 1]), f32(o[:, 2]), f32(d[:, 0]), f32(d[:, 1]), f32(d[:, 2]), f32(thr[:, 0]),
               f32(thr[:, 1]), f32(thr[:, 2]), u32(pixel), u32(flags), u32(bounce), f32(t), f32(u), f32(v),
               np.ascontiguousarray(prim, np.int32), np.ascontiguousarray(inst, np.int32)]
        out = dict(radiance=np.zeros((n, 3), np.float32), out_alive=np.zeros(n, np.uint32))
        for k in ("nox", "noy", "noz", "ndx", "ndy", "ndz", "nthr_r", "nthr_g", "nthr_b"):
            out[k] = np.zeros(n, np.float32)
        out["nflags"] = np.zeros(n, np.uint32)
        out["shadow_alive"] = np.zeros(n, np.uint32)
        for k in ("sox", "soy", "soz", "sdx", "sdy", "sdz", "slen", "sc_r", "sc_g", "sc_b"):
            out[k] = np.zeros(n, np.float32)
        order = ["radiance", "out_alive", "nox", "noy", "noz", "ndx", "ndy", "ndz", "nthr_r", "nthr_g", "nthr_b",
                 "nflags", "shadow_alive", "sox", "soy", "soz", "sdx", "sdy", "sdz", "slen", "sc_r", "sc_g", "sc_b"]
        out["npdf"] = np.zeros(n, np.float32)
        in_pdf = None if in_pdf is None else f32(in_pdf)
        assert in_pdf is None or in_pdf.shape == (n,)
        io = ShadeBatchIO(n, *[_p(a).value for a in ins], sample, *[_p(out[k]).value for k in order],
                          None if in_pdf is None else _p(in_pdf).value, _p(out["npdf"]).value)
        self._chk(lib().pt_shade_batch(self._h, C.byref(io)), "pt_shade_batch")
        return out
