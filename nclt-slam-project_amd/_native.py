"""ctypes binding of csrc/libreloc_hip.so (C-ABI declared in include/reloc.h).

There is deliberately no fallback: if the library is missing, cannot be loaded, or no gfx950
device is usable, every entry point raises.  Nothing here imports or calls oracle/.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RELOC_LIB: developer switch used by tools/exp_*.py to time experimental builds of the same library; like the library's own
# switches it is honoured only under RELOC_DEV=1
LIB_PATH = (os.environ.get("RELOC_LIB") if os.environ.get("RELOC_DEV") == "1" else None) or os.path.join(_HERE, "csrc", "libreloc_hip.so")

c_ctx = C.c_void_p
i32, i64, u64, f32, f64 = C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double


class RelocError(RuntimeError):
    """Raised for every failure of the native library (the cv2 shim re-raises it as cv2.error)."""


class P:
    """A pointer argument (every pointer or array parameter of include/reloc.h but `reloc_ctx *`) that converts itself:
    a C-contiguous numpy array passes its data pointer and an out-parameter of outs() its address; None, an int address,
    byref(...), a c_void_p and a ctypes array pass as a plain c_void_p argument takes them.  A strided array raises
    RelocError: from ptr() and the checked view as it is, from a call of the raw library inside ctypes.ArgumentError,
    which is how ctypes reports whatever a from_param raises."""

    @classmethod
    def from_param(cls, a):
        if isinstance(a, np.ndarray):
            if not a.flags.c_contiguous:    # its base address with a dense byte count would read or write the wrong bytes
                raise RelocError(f"a pointer argument must be a C-contiguous array, got strides {a.strides} for shape {a.shape}")
            return C.c_void_p(a.ctypes.data)
        if isinstance(a, (i32, i64, u64, f32, f64)):
            return C.byref(a)
        return C.c_void_p.from_param(a)


def outs(*types):
    """fresh ctypes objects for the out-parameters of one call: pass them as they are, read their .value afterwards"""
    return tuple(t() for t in types)


# name -> (restype, argtypes); mirrors include/reloc.h one to one (tests/test_abi.py compares the types with the header).
# A pointer RETURN is a plain c_void_p.
SIGNATURES = {
    "reloc_last_error": (C.c_char_p, []),
    "reloc_device_count": (C.c_int, []),
    "reloc_create": (c_ctx, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "reloc_destroy": (None, [c_ctx]),
    "reloc_set_stream": (C.c_int, [c_ctx, P]),
    "reloc_sync": (C.c_int, [c_ctx]),
    "reloc_dev_alloc": (C.c_void_p, [c_ctx, i64]),
    "reloc_dev_free": (C.c_int, [c_ctx, P]),
    "reloc_h2d": (C.c_int, [c_ctx, P, P, i64]),
    "reloc_d2h": (C.c_int, [c_ctx, P, P, i64]),
    "reloc_timer_begin": (C.c_int, [c_ctx]),
    "reloc_timer_end": (C.c_int, [c_ctx, P]),
    "reloc_profile_enable": (C.c_int, [c_ctx, C.c_int]),
    "reloc_profile_get": (C.c_int, [c_ctx, C.c_int, P, P]),
    "reloc_gray_u8": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "reloc_orb_detect_compute": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P]),
    "reloc_orb_frame_dev": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "reloc_frame_desc_dev": (C.c_void_p, [c_ctx]),
    "reloc_frame_xy_dev": (C.c_void_p, [c_ctx]),
    "reloc_frame_count_dev": (C.c_void_p, [c_ctx]),
    "reloc_frame_debug_plane": (C.c_int, [c_ctx, C.c_int, C.c_int, P, P, P]),
    "reloc_orb_debug_levels": (C.c_int, [c_ctx, P, P, P]),
    "reloc_set_orb_mask": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int]),
    "reloc_get_orb_mask": (C.c_int, [c_ctx, P, P]),
    "reloc_orb_detect_compute_masked": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, P, C.c_int, C.c_int, P, P, P, P, P, P, P]),
    "reloc_orb_mask_level": (C.c_int, [c_ctx, C.c_int, P, P, P]),
    "reloc_set_orb_params": (C.c_int, [c_ctx, C.c_int, f64, C.c_int, C.c_int]),
    "reloc_get_orb_params": (C.c_int, [c_ctx, P, P, P, P]),
    "reloc_orb_detect_compute_params": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, P, C.c_int, C.c_int, C.c_int, f64, C.c_int,
                                                  C.c_int, P, P, P, P, P, P, P]),
    "reloc_record_frame": (C.c_int, [c_ctx, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P]),
    "reloc_depth_points": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, P, f32, f32, P, P]),
    "reloc_db_ratio_counts": (C.c_int, [c_ctx, P, C.c_int, f64, P]),
    "reloc_match_mutual": (C.c_int, [c_ctx, P, C.c_int, P, C.c_int, P, P, P, P]),
    "reloc_match_knn2": (C.c_int, [c_ctx, P, C.c_int, P, C.c_int, P, P]),
    "reloc_match_ratio": (C.c_int, [c_ctx, P, C.c_int, P, C.c_int, f64, P, P, P, P]),
    "reloc_set_match_policy": (C.c_int, [c_ctx, C.c_int, f64]),
    "reloc_get_match_policy": (C.c_int, [c_ctx, P, P]),
    "reloc_db_upload": (C.c_int, [c_ctx, P, P, P, P, i64]),
    "reloc_db_records": (i64, [c_ctx]),
    "reloc_db_rows": (i64, [c_ctx]),
    "reloc_db_counts_dev": (C.c_void_p, [c_ctx]),
    "reloc_db_match_counts": (C.c_int, [c_ctx, P, C.c_int, P]),
    "reloc_db_match_counts_dev": (C.c_int, [c_ctx, P, P, C.c_int, P]),
    "reloc_hamming_matrix": (C.c_int, [c_ctx, P, i64, P, i64, P]),
    "reloc_hamming_matrix_dev": (C.c_int, [c_ctx, P, i64, P, i64, P]),
    "reloc_pnp_score": (C.c_int, [c_ctx, P, P, C.c_int, P, C.c_int, P, f32, P, P]),
    "reloc_pnp_ransac": (C.c_int, [c_ctx, P, P, C.c_int, P, C.c_int, f32, f64, u64, P, P, P, P, P]),
    "reloc_pnp_debug_hypotheses": (C.c_int, [c_ctx, C.c_int, C.c_int, P, P, P]),
    "reloc_set_camera": (C.c_int, [c_ctx, P, P, P]),
    "reloc_set_distortion": (C.c_int, [c_ctx, P, C.c_int]),
    "reloc_get_distortion": (C.c_int, [c_ctx, P]),
    "reloc_undistort_points": (C.c_int, [c_ctx, P, C.c_int, P, P, P]),
    "reloc_pnp_score_dist": (C.c_int, [c_ctx, P, P, C.c_int, P, C.c_int, P, P, f32, P, P]),
    "reloc_pnp_ransac_dist": (C.c_int, [c_ctx, P, P, C.c_int, P, P, C.c_int, f32, f64, u64, P, P, P, P, P]),
    "reloc_set_clahe": (C.c_int, [c_ctx, f64, C.c_int, C.c_int]),
    "reloc_get_clahe": (C.c_int, [c_ctx, P, P, P]),
    "reloc_clahe_u8": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, f64, C.c_int, C.c_int, P]),
    "reloc_set_rectify_map": (C.c_int, [c_ctx, P, P, C.c_int, C.c_int]),
    "reloc_get_rectify_map": (C.c_int, [c_ctx, P, P]),
    "reloc_remap_u8": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "reloc_remap_u16": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, P, C.c_int, C.c_int, C.c_int, P]),
    "reloc_convert_maps": (C.c_int, [c_ctx, P, P, C.c_int, C.c_int, C.c_int, P, P]),
    "reloc_resize_u8": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_int, C.c_int, f64, f64, C.c_int]),
    "reloc_resize_u16": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, P, C.c_int, C.c_int, f64, f64]),
    "reloc_set_resize": (C.c_int, [c_ctx, C.c_int, C.c_int, C.c_int, C.c_int]),
    "reloc_get_resize": (C.c_int, [c_ctx, P, P, P, P]),
    "reloc_bayer_u8": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "reloc_set_bayer": (C.c_int, [c_ctx, C.c_int]),
    "reloc_get_bayer": (C.c_int, [c_ctx, P]),
    "reloc_cvt_gray_u8": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "reloc_yuv422_bgr_u8": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "reloc_set_pixel_format": (C.c_int, [c_ctx, C.c_int]),
    "reloc_get_pixel_format": (C.c_int, [c_ctx, P]),
    "reloc_set_stereo": (C.c_int, [c_ctx, f64, C.c_int, C.c_int, C.c_int, C.c_int]),
    "reloc_get_stereo": (C.c_int, [c_ctx, P, P, P, P, P]),
    "reloc_stereo_depth": (C.c_int, [c_ctx, P, P, C.c_int, C.c_int, C.c_int, P, C.c_int, f64, f64, C.c_int, C.c_int, C.c_int, C.c_int,
                                     P, P, P]),
    "reloc_record_frame_stereo": (C.c_int, [c_ctx, c_ctx, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P]),
    "reloc_tick_accumulate_stereo_dev": (C.c_int, [c_ctx, c_ctx, P, C.c_int, C.c_int, C.c_int, P, C.c_int]),
    "reloc_stereo_debug": (C.c_int, [c_ctx, P, P, P, P]),
    "reloc_stereo_depth_image": (C.c_int, [c_ctx, P, P, C.c_int, C.c_int, C.c_int, f64, f64, C.c_int, C.c_int, C.c_int, C.c_int,
                                           P, P, P]),
    "reloc_stereo_frame_depth": (C.c_int, [c_ctx, c_ctx, P, P, C.c_int, C.c_int, C.c_int, P, P, P]),
    "reloc_stereo_frame_points": (C.c_int, [c_ctx, c_ctx, P, P, C.c_int, C.c_int, C.c_int, C.c_int, f32, f32, P, P]),
    "reloc_stereo_dense_debug": (C.c_int, [c_ctx, P, P, P, P, P]),
    "reloc_filter_speckles": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "reloc_set_stereo_speckle": (C.c_int, [c_ctx, C.c_int, C.c_int]),
    "reloc_get_stereo_speckle": (C.c_int, [c_ctx, P, P]),
    "reloc_set_stereo_sgm": (C.c_int, [c_ctx, C.c_int, C.c_int, C.c_int]),
    "reloc_get_stereo_sgm": (C.c_int, [c_ctx, P, P, P]),
    "reloc_stereo_sgm_image": (C.c_int, [c_ctx, P, P, C.c_int, C.c_int, C.c_int, f64, f64, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, P, P, P]),
    "reloc_stereo_sgm_debug": (C.c_int, [c_ctx, P, P, P, P]),
    "reloc_set_stereo_cost": (C.c_int, [c_ctx, C.c_int]),
    "reloc_get_stereo_cost": (C.c_int, [c_ctx, P]),
    "reloc_stereo_depth_cost": (C.c_int, [c_ctx, P, P, C.c_int, C.c_int, C.c_int, P, C.c_int, f64, f64, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, P, P, P]),
    "reloc_stereo_image_cost": (C.c_int, [c_ctx, P, P, C.c_int, C.c_int, C.c_int, f64, f64, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_int, P, P, P]),
    "reloc_census": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, P]),
    "reloc_occ_configure": (C.c_int, [c_ctx, f64, f64, f64, C.c_int, C.c_int, f64, f64, C.c_int]),
    "reloc_occ_integrate_points": (C.c_int, [c_ctx, P, C.c_int, P, P]),
    "reloc_occ_integrate_depth": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, P, f32, f32, P, P]),
    "reloc_occ_integrate_stereo_dev": (C.c_int, [c_ctx, C.c_int, f32, f32, P, P]),
    "reloc_occ_read": (C.c_int, [c_ctx, P, P, P]),
    "reloc_corr_set_map": (C.c_int, [c_ctx, P, C.c_int, C.c_int, f64, f64, f64, C.c_int]),
    "reloc_corr_set_map_from_occ": (C.c_int, [c_ctx, C.c_int]),
    "reloc_corr_configure": (C.c_int, [c_ctx, P, C.c_int, f64, f64, f64, C.c_int]),
    "reloc_corr_match_points": (C.c_int, [c_ctx, P, C.c_int, P, f64, f64, P, P]),
    "reloc_corr_match_depth": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, P, f32, f32, P, f64, f64, P, P]),
    "reloc_corr_match_stereo_dev": (C.c_int, [c_ctx, C.c_int, f32, f32, P, f64, f64, P, P]),
    "reloc_corr_read_map": (C.c_int, [c_ctx, P, P, P]),
    "reloc_route_set_map": (C.c_int, [c_ctx, P, C.c_int, C.c_int, P, C.c_int, C.c_int, P, P]),
    "reloc_route_set_map_from_occ": (C.c_int, [c_ctx, P, C.c_int, C.c_int, P, P]),
    "reloc_route_read_clearance": (C.c_int, [c_ctx, P, P, P]),
    "reloc_route_clearance_at": (C.c_int, [c_ctx, P, C.c_int, P]),
    "reloc_route_set_costmap": (C.c_int, [c_ctx, P, C.c_int, C.c_int]),
    "reloc_route_search": (C.c_int, [c_ctx, C.c_int, C.c_int, P, C.c_int, P, C.c_int, P]),
    "reloc_obs_set_filter": (C.c_int, [c_ctx, C.c_int, C.c_int, f32, f32, C.c_int, f64, f64, f64, f32]),
    "reloc_obs_get_filter": (C.c_int, [c_ctx, P, P, P, P, P, P, P, P, P]),
    "reloc_obs_filter_depth": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, P, P]),
    "reloc_obs_profile_depth": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, f32, f32, C.c_int, C.c_int, f32, C.c_int, P, P]),
    "reloc_obs_profile_stereo_dev": (C.c_int, [c_ctx, C.c_int, f32, f32, C.c_int, C.c_int, f32, C.c_int, P, P]),
    "reloc_obs_grid_configure": (C.c_int, [c_ctx, C.c_int, f64, f32, f32, f32, f32, C.c_int, f32, f32, C.c_int, C.c_int, C.c_int]),
    "reloc_obs_grid_update_depth": (C.c_int, [c_ctx, C.c_int, C.c_int, P, C.c_int, C.c_int, C.c_int, P, C.c_int]),
    "reloc_obs_grid_update_stereo_dev": (C.c_int, [c_ctx, C.c_int, C.c_int, P, C.c_int]),
    "reloc_obs_grid_profile": (C.c_int, [c_ctx, P, C.c_int, f64, P]),
    "reloc_obs_grid_read": (C.c_int, [c_ctx, P, P, P, P, P]),
    "reloc_morph_rect": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "reloc_tick_debug": (C.c_int, [c_ctx, P, P, P, P, P, P, P]),
    "reloc_tick_debug_matches": (C.c_int, [c_ctx, C.c_int, P, P, P, P, P, P]),
    "reloc_debug_local_candidates": (C.c_int, [c_ctx, P, C.c_int, P, P]),
    "reloc_debug_rank_counts": (C.c_int, [c_ctx, P, C.c_int, i64, C.c_int, i64, C.c_int, C.c_int, P, P, P, P]),
    "reloc_tick": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, P, C.c_int, u64, P, P, P, P, P, P]),
    "reloc_get_params": (C.c_int, [c_ctx, P]),
    "reloc_set_params": (C.c_int, [c_ctx, P]),
    "reloc_db_reserve": (C.c_int, [c_ctx, i64, i64]),
    "reloc_db_append": (C.c_int, [c_ctx, P, P, P, C.c_int, P, P]),
    "reloc_db_select": (C.c_int, [c_ctx, C.c_int]),
    "reloc_db_share": (C.c_int, [c_ctx, c_ctx]),
    "reloc_d2d": (C.c_int, [c_ctx, P, P, i64]),
    "reloc_host_alloc": (C.c_void_p, [i64]),
    "reloc_host_free": (C.c_int, [P]),
    "reloc_get_stream": (C.c_void_p, [c_ctx]),
    "reloc_tick_result_dev": (C.c_void_p, [c_ctx]),
    "reloc_tick_result_to": (C.c_int, [c_ctx, P]),
    "reloc_set_exclusive": (C.c_int, [c_ctx, C.c_int]),
    "reloc_db_fetch": (C.c_int, [c_ctx, i64, P, P, P, P, P, P]),
    "reloc_tick_result_ex": (C.c_int, [c_ctx, P, P, P, P, P, P, P, P]),
    "reloc_tick_accumulate_dev": (C.c_int, [c_ctx, P, C.c_int, C.c_int, P, C.c_int]),
    "reloc_accumulate_result": (C.c_int, [c_ctx, P, P, P]),
    "reloc_tick_dev": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, P, C.c_int, u64]),
    "reloc_tick_batch_dev": (C.c_int, [P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, C.c_int, P]),
    "reloc_shard_scan_batch_dev": (C.c_int, [P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, C.c_int, i64, P]),
    "reloc_shard_merge_dev": (C.c_int, [c_ctx, P, C.c_int, i64, C.c_int, C.c_int, i64, i64, P, P, P]),
    "reloc_shard_solve_batch_dev": (C.c_int, [P, C.c_int, P, C.c_int, P, P, P]),
    "reloc_tick_result": (C.c_int, [c_ctx, P, P, P, P, P, P]),
    "reloc_tick_wait": (C.c_int, [c_ctx]),
    "reloc_tick_scan_dev": (C.c_int, [c_ctx, P, C.c_int, C.c_int, C.c_int, P, P, P, C.c_int]),
    "reloc_tick_solve_dev": (C.c_int, [c_ctx, P, C.c_int, P, C.c_int, u64]),
}

# the entry points whose int is a status (0, or a RELOC_E_* code with reloc_last_error set): every int but the one count
STATUS = frozenset(name for name, (res, _) in SIGNATURES.items() if res is C.c_int) - {"reloc_device_count"}


class RelocParams(C.Structure):
    """mirror of `reloc_params` (include/reloc.h)"""
    _fields_ = [("nfeatures", i32), ("max_candidates", i32), ("min_matches", i32), ("min_inliers", i32),
                ("ransac_iterations", i32), ("global_max_candidates", i32), ("global_min_inliers", i32),
                ("accum_min_kpts", i32), ("candidate_radius_m", f64), ("heading_tol_deg", f64), ("reproj_max_px", f64),
                ("ransac_reproj_px", f64), ("ransac_confidence", f64), ("consistency_m", f64),
                ("global_reproj_max_px", f64), ("accum_min_dist_m", f64), ("accum_depth_min_m", f64),
                ("accum_depth_max_m", f64), ("gray_coeff_bits", i32), ("reserved0", i32)]


_lib = _api = None


def _one_hip_runtime():
    """A process must run on ONE HIP runtime.  libreloc_hip.so needs `libamdhip64.so.7` and would take /opt/rocm's;
    PyTorch-ROCm ships its own copy under torch/lib with the same SONAME.  Whichever is mapped first serves both -- and
    torch on /opt/rocm's runtime reports "No HIP GPUs are available".  So, when torch is installed but not imported yet,
    its bundled runtime is mapped here first (without importing torch): afterwards the import order of torch and this
    package does not matter.  Without torch the library uses /opt/rocm's runtime.  RELOC_HIP_RUNTIME=system skips this."""
    import sys
    if os.environ.get("RELOC_HIP_RUNTIME") == "system" or "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(rt):
            C.CDLL(rt, mode=C.RTLD_GLOBAL)
    except (ImportError, OSError, ValueError):      # no torch, or a CPU-only torch: /opt/rocm's runtime is used
        pass


def load(strict: bool = True):
    """Loads the shared library and binds every symbol of include/reloc.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RelocError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc, gfx950).  There is no CPU fallback.")
    _one_hip_runtime()
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise RelocError(f"cannot load {LIB_PATH}: {e}") from e
    missing = []
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing and strict:
        raise RelocError(f"{LIB_PATH} lacks symbols declared in include/reloc.h: {missing}")
    _lib = lib
    return lib


class _Api:
    """see api()"""

    def __init__(self, lib):
        for name in SIGNATURES:
            fn = getattr(lib, name, None)
            if fn is not None:
                setattr(self, name, self._checked(fn, name) if name in STATUS else fn)

    @staticmethod
    def _checked(fn, name):
        def call(*args):
            try:
                rc = fn(*args)
            except C.ArgumentError as e:        # ctypes' wrapping of what a from_param raised: P's RelocError, a TypeError
                raise RelocError(f"{name}: {e}") from e
            if rc != 0:
                check(rc, name)
        return call


def api():
    """The checked view of the library load() returns: the same entry points as attributes, but one of STATUS raises
    RelocError on a non-zero code -- with check()'s text -- or on an argument that does not convert, and returns nothing.
    Those that return a pointer, a count, a string or nothing are load()'s own functions."""
    global _api
    if _api is None:
        _api = _Api(load())
    return _api


def last_error() -> str:
    return load().reloc_last_error().decode("utf-8", "replace")


def check(rc: int, what: str = ""):
    if rc != 0:
        raise RelocError(f"{what or 'libreloc_hip'} failed (code {rc}): {last_error()}")


def ptr(a):
    """void* of a C-contiguous numpy array (or None), for calls of the raw library that spell the conversion out"""
    return C.c_void_p(a) if isinstance(a, int) else P.from_param(a)


def u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)
