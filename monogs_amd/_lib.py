"""ctypes binding of libmonogs_raster.so (the C ABI declared in include/monogs_raster.h).

There is no fallback: if the library is missing, stale or fails to load, importing the product
path raises.  The library is built in-tree (monogs_amd/lib/) by ``__graft_entry__.build()`` or
``make -C monogs_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGS_LIB_PATH") or os.path.join(_HERE, "lib", "libmonogs_raster.so")   # (override: kernel experiments)
ABI_VERSION = 30
FLAG_EXCLUSIVE_DEVICE = 1          # MGS_FLAG_* bits of mgs_camera.flags (include/monogs_raster.h)
FLAG_INTRINSICS_GRAD = 2

c_float_p = C.c_void_p   # device pointers travel as integers (tensor.data_ptr())


class MgsCamera(C.Structure):
    _fields_ = [
        ("image_height", C.c_int32), ("image_width", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32), ("scale_dim", C.c_int32), ("flags", C.c_int32),
        ("bg", C.c_void_p), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p),
        ("projmatrix_raw", C.c_void_p), ("campos", C.c_void_p),
    ]


class MgsTiming(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "preprocess_ms", "depth_sort_ms", "scan_ms", "duplicate_ms", "sort_ms", "ranges_ms", "blend_fwd_ms",
        "blend_bwd_ms", "geom_bwd_ms")]

    def as_dict(self):
        return {n: float(getattr(self, n)) for n, _ in self._fields_}


class MgsKeyframeParams(C.Structure):
    _fields_ = [("K", C.c_int32), ("window_size", C.c_int32), ("window_full", C.c_int32), ("check_overlap", C.c_int32),
                ("kf_interval", C.c_int32), ("frames_since_last_kf", C.c_int32),
                ("kf_translation", C.c_float), ("kf_min_translation", C.c_float), ("kf_overlap", C.c_float),
                ("kf_cutoff", C.c_float), ("n_dont_touch", C.c_int32)]


class MgsFramePrepare(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb_u8", C.c_void_p), ("map_x", C.c_void_p), ("map_y", C.c_void_p),
                ("depth_u16", C.c_void_p), ("depth_scale", C.c_double), ("segmentation", C.c_void_p),
                ("masked_ids", C.c_uint32 * 8), ("rgb_out", C.c_void_p), ("depth_out", C.c_void_p), ("mask_out", C.c_void_p),
                ("grad_mask_out", C.c_void_p), ("intensity_out", C.c_void_p), ("edge_threshold", C.c_float), ("eps", C.c_float),
                ("scratch", C.c_void_p)]


class MgsStereo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "num_disparities", "block_size", "p1", "p2", "uniqueness_ratio",
                                         "disp12_max_diff", "pre_filter_cap")] + [("bf", C.c_double)] + [
        (n, C.c_void_p) for n in ("left_u8", "right_u8", "map_lx", "map_ly", "map_rx", "map_ry", "rgb_out", "disp16_out",
                                  "depth_out", "left_rect_out", "right_rect_out", "sum_out", "scratch")]


class MgsTsdfVolume(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_float * 3), ("voxel", C.c_float),
                ("tsdf", C.c_void_p), ("weight", C.c_void_p), ("r", C.c_void_p), ("g", C.c_void_p), ("b", C.c_void_p)]


class MgsTsdfFrame(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("depth", C.c_void_p), ("opacity", C.c_void_p), ("rgb", C.c_void_p),
                ("viewmatrix", C.c_void_p)] + [(n, C.c_float) for n in (
                    "fx", "fy", "cx", "cy", "trunc", "depth_min", "depth_max", "opacity_min", "max_weight")] + [("flags", C.c_int32)]


class MgsMeshRender(C.Structure):
    _fields_ = [("V", C.c_int32), ("T", C.c_int32)] + [(n, C.c_void_p) for n in (
        "vertices", "triangles", "colors", "face_labels", "viewmatrix")] + [("W", C.c_int32), ("H", C.c_int32)] + [
            (n, C.c_float) for n in ("fx", "fy", "cx", "cy", "near", "far")] + [("flags", C.c_int32), ("bg", C.c_float * 3)] + [
                (n, C.c_void_p) for n in ("depth", "tri_id", "rgb", "label", "status")]


class MgsPseudoDepthParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("init_mean", "init_sigma", "opacity_min", "sigma_in", "sigma_out")]


# symbol -> (restype, argtypes); exactly the declarations of include/monogs_raster.h
SIGNATURES = {
    "mgs_abi_version": (C.c_int, []),
    "mgs_last_error": (C.c_char_p, []),
    "mgs_geometry_bytes": (C.c_size_t, [C.c_int32]),
    "mgs_image_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "mgs_binning_bytes": (C.c_size_t, [C.c_uint64, C.c_int32, C.c_int32]),
    "mgs_backward_bytes": (C.c_size_t, [C.c_int32]),
    "mgs_forward_preprocess": (C.c_int, [C.POINTER(MgsCamera), C.c_int32] + [C.c_void_p] * 7
                               + [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint32),
                                  C.POINTER(MgsTiming), C.c_void_p]),
    "mgs_forward_capacity": (C.c_int, [C.POINTER(MgsCamera), C.c_int32] + [C.c_void_p] * 7 + [C.c_void_p] * 3 + [C.c_uint64]
                             + [C.c_void_p] * 7 + [C.POINTER(MgsTiming), C.c_void_p]),
    "mgs_forward_render": (C.c_int, [C.POINTER(MgsCamera), C.c_int32, C.c_uint64] + [C.c_void_p] * 8
                           + [C.POINTER(MgsTiming), C.c_void_p]),
    "mgs_debug_set_radix_spin_limit": (C.c_int, [C.c_uint32]),
    "mgs_debug_set_option": (C.c_int, [C.c_char_p, C.c_int64]),
    "mgs_binning_path": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "mgs_debug_sort_temp_bytes": (C.c_size_t, [C.c_uint64, C.c_int32]),
    "mgs_debug_sort_pairs": (C.c_int, [C.c_void_p] * 4 + [C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p]),
    "mgs_forward_render_capacity": (C.c_int, [C.POINTER(MgsCamera), C.c_int32, C.c_uint64] + [C.c_void_p] * 8
                                    + [C.POINTER(MgsTiming), C.c_void_p]),
    "mgs_backward": (C.c_int, [C.POINTER(MgsCamera), C.c_int32, C.c_uint64] + [C.c_void_p] * 7
                     + [C.c_void_p] * 4 + [C.c_void_p] * 4 + [C.c_void_p] * 9
                     + [C.c_void_p, C.c_int32, C.POINTER(MgsTiming), C.c_void_p]),
    "mgs_backward_tau": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "mgs_debug_scratch_field": (C.c_int, [C.c_char_p, C.c_int32, C.c_uint64, C.c_int32, C.c_int32,
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mgs_debug_blend_stats": (C.c_int, [C.POINTER(MgsCamera), C.c_int32, C.c_uint64] + [C.c_void_p] * 5),
    "mgs_debug_blend_mask_stats": (C.c_int, [C.POINTER(MgsCamera), C.c_int32, C.c_uint64] + [C.c_void_p] * 5),
    "mgs_features_forward": (C.c_int, [C.POINTER(MgsCamera), C.c_int32, C.c_int32, C.c_uint64] + [C.c_void_p] * 7
                             + [C.c_float, C.c_void_p]),
    "mgs_features_backward": (C.c_int, [C.POINTER(MgsCamera), C.c_int32, C.c_int32, C.c_uint64] + [C.c_void_p] * 5 + [C.c_void_p]),
    "mgs_label_scratch_bytes": (C.c_size_t, []),
    "mgs_label_prepare": (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 5),
    "mgs_label_loss_grads": (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 7),
    "mgs_label_confusion": (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 6),
    "mgs_viewer_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "mgs_viewer_ellipsoids": (C.c_int, [C.POINTER(MgsCamera), C.c_int32, C.c_uint64] + [C.c_void_p] * 3 + [C.c_float]
                              + [C.c_void_p] * 3),
    "mgs_viewer_lines": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "mgs_viewer_compose": (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3),
    "mgs_debug_valu_ceiling": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mgs_debug_set_blend_events": (C.c_int, [C.c_void_p] * 4),
    "mgs_debug_last_backward_split": (C.c_int, []),
    "mgs_debug_last_tile_sort_bands": (C.c_int, []),
    "mgs_debug_forward_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.POINTER(C.c_uint64)]),
    "mgs_mark_visible": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgs_loss_scratch_bytes": (C.c_size_t, []),
    "mgs_loss_forward": (C.c_int, [C.c_int32] * 4 + [C.c_float] + [C.c_void_p] * 9 + [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgs_loss_backward": (C.c_int, [C.c_int32] * 4 + [C.c_float] + [C.c_void_p] * 9
                          + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgs_loss_grads": (C.c_int, [C.c_int32] * 4 + [C.c_float] + [C.c_void_p] * 9 + [C.c_void_p] * 4),
    "mgs_ssim_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "mgs_ssim_forward": (C.c_int, [C.c_int32] * 5 + [C.c_float] * 2 + [C.c_void_p] * 5),
    "mgs_ssim_backward": (C.c_int, [C.c_int32] * 4 + [C.c_float] * 2 + [C.c_void_p] * 6),
    "mgs_refine_loss_forward": (C.c_int, [C.c_int32] * 2 + [C.c_float] + [C.c_void_p] * 5),
    "mgs_refine_loss_backward": (C.c_int, [C.c_int32] * 2 + [C.c_float] + [C.c_void_p] * 6),
    "mgs_refine_loss_grads": (C.c_int, [C.c_int32] * 2 + [C.c_float] + [C.c_void_p] * 5),
    "mgs_backproject": (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 6 + [C.c_float] * 4 + [C.c_void_p] * 6),
    "mgs_camera_setup": (C.c_int, [C.c_void_p] * 7),
    "mgs_pose_step": (C.c_int, [C.c_void_p] * 12 + [C.c_int32] + [C.c_float] * 7
                      + [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p] + [C.c_void_p] * 4 + [C.c_void_p]),
    "mgs_pose_step_batch": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)] + [C.c_float] * 7 + [C.c_int32, C.c_void_p]),
    "mgs_adam_step": (C.c_int, [C.c_int32] + [C.c_void_p] * 6 + [C.c_double] * 3 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgs_window_stats": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_void_p]),
    "mgs_window_apply": (C.c_int, [C.c_int32] + [C.c_void_p] * 7),
    "mgs_lr_schedule_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_void_p]),
    "mgs_densify_stats": (C.c_int, [C.c_int32] + [C.c_void_p] * 6),
    "mgs_sum_buffers": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_void_p]),
    "mgs_activate_forward": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "mgs_activate_backward": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 10),
    "mgs_knn_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "mgs_dist2_knn": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgs_median_scratch_bytes": (C.c_size_t, [C.c_uint64]),
    "mgs_masked_median": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float] + [C.c_void_p] * 4),
    "mgs_pseudo_depth_scratch_bytes": (C.c_size_t, [C.c_uint64]),
    "mgs_pseudo_depth": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(MgsPseudoDepthParams)] + [C.c_void_p] * 4),
    "mgs_covisibility": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgs_keyframe_decide": (C.c_int, [C.POINTER(MgsKeyframeParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p,
                                      C.c_void_p]),
    "mgs_metrics_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "mgs_image_metrics": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "mgs_grad_mask_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "mgs_grad_mask": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_float] + [C.c_void_p] * 4),
    "mgs_frame_prepare": (C.c_int, [C.POINTER(MgsFramePrepare), C.c_void_p]),
    "mgs_stereo_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "mgs_stereo_depth": (C.c_int, [C.POINTER(MgsStereo), C.c_void_p]),
    "mgs_tsdf_integrate": (C.c_int, [C.POINTER(MgsTsdfVolume), C.POINTER(MgsTsdfFrame), C.c_void_p]),
    "mgs_tsdf_extract_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "mgs_tsdf_extract_count": (C.c_int, [C.POINTER(MgsTsdfVolume), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgs_tsdf_extract_emit": (C.c_int, [C.POINTER(MgsTsdfVolume)] + [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32, C.c_void_p]),
    "mgs_nn_grid_min": (C.c_int32, []),
    "mgs_nn_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "mgs_nn_dist2": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4),
    "mgs_mesh_sample_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "mgs_mesh_sample": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_uint32] + [C.c_void_p] * 6),
    "mgs_mesh_mark_seen": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_float] * 4 + [C.c_void_p]
                           + [C.c_float] * 3 + [C.c_void_p, C.c_void_p]),
    "mgs_recon_metrics_scratch_bytes": (C.c_size_t, []),
    "mgs_recon_metrics": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgs_mesh_render_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "mgs_mesh_render": (C.c_int, [C.POINTER(MgsMeshRender), C.c_void_p, C.c_void_p]),
    "mgs_depth_l1_scratch_bytes": (C.c_size_t, []),
    "mgs_depth_l1": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgs_object_motion_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "mgs_object_transform_forward": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 9),
    "mgs_object_transform_backward": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 12),
    "mgs_pose_tangent_bytes": (C.c_size_t, [C.c_int32]),
    "mgs_pose_jacobian": (C.c_int, [C.POINTER(MgsCamera), C.c_int32, C.c_uint64] + [C.c_void_p] * 11),
    "mgs_gn_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "mgs_gn_normal_equations": (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 10 + [C.c_float] * 2 + [C.c_void_p] * 3),
    "mgs_pose_gn_step": (C.c_int, [C.c_void_p] * 5 + [C.c_float] * 5 + [C.c_void_p, C.c_int32] + [C.c_void_p] * 6),
}

_lib = None


class MonoGSNativeError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle.  Raises if the HIP library is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MonoGSNativeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C monogs_amd/csrc`.  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    if lib.mgs_abi_version() != ABI_VERSION:
        raise MonoGSNativeError(f"ABI mismatch: library {lib.mgs_abi_version()} vs binding {ABI_VERSION}; rebuild")
    # measurement knobs for A/B runs of whole programs (tools/, bench.py): MGS_DEBUG_OPTIONS="name=value,name=value"
    # -> mgs_debug_set_option at load time (read here, once; nothing on the launch path consults the environment)
    for kv in filter(None, os.environ.get("MGS_DEBUG_OPTIONS", "").split(",")):
        k, _, v = kv.partition("=")
        if lib.mgs_debug_set_option(k.strip().encode(), int(v)) != 0:
            raise MonoGSNativeError(f"MGS_DEBUG_OPTIONS: {lib.mgs_last_error().decode()}")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().mgs_last_error().decode("utf-8", "replace")
        # argument errors mirror the upstream extension's Python exceptions
        raise Exception(msg) if rc == 1 else MonoGSNativeError(f"{what}: {msg}")
