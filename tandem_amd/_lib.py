"""ctypes loader for libdr_mi355x.so (the C ABI in include/dr_mi355x.h).

There is no CPU fallback: if the HIP library is missing the import of any operator fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DR_MI355X_LIB: load another build of the same C ABI (used for within-box A/B timing of kernel variants)
LIB_PATH = os.environ.get("DR_MI355X_LIB") or os.path.join(_HERE, "libdr_mi355x.so")

DR_OK = 0
ERR_NAMES = {1: "DR_ERR_ARG", 2: "DR_ERR_PROTOCOL", 3: "DR_ERR_DEVICE", 4: "DR_ERR_IO", 5: "DR_ERR_CAPACITY",
             6: "DR_ERR_UNSUPPORTED"}


class DrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERR_NAMES.get(code, code), msg))
        self.code = code


class FusionOptions(C.Structure):
    """struct DrFusionOptions, dr_fusion.h:18-36 (same field order as drf_options_t)."""
    _fields_ = [("voxel_size", C.c_float), ("num_buckets", C.c_int), ("bucket_size", C.c_int),
                ("num_blocks", C.c_int), ("block_size", C.c_int), ("max_sdf_weight", C.c_int),
                ("truncation_distance", C.c_float), ("max_sensor_depth", C.c_float),
                ("min_sensor_depth", C.c_float), ("num_render_streams", C.c_int),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("height", C.c_int), ("width", C.c_int)]


_lib = None
u8p, f32p, vp = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.c_void_p
f64p = C.POINTER(C.c_double)

SIGNATURES = {
    "dr_last_error": (C.c_char_p, []),
    "dr_version": (C.c_char_p, []),
    "drm_create": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(vp)]),
    "drm_destroy": (None, [vp]),
    "drm_call_async": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(u8p), f32p, C.POINTER(f32p),
                                 C.c_float, C.c_float, C.c_float]),
    "drm_ready": (C.c_int, [vp]),
    "drm_wait": (C.c_int, [vp]),
    "drm_get_result": (C.c_int, [vp, f32p, f32p, f32p, f32p]),
    "drm_get_result_view": (C.c_int, [vp, C.POINTER(f32p), C.POINTER(f32p), C.POINTER(f32p), C.POINTER(f32p)]),
    "drm_host_alloc": (vp, [C.c_size_t]),
    "drm_host_free": (None, [vp]),
    "drm_upload": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(u8p), f32p, C.POINTER(f32p),
                             C.c_float, C.c_float, C.c_float]),
    "drm_forward": (C.c_int, [vp, C.c_int, f32p]),
    "drm_download": (C.c_int, [vp, f32p, f32p, f32p, f32p]),
    "drm_get_stage_output": (C.c_int, [vp, C.c_int, f32p, f32p]),
    "drm_get_tensor": (C.c_int, [vp, C.c_char_p, f32p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "drm_profile": (C.c_int, [vp, C.c_char_p, C.c_size_t, f32p, C.c_int, C.POINTER(C.c_int)]),
    "drm_work": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "drm_debug_conv": (C.c_int, [C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, f32p, C.c_int,
                                 f32p, C.POINTER(C.c_int)]),
    "drm_debug_tail": (C.c_int, [C.c_int, f32p, f32p, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p]),
    "drm_debug_regress": (C.c_int, [C.c_int, f32p, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, f32p, f32p,
                                    C.c_char_p]),
    "drm_debug_prob_regress": (C.c_int, [C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                         f32p, f32p, f32p, C.c_char_p]),
    "drm_debug_edge_filter": (C.c_int, [C.c_int, f32p, f32p, C.c_int, C.c_int, f32p, C.c_uint, f32p, f32p, f32p, C.POINTER(C.c_uint)]),
    "drm_autotune":(C.c_int, [vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "drm_set_view_shard": (C.c_int, [vp, C.c_int]),
    "drm_forward_phase": (C.c_int, [vp, C.c_int]),
    "drm_comm_available": (C.c_int, []),
    "drm_comm_unique_id": (C.c_int, [u8p]),
    "drm_comm_init": (C.c_int, [vp, C.c_int, C.c_int, u8p]),
    "drm_comm_destroy": (C.c_int, [vp]),
    "drm_comm_count": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "drm_device_tensor": (C.c_int, [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t)]),
    "drf_create": (C.c_int, [C.POINTER(FusionOptions), C.c_int, C.POINTER(vp)]),
    "drf_destroy": (None, [vp]),
    "drf_integrate_scan_async": (C.c_int, [vp, u8p, f32p, f32p]),
    "drf_render_async": (C.c_int, [vp, C.POINTER(f32p), C.c_int]),
    "drf_get_render_result": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(f32p), C.c_int]),
    "drf_extract_mesh_async": (C.c_int, [vp, f32p, f32p]),
    "drf_get_mesh_sync": (C.c_int, [vp, C.c_size_t, C.POINTER(C.c_size_t), f32p, f32p]),
    "drf_mesh_num_triangles": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
    "drf_save_mesh": (C.c_int, [vp, C.c_char_p, f32p, f32p]),
    "drf_get_render_device": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)]),
    "drf_synchronize": (C.c_int, [vp]),
    "drf_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_export_blocks": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int32), u8p, C.POINTER(C.c_int)]),
    "drf_fast_div_status": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "drf_test_combine": (C.c_int, [vp, C.c_size_t, u8p, u8p, C.c_int, u8p]),
    "drf_integrate_device": (C.c_int, [vp, vp, vp, f32p]),
    "drt_create": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(vp)]),
    "drt_destroy": (None, [vp]),
    "drt_set_k": (C.c_int, [vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]),
    "drt_init": (C.c_int, [vp, C.c_int]),
    "drt_set_reference": (C.c_int, [vp, C.c_int, f32p, f32p, f32p, f32p, C.c_float, f64p]),
    "drt_set_new": (C.c_int, [vp, f32p]),
    "drt_calc_res": (C.c_int, [vp, f64p, C.c_float, f64p, C.c_float, f64p, f64p]),
    "drt_calc_g": (C.c_int, [vp, f64p, f64p, C.c_float, f64p, f64p]),
    "drt_append_dense_reference": (C.c_int, [vp, vp, f32p, f32p, C.c_int, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int)]),
    "drt_synchronize": (C.c_int, [vp]),
    "drt_start_timing": (C.c_int, [vp]),
    "drt_end_timing_ms": (C.c_int, [vp, C.POINTER(C.c_float)]),
    "drt_get_points": (C.c_int, [vp, f32p, f32p, f32p, f32p, C.c_int, C.POINTER(C.c_int)]),
    "drt_get_warped": (C.c_int, [vp, C.c_int, f32p, C.c_int]),
    "drt_get_zbuffer": (C.c_int, [vp, f32p]),
    "dr_device_alloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(vp)]),
    "dr_device_free": (C.c_int, [vp]),
    "dr_memcpy_d2d": (C.c_int, [vp, vp, C.c_size_t]),
    "dr_memcpy_h2d": (C.c_int, [vp, vp, C.c_size_t]),
    "dr_memcpy_d2h": (C.c_int, [vp, vp, C.c_size_t]),
    "dr_guard_set": (C.c_int, [C.c_size_t]),
    "dr_guard_check": (C.c_int, [C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    "dr_guard_clear": (C.c_int, []),
    "drm_set_feature_cache": (C.c_int, [vp, C.c_int]),
    "drm_feature_cache_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_bench_sequence": (C.c_int, [vp, vp, vp, f32p, C.c_int, C.c_int, f32p]),
    "drf_visited_blocks": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_bench_render_host": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp)]),
    "drf_bench_integrate": (C.c_int, [vp, vp, vp, f32p, C.c_int, f32p, f32p]),
    "drf_streaming_min_radius": (C.c_int, [C.POINTER(FusionOptions), f32p]),
    "drf_set_streaming": (C.c_int, [vp, C.c_float, C.c_size_t]),
    "drf_stream_out_region": (C.c_int, [vp, f32p, f32p]),
    "drf_stream_in_region": (C.c_int, [vp, f32p, f32p]),
    "drf_streaming_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_export_host_blocks": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int32), u8p, C.POINTER(C.c_int)]),
    "drf_set_render_scope": (C.c_int, [vp, C.c_int, C.c_size_t]),
    "drf_render_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_set_render_bands": (C.c_int, [vp, C.c_int]),
    "drf_render_band_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_set_mesh_scope": (C.c_int, [vp, C.c_int]),
    "drf_mesh_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_extract_mesh_update_async": (C.c_int, [vp, f32p, f32p]),
    "drf_mesh_update_size": (C.c_int, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "drf_get_mesh_update_sync": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_size_t), f32p, f32p, C.POINTER(C.c_int)]),
    "drf_mesh_update_reset": (C.c_int, [vp]),
    "drf_mesh_update_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_map_info": (C.c_int, [C.c_char_p, f32p, C.POINTER(C.c_uint64)]),
    "drf_save_map": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "drf_load_map": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "drf_merge_map": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "drf_merge_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_transform_map": (C.c_int, [vp, C.c_char_p, f32p, C.c_char_p, C.c_size_t]),
    "drf_transform_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_align_system": (C.c_int, [vp, C.c_char_p, C.c_char_p, f32p, C.c_void_p, f64p, C.POINTER(C.c_uint64)]),
    "drf_align_map": (C.c_int, [vp, C.c_char_p, C.c_char_p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_align_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_locate_system": (C.c_int, [vp, f32p, f32p, C.c_void_p, f64p, C.POINTER(C.c_uint64)]),
    "drf_locate_frame": (C.c_int, [vp, f32p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_locate_system_device": (C.c_int, [vp, C.c_void_p, f32p, C.c_void_p, f64p, C.POINTER(C.c_uint64)]),
    "drf_locate_frame_device": (C.c_int, [vp, C.c_void_p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_locate_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_set_locate_scope": (C.c_int, [vp, C.c_int, C.c_size_t]),
    "drf_locate_stage_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_track_system": (C.c_int, [vp, f32p, f32p, f32p, f32p, C.c_void_p, f64p, C.POINTER(C.c_uint64)]),
    "drf_track_frame": (C.c_int, [vp, f32p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_track_system_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, f32p, f32p, C.c_void_p, f64p, C.POINTER(C.c_uint64)]),
    "drf_track_frame_device": (C.c_int, [vp, C.c_void_p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_track_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_track_colour_system": (C.c_int, [vp, C.c_void_p, f32p, C.c_void_p, f32p, f32p, f32p, C.c_void_p, f64p, C.POINTER(C.c_uint64)]),
    "drf_track_colour_frame": (C.c_int, [vp, C.c_void_p, f32p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_track_colour_system_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, f32p, f32p, C.c_void_p, f64p, C.POINTER(C.c_uint64)]),
    "drf_track_colour_frame_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_track_colour_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_track_reduce": (C.c_int, [vp, C.c_int, C.c_float, C.c_void_p, f32p, C.c_void_p, f32p]),
    "drf_track_reduce_device": (C.c_int, [vp, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "drf_track_pyramid_system": (C.c_int, [vp, C.c_int, C.c_void_p, f32p, C.c_void_p, f32p, f32p, f32p, C.c_void_p, f64p, C.POINTER(C.c_uint64)]),
    "drf_track_pyramid_system_device": (C.c_int, [vp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, f32p, f32p, C.c_void_p, f64p, C.POINTER(C.c_uint64)]),
    "drf_track_pyramid_frame": (C.c_int, [vp, C.c_void_p, f32p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_track_pyramid_frame_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_track_pyramid_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_track_pyramid_level_stats": (C.c_int, [vp, C.c_int, C.POINTER(C.c_uint64)]),
    "drf_track_exposure_system": (C.c_int, [vp, C.c_int, C.c_void_p, f32p, C.c_void_p, f32p, f32p, f32p, C.c_double, C.c_double, C.c_void_p, f64p, C.POINTER(C.c_uint64)]),
    "drf_track_exposure_system_device": (C.c_int, [vp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, f32p, f32p, C.c_double, C.c_double, C.c_void_p, f64p,
                                                   C.POINTER(C.c_uint64)]),
    "drf_track_exposure_frame": (C.c_int, [vp, C.c_void_p, f32p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_track_exposure_frame_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "drf_track_exposure_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_track_exposure_level_stats": (C.c_int, [vp, C.c_int, C.POINTER(C.c_uint64)]),
    "drf_score_poses": (C.c_int, [vp, f32p, f32p, C.c_size_t, C.c_void_p, f64p, C.POINTER(C.c_uint32), f64p]),
    "drf_score_poses_device": (C.c_int, [vp, C.c_void_p, f32p, C.c_size_t, C.c_void_p, f64p, C.POINTER(C.c_uint32), f64p]),
    "drf_search_frame": (C.c_int, [vp, f32p, f32p, C.c_size_t, f64p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, f32p, C.c_void_p, f64p]),
    "drf_search_frame_device": (C.c_int, [vp, C.c_void_p, f32p, C.c_size_t, f64p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, f32p, C.c_void_p, f64p]),
    "drf_search_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_set_search_scope": (C.c_int, [vp, C.c_int, C.c_size_t]),
    "drf_search_stage_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drf_score_colour_poses": (C.c_int, [vp, C.c_void_p, f32p, f32p, C.c_size_t, C.c_void_p, f64p, f64p, C.POINTER(C.c_uint32), f64p]),
    "drf_score_colour_poses_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, f32p, C.c_size_t, C.c_void_p, f64p, f64p, C.POINTER(C.c_uint32), f64p]),
    "drf_search_colour_frame": (C.c_int, [vp, C.c_void_p, f32p, f32p, C.c_size_t, f64p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, f32p, C.c_void_p, f64p]),
    "drf_search_colour_frame_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, f32p, C.c_size_t, f64p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, f32p, C.c_void_p,
                                                 f64p]),
}


class AlignOptions(C.Structure):
    """drf_align_options_t: a zero field means its default."""
    _fields_ = [("max_iters", C.c_int), ("min_weight", C.c_int), ("band", C.c_float), ("huber", C.c_float),
                ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("min_valid", C.c_double)]


class LocateOptions(C.Structure):
    """drf_locate_options_t: a zero field means its default."""
    _fields_ = [("max_iters", C.c_int), ("min_weight", C.c_int), ("step", C.c_int), ("band", C.c_float), ("huber", C.c_float),
                ("centre_depth", C.c_float), ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("min_valid", C.c_double)]


class TrackOptions(C.Structure):
    """drf_track_options_t: a zero field means its default."""
    _fields_ = [("max_renders", C.c_int), ("inner_iters", C.c_int), ("step", C.c_int), ("dist_max", C.c_float), ("max_jump", C.c_float),
                ("huber", C.c_float), ("centre_depth", C.c_float), ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("min_valid", C.c_double)]


class TrackColourOptions(C.Structure):
    """drf_track_colour_options_t: a zero field means its default."""
    _fields_ = [("track", TrackOptions), ("photo_weight", C.c_float)]


class TrackPyramidOptions(C.Structure):
    """drf_track_pyramid_options_t: a zero field means its default."""
    _fields_ = [("colour", TrackColourOptions), ("levels", C.c_int), ("coarse_renders", C.c_int)]


class TrackExposureOptions(C.Structure):
    """drf_track_exposure_options_t: a zero field means its default (offset_init is used as given)."""
    _fields_ = [("pyramid", TrackPyramidOptions), ("gain_init", C.c_float), ("offset_init", C.c_float), ("gain_min", C.c_float), ("gain_max", C.c_float),
                ("eps_gain", C.c_double), ("eps_offset", C.c_double)]


SEARCH_MAX_TOP = 32  # DRF_SEARCH_MAX_TOP


class ScoreOptions(C.Structure):
    """drf_score_options_t: a zero field means its default."""
    _fields_ = [("step", C.c_int), ("min_weight", C.c_int), ("band", C.c_float), ("huber", C.c_float), ("outside_cost", C.c_float),
                ("unobserved_cost", C.c_float)]


class SearchOptions(C.Structure):
    """drf_search_options_t: a zero field means its default."""
    _fields_ = [("score", ScoreOptions), ("trans_step", C.c_float), ("half", C.c_int * 3), ("top_k", C.c_int), ("score_only", C.c_int),
                ("accept_valid", C.c_double)]


class SearchEntryStruct(C.Structure):
    """drf_search_entry_t."""
    _fields_ = [("index", C.c_uint64), ("score", C.c_double), ("cost", C.c_double), ("counts", C.c_uint32 * 4), ("track_status", C.c_int),
                ("locate_status", C.c_int), ("samples", C.c_uint64), ("valid", C.c_uint64), ("located_cost", C.c_double), ("T", C.c_double * 16)]


class SearchResultStruct(C.Structure):
    """drf_search_result_t."""
    _fields_ = [("status", C.c_int), ("n_entries", C.c_int), ("winner", C.c_int), ("refined", C.c_int), ("n_candidates", C.c_uint64),
                ("entries", SearchEntryStruct * SEARCH_MAX_TOP)]


class ScoreColourOptions(C.Structure):
    """drf_score_colour_options_t: a zero field means its default."""
    _fields_ = [("score", ScoreOptions), ("photo_weight", C.c_float), ("photo_cap", C.c_float)]


class SearchColourOptions(C.Structure):
    """drf_search_colour_options_t: a zero field means its default."""
    _fields_ = [("search", SearchOptions), ("photo_weight", C.c_float), ("photo_cap", C.c_float)]


class SearchColourEntryStruct(C.Structure):
    """drf_search_colour_entry_t: drf_search_entry_t's fields, then the colour sums."""
    _fields_ = SearchEntryStruct._fields_ + [("photo", C.c_double), ("final_score", C.c_double), ("final_photo", C.c_double)]


class SearchColourResultStruct(C.Structure):
    """drf_search_colour_result_t."""
    _fields_ = [("status", C.c_int), ("n_entries", C.c_int), ("winner", C.c_int), ("refined", C.c_int), ("n_candidates", C.c_uint64),
                ("entries", SearchColourEntryStruct * SEARCH_MAX_TOP)]


class AlignResultStruct(C.Structure):
    """drf_align_result_t."""
    _fields_ = [("T", C.c_double * 16), ("sums", C.c_double * 28), ("samples", C.c_uint64), ("valid0", C.c_uint64), ("valid", C.c_uint64),
                ("cost0", C.c_double), ("cost", C.c_double), ("iterations", C.c_int), ("status", C.c_int)]


class ExposureResultStruct(C.Structure):
    """drf_exposure_result_t."""
    _fields_ = [("pose", AlignResultStruct), ("gain", C.c_double), ("offset", C.c_double), ("ext", C.c_double * 17), ("photometric", C.c_uint64), ("held", C.c_uint64)]


HOOKS_LIB_PATH = os.path.join(_HERE, "libdr_mi355x_hooks.so")  # the PARITY build (-DDR_PARITY_HOOKS): superseded kernel generations selectable
_loaded = {}


def switch(path=None):
    """Make `path` (default: the product library) the library every operator object created from now on talks to.  Test
    infrastructure: the -m gpu cases that compare kernel generations switch to HOOKS_LIB_PATH for their duration (tests/conftest.py::
    parity_hooks).  Objects created before a switch must be closed first: a handle belongs to the library that made it."""
    global _lib, LIB_PATH
    LIB_PATH = path or os.environ.get("DR_MI355X_LIB") or os.path.join(_HERE, "libdr_mi355x.so")
    _lib = _loaded.get(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise ImportError("tandem_amd: %s not built -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError = ABI/header mismatch: fail loudly
            fn.restype, fn.argtypes = res, args
        _lib = _loaded[LIB_PATH] = L
    return _lib


def check(code):
    if code != DR_OK:
        raise DrError(code, lib().dr_last_error().decode(errors="replace"))


def fptr(a):
    return a.ctypes.data_as(f32p)
