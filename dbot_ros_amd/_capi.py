"""ctypes binding of librbsensor_mi355x.so (include/rbsensor_mi355x.h).

The library is the product; this module only declares its prototypes.  Loading fails loudly
when the shared object has not been built (``python -c 'import __graft_entry__ as g; g.build()'``
or ``make -C dbot_ros_amd/csrc``) -- there is no Python or CPU fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RBS_LIB_PATH selects an alternative build of the SAME library (kernel tuning experiments)
LIB_PATH = os.environ.get("RBS_LIB_PATH") or os.path.join(_HERE, "lib", "librbsensor_mi355x.so")

RBS_ABI_VERSION = 2
RBS_OK = 0
RBS_ERR_INVALID_ARGUMENT = -1
RBS_ERR_NO_DEVICE = -2
RBS_ERR_OUT_OF_MEMORY = -3
RBS_ERR_HIP = -4
RBS_ERR_UNSUPPORTED = -5
RBS_IPC_BLOB_BYTES = 512
RBS_PRECISION_DEFAULT, RBS_PRECISION_F64, RBS_PRECISION_F32 = 0, 1, 2
RBS_STATE_DEFAULT, RBS_STATE_WINDOWED, RBS_STATE_DENSE = 0, 1, 2
PRECISIONS = {None: 0, "default": 0, "f64": 1, "f32": 2}
LAYOUTS = {None: 0, "default": 0, "window": 1, "windowed": 1, "dense": 2}
RBS_OCC_DEFAULT, RBS_OCC_DEVICE_RULE, RBS_OCC_REFERENCE = 0, 1, 2
OPTIONS = {"shared_trail": 1, "shared_trail_enter": 2, "shared_trail_every": 3, "tracker_split_max": 4, "timing_every": 5}
OCC_MODES = {None: 0, "default": 0, "device": 1, "eager": 1, "reference": 2, "lazy": 2, "exact": 2}

# every symbol include/rbsensor_mi355x.h declares
EXPORTS = (
    "rbs_abi_version", "rbs_device_count", "rbs_create", "rbs_destroy", "rbs_last_error",
    "rbs_reset", "rbs_set_observation", "rbs_set_observation_f32",
    "rbs_set_observation_native_f32", "rbs_set_observation_device", "rbs_get_observation", "rbs_loglikes",
    "rbs_acquire_frame_buffer", "rbs_commit_frame_buffer", "rbs_loglikes_prefetch", "rbs_set_observation_prefetched",
    "rbs_loglikes_deltas", "rbs_get_poses", "rbs_deltas_buffer", "rbs_set_observation_borrowed", "rbs_set_observation_borrowed_f32", "rbs_shared_trail_state",
    "rbs_shared_trail_rebase", "rbs_window_fraction", "rbs_set_option",
    "rbs_loglikes_device", "rbs_synchronize", "rbs_get_occlusion", "rbs_set_occlusion",
    "rbs_occlusion_device_ptr", "rbs_occlusion_next_device_ptr", "rbs_export_plane", "rbs_import_plane",
    "rbs_export_window", "rbs_import_window", "rbs_stream_join", "rbs_ipc_export", "rbs_ipc_attach", "rbs_stage_windows", "rbs_peer_resample",
    "rbs_get_window", "rbs_get_background", "rbs_raster_kernel_ms", "rbs_set_timing_every",
    "rbs_render_depth",
    "rbs_last_kernel_ms", "rbs_timing_summary",
    "rbs_tracker_create", "rbs_tracker_destroy", "rbs_tracker_initialize", "rbs_tracker_track",
    "rbs_tracker_submit", "rbs_tracker_result", "rbs_tracker_track_f64", "rbs_tracker_submit_f64",
    "rbs_tracker_get", "rbs_tracker_set_posterior", "rbs_tracker_posterior", "rbs_tracker_posterior_ms",
    "rbs_gauss_create", "rbs_gauss_destroy", "rbs_gauss_initialize", "rbs_gauss_track", "rbs_gauss_track_f64",
    "rbs_gauss_get_prior", "rbs_gauss_get_sigma_poses", "rbs_gauss_get_render", "rbs_gauss_get_moments",
    "rbs_gauss_kernel_ms", "rbs_gauss_submit", "rbs_gauss_submit_f64", "rbs_gauss_result",
    "rbs_find_default_params", "rbs_find_create", "rbs_find_destroy", "rbs_find_run", "rbs_find_get_stage",
    "rbs_find_stage_ms", "rbs_find_last_error",
    "rbs_find_default_foreground", "rbs_find_set_foreground", "rbs_find_get_plane", "rbs_find_get_seed_frame",
    "rbs_find_default_refinement", "rbs_find_set_refinement", "rbs_find_get_covariance", "rbs_find_get_perturbations",
    "rbs_find_default_gate", "rbs_find_set_gate", "rbs_find_get_evidence", "rbs_find_gate_ms", "rbs_find_scene_set_gate",
    "rbs_find_scene_default_params", "rbs_find_scene_create", "rbs_find_scene_destroy", "rbs_find_scene_set_foreground",
    "rbs_find_scene_set_refinement", "rbs_find_scene_run", "rbs_find_scene_get_order", "rbs_find_scene_get_residual",
    "rbs_find_scene_body_finder", "rbs_find_scene_get_polish", "rbs_find_scene_stage_ms", "rbs_find_scene_last_error",
    "rbs_assess_default_params", "rbs_assess_poses", "rbs_assess_verdict", "rbs_assess_get_plane", "rbs_assess_kernel_ms",
    "rbs_contour_default_params", "rbs_contour_poses", "rbs_contour_verdict", "rbs_contour_kernel_ms",
    "rbs_occlusion_mean", "rbs_occlusion_mean_ms", "rbs_occlusion_bodies",
    "rbs_tracker_set_occlusion_map", "rbs_tracker_occlusion_map", "rbs_tracker_occlusion_map_ms",
    "rbs_object_map", "rbs_object_map_ms", "rbs_object_map_info", "rbs_object_segment_default_params", "rbs_object_segment",
    "rbs_tracker_set_object_map", "rbs_tracker_object_map", "rbs_tracker_object_map_ms", "rbs_tracker_poses",
    "rbs_modes_default_params", "rbs_pose_modes", "rbs_tracker_set_modes", "rbs_tracker_modes", "rbs_tracker_modes_ms",
    "rbs_refine_default_params", "rbs_refine_check_params", "rbs_refine_poses", "rbs_refine_get_history", "rbs_refine_kernel_ms",
)
RBS_REFINE_MAX_ITERATIONS, RBS_REFINE_CONVERGED, RBS_REFINE_TOO_FEW_PIXELS, RBS_REFINE_DEGENERATE, RBS_REFINE_FROZEN = range(5)
RBS_REFINE_MAX_ITERS = 32
RBS_MODES_MAX = 8
RBS_ASSESS_OUT_OF_VIEW, RBS_ASSESS_OCCLUDED, RBS_ASSESS_SUPPORTED, RBS_ASSESS_LOST = range(4)
RBS_CONTOUR_NO_RIM, RBS_CONTOUR_UNDECIDED, RBS_CONTOUR_PRESENT, RBS_CONTOUR_ABSENT = range(4)
RBS_FIND_SEEDS, RBS_FIND_COARSE, RBS_FIND_CANDIDATES, RBS_FIND_SURVIVORS, RBS_FIND_CHILDREN, RBS_FIND_RESULT = range(6)


class RbsTrackerParams(C.Structure):
    _fields_ = [
        ("linear_sigma", C.c_double * 3),
        ("angular_sigma", C.c_double * 3),
        ("velocity_factor", C.c_double),
        ("max_kl_divergence", C.c_double),
        ("n_particles", C.c_int32),
    ]


class RbsTrackerPosteriorInfo(C.Structure):
    _fields_ = [
        ("n", C.c_int32),
        ("survivors", C.c_int32),
        ("resampled", C.c_int32),
        ("frame", C.c_int32),
        ("ess", C.c_double),
    ]


class RbsModesParams(C.Structure):
    _fields_ = [
        ("h_t", C.c_double),
        ("h_r", C.c_double),
        ("separation", C.c_double),
        ("k_max", C.c_int32),
        ("reserved", C.c_int32),
    ]


class RbsMode(C.Structure):
    _fields_ = [
        ("seed", C.c_int32),
        ("reserved", C.c_int32),
        ("density", C.c_double),
        ("mass", C.c_double),
        ("core_mass", C.c_double),
        ("delta", C.c_double * 6),
    ]


class RbsBodyModes(C.Structure):
    _fields_ = [
        ("n_modes", C.c_int32),
        ("reserved", C.c_int32),
        ("mode", RbsMode * RBS_MODES_MAX),
    ]


class RbsGaussParams(C.Structure):
    _fields_ = [
        ("linear_sigma", C.c_double * 3),
        ("angular_sigma", C.c_double * 3),
        ("velocity_factor", C.c_double),
        ("ut_alpha", C.c_double),
        ("fg_noise_std", C.c_double),
        ("bg_depth", C.c_double),
        ("bg_noise_std", C.c_double),
        ("tail_weight", C.c_double),
        ("uniform_tail_min", C.c_double),
        ("uniform_tail_max", C.c_double),
    ]


class RbsFindParams(C.Structure):
    _fields_ = [
        ("coarse_downsampling", C.c_int32),
        ("seed_stride", C.c_int32),
        ("min_depth", C.c_double),
        ("max_depth", C.c_double),
        ("depth_offset", C.c_double),
        ("max_seeds", C.c_int32),
        ("n_rotations", C.c_int32),
        ("n_candidates", C.c_int32),
        ("nms_translation", C.c_double),
        ("nms_angle", C.c_double),
        ("n_survivors", C.c_int32),
        ("rounds", C.c_int32),
        ("children", C.c_int32),
        ("sigma_translation", C.c_double),
        ("sigma_angle", C.c_double),
        ("decay", C.c_double),
        ("batch", C.c_int32),
        ("seed", C.c_uint64),
        ("min_score", C.c_double),
    ]


class RbsFindForeground(C.Structure):
    _fields_ = [
        ("enabled", C.c_int32),
        ("plane_trials", C.c_int32),
        ("ransac_sigmas", C.c_double),
        ("mask_sigmas", C.c_double),
        ("min_inlier_fraction", C.c_double),
    ]


class RbsFindRefinement(C.Structure):
    _fields_ = [
        ("enabled", C.c_int32),
        ("elite", C.c_int32),
        ("mix", C.c_double),
        ("shrink", C.c_double),
        ("jitter", C.c_double),
    ]


class RbsFindGate(C.Structure):
    _fields_ = [
        ("enabled", C.c_int32),
        ("require_confirmed", C.c_int32),
        ("radius", C.c_int32),
        ("min_rim_pixels", C.c_int32),
        ("min_pixels", C.c_int32),
        ("sigmas", C.c_double),
        ("min_support_fraction", C.c_double),
        ("min_visible_fraction", C.c_double),
        ("min_valid_fraction", C.c_double),
        ("min_contour_fraction", C.c_double),
        ("min_flush_fraction", C.c_double),
    ]


class RbsFindSceneParams(C.Structure):
    _fields_ = [
        ("explain_sigmas", C.c_double),
        ("explain_radius", C.c_int32),
        ("polish_sweeps", C.c_int32),
        ("polish_children", C.c_int32),
        ("reserved", C.c_int32),
        ("polish_sigma_translation", C.c_double),
        ("polish_sigma_angle", C.c_double),
        ("polish_decay", C.c_double),
    ]


class RbsAssessParams(C.Structure):
    _fields_ = [
        ("sigmas", C.c_double),
        ("min_support_fraction", C.c_double),
        ("min_visible_fraction", C.c_double),
        ("min_pixels", C.c_int32),
        ("reserved", C.c_int32),
    ]


class RbsAssessBody(C.Structure):
    _fields_ = [
        ("rendered", C.c_int32),
        ("valid", C.c_int32),
        ("support", C.c_int32),
        ("in_front", C.c_int32),
        ("behind", C.c_int32),
        ("verdict", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


class RbsRefineParams(C.Structure):
    _fields_ = [
        ("gate_sigmas", C.c_double),
        ("huber_sigmas", C.c_double),
        ("damping", C.c_double),
        ("max_rotation", C.c_double),
        ("max_translation", C.c_double),
        ("eps_rotation", C.c_double),
        ("eps_translation", C.c_double),
        ("min_pixels", C.c_int32),
        ("iters", C.c_int32),
    ]


class RbsRefineBody(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("iterations", C.c_int32),
        ("count_first", C.c_int32),
        ("count_last", C.c_int32),
        ("rms_first", C.c_double),
        ("rms_last", C.c_double),
    ]


class RbsRefineHistory(C.Structure):
    _fields_ = [
        ("pose", C.c_double * 12),
        ("sums", C.c_double * 28),
        ("delta", C.c_double * 6),
        ("count", C.c_int32),
        ("status", C.c_int32),
    ]


class RbsContourParams(C.Structure):
    _fields_ = [
        ("radius", C.c_int32),
        ("min_rim_pixels", C.c_int32),
        ("min_valid_fraction", C.c_double),
        ("min_contour_fraction", C.c_double),
        ("min_flush_fraction", C.c_double),
    ]


class RbsContourBody(C.Structure):
    _fields_ = [
        ("rim", C.c_int32),
        ("valid", C.c_int32),
        ("flush", C.c_int32),
        ("in_front", C.c_int32),
        ("beyond", C.c_int32),
        ("verdict", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


class RbsOcclusionBody(C.Structure):
    _fields_ = [
        ("rendered", C.c_int32),
        ("occluded", C.c_int32),
        ("sum_q32", C.c_int64),
        ("reserved", C.c_int32 * 4),
    ]


class RbsObjectSegmentParams(C.Structure):
    _fields_ = [
        ("min_cover", C.c_double),
        ("sigmas", C.c_double),
        ("depth_sigmas", C.c_double),
        ("reserved", C.c_double),
    ]


class RbsConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("device_id", C.c_int32),
        ("rows", C.c_int32),
        ("cols", C.c_int32),
        ("K", C.c_double * 9),
        ("max_particles", C.c_int32),
        ("n_objects", C.c_int32),
        ("vertices", C.POINTER(C.c_double)),
        ("vertex_counts", C.POINTER(C.c_int32)),
        ("triangles", C.POINTER(C.c_int32)),
        ("triangle_counts", C.POINTER(C.c_int32)),
        ("p_occluded_visible", C.c_double),
        ("p_occluded_occluded", C.c_double),
        ("initial_occlusion_prob", C.c_double),
        ("tail_weight", C.c_double),
        ("model_sigma", C.c_double),
        ("sigma_factor", C.c_double),
        ("delta_time", C.c_double),
        ("likelihood_precision", C.c_int32),
        ("state_layout", C.c_int32),
        ("n_devices", C.c_int32),
        ("device_ids", C.POINTER(C.c_int32)),
        ("state_slab_px", C.c_int32),
        ("occlusion_mode", C.c_int32),
    ]


_lib = None


def load():
    """Return the loaded library (cached). Raises OSError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(make -C dbot_ros_amd/csrc, or __graft_entry__.build()). "
            "dbot_ros_amd has no CPU fallback.")
    # When torch is in the process its bundled libamdhip64.so.7 must be the one HIP runtime;
    # importing it first makes our DT_NEEDED resolve to the already-loaded copy.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is plumbing, not a requirement of the C-ABI
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    H = C.c_void_p
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    lib.rbs_abi_version.restype = C.c_int32
    lib.rbs_abi_version.argtypes = []
    lib.rbs_device_count.restype = C.c_int32
    lib.rbs_device_count.argtypes = []
    lib.rbs_create.restype = C.c_int32
    lib.rbs_create.argtypes = [C.POINTER(RbsConfig), C.POINTER(H)]
    lib.rbs_destroy.restype = None
    lib.rbs_destroy.argtypes = [H]
    lib.rbs_last_error.restype = C.c_char_p
    lib.rbs_last_error.argtypes = [H]
    lib.rbs_reset.restype = C.c_int32
    lib.rbs_reset.argtypes = [H]
    lib.rbs_set_observation.restype = C.c_int32
    lib.rbs_set_observation.argtypes = [H, dp, C.c_size_t]
    lib.rbs_set_observation_borrowed.restype = C.c_int32
    lib.rbs_set_observation_borrowed.argtypes = [H, dp, C.c_size_t]
    lib.rbs_set_observation_borrowed_f32.restype = C.c_int32
    lib.rbs_set_observation_borrowed_f32.argtypes = [H, fp, C.c_size_t]
    lib.rbs_set_observation_f32.restype = C.c_int32
    lib.rbs_set_observation_f32.argtypes = [H, fp, C.c_size_t]
    lib.rbs_set_observation_native_f32.restype = C.c_int32
    lib.rbs_set_observation_native_f32.argtypes = [H, fp, C.c_int32, C.c_int32, C.c_int32]
    lib.rbs_acquire_frame_buffer.restype = C.c_int32
    lib.rbs_acquire_frame_buffer.argtypes = [H, C.POINTER(C.POINTER(C.c_float))]
    lib.rbs_commit_frame_buffer.restype = C.c_int32
    lib.rbs_commit_frame_buffer.argtypes = [H]
    lib.rbs_get_observation.restype = C.c_int32
    lib.rbs_get_observation.argtypes = [H, fp]
    lib.rbs_loglikes.restype = C.c_int32
    lib.rbs_loglikes.argtypes = [H, dp, ip, C.c_int32, C.c_int32, dp]
    lib.rbs_loglikes_deltas.restype = C.c_int32
    lib.rbs_loglikes_deltas.argtypes = [H, dp, dp, C.c_int32, ip, C.c_int32, C.c_int32, dp]
    lib.rbs_deltas_buffer.restype = C.c_int32
    lib.rbs_deltas_buffer.argtypes = [H, C.POINTER(dp)]
    lib.rbs_get_poses.restype = C.c_int32
    lib.rbs_get_poses.argtypes = [H, dp, C.c_int32]
    lib.rbs_loglikes_device.restype = C.c_int32
    lib.rbs_loglikes_device.argtypes = [H, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p]
    lib.rbs_synchronize.restype = C.c_int32
    lib.rbs_synchronize.argtypes = [H]
    lib.rbs_get_occlusion.restype = C.c_int32
    lib.rbs_get_occlusion.argtypes = [H, C.c_int32, fp]
    lib.rbs_set_occlusion.restype = C.c_int32
    lib.rbs_set_occlusion.argtypes = [H, C.c_int32, fp]
    lib.rbs_occlusion_device_ptr.restype = C.c_int32
    lib.rbs_occlusion_device_ptr.argtypes = [H, C.c_int32, C.POINTER(C.c_void_p)]
    lib.rbs_occlusion_next_device_ptr.restype = C.c_int32
    lib.rbs_occlusion_next_device_ptr.argtypes = [H, C.c_int32, C.POINTER(C.c_void_p)]
    lib.rbs_set_observation_device.restype = C.c_int32
    lib.rbs_set_observation_device.argtypes = [H, C.c_void_p, C.c_void_p]
    lib.rbs_get_window.restype = C.c_int32
    lib.rbs_get_window.argtypes = [H, C.c_int32, C.POINTER(C.c_int32)]
    lib.rbs_shared_trail_state.restype = C.c_int32
    lib.rbs_shared_trail_state.argtypes = [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.rbs_shared_trail_rebase.restype = C.c_int32
    lib.rbs_shared_trail_rebase.argtypes = [H, C.c_int32]
    lib.rbs_set_option.restype = C.c_int32
    lib.rbs_set_option.argtypes = [H, C.c_int32, C.c_double]
    lib.rbs_window_fraction.restype = C.c_int32
    lib.rbs_window_fraction.argtypes = [H, C.POINTER(C.c_double)]
    lib.rbs_get_background.restype = C.c_int32
    lib.rbs_get_background.argtypes = [H, C.POINTER(C.c_float)]
    lib.rbs_raster_kernel_ms.restype = C.c_int32
    lib.rbs_raster_kernel_ms.argtypes = [H, C.c_int32, C.POINTER(C.c_float)]
    lib.rbs_set_timing_every.restype = C.c_int32
    lib.rbs_set_timing_every.argtypes = [H, C.c_int32]
    lib.rbs_export_plane.restype = C.c_int32
    lib.rbs_export_plane.argtypes = [H, C.c_int32, C.c_void_p, C.c_void_p]
    lib.rbs_import_plane.restype = C.c_int32
    lib.rbs_import_plane.argtypes = [H, C.c_int32, C.c_void_p, C.c_void_p]
    lib.rbs_loglikes_prefetch.restype = C.c_int32
    lib.rbs_loglikes_prefetch.argtypes = [H, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                          C.POINTER(C.c_float), C.c_size_t]
    lib.rbs_set_observation_prefetched.restype = C.c_int32
    lib.rbs_set_observation_prefetched.argtypes = [H]
    lib.rbs_export_window.restype = C.c_int32
    lib.rbs_export_window.argtypes = [H, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.rbs_import_window.restype = C.c_int32
    lib.rbs_import_window.argtypes = [H, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    lib.rbs_stream_join.restype = C.c_int32
    lib.rbs_stream_join.argtypes = [H, C.c_void_p]
    lib.rbs_ipc_export.restype = C.c_int32
    lib.rbs_ipc_export.argtypes = [H, C.c_void_p]
    lib.rbs_ipc_attach.restype = C.c_int32
    lib.rbs_ipc_attach.argtypes = [H, C.c_int32, C.c_int32, C.c_void_p]
    lib.rbs_stage_windows.restype = C.c_int32
    lib.rbs_stage_windows.argtypes = [H, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.rbs_peer_resample.restype = C.c_int32
    lib.rbs_peer_resample.argtypes = [H, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rbs_render_depth.restype = C.c_int32
    lib.rbs_render_depth.argtypes = [H, dp, fp]
    lib.rbs_last_kernel_ms.restype = C.c_int32
    lib.rbs_last_kernel_ms.argtypes = [H, C.POINTER(C.c_float)]
    lib.rbs_timing_summary.restype = C.c_int32
    lib.rbs_timing_summary.argtypes = [H, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       C.POINTER(C.c_int32)]
    lib.rbs_tracker_create.restype = C.c_int32
    lib.rbs_tracker_create.argtypes = [H, C.POINTER(RbsTrackerParams), C.POINTER(H)]
    lib.rbs_tracker_destroy.restype = None
    lib.rbs_tracker_destroy.argtypes = [H]
    lib.rbs_tracker_initialize.restype = C.c_int32
    lib.rbs_tracker_initialize.argtypes = [H, dp]
    lib.rbs_tracker_track.restype = C.c_int32
    lib.rbs_tracker_track.argtypes = [H, fp, dp, dp, C.c_uint64, dp, ip]
    lib.rbs_tracker_track_f64.restype = C.c_int32
    lib.rbs_tracker_track_f64.argtypes = [H, dp, dp, dp, C.c_uint64, dp, ip]
    lib.rbs_tracker_submit_f64.restype = C.c_int32
    lib.rbs_tracker_submit_f64.argtypes = [H, dp, dp, dp, C.c_uint64]
    lib.rbs_tracker_submit.restype = C.c_int32
    lib.rbs_tracker_submit.argtypes = [H, fp, dp, dp, C.c_uint64]
    lib.rbs_tracker_result.restype = C.c_int32
    lib.rbs_tracker_result.argtypes = [H, dp, ip]
    lib.rbs_tracker_get.restype = C.c_int32
    lib.rbs_tracker_get.argtypes = [H, dp, dp, ip]
    lib.rbs_tracker_set_posterior.restype = C.c_int32
    lib.rbs_tracker_set_posterior.argtypes = [H, C.c_int32]
    lib.rbs_tracker_posterior.restype = C.c_int32
    lib.rbs_tracker_posterior.argtypes = [H, C.POINTER(RbsTrackerPosteriorInfo), dp, dp]
    lib.rbs_tracker_posterior_ms.restype = C.c_int32
    lib.rbs_tracker_posterior_ms.argtypes = [H, fp]
    lib.rbs_modes_default_params.restype = None
    lib.rbs_modes_default_params.argtypes = [C.POINTER(RbsModesParams)]
    lib.rbs_pose_modes.restype = C.c_int32
    lib.rbs_pose_modes.argtypes = [H, dp, dp, C.c_int32, C.POINTER(RbsModesParams), C.POINTER(RbsBodyModes)]
    lib.rbs_tracker_set_modes.restype = C.c_int32
    lib.rbs_tracker_set_modes.argtypes = [H, C.POINTER(RbsModesParams)]
    lib.rbs_tracker_modes.restype = C.c_int32
    lib.rbs_tracker_modes.argtypes = [H, ip, C.POINTER(RbsBodyModes)]
    lib.rbs_tracker_modes_ms.restype = C.c_int32
    lib.rbs_tracker_modes_ms.argtypes = [H, fp]
    lib.rbs_gauss_create.restype = C.c_int32
    lib.rbs_gauss_create.argtypes = [H, C.POINTER(RbsGaussParams), C.POINTER(H)]
    lib.rbs_gauss_destroy.restype = None
    lib.rbs_gauss_destroy.argtypes = [H]
    lib.rbs_gauss_initialize.restype = C.c_int32
    lib.rbs_gauss_initialize.argtypes = [H, dp, dp]
    lib.rbs_gauss_track.restype = C.c_int32
    lib.rbs_gauss_track.argtypes = [H, fp, dp, dp]
    lib.rbs_gauss_track_f64.restype = C.c_int32
    lib.rbs_gauss_track_f64.argtypes = [H, dp, dp, dp]
    lib.rbs_gauss_get_prior.restype = C.c_int32
    lib.rbs_gauss_get_prior.argtypes = [H, dp, dp, dp]
    lib.rbs_gauss_get_sigma_poses.restype = C.c_int32
    lib.rbs_gauss_get_sigma_poses.argtypes = [H, dp, ip]
    lib.rbs_gauss_get_render.restype = C.c_int32
    lib.rbs_gauss_get_render.argtypes = [H, C.c_int32, fp]
    lib.rbs_gauss_get_moments.restype = C.c_int32
    lib.rbs_gauss_get_moments.argtypes = [H, dp, ip]
    lib.rbs_gauss_kernel_ms.restype = C.c_int32
    lib.rbs_gauss_kernel_ms.argtypes = [H, fp]
    lib.rbs_gauss_submit.restype = C.c_int32
    lib.rbs_gauss_submit.argtypes = [H, fp]
    lib.rbs_gauss_submit_f64.restype = C.c_int32
    lib.rbs_gauss_submit_f64.argtypes = [H, dp]
    lib.rbs_gauss_result.restype = C.c_int32
    lib.rbs_gauss_result.argtypes = [H, dp, dp]
    lp = C.POINTER(C.c_int64)
    lib.rbs_find_default_params.restype = None
    lib.rbs_find_default_params.argtypes = [C.POINTER(RbsFindParams)]
    lib.rbs_find_create.restype = C.c_int32
    lib.rbs_find_create.argtypes = [H, C.POINTER(RbsFindParams), C.POINTER(H)]
    lib.rbs_find_destroy.restype = None
    lib.rbs_find_destroy.argtypes = [H]
    lib.rbs_find_run.restype = C.c_int32
    lib.rbs_find_run.argtypes = [H, fp, C.c_int32, dp, dp, ip, ip]
    lib.rbs_find_get_stage.restype = C.c_int32
    lib.rbs_find_get_stage.argtypes = [H, C.c_int32, C.c_int32, dp, dp, lp, lp, dp]
    lib.rbs_find_stage_ms.restype = C.c_int32
    lib.rbs_find_stage_ms.argtypes = [H, fp]
    lib.rbs_find_default_foreground.restype = None
    lib.rbs_find_default_foreground.argtypes = [C.POINTER(RbsFindForeground)]
    lib.rbs_find_set_foreground.restype = C.c_int32
    lib.rbs_find_set_foreground.argtypes = [H, C.POINTER(RbsFindForeground)]
    lib.rbs_find_get_plane.restype = C.c_int32
    lib.rbs_find_get_plane.argtypes = [H, dp]
    lib.rbs_find_get_seed_frame.restype = C.c_int32
    lib.rbs_find_get_seed_frame.argtypes = [H, fp, lp]
    lib.rbs_find_default_refinement.restype = None
    lib.rbs_find_default_refinement.argtypes = [C.POINTER(RbsFindRefinement)]
    lib.rbs_find_set_refinement.restype = C.c_int32
    lib.rbs_find_set_refinement.argtypes = [H, C.POINTER(RbsFindRefinement)]
    lib.rbs_find_get_covariance.restype = C.c_int32
    lib.rbs_find_get_covariance.argtypes = [H, C.c_int32, dp, lp]
    lib.rbs_find_get_perturbations.restype = C.c_int32
    lib.rbs_find_get_perturbations.argtypes = [H, C.c_int32, dp, lp]
    lib.rbs_find_default_gate.restype = None
    lib.rbs_find_default_gate.argtypes = [C.POINTER(RbsFindGate)]
    lib.rbs_find_set_gate.restype = C.c_int32
    lib.rbs_find_set_gate.argtypes = [H, C.POINTER(RbsFindGate)]
    lib.rbs_find_get_evidence.restype = C.c_int32
    lib.rbs_find_get_evidence.argtypes = [H, C.c_int32, ip, ip, lp]
    lib.rbs_find_gate_ms.restype = C.c_int32
    lib.rbs_find_gate_ms.argtypes = [H, fp]
    lib.rbs_find_last_error.restype = C.c_char_p
    lib.rbs_find_last_error.argtypes = [H]
    up = C.POINTER(C.c_uint32)
    lib.rbs_find_scene_default_params.restype = None
    lib.rbs_find_scene_default_params.argtypes = [C.POINTER(RbsFindSceneParams)]
    lib.rbs_find_scene_create.restype = C.c_int32
    lib.rbs_find_scene_create.argtypes = [H, C.POINTER(RbsFindParams), C.POINTER(RbsFindSceneParams), C.POINTER(H)]
    lib.rbs_find_scene_destroy.restype = None
    lib.rbs_find_scene_destroy.argtypes = [H]
    lib.rbs_find_scene_set_foreground.restype = C.c_int32
    lib.rbs_find_scene_set_foreground.argtypes = [H, C.POINTER(RbsFindForeground)]
    lib.rbs_find_scene_set_refinement.restype = C.c_int32
    lib.rbs_find_scene_set_refinement.argtypes = [H, C.POINTER(RbsFindRefinement)]
    lib.rbs_find_scene_set_gate.restype = C.c_int32
    lib.rbs_find_scene_set_gate.argtypes = [H, C.POINTER(RbsFindGate)]
    lib.rbs_find_scene_run.restype = C.c_int32
    lib.rbs_find_scene_run.argtypes = [H, fp, C.c_uint32, dp, dp, dp, up, dp]
    lib.rbs_find_scene_get_order.restype = C.c_int32
    lib.rbs_find_scene_get_order.argtypes = [H, ip, ip, dp]
    lib.rbs_find_scene_get_residual.restype = C.c_int32
    lib.rbs_find_scene_get_residual.argtypes = [H, C.c_int32, fp]
    lib.rbs_find_scene_body_finder.restype = H
    lib.rbs_find_scene_body_finder.argtypes = [H, C.c_int32]
    lib.rbs_find_scene_get_polish.restype = C.c_int32
    lib.rbs_find_scene_get_polish.argtypes = [H, C.c_int32, dp, dp, ip, ip]
    lib.rbs_find_scene_stage_ms.restype = C.c_int32
    lib.rbs_find_scene_stage_ms.argtypes = [H, fp, fp]
    lib.rbs_find_scene_last_error.restype = C.c_char_p
    lib.rbs_find_scene_last_error.argtypes = [H]
    lib.rbs_assess_default_params.restype = None
    lib.rbs_assess_default_params.argtypes = [C.POINTER(RbsAssessParams)]
    lib.rbs_assess_poses.restype = C.c_int32
    lib.rbs_assess_poses.argtypes = [H, C.POINTER(RbsAssessParams), fp, dp, C.c_int32, C.POINTER(RbsAssessBody)]
    lib.rbs_assess_verdict.restype = C.c_int32
    lib.rbs_assess_verdict.argtypes = [C.POINTER(RbsAssessParams), C.POINTER(RbsAssessBody), ip]
    lib.rbs_assess_get_plane.restype = C.c_int32
    lib.rbs_assess_get_plane.argtypes = [H, C.c_int32, C.c_int32, fp]
    lib.rbs_assess_kernel_ms.restype = C.c_int32
    lib.rbs_assess_kernel_ms.argtypes = [H, fp]
    lib.rbs_contour_default_params.restype = None
    lib.rbs_contour_default_params.argtypes = [C.POINTER(RbsContourParams)]
    lib.rbs_contour_poses.restype = C.c_int32
    lib.rbs_contour_poses.argtypes = [H, C.POINTER(RbsAssessParams), C.POINTER(RbsContourParams), fp, dp, C.c_int32,
                                      C.POINTER(RbsAssessBody), C.POINTER(RbsContourBody)]
    lib.rbs_contour_verdict.restype = C.c_int32
    lib.rbs_contour_verdict.argtypes = [C.POINTER(RbsContourParams), C.POINTER(RbsContourBody), ip]
    lib.rbs_contour_kernel_ms.restype = C.c_int32
    lib.rbs_contour_kernel_ms.argtypes = [H, fp]
    lib.rbs_refine_default_params.restype = None
    lib.rbs_refine_default_params.argtypes = [C.POINTER(RbsRefineParams)]
    lib.rbs_refine_check_params.restype = C.c_int32
    lib.rbs_refine_check_params.argtypes = [C.POINTER(RbsRefineParams)]
    lib.rbs_refine_poses.restype = C.c_int32
    lib.rbs_refine_poses.argtypes = [H, C.POINTER(RbsRefineParams), fp, dp, C.c_int32, dp, C.POINTER(RbsRefineBody)]
    lib.rbs_refine_get_history.restype = C.c_int32
    lib.rbs_refine_get_history.argtypes = [H, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RbsRefineHistory)]
    lib.rbs_refine_kernel_ms.restype = C.c_int32
    lib.rbs_refine_kernel_ms.argtypes = [H, fp]
    lib.rbs_occlusion_mean.restype = C.c_int32
    lib.rbs_occlusion_mean.argtypes = [H, ip, dp, C.c_int32, fp]
    lib.rbs_occlusion_mean_ms.restype = C.c_int32
    lib.rbs_occlusion_mean_ms.argtypes = [H, fp]
    lib.rbs_occlusion_bodies.restype = C.c_int32
    lib.rbs_occlusion_bodies.argtypes = [H, fp, dp, C.c_int32, C.c_double, C.POINTER(RbsOcclusionBody)]
    lib.rbs_tracker_set_occlusion_map.restype = C.c_int32
    lib.rbs_tracker_set_occlusion_map.argtypes = [H, C.c_int32]
    lib.rbs_tracker_occlusion_map.restype = C.c_int32
    lib.rbs_tracker_occlusion_map.argtypes = [H, ip, fp]
    lib.rbs_tracker_occlusion_map_ms.restype = C.c_int32
    lib.rbs_tracker_occlusion_map_ms.argtypes = [H, fp]
    lib.rbs_object_map.restype = C.c_int32
    lib.rbs_object_map.argtypes = [H, dp, C.c_int32, ip, dp, C.c_int32, fp, fp, fp]
    lib.rbs_object_map_ms.restype = C.c_int32
    lib.rbs_object_map_ms.argtypes = [H, fp]
    lib.rbs_object_map_info.restype = C.c_int32
    lib.rbs_object_map_info.argtypes = [H, ip]
    lib.rbs_object_segment_default_params.restype = None
    lib.rbs_object_segment_default_params.argtypes = [C.POINTER(RbsObjectSegmentParams)]
    lib.rbs_object_segment.restype = C.c_int32
    lib.rbs_object_segment.argtypes = [H, C.POINTER(RbsObjectSegmentParams), fp, fp, fp, ip, ip, ip, fp, C.c_int32, ip]
    lib.rbs_tracker_set_object_map.restype = C.c_int32
    lib.rbs_tracker_set_object_map.argtypes = [H, C.c_int32]
    lib.rbs_tracker_object_map.restype = C.c_int32
    lib.rbs_tracker_object_map.argtypes = [H, ip, fp, fp, fp]
    lib.rbs_tracker_object_map_ms.restype = C.c_int32
    lib.rbs_tracker_object_map_ms.argtypes = [H, fp]
    lib.rbs_tracker_poses.restype = C.c_int32
    lib.rbs_tracker_poses.argtypes = [H, dp]
    _lib = lib
    return lib
