"""ctypes binding of include/oatgpu.h (one declaration per exported symbol)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    """The product library.  Only with OATGPU_MEASURE_PY=1 in the environment does OATGPU_LIB redirect the binding to
    another build (the A/B tools under tools/ set both): nothing else in the environment changes what is loaded."""
    if os.environ.get("OATGPU_MEASURE_PY") == "1" and os.environ.get("OATGPU_LIB"):
        return os.environ["OATGPU_LIB"]
    return os.path.join(_HERE, "lib", "liboatgpu.so")


class OatGpuError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"oatgpu error {code}: {text}")
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("n_streams", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
        ("ring_depth", C.c_int32), ("channels", C.c_int32),
        ("history", C.c_int32), ("nmixtures", C.c_int32),
        ("var_threshold", C.c_float), ("background_ratio", C.c_float), ("var_threshold_gen", C.c_float),
        ("var_init", C.c_float), ("var_min", C.c_float), ("var_max", C.c_float), ("ct", C.c_float),
        ("tau", C.c_float), ("detect_shadows", C.c_int32), ("shadow_value", C.c_int32),
        ("h_lo", C.c_int32), ("h_hi", C.c_int32), ("s_lo", C.c_int32), ("s_hi", C.c_int32),
        ("v_lo", C.c_int32), ("v_hi", C.c_int32), ("erode", C.c_int32), ("dilate", C.c_int32),
        ("min_area", C.c_double), ("max_area", C.c_double),
        ("diff_threshold", C.c_int32), ("blur", C.c_int32),
        ("mog_restore_nmodes", C.c_int32), ("reserved_", C.c_int32),
    ]


class Position(C.Structure):
    _fields_ = [("valid", C.c_int32), ("first_pixel", C.c_int32), ("x", C.c_double), ("y", C.c_double),
                ("area", C.c_double), ("a00", C.c_int64), ("a10", C.c_int64), ("a01", C.c_int64),
                ("velocity_valid", C.c_int32), ("raw_valid", C.c_int32), ("vx", C.c_double), ("vy", C.c_double),
                ("raw_x", C.c_double), ("raw_y", C.c_double)]


class Profile(C.Structure):
    _fields_ = [("steps", C.c_int64), ("mog_ms", C.c_double), ("morph_ms", C.c_double),
                ("blob_ms", C.c_double), ("total_ms", C.c_double), ("event_pair_ms", C.c_double),
                ("mog_frames", C.c_int64), ("dropped", C.c_int64)]


class Traffic(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("launches", "pixels", "lane_bytes_read", "lane_bytes_written",
                                         "sector32_bytes_read", "sector32_bytes_written",
                                         "sector64_bytes_read", "sector64_bytes_written")]


class Marker(C.Structure):
    """oatgpu_marker: one marker's detector (windows as oatgpu_set_detector's)."""
    _fields_ = [("h_lo", C.c_int32), ("h_hi", C.c_int32), ("s_lo", C.c_int32), ("s_hi", C.c_int32),
                ("v_lo", C.c_int32), ("v_hi", C.c_int32), ("erode", C.c_int32), ("dilate", C.c_int32),
                ("min_area", C.c_double), ("max_area", C.c_double)]


class Combined(C.Structure):
    """oatgpu_combined: what `posicom mean` publishes for one camera."""
    _fields_ = [("position_valid", C.c_int32), ("heading_valid", C.c_int32), ("velocity_valid", C.c_int32),
                ("n_valid", C.c_int32), ("x", C.c_double), ("y", C.c_double), ("hx", C.c_double), ("hy", C.c_double)]


class Region(C.Structure):
    """oatgpu_region: one `posifilt region` polygon (name of at most 9 bytes, n_points x/y pairs)."""
    _fields_ = [("name", C.c_char * 10), ("n_points", C.c_int32), ("xy", C.POINTER(C.c_double))]


class MarkerFilters(C.Structure):
    """oatgpu_marker_filters: the chain kalman -> homography -> region behind the combined record."""
    _fields_ = [("kalman", C.c_int32), ("dt", C.c_double), ("timeout", C.c_double), ("sigma_accel", C.c_double),
                ("sigma_noise", C.c_double), ("homography", C.c_int32), ("h", C.c_double * 9), ("n_regions", C.c_int32),
                ("regions", C.POINTER(Region))]


class Filtered(C.Structure):
    """oatgpu_filtered: the combined record of one camera behind the chain."""
    _fields_ = [("position_valid", C.c_int32), ("velocity_valid", C.c_int32), ("heading_valid", C.c_int32),
                ("region_valid", C.c_int32), ("region", C.c_int32), ("reserved_", C.c_int32), ("x", C.c_double), ("y", C.c_double),
                ("vx", C.c_double), ("vy", C.c_double), ("hx", C.c_double), ("hy", C.c_double)]


class Track(C.Structure):
    """oatgpu_track: one track slot of one camera (oatgpu_set_tracks), 96 bytes."""
    _fields_ = [("filtered", Filtered), ("id", C.c_int64), ("rank", C.c_int32), ("age", C.c_int32), ("missed", C.c_int32),
                ("reserved_", C.c_int32)]


class Shape(C.Structure):
    """oatgpu_shape: second moments, extents and body axis of one ranked blob (oatgpu_set_target_shapes), 104 bytes."""
    _fields_ = [("valid", C.c_int32), ("axis_valid", C.c_int32), ("a20", C.c_int64), ("a11", C.c_int64), ("a02", C.c_int64),
                ("x_min", C.c_int32), ("y_min", C.c_int32), ("x_max", C.c_int32), ("y_max", C.c_int32), ("mu20", C.c_double),
                ("mu11", C.c_double), ("mu02", C.c_double), ("axis_x", C.c_double), ("axis_y", C.c_double), ("major", C.c_double),
                ("minor", C.c_double)]


class CropWindow(C.Structure):
    """oatgpu_crop_window: one window of oatgpu_crop_windows_dev -- centre, direction of the window's +x, upright or not; 40 bytes."""
    _fields_ = [("valid", C.c_int32), ("upright", C.c_int32), ("cx", C.c_double), ("cy", C.c_double), ("ax", C.c_double),
                ("ay", C.c_double)]


class CropTensorFmt(C.Structure):
    """oatgpu_crop_tensor_fmt: the element type of a crop tensor and, for float16 / float32, scale and bias per channel; 32 bytes."""
    _fields_ = [("dtype", C.c_int32), ("reserved", C.c_int32), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


E_RING_FULL = -4
E_RING_EMPTY = -5
ABI_VERSION = 9          # must equal OATGPU_ABI_VERSION of include/oatgpu.h
MAX_TARGETS = 8          # OATGPU_MAX_TARGETS
CROP_OFF, CROP_UPRIGHT, CROP_AXIS = 0, 1, 2      # OATGPU_CROP_*
CROP_MAX_SIDE, CROP_MAX_WINDOWS = 256, 8         # OATGPU_CROP_MAX_SIDE, OATGPU_CROP_MAX_WINDOWS
TENSOR_U8, TENSOR_F16, TENSOR_F32 = 0, 1, 2      # OATGPU_TENSOR_*
TAP_THRESHOLD, TAP_MORPH, TAP_FINAL = 0, 1, 2
BAYER_RGGB, BAYER_BGGR, BAYER_GRBG, BAYER_GBRG = 1, 2, 3, 4      # OATGPU_BAYER_*: the tile at rows 0-1, columns 0-1

_u8p = C.POINTER(C.c_uint8)
_fp = C.POINTER(C.c_float)
_ctx = C.c_void_p

# name -> (restype, argtypes); mirrors include/oatgpu.h line by line
SIGNATURES = {
    "oatgpu_abi_version": (C.c_int, []),
    "oatgpu_default_config": (C.c_int, [C.POINTER(Config)]),
    "oatgpu_create": (_ctx, [C.POINTER(Config)]),
    "oatgpu_destroy": (None, [_ctx]),
    "oatgpu_last_error": (C.c_char_p, [_ctx]),
    "oatgpu_device_count": (C.c_int, []),
    "oatgpu_device_open_retries": (C.c_int, []),
    "oatgpu_device_numa_node": (C.c_int, [C.c_int32]),
    "oatgpu_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "oatgpu_host_unregister": (C.c_int, [C.c_void_p]),
    "oatgpu_host_alloc": (C.c_void_p, [C.c_size_t]),
    "oatgpu_host_free": (None, [C.c_void_p]),
    "oatgpu_set_stream": (C.c_int, [_ctx, C.c_void_p]),
    "oatgpu_get_stream": (C.c_void_p, [_ctx]),
    "oatgpu_synchronize": (C.c_int, [_ctx]),
    "oatgpu_set_detector": (C.c_int, [_ctx] + [C.c_int32] * 8 + [C.c_double, C.c_double]),
    "oatgpu_set_kalman": (C.c_int, [_ctx, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double]),
    "oatgpu_set_roi_mask": (C.c_int, [_ctx, C.c_int32, _u8p]),
    "oatgpu_bsub_filter": (C.c_int, [_ctx, C.c_int32, _u8p, _u8p, C.c_double]),
    "oatgpu_bsub_set_background": (C.c_int, [_ctx, C.c_int32, _u8p]),
    "oatgpu_mask_filter": (C.c_int, [_ctx, C.c_int32, _u8p, _u8p]),
    "oatgpu_thresh_filter": (C.c_int, [_ctx, _u8p, _u8p, C.c_int32, C.c_int32]),
    "oatgpu_undistort_map": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32,
                                       C.POINTER(C.c_int16), C.POINTER(C.c_uint16)]),
    "oatgpu_set_undistort": (C.c_int, [_ctx, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32]),
    "oatgpu_undistort_filter": (C.c_int, [_ctx, C.c_int32, _u8p, _u8p]),
    "oatgpu_undistort_dev": (C.c_int, [_ctx, C.c_void_p, C.c_void_p]),
    "oatgpu_set_track_undistort": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_debayer_filter": (C.c_int, [_ctx, C.c_int32, _u8p, _u8p]),
    "oatgpu_debayer_dev": (C.c_int, [_ctx, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p]),
    "oatgpu_set_track_bayer": (C.c_int, [_ctx, C.POINTER(C.c_int32), C.c_int32]),
    "oatgpu_set_tracker_bayer": (C.c_int, [_ctx, C.POINTER(C.c_int32), C.c_int32]),
    "oatgpu_set_tracker_undistort": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_set_markers": (C.c_int, [_ctx, C.c_int32, C.POINTER(Marker), C.c_int32]),
    "oatgpu_set_marker_window": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.POINTER(Marker)]),
    "oatgpu_track_markers_dev": (C.c_int, [_ctx, C.c_void_p, C.c_double, C.POINTER(Position), C.POINTER(Position),
                                           C.POINTER(Combined)]),
    "oatgpu_track_markers": (C.c_int, [_ctx, C.POINTER(_u8p), C.c_int32, C.c_double, C.POINTER(Position), C.POINTER(Position),
                                       C.POINTER(Combined)]),
    "oatgpu_read_marker_mask": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_int32, _u8p]),
    "oatgpu_set_marker_pipeline": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_track_collect_markers": (C.c_int, [_ctx, C.POINTER(Position), C.POINTER(Position), C.POINTER(Combined)]),
    "oatgpu_track_markers_sequence_dev": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.c_int32, C.c_double, C.POINTER(Position),
                                                    C.POINTER(Position), C.POINTER(Combined)]),
    "oatgpu_set_marker_filters": (C.c_int, [_ctx, C.POINTER(MarkerFilters)]),
    "oatgpu_marker_filtered": (C.c_int, [_ctx, C.POINTER(Filtered), C.c_int32]),
    "oatgpu_set_tracker_filters": (C.c_int, [_ctx, C.POINTER(MarkerFilters)]),
    "oatgpu_tracker_filtered": (C.c_int, [_ctx, C.POINTER(Filtered), C.c_int32]),
    "oatgpu_set_targets": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_targets": (C.c_int, [_ctx, C.POINTER(Position), C.POINTER(C.c_int32), C.c_int32]),
    "oatgpu_set_tracks": (C.c_int, [_ctx, C.POINTER(MarkerFilters), C.c_double]),
    "oatgpu_tracks": (C.c_int, [_ctx, C.POINTER(Track), C.c_int32]),
    "oatgpu_tracks_update": (C.c_int, [_ctx, C.POINTER(Position), C.POINTER(Track)]),
    "oatgpu_set_target_shapes": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_target_shapes": (C.c_int, [_ctx, C.POINTER(Shape), C.c_int32]),
    "oatgpu_set_target_crops": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_int32]),
    "oatgpu_target_crops": (C.c_int, [_ctx, _u8p, C.c_int32]),
    "oatgpu_crop_windows_dev": (C.c_int, [_ctx, C.c_void_p, C.POINTER(CropWindow), C.c_int32, C.c_int32, C.c_int32, _u8p]),
    "oatgpu_set_target_crop_tensor": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.POINTER(CropTensorFmt), C.c_void_p,
                                                C.c_int32]),
    "oatgpu_target_crop_tensor_sets": (C.c_int, [_ctx]),
    "oatgpu_crop_tensor_windows_dev": (C.c_int, [_ctx, C.c_void_p, C.POINTER(CropWindow), C.c_int32, C.c_int32, C.c_int32,
                                                 C.POINTER(CropTensorFmt), C.c_void_p]),
    "oatgpu_set_target_mask_tensor": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_int32]),
    "oatgpu_target_mask_tensor_sets": (C.c_int, [_ctx]),
    "oatgpu_mog_apply": (C.c_int, [_ctx, C.c_int32, _u8p, _u8p, C.c_double]),
    "oatgpu_mog_filter": (C.c_int, [_ctx, C.c_int32, _u8p, _u8p, C.c_double]),
    "oatgpu_bgr2hsv": (C.c_int, [_ctx, _u8p, _u8p]),
    "oatgpu_cvt_color": (C.c_int, [_ctx, C.c_int32, C.c_int32, _u8p, _u8p]),
    "oatgpu_set_fusion": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_set_deferred": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_fetch_frame": (C.c_int, [_ctx, _u8p]),
    "oatgpu_fetch_position": (C.c_int, [_ctx, C.POINTER(Position)]),
    "oatgpu_set_early_blob": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_early_blob_timeouts": (C.c_int64, [_ctx]),
    "oatgpu_set_k1_workgroup": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_last_step_shape": (C.c_int, [_ctx, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "oatgpu_set_rowscan_rows": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_last_step_rowscan_rows": (C.c_int, [_ctx]),
    "oatgpu_set_homography": (C.c_int, [_ctx, C.c_int32, C.POINTER(C.c_double)]),
    "oatgpu_detect_hsv": (C.c_int, [_ctx, C.c_int32, _u8p, C.POINTER(Position)]),
    "oatgpu_detect_thresh": (C.c_int, [_ctx, C.c_int32, _u8p, C.POINTER(Position)]),
    "oatgpu_detect_diff": (C.c_int, [_ctx, C.c_int32, _u8p, C.POINTER(Position)]),
    "oatgpu_set_diff_tracker": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_diff_reset": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_diff_batch_dev": (C.c_int, [_ctx, C.c_void_p, C.POINTER(Position)]),
    "oatgpu_diff_batch": (C.c_int, [_ctx, C.POINTER(_u8p), C.c_int32, C.POINTER(Position)]),
    "oatgpu_diff_sequence_dev": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Position)]),
    "oatgpu_read_diff_mask": (C.c_int, [_ctx, C.c_int32, C.c_int32, _u8p]),
    "oatgpu_set_bsub_tracker": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_bsub_reset": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_bsub_track_batch_dev": (C.c_int, [_ctx, C.c_void_p, C.c_double, C.POINTER(Position)]),
    "oatgpu_bsub_track_batch": (C.c_int, [_ctx, C.POINTER(_u8p), C.c_int32, C.c_double, C.POINTER(Position)]),
    "oatgpu_bsub_track_sequence_dev": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.c_int32, C.c_double, C.POINTER(Position)]),
    "oatgpu_bsub_get_state": (C.c_int, [_ctx, C.c_int32, _u8p, _fp]),
    "oatgpu_read_bsub_mask": (C.c_int, [_ctx, C.c_int32, C.c_int32, _u8p]),
    "oatgpu_track_batch": (C.c_int, [_ctx, C.POINTER(_u8p), C.c_int32, C.c_double, C.POINTER(Position)]),
    "oatgpu_track_batch_dev": (C.c_int, [_ctx, C.c_void_p, C.c_double, C.POINTER(Position)]),
    "oatgpu_track_enqueue": (C.c_int, [_ctx, C.POINTER(_u8p), C.c_int32, C.c_double]),
    "oatgpu_track_enqueue_dev": (C.c_int, [_ctx, C.c_void_p, C.c_double]),
    "oatgpu_track_sequence_dev": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.c_int32, C.c_double, C.POINTER(Position)]),
    "oatgpu_track_sequence_dev_timed": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.c_int32, C.c_double, C.POINTER(Position),
                                                  C.POINTER(C.c_double)]),
    "oatgpu_track_sequence_dev_latency": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.c_int32, C.c_double, C.POINTER(Position),
                                                    C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "oatgpu_track_collect": (C.c_int, [_ctx, C.POINTER(Position)]),
    "oatgpu_track_outstanding": (C.c_int, [_ctx]),
    "oatgpu_track_input_consumed": (C.c_int, [_ctx]),
    "oatgpu_track_input_consumed_stream": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_track_stage": (C.c_int, [_ctx, C.c_int32, _u8p]),
    "oatgpu_track_enqueue_staged": (C.c_int, [_ctx, C.c_double]),
    "oatgpu_track_stage_abort": (C.c_int, [_ctx]),
    "oatgpu_set_stage_copy": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_track_ready": (C.c_int, [_ctx]),
    "oatgpu_read_mask": (C.c_int, [_ctx, C.c_int32, C.c_int32, _u8p]),
    "oatgpu_mog_get_state": (C.c_int, [_ctx, C.c_int32, _u8p, _fp, _fp, _fp, C.POINTER(C.c_int32)]),
    "oatgpu_mog_set_state": (C.c_int, [_ctx, C.c_int32, _u8p, _fp, _fp, _fp, C.c_int32]),
    "oatgpu_mog_save": (C.c_int, [_ctx, C.c_int32, C.c_char_p]),
    "oatgpu_mog_load": (C.c_int, [_ctx, C.c_int32, C.c_char_p]),
    "oatgpu_profile_enable": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_profile_read": (C.c_int, [_ctx, C.POINTER(Profile)]),
    "oatgpu_profile_reset": (C.c_int, [_ctx]),
    "oatgpu_traffic_audit": (C.c_int, [_ctx, C.c_int32]),
    "oatgpu_traffic_read": (C.c_int, [_ctx, C.POINTER(Traffic)]),
    "oatgpu_measure_hbm": (C.c_int, [_ctx, C.c_size_t, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

_lib = None


def load():
    """Loads liboatgpu.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7.  If torch is
    # imported AFTER this library has pulled in /opt/rocm's runtime, torch finds no GPU; imported
    # first, both share torch's copy (same SONAME).  So when torch is installed, load it first.
    import sys
    if "torch" not in sys.modules and os.environ.get("OATGPU_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: the HIP extension has not been built "
            "(run `make` or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.oatgpu_abi_version() != ABI_VERSION:
        raise ImportError("liboatgpu.so ABI version mismatch")
    _lib = lib
    return lib


def check(lib, ctx, rc):
    if rc != 0:
        msg = lib.oatgpu_last_error(ctx)
        raise OatGpuError(rc, msg.decode() if msg else "")


def u8(a):
    return a.ctypes.data_as(_u8p)


def f32(a):
    return a.ctypes.data_as(_fp)
