"""ctypes binding of libfrm.so (include/frm.h).

The library is built in-tree by `make -C fractal-ray-marching_amd` (or
__graft_entry__.build()) into fractal-ray-marching_amd/lib/libfrm.so. There is no
fallback: if the library is missing, importing the renderer raises.
"""
import ctypes
import os

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# FRM_LIB overrides the library path (A/B experiments with alternative builds).
LIB_PATH = os.environ.get("FRM_LIB") or os.path.join(PKG_ROOT, "lib", "libfrm.so")

FRM_OK = 0
FRM_ERR_INVALID_ARGUMENT = 1
FRM_ERR_NO_DEVICE = 2
FRM_ERR_HIP = 3
FRM_ERR_OUT_OF_MEMORY = 4
FRM_ERR_NOT_READY = 5
FRM_ERR_BUFFER_TOO_SMALL = 6
FRM_ERR_UNSUPPORTED = 7
FRM_ERR_COMPILE = 8

FRM_NUM_SCENES = 19
FRM_MAX_FRAMES_IN_FLIGHT = 8
FRM_MAX_DEVICES = 16
FRM_MAX_BATCH = 32
FRM_MAX_SHUTTER_SAMPLES = 32
FRM_MAX_DOF_RADIUS = 16
FRM_MAX_SUPERSAMPLE = 4
FRM_ADAPTIVE_DEFAULT_THRESHOLD = 16
FRM_DEFAULT_MAX_STEPS = 5000
FRM_MAX_STEPS_LIMIT = 4194303
FRM_MAX_NUM_ITERATIONS = 65536
FRM_NUM_COUNTERS = 8
FRM_FLAG_SCENE_SPHERE = 0x1
FRM_FLAG_SIMPLE_KERNEL = 0x2
FRM_FLAG_PERSISTENT_KERNEL = 0x4
FRM_FLAG_UNBOUNDED_ITERATIONS = 0x8
FRM_FLAG_HW_MATH = 0x10
FRM_KERNEL_PERSISTENT = 0
FRM_KERNEL_SIMPLE = 1
FRM_BLIT_SRGB = 0x1
FRM_BLIT_BGRA = 0x2


class FrmParameters(ctypes.Structure):
    """src/parameters.rs:6-15, byte for byte (96 bytes)."""

    _fields_ = [
        ("camera_matrix", ctypes.c_float * 16),
        ("aspect_scale", ctypes.c_float * 2),
        ("time", ctypes.c_float),
        ("num_iterations", ctypes.c_uint32),
        ("scene_index", ctypes.c_uint32),
        ("padding", ctypes.c_uint8 * 12),
    ]


class FrmConfig(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32),
        ("max_steps", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("frames_in_flight", ctypes.c_uint32),
        ("device_count", ctypes.c_uint32),  # ABI 5: a group context over devices[0..count-1]
        ("devices", ctypes.c_int32 * 16),
    ]


class FrmStats(ctypes.Structure):
    _fields_ = [
        ("pixels", ctypes.c_uint64),
        ("hit_pixels", ctypes.c_uint64),
        ("primary_steps", ctypes.c_uint64),
        ("shadow_steps", ctypes.c_uint64),
        ("normal_evals", ctypes.c_uint64),
        ("fractal_bodies", ctypes.c_uint64),
        ("fractal_bailouts", ctypes.c_uint64),
        ("march_steps", ctypes.c_uint64),
        ("wom_ops", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class FrmCamera(ctypes.Structure):
    """frm_camera (include/frm.h): src/camera.rs:5-14."""

    _fields_ = [
        ("position", ctypes.c_float * 3),
        ("pitch", ctypes.c_float),
        ("yaw", ctypes.c_float),
        ("movement_per_second", ctypes.c_float),
        ("orbit_angle_per_second", ctypes.c_float),
        ("lock_yaw_mode", ctypes.c_int32),
        ("lock_pitch", ctypes.c_int32),
    ]


class FrmTiming(ctypes.Structure):
    _fields_ = [("time_factor", ctypes.c_float)]


assert ctypes.sizeof(FrmParameters) == 96

_P = ctypes.POINTER
_u8p = ctypes.POINTER(ctypes.c_uint8)

# (name, restype, argtypes) for every entry point declared in include/frm.h
SIGNATURES = [
    ("frm_abi_version", ctypes.c_uint32, []),
    ("frm_last_error", ctypes.c_char_p, [ctypes.c_void_p]),
    ("frm_device_count", ctypes.c_int, [_P(ctypes.c_int32)]),
    ("frm_create", ctypes.c_int, [_P(ctypes.c_void_p), _P(FrmConfig)]),
    ("frm_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("frm_resize", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]),
    ("frm_set_supersampling", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    ("frm_get_supersampling", ctypes.c_int, [ctypes.c_void_p, _P(ctypes.c_uint32)]),
    ("frm_resolve", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    ("frm_set_adaptive", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]),
    ("frm_get_adaptive", ctypes.c_int, [ctypes.c_void_p, _P(ctypes.c_uint32), _P(ctypes.c_uint32)]),
    ("frm_refine", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    ("frm_debug_refine_mask", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    ("frm_set_parameters", ctypes.c_int, [ctypes.c_void_p, _P(FrmParameters)]),
    ("frm_render", ctypes.c_int, [ctypes.c_void_p, _P(FrmStats)]),
    ("frm_read_frame", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    ("frm_synchronize", ctypes.c_int, [ctypes.c_void_p]),
    ("frm_kernel_for_pixels", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]),
    ("frm_reload", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    ("frm_present", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    ("frm_blit", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]),
    ("frm_read_frame_async", ctypes.c_int, [ctypes.c_void_p, _P(ctypes.c_uint64)]),
    ("frm_present_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P(ctypes.c_uint64)]),
    ("frm_frame_pixels", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.POINTER(ctypes.c_uint8)), _P(ctypes.c_size_t)]),
    ("frm_group_band_rows", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, _P(ctypes.c_uint32)]),
    ("frm_band_rows_for", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P(ctypes.c_uint32)]),
    ("frm_render_bands", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    ("frm_render_bands_batch", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    ("frm_render_shutter", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, _P(FrmStats)]),
    ("frm_accumulate", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_size_t, ctypes.c_void_p]),
    ("frm_unshuffle_bands", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
      ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]),
    ("frm_stats_from_counters", ctypes.c_int, [ctypes.c_void_p, _P(ctypes.c_uint64), _P(FrmStats)]),
    ("frm_eval_scene", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    ("frm_eval_math", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    ("frm_debug_pixel_keys", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    ("frm_debug_set_pixel_keys", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    ("frm_debug_pixel_order", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, _P(ctypes.c_uint32)]),
    ("frm_debug_trace", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    ("frm_parameters_default", None, [_P(FrmParameters)]),
    ("frm_parameters_update_aspect", None, [_P(FrmParameters), ctypes.c_uint32, ctypes.c_uint32]),
    ("frm_parameters_update_time", None, [_P(FrmParameters), ctypes.c_float]),
    ("frm_parameters_update_num_iterations", None, [_P(FrmParameters), ctypes.c_int32]),
    ("frm_parameters_update_scene_index", None, [_P(FrmParameters), ctypes.c_int32]),
    ("frm_parameters_update_camera", None,
     [_P(FrmParameters), _P(ctypes.c_float), ctypes.c_float, ctypes.c_float]),
    ("frm_camera_default", None, [_P(FrmCamera)]),
    ("frm_camera_update", None, [_P(FrmCamera), ctypes.c_uint32, ctypes.c_float]),
    ("frm_camera_update_speed", None, [_P(FrmCamera), ctypes.c_float]),
    ("frm_camera_update_orbit_speed", None, [_P(FrmCamera), ctypes.c_float]),
    ("frm_camera_reset_orbit_speed", None, [_P(FrmCamera)]),
    ("frm_camera_toggle_lock_pitch", None, [_P(FrmCamera)]),
    ("frm_camera_cycle_lock_yaw_mode", None, [_P(FrmCamera), ctypes.c_int32]),
    ("frm_camera_rotate_from_cursor", None, [_P(FrmCamera), ctypes.c_float, ctypes.c_float]),
    ("frm_parameters_update_camera_from", None, [_P(FrmParameters), _P(FrmCamera)]),
    ("frm_timing_init", None, [_P(FrmTiming)]),
    ("frm_timing_update", ctypes.c_float, [_P(FrmTiming), _P(FrmParameters), ctypes.c_float]),
    ("frm_timing_update_time_factor", None, [_P(FrmTiming), ctypes.c_float]),
    ("frm_timing_stop_time", None, [_P(FrmTiming)]),
    ("frm_shutter_parameters", None,
     [_P(FrmParameters), _P(FrmCamera), _P(FrmTiming), ctypes.c_uint32, ctypes.c_float, ctypes.c_uint32,
      ctypes.c_float, ctypes.c_void_p]),
    ("frm_panorama_parameters", None, [_P(FrmParameters), ctypes.c_uint32, ctypes.c_void_p]),
    ("frm_panorama_face_size", ctypes.c_int, [ctypes.c_uint32, _P(ctypes.c_uint32)]),
    ("frm_equirect_tables", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("frm_project_equirect", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]),
    ("frm_set_panorama", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    ("frm_get_panorama", ctypes.c_int, [ctypes.c_void_p, _P(ctypes.c_uint32)]),
    ("frm_dof_coc", ctypes.c_int,
     [ctypes.c_float, ctypes.c_float, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    ("frm_depth_of_field", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_float, ctypes.c_float, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
      ctypes.c_void_p]),
    ("frm_set_depth_of_field", ctypes.c_int, [ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_uint32]),
    ("frm_get_depth_of_field", ctypes.c_int,
     [ctypes.c_void_p, _P(ctypes.c_float), _P(ctypes.c_float), _P(ctypes.c_uint32)]),
    ("frm_read_depth", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
]

_lib = None


class FrmError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libfrm error {code}: {message}")
        self.code = code


def load():
    """Load libfrm.so (raises OSError with a build hint if it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} not found: build it with `make -C {PKG_ROOT}` "
                      "(there is no CPU fallback)")
    # One HIP runtime per process. PyTorch-ROCm bundles its own libamdhip64 with the same
    # SONAME (libamdhip64.so.7) as /opt/rocm's: when torch is loaded first, libfrm binds to
    # that copy, so torch streams, events and torch.cuda.synchronize() and libfrm share one
    # runtime. Loaded the other way round, torch would bring up a second runtime and fail
    # ("No HIP GPUs are available"). Plain C users of libfrm get /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is None and os.environ.get("FRM_LIB"):
            continue  # an A/B build of an earlier ABI (tools/ab_r5.sh) may lack newer entry points
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc, ctx=None):
    if rc != FRM_OK:
        msg = load().frm_last_error(ctx)
        raise FrmError(rc, msg.decode() if msg else "")
    return rc
