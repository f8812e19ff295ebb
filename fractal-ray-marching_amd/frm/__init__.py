"""frm — MI355X-native offscreen fractal ray-marcher (host-side package).

Mirrors the reference's host interface (src/parameters.rs, src/camera.rs,
src/graphics.rs) over the C ABI of include/frm.h (libfrm.so, HIP kernels for gfx950).
"""
from ._lib import (FRM_DEFAULT_MAX_STEPS, FRM_FLAG_PERSISTENT_KERNEL, FRM_FLAG_SCENE_SPHERE, FRM_FLAG_SIMPLE_KERNEL,
                   FRM_FLAG_HW_MATH, FRM_FLAG_UNBOUNDED_ITERATIONS,
                   FRM_MAX_BATCH, FRM_MAX_FRAMES_IN_FLIGHT, FRM_MAX_NUM_ITERATIONS, FRM_MAX_SUPERSAMPLE, FRM_NUM_COUNTERS, FRM_NUM_SCENES,
                   FRM_ADAPTIVE_DEFAULT_THRESHOLD, FRM_MAX_SHUTTER_SAMPLES, FRM_MAX_DOF_RADIUS,
                   FrmError, LIB_PATH,
                   load)
from .parameters import (Camera, HeldKeys, Parameters, Timing, dof_coc, equirect_tables, panorama_face_size,
                         panorama_parameters, shutter_parameters)
from .renderer import Renderer, device_count
from .workloads import FRAME_SECONDS, POSES, POWER8_TIME, WORKLOADS, Workload, frame_sequence, make_parameters

__all__ = [
    "Camera", "HeldKeys", "Parameters", "Renderer", "Timing", "FrmError", "device_count", "load", "LIB_PATH",
    "FRAME_SECONDS", "POSES", "POWER8_TIME", "WORKLOADS", "Workload", "frame_sequence", "make_parameters",
    "shutter_parameters", "FRM_MAX_SHUTTER_SAMPLES",
    "panorama_parameters", "panorama_face_size", "equirect_tables",
    "dof_coc", "FRM_MAX_DOF_RADIUS",
    "FRM_DEFAULT_MAX_STEPS", "FRM_FLAG_PERSISTENT_KERNEL", "FRM_FLAG_SCENE_SPHERE", "FRM_FLAG_SIMPLE_KERNEL",
    "FRM_FLAG_UNBOUNDED_ITERATIONS", "FRM_FLAG_HW_MATH",
    "FRM_MAX_BATCH", "FRM_MAX_FRAMES_IN_FLIGHT", "FRM_MAX_NUM_ITERATIONS", "FRM_MAX_SUPERSAMPLE", "FRM_NUM_COUNTERS",
    "FRM_NUM_SCENES", "FRM_ADAPTIVE_DEFAULT_THRESHOLD",
]
