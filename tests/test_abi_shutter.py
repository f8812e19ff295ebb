"""The motion-blur entry points at the C ABI boundary (include/frm.h, no GPU needed): declared,
exported, bound, refusing bad arguments with status codes, and the host mirror that steps a
frame's state through its shutter interval (frm_shutter_parameters)."""
import ctypes
import os
import re

import numpy as np

import frm
from frm import _lib
from helpers import params_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "frm.h")
NAMES = ("frm_render_shutter", "frm_accumulate")

DT, SHUTTER, ORBIT = 0.05, 0.5, 2.0
KEYS = frm.HeldKeys.MOVE_FORWARD | frm.HeldKeys.YAW_LEFT


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_points():
    src = header_without_comments()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert re.search(r"\bvoid\s+frm_shutter_parameters\s*\(", src)
    m = re.search(r"#define\s+FRM_MAX_SHUTTER_SAMPLES\s+(\d+)u?\b", src)
    b = re.search(r"#define\s+FRM_MAX_BATCH\s+(\d+)u?\b", src)
    assert m and b and int(m.group(1)) == int(b.group(1)) == 32
    assert re.search(r"#define\s+FRM_ABI_VERSION\s+5u\b", src)  # additive: the version stays


def test_library_exports_and_bindings(frm_lib):
    bound = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    for name in NAMES + ("frm_shutter_parameters",):
        assert hasattr(frm_lib, name), f"libfrm.so does not export {name}"
        assert name in bound, f"_lib.SIGNATURES does not bind {name}"
    assert bound["frm_render_shutter"][0] is ctypes.c_int and len(bound["frm_render_shutter"][1]) == 4
    assert bound["frm_accumulate"][0] is ctypes.c_int and len(bound["frm_accumulate"][1]) == 14
    assert bound["frm_shutter_parameters"][0] is None and len(bound["frm_shutter_parameters"][1]) == 8
    assert _lib.FRM_MAX_SHUTTER_SAMPLES == 32 and frm.FRM_MAX_SHUTTER_SAMPLES == 32
    assert frm_lib.frm_abi_version() == 5


def test_null_arguments_are_codes(frm_lib):
    L = frm_lib
    p = _lib.FrmParameters()
    assert L.frm_render_shutter(None, 1, ctypes.addressof(p), None) == _lib.FRM_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.frm_last_error(None)
    assert L.frm_accumulate(None, None, 0, 4, 1, 1, 1, 1, None, 0, 1, None, 0, None) == _lib.FRM_ERR_INVALID_ARGUMENT
    # NULL pointers leave the output alone instead of crashing
    out = (_lib.FrmParameters * 2)()
    before = bytes(out)
    L.frm_shutter_parameters(None, None, None, 0, 0.1, 2, 0.5, ctypes.addressof(out))
    assert bytes(out) == before


def test_renderer_has_the_python_surface():
    for attr in ("render_shutter", "accumulate"):
        assert hasattr(frm.Renderer, attr), attr
    assert callable(frm.shutter_parameters)
    assert "shutter_parameters" in frm.__all__ and "FRM_MAX_SHUTTER_SAMPLES" in frm.__all__


def state():
    p = params_for(18, 6, frm.POWER8_TIME, 33, 17)
    cam = frm.Camera((1.5, 0.9, -1.5), 0.3, -0.1)
    cam.raw.orbit_angle_per_second = ORBIT
    cam.raw.lock_yaw_mode = 1
    timing = frm.Timing()
    timing.raw.time_factor = 1.5
    p.update_camera(cam)
    return p, cam, timing


def snapshot(p, cam, timing):
    return (p.to_bytes(), bytes(ctypes.string_at(ctypes.addressof(cam.raw), ctypes.sizeof(cam.raw))),
            bytes(ctypes.string_at(ctypes.addressof(timing.raw), ctypes.sizeof(timing.raw))))


def test_one_sample_is_the_frame_itself(frm_lib):
    p, cam, timing = state()
    before = snapshot(p, cam, timing)
    out = frm.shutter_parameters(p, cam, timing, KEYS, DT, 1, SHUTTER)
    assert len(out) == 1 and out[0].to_bytes() == p.to_bytes()
    assert snapshot(p, cam, timing) == before


def test_four_samples_equal_a_manual_stepping(frm_lib):
    p, cam, timing = state()
    before = snapshot(p, cam, timing)
    out = frm.shutter_parameters(p, cam, timing, KEYS, DT, 4, SHUTTER)
    assert snapshot(p, cam, timing) == before  # the inputs are untouched
    assert len(out) == 4 and out[0].to_bytes() == p.to_bytes()
    # the same steps by hand, on copies: h = shutter * dt / samples in f32, in this order
    h = np.float32(SHUTTER) * np.float32(DT) / np.float32(4)
    assert h.dtype == np.float32
    p2 = frm.Parameters.from_bytes(p.to_bytes())
    cam2, timing2 = frm.Camera(), frm.Timing()
    ctypes.memmove(ctypes.addressof(cam2.raw), ctypes.addressof(cam.raw), ctypes.sizeof(cam.raw))
    timing2.raw.time_factor = timing.raw.time_factor
    for s in range(1, 4):
        delta = timing2.update(p2, float(h))
        cam2.update(KEYS, delta)
        p2.update_camera(cam2)
        assert out[s].to_bytes() == p2.to_bytes(), f"sub-frame {s}"
    assert out[3].time > out[0].time and out[3].camera_matrix != out[0].camera_matrix
