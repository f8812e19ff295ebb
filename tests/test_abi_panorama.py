"""The panorama entry points at the C ABI boundary (include/frm.h, no GPU needed): declared, exported,
bound, refusing bad arguments with status codes, and the host functions: the six face parameter
sets (frm_panorama_parameters), the direction tables (frm_equirect_tables) and the default face size."""
import ctypes
import os
import re

import numpy as np
import pytest

import frm
import panorama_reference as ref
from frm import _lib
from helpers import params_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "frm.h")
DESIGN = os.path.join(ROOT, "DESIGN.md")
INT_NAMES = {"frm_panorama_face_size": 2, "frm_equirect_tables": 6, "frm_project_equirect": 10,
             "frm_set_panorama": 2, "frm_get_panorama": 2}


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_points():
    src = header_without_comments()
    for name in INT_NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert re.search(r"\bvoid\s+frm_panorama_parameters\s*\(", src)
    assert re.search(r"#define\s+FRM_ABI_VERSION\s+5u\b", src)  # additive: the version stays


def test_header_and_reference_state_the_same_sequence():
    """The pinned lines stand in include/frm.h and DESIGN.md as they do in tests/panorama_reference.py's
    docstring."""
    squeeze = lambda s: re.sub(r"[\s*]+", "", s)  # noqa: E731
    header, doc, design = squeeze(open(HEADER).read()), squeeze(ref.__doc__), squeeze(open(DESIGN).read())
    for line in ("dx = cos_lat*sin_lon;  dy = sin_lat;  dz = cos_lat*cos_lon",
                 "face: |dz| >= |dx| && |dz| >= |dy| ? (dz > 0 ? 0 : 1)",
                 ": |dx| >= |dy|                 ? (dx > 0 ? 2 : 3)",
                 ":                                (dy > 0 ? 4 : 5)",
                 "u = A / m;  v = B / m",
                 "fx = u*(0.5f*N) + (0.5f*M - 0.5f);   fy = (0.5f*M - 0.5f) - v*(0.5f*N)",
                 "x0 = floor(fx); tx = fx - x0;  y0 = floor(fy); ty = fy - y0",
                 "x0, x0+1, y0, y0+1 clamped to [0, M-1]",
                 "mix(a, b, t) = a*(1.0f - t) + b*t"):
        assert squeeze(line) in header, line
        assert squeeze(line) in doc, line
        assert squeeze(line) in design, line


def test_library_exports_and_bindings(frm_lib):
    bound = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    for name, nargs in INT_NAMES.items():
        assert hasattr(frm_lib, name), f"libfrm.so does not export {name}"
        assert name in bound, f"_lib.SIGNATURES does not bind {name}"
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == nargs, name
    assert hasattr(frm_lib, "frm_panorama_parameters")
    assert bound["frm_panorama_parameters"][0] is None and len(bound["frm_panorama_parameters"][1]) == 3
    assert frm_lib.frm_abi_version() == 5


def test_python_surface():
    for attr in ("set_panorama", "project_equirect"):
        assert hasattr(frm.Renderer, attr), attr
    for name in ("panorama_parameters", "panorama_face_size", "equirect_tables"):
        assert callable(getattr(frm, name)) and name in frm.__all__, name


def test_null_and_range_arguments_are_codes(frm_lib):
    L, bad = frm_lib, _lib.FRM_ERR_INVALID_ARGUMENT
    n = ctypes.c_uint32(77)
    assert L.frm_set_panorama(None, 4) == bad and b"NULL" in L.frm_last_error(None)
    assert L.frm_get_panorama(None, ctypes.byref(n)) == bad
    assert L.frm_project_equirect(None, None, 0, 0, 1, None, 0, 1, 1, None) == bad
    assert L.frm_panorama_face_size(16, None) == bad
    assert L.frm_panorama_face_size(0, ctypes.byref(n)) == bad and n.value == 77
    assert L.frm_panorama_face_size(32769, ctypes.byref(n)) == bad and n.value == 77
    t = np.zeros(8, np.float32)
    ptr = t.ctypes.data
    assert L.frm_equirect_tables(2, 2, None, ptr, ptr, ptr) == bad
    assert L.frm_equirect_tables(0, 2, ptr, ptr, ptr, ptr) == bad
    assert L.frm_equirect_tables(2, 32769, ptr, ptr, ptr, ptr) == bad
    assert not t.any()
    # NULL pointers and a face size of 0 leave the output alone instead of crashing
    out = (_lib.FrmParameters * 6)()
    before = bytes(out)
    p = _lib.FrmParameters()
    L.frm_panorama_parameters(None, 4, ctypes.addressof(out))
    L.frm_panorama_parameters(ctypes.byref(p), 0, ctypes.addressof(out))
    L.frm_panorama_parameters(ctypes.byref(p), 4, None)
    assert bytes(out) == before
    with pytest.raises(ValueError):
        frm.panorama_parameters(frm.Parameters(), 0)


def cameras():
    plain = params_for(18, 6, frm.POWER8_TIME, 33, 17)
    plain.update_camera(frm.Camera())
    moved = params_for(3, 4, 1.25, 640, 360)
    moved.update_camera(frm.Camera((1.5, 0.9, -1.5), 0.7, -0.4))
    zero = frm.Parameters()  # the all-zero block: negated zeros keep their sign bit
    return {"default": plain, "yawed-pitched-translated": moved, "zero": zero}


@pytest.mark.parametrize("name", ["default", "yawed-pitched-translated", "zero"])
@pytest.mark.parametrize("N", [1, 5, 14, 1024])
def test_panorama_parameters_equal_the_reference(frm_lib, name, N):
    p = cameras()[name]
    before = p.to_bytes()
    got = frm.panorama_parameters(p, N)
    assert p.to_bytes() == before  # the input is untouched
    want = ref.face_parameters(p, N)
    assert len(got) == 6
    a = float(ref.CAMERA_DIRECTION_Z * (np.float32(N + 2) / np.float32(N)))
    c = np.array(p.camera_matrix, np.float32).reshape(4, 4)
    for f in range(6):
        assert got[f].to_bytes() == want[f], f
        assert got[f].aspect_scale == (a, a)  # the caller's aspect is ignored
        assert (got[f].time, got[f].scene_index, got[f].num_iterations) == (p.time, p.scene_index, p.num_iterations)
        cf = np.array(got[f].camera_matrix, np.float32).reshape(4, 4)
        assert np.array_equal(cf[:, 3], c[:, 3])  # column 3 is unchanged
        # C_f = C * [r u w], exactly
        F = np.array(ref.FACES[f], np.float32).T
        assert np.array_equal(cf[:, :3], c[:, :3] @ F)
    if name != "zero":
        assert len({g.to_bytes() for g in got}) == 6


@pytest.mark.parametrize("W", [1, 2, 33, 4096])
@pytest.mark.parametrize("H", [1, 2, 33, 4096])
def test_equirect_tables_within_one_ulp_of_float64(frm_lib, W, H):
    got = frm.equirect_tables(W, H)
    want = ref.tables(W, H)
    for g, w, n in zip(got, want, (W, W, H, H)):
        assert g.dtype == np.float32 and g.shape == (n,)
        w32 = w.astype(np.float32)
        assert np.all(np.abs(g.astype(np.float64) - w) <= np.spacing(np.abs(w32)).astype(np.float64)), (W, H)
    sl, cl, sp, cp = got
    assert np.all(cp > 0)  # no pixel centre reaches a pole


def test_default_face_size(frm_lib):
    for width, want in ((1, 1), (4, 1), (5, 2), (48, 12), (130, 33), (4096, 1024), (32768, 8192)):
        assert frm.panorama_face_size(width) == want == -(-width // 4)
    with pytest.raises(frm.FrmError) as e:
        frm.panorama_face_size(0)
    assert e.value.code == _lib.FRM_ERR_INVALID_ARGUMENT
