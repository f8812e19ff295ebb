"""The depth-of-field entry points at the C ABI boundary (include/frm.h, no GPU needed): declared,
exported, bound, refusing bad arguments with status codes, the pinned sequence stated identically in
its three places, and the host function frm_dof_coc bit for bit against tests/dof_reference.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import dof_reference as ref
import frm
from frm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "frm.h")
DESIGN = os.path.join(ROOT, "DESIGN.md")
INT_NAMES = {"frm_dof_coc": 6, "frm_depth_of_field": 13, "frm_set_depth_of_field": 4, "frm_get_depth_of_field": 4,
             "frm_read_depth": 3}
PINNED = (
    "A frame S of W x H RGBA8 sRGB texels.",
    "A depth plane Z of W x H f32 values.",
    "A, the aperture: the blur radius, in pixels, of a point at infinity. Finite, >= 0.",
    "F, the focus distance. Finite, > 0.",
    "R, the largest radius: an integer in 0..FRM_MAX_DOF_RADIUS, with FRM_MAX_DOF_RADIUS = 16.",
    "All arithmetic is f32 with no contraction, and every division is an IEEE division.",
    "c = A * fabsf(1.0f - F / Z[q])      (thin lens; Z = +inf gives c = A; Z = 0 gives +inf, or NaN when A = 0)",
    "if (!(c >= 0.0f)) c = 0.0f          (NaN: in focus)",
    "if (c > (float)R) c = (float)R",
    "a = c * c;   w = 1.0f / (kPi * a + 1.0f)",
    "D, the blit's sRGB decode table.",
    "kPi = f32(pi).",
    "Start with sw = sr = sg = sb = 0.0f. Loop dy from -R to R, outer, top to bottom.",
    "Loop dx from -R to R, inner, left to right. Let q = p + (dx, dy). Skip q when it lies outside the frame: "
    "the window is clipped, not clamped.",
    "use_p = (Z[q] > Z[p]) && (c[p] < c[q])       (a sample behind p spreads no wider than p's own circle:",
    "a_e = use_p ? a[p] : a[q]                      no background bleeding onto a sharper foreground)",
    "w_e = use_p ? w[p] : w[q]",
    "if ((float)(dx*dx + dy*dy) <= a_e):",
    "sw = sw + w_e",
    "sr = sr + w_e * D[S[q].r]                  (one multiply, one add; likewise g, b)",
    "out[p] = encode(sr / sw), encode(sg / sw), encode(sb / sw), 255",
    "The source alpha is ignored.",
)


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_points():
    src = header_without_comments()
    for name in INT_NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert re.search(r"#define\s+FRM_MAX_DOF_RADIUS\s+16u\b", src)
    assert re.search(r"#define\s+FRM_ABI_VERSION\s+5u\b", src)  # additive: the version stays


def test_header_design_and_reference_state_the_same_sequence():
    """The pinned lines stand in include/frm.h and DESIGN.md as they do in tests/dof_reference.py's docstring
    (white space, the comment's asterisks and the document's code marks aside)."""
    squeeze = lambda s: re.sub(r"[\s*`]+", "", s)  # noqa: E731
    texts = {"include/frm.h": squeeze(open(HEADER).read()), "tests/dof_reference.py": squeeze(ref.__doc__),
             "DESIGN.md": squeeze(open(DESIGN).read())}
    for line in PINNED:
        for where, text in texts.items():
            assert squeeze(line) in text, (where, line)
    design = open(DESIGN).read()
    assert re.search(r"^#+ .*Depth of field", design, flags=re.M)
    for limit in ("ray distance", "sphere around the camera", "one surface per pixel"):
        assert squeeze(limit) in texts["include/frm.h"] and squeeze(limit) in texts["DESIGN.md"], limit


def test_library_exports_and_bindings(frm_lib):
    bound = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    for name, nargs in INT_NAMES.items():
        assert hasattr(frm_lib, name), f"libfrm.so does not export {name}"
        assert name in bound, f"_lib.SIGNATURES does not bind {name}"
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == nargs, name
    assert frm_lib.frm_abi_version() == 5
    assert frm.FRM_MAX_DOF_RADIUS == ref.MAX_RADIUS == 16


def test_python_surface():
    for attr in ("set_depth_of_field", "depth_of_field", "read_depth"):
        assert hasattr(frm.Renderer, attr), attr
    assert callable(frm.dof_coc) and "dof_coc" in frm.__all__
    import inspect
    assert "depth_of_field" in inspect.signature(frm.Renderer.__init__).parameters


def special_depths():
    f = np.float32
    tiny, huge = np.finfo(f).tiny, np.finfo(f).max
    return np.array([np.inf, -np.inf, 0.0, -0.0, np.nan, 1.0, 2.0, 4.0, 0.5, -1.0, -2.0, tiny, -tiny, huge, -huge,
                     1e-45, 3.4e38, 1.0000001, 0.99999994, 2.0000002, 1.9999999], f)


@pytest.mark.parametrize("aperture,focus,radius", [(8.0, 2.0, 16), (0.0, 2.0, 16), (3.5, 0.7, 4), (1e30, 1e-3, 16),
                                                   (2.0, 2.0, 0), (1e-30, 1e30, 1), (0.1, 3.0, 16), (16.0, 1.0, 15),
                                                   (3.4e38, 3.4e38, 16), (1e-45, 1e-45, 16)])
def test_dof_coc_equals_the_reference(frm_lib, aperture, focus, radius):
    rng = np.random.default_rng(int(radius * 1000 + focus * 10))
    z = np.concatenate([rng.uniform(0.01, 50.0, 3000), np.exp(rng.uniform(-80, 80, 1000)),
                        focus * (1.0 + rng.uniform(-1e-5, 1e-5, 500)), -rng.uniform(0.01, 50.0, 100)])
    z = np.concatenate([special_depths(), z.astype(np.float32)])[:4620].reshape(-1, 3)  # any shape
    before = z.copy()
    got = frm.dof_coc(aperture, focus, radius, z)
    want = ref.coc(aperture, focus, radius, z)
    assert got.shape == z.shape and got.dtype == np.float32
    assert got.tobytes() == want.tobytes()
    assert z.tobytes() == before.tobytes()
    assert np.all((got >= 0) & (got <= radius))  # never NaN, never above R


def test_null_and_range_arguments_are_codes(frm_lib):
    L, bad = frm_lib, _lib.FRM_ERR_INVALID_ARGUMENT
    z = np.array([1.0, 2.0], np.float32)
    out = np.full(2, 77.0, np.float32)
    zp, op = z.ctypes.data, out.ctypes.data
    assert L.frm_dof_coc(1.0, 1.0, 4, None, 2, op) == bad and b"NULL" in L.frm_last_error(None)
    assert L.frm_dof_coc(1.0, 1.0, 4, zp, 2, None) == bad
    assert L.frm_dof_coc(1.0, 1.0, 17, zp, 2, op) == bad
    for aperture in (-1.0, float("nan"), float("inf"), -0.5):
        assert L.frm_dof_coc(aperture, 1.0, 4, zp, 2, op) == bad, aperture
    for focus in (0.0, -1.0, float("nan"), float("inf")):
        assert L.frm_dof_coc(1.0, focus, 4, zp, 2, op) == bad, focus
    assert np.all(out == 77.0)  # nothing written by a refused call
    assert L.frm_dof_coc(1.0, 1.0, 16, zp, 0, op) == 0 and np.all(out == 77.0)  # n = 0
    assert L.frm_dof_coc(-0.0, 1.0, 0, zp, 2, op) == 0 and np.all(out == 0.0)  # -0 >= 0, R = 0
    a, f, r = ctypes.c_float(5), ctypes.c_float(6), ctypes.c_uint32(7)
    assert L.frm_set_depth_of_field(None, 1.0, 1.0, 4) == bad and b"NULL" in L.frm_last_error(None)
    assert L.frm_get_depth_of_field(None, ctypes.byref(a), ctypes.byref(f), ctypes.byref(r)) == bad
    assert (a.value, f.value, r.value) == (5, 6, 7)
    assert L.frm_read_depth(None, op, 2) == bad
    assert L.frm_depth_of_field(None, None, 0, None, 0, 1, 1, 1.0, 1.0, 1, None, 0, None) == bad
    with pytest.raises(frm.FrmError) as e:
        frm.dof_coc(1.0, 0.0, 4, z)
    assert e.value.code == bad
