"""The supersampling entry points at the C ABI boundary (include/frm.h, no GPU needed): declared,
exported, bound, and refusing bad arguments with status codes."""
import ctypes
import os
import re

import frm
from frm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "frm.h")
NAMES = ("frm_set_supersampling", "frm_get_supersampling", "frm_resolve")


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_points():
    src = header_without_comments()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    m = re.search(r"#define\s+FRM_MAX_SUPERSAMPLE\s+(\d+)u?\b", src)
    assert m and int(m.group(1)) == 4
    assert re.search(r"#define\s+FRM_ABI_VERSION\s+5u\b", src)  # additive: the version stays


def test_library_exports_and_bindings(frm_lib):
    bound = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    for name in NAMES:
        assert hasattr(frm_lib, name), f"libfrm.so does not export {name}"
        assert name in bound, f"_lib.SIGNATURES does not bind {name}"
        assert bound[name][0] is ctypes.c_int
    assert len(bound["frm_set_supersampling"][1]) == 2
    assert len(bound["frm_get_supersampling"][1]) == 2
    assert len(bound["frm_resolve"][1]) == 9
    assert _lib.FRM_MAX_SUPERSAMPLE == 4 and frm.FRM_MAX_SUPERSAMPLE == 4


def test_null_arguments_are_codes(frm_lib):
    L = frm_lib
    out = ctypes.c_uint32(7)
    assert L.frm_set_supersampling(None, 2) == _lib.FRM_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.frm_last_error(None)
    assert L.frm_get_supersampling(None, ctypes.byref(out)) == _lib.FRM_ERR_INVALID_ARGUMENT
    assert L.frm_resolve(None, None, 0, 1, 1, 2, None, 0, None) == _lib.FRM_ERR_INVALID_ARGUMENT


def test_renderer_has_the_python_surface():
    import inspect
    assert "supersampling" in inspect.signature(frm.Renderer.__init__).parameters
    for attr in ("set_supersampling", "resolve", "render_width", "render_height"):
        assert hasattr(frm.Renderer, attr), attr
