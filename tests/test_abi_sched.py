"""frm_debug_pixel_order at the C ABI boundary (include/frm.h, no GPU needed): declared, exported,
bound, and refusing bad arguments with (negative) status codes, as frm_debug_pixel_keys does."""
import ctypes
import inspect
import os
import re

import numpy as np

import frm
from frm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "frm.h")


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_point():
    src = header_without_comments()
    m = re.search(r"\bint\s+frm_debug_pixel_order\s*\(([^)]*)\)\s*;", src)
    assert m, "frm_debug_pixel_order is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 4
    assert args[0].startswith("frm_ctx*") and args[1].startswith("uint32_t*") and args[2].startswith("size_t")
    assert args[3].startswith("uint32_t*")
    assert re.search(r"#define\s+FRM_ABI_VERSION\s+5u\b", src)  # additive: the version stays


def test_library_exports_and_binding(frm_lib):
    bound = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    assert hasattr(frm_lib, "frm_debug_pixel_order"), "libfrm.so does not export frm_debug_pixel_order"
    assert "frm_debug_pixel_order" in bound, "_lib.SIGNATURES does not bind frm_debug_pixel_order"
    assert bound["frm_debug_pixel_order"][0] is ctypes.c_int
    assert len(bound["frm_debug_pixel_order"][1]) == 4
    assert frm_lib.frm_abi_version() == 5


def test_null_arguments_are_codes(frm_lib):
    L = frm_lib
    out = np.zeros(4, np.uint32)
    ranked = ctypes.c_uint32(7)
    # a count or a negative frm_status: a code can never be read as "1 entry copied"
    assert L.frm_debug_pixel_order(None, out.ctypes.data, 4, ctypes.byref(ranked)) == -_lib.FRM_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.frm_last_error(None)
    assert L.frm_debug_pixel_order(None, None, 0, None) == -_lib.FRM_ERR_INVALID_ARGUMENT
    assert ranked.value == 7 and not out.any()
    keys = np.zeros(4, np.uint8)
    assert L.frm_debug_pixel_keys(None, keys.ctypes.data, 4) == -_lib.FRM_ERR_INVALID_ARGUMENT


def test_renderer_has_the_python_surface():
    assert list(inspect.signature(frm.Renderer.pixel_order).parameters) == ["self", "n"]
