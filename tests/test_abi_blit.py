"""frm_blit at the C ABI boundary (include/frm.h, no GPU needed): declared, exported, bound, and
refusing bad arguments with status codes."""
import ctypes
import inspect
import os
import re

import frm
from frm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "frm.h")


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_point():
    src = header_without_comments()
    m = re.search(r"\bint\s+frm_blit\s*\(([^)]*)\)\s*;", src)
    assert m, "frm_blit is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11
    assert args[0].startswith("frm_ctx*") and args[1].startswith("const uint8_t*") and args[-1].startswith("void*")
    assert re.search(r"#define\s+FRM_ABI_VERSION\s+5u\b", src)  # additive: the version stays


def test_library_exports_and_binding(frm_lib):
    bound = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    assert hasattr(frm_lib, "frm_blit"), "libfrm.so does not export frm_blit"
    assert "frm_blit" in bound, "_lib.SIGNATURES does not bind frm_blit"
    assert bound["frm_blit"][0] is ctypes.c_int
    assert len(bound["frm_blit"][1]) == 11
    assert frm_lib.frm_abi_version() == 5


def test_null_arguments_are_codes(frm_lib):
    L = frm_lib
    assert L.frm_blit(None, None, 0, 1, 1, None, 0, 1, 1, 0, None) == _lib.FRM_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.frm_last_error(None)
    # a NULL context is refused before anything else is looked at
    assert L.frm_blit(None, 16, 4, 1, 1, 32, 4, 1, 1, 0, None) == _lib.FRM_ERR_INVALID_ARGUMENT


def test_renderer_has_the_python_surface():
    params = list(inspect.signature(frm.Renderer.blit).parameters)
    assert params == ["self", "src_ptr", "src_bytes", "src_w", "src_h", "dst_ptr", "dst_bytes", "out_w", "out_h",
                      "srgb", "bgra", "stream"]
