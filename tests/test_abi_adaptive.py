"""The adaptive supersampling entry points at the C ABI boundary (include/frm.h, no GPU needed):
the header compiles as C and declares them, the library exports them, the bindings know them, and
bad arguments come back as status codes."""
import ctypes
import os
import re
import subprocess

import frm
from frm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "frm.h")
NAMES = ("frm_set_adaptive", "frm_get_adaptive", "frm_refine", "frm_debug_refine_mask")


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "frm.h"\n'
                   "int use(frm_ctx* c, const frm_parameters* p, uint8_t* a, uint8_t* b, uint64_t* n) {\n"
                   "  uint32_t f, t;\n"
                   "  return frm_set_adaptive(c, 2u, FRM_ADAPTIVE_DEFAULT_THRESHOLD) + frm_get_adaptive(c, &f, &t) +\n"
                   "         frm_refine(c, p, a, 4, 1, 1, 2u, 16u, b, 4, n, 0) + frm_debug_refine_mask(c, a, 1);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_header_declares_the_entry_points():
    src = header_without_comments()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    m = re.search(r"#define\s+FRM_ADAPTIVE_DEFAULT_THRESHOLD\s+(\d+)u?\b", src)
    assert m and int(m.group(1)) == 16
    assert re.search(r"#define\s+FRM_ABI_VERSION\s+5u\b", src)  # additive: the version stays


def test_library_exports_and_bindings(frm_lib):
    bound = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    for name in NAMES:
        assert hasattr(frm_lib, name), f"libfrm.so does not export {name}"
        assert name in bound, f"_lib.SIGNATURES does not bind {name}"
        assert bound[name][0] is ctypes.c_int
    assert [len(bound[n][1]) for n in NAMES] == [3, 3, 12, 3]
    assert frm_lib.frm_abi_version() == 5
    assert _lib.FRM_ADAPTIVE_DEFAULT_THRESHOLD == 16 and frm.FRM_ADAPTIVE_DEFAULT_THRESHOLD == 16


def test_null_arguments_are_codes(frm_lib):
    L = frm_lib
    f, t = ctypes.c_uint32(7), ctypes.c_uint32(7)
    assert L.frm_set_adaptive(None, 2, 16) == _lib.FRM_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.frm_last_error(None)
    assert L.frm_get_adaptive(None, ctypes.byref(f), ctypes.byref(t)) == _lib.FRM_ERR_INVALID_ARGUMENT
    assert (f.value, t.value) == (7, 7)
    assert L.frm_refine(None, None, None, 0, 1, 1, 2, 16, None, 0, None, None) == _lib.FRM_ERR_INVALID_ARGUMENT
    assert L.frm_debug_refine_mask(None, None, 0) == -_lib.FRM_ERR_INVALID_ARGUMENT


def test_renderer_has_the_python_surface():
    import inspect
    assert "adaptive" in inspect.signature(frm.Renderer.__init__).parameters
    for attr in ("set_adaptive", "adaptive", "refine", "refine_mask"):
        assert hasattr(frm.Renderer, attr), attr
    sig = inspect.signature(frm.Renderer.set_adaptive)
    assert sig.parameters["threshold"].default == _lib.FRM_ADAPTIVE_DEFAULT_THRESHOLD
