"""TEST INFRASTRUCTURE ONLY — ctypes wrapper of the CPU oracle (oracle/frm_oracle.c).

Imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg only; the
product never uses it. See frm_oracle.c for what is restated and how parity is pinned.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "build", "libfrm_oracle.so")

MODE_FRM = 0   # bit-exact spec of the kernel's builtins (gate P0)
MODE_LIBM = 1  # double-precision libm builtins rounded to f32 (gate P1)

INFO_HIT = 1
INFO_SUN_HIT = 2
INFO_NAN = 4
INFO_SHADOW_FIRST_NONPOS = 8
INFO_ZERO_NORMAL = 16

# per-pixel trace (render(trace=True)): the geometric inputs of the shading
TRACE_FIELDS = ("hit", "steps", "nx", "ny", "nz", "sun_hit", "sun_closeness", "cr", "cg", "cb")

MATH_FN = {"sin": 0, "cos": 1, "acos": 2, "atan2": 3, "log": 4, "log2": 5, "exp2": 6,
           "pow": 7, "sqrt": 8, "div": 9}

# domain census (render(census=True), scene_de_census): names in frm_oracle.c's enum order
_CLOSENESS = ("divs", "t0_dpos", "t0_dnonpos", "t0_dnan", "t_tiny", "q_subnormal", "q_inf", "q_nan")
_ENDS = ("end_hit", "end_steps", "end_far", "end_nan")
CENSUS_COUNTS = (("mb_bodies", "mb_comp_zero", "mb_comp_tiny", "mb_r_small", "mb_lengths", "mb_dot_wide",
                  "mb_dists", "mb_mag_not_normal", "mb_dr_ge_2p64", "mb_dr_ge_2p125", "mb_dr_inf", "mb_dr_nan",
                  "mb_de_nan", "mb_de_neg", "mb_de_zero", "mb_de_subnormal")
                 + tuple("primary_" + n for n in _CLOSENESS) + tuple("shadow_" + n for n in _CLOSENESS)
                 + tuple("primary_" + n for n in _ENDS) + tuple("shadow_" + n for n in _ENDS)
                 + ("de_evals", "de_nan", "de_inf", "de_zero", "de_subnormal"))
# a maximum that was never met is 0, a minimum +inf
CENSUS_EXTREMES = ("mb_dr_max_finite", "primary_t_max_finite", "shadow_t_max_finite",
                   "mb_de_min_nonzero", "primary_t_min_nonzero", "shadow_t_min_nonzero")
CENSUS_MAXIMA = 3

_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE])


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        lib = ctypes.CDLL(LIB_PATH)
        u8p, f32p, u32p, u64p = (ctypes.c_void_p,) * 4
        lib.om_render.argtypes = [u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_uint32, ctypes.c_int, u32p, ctypes.c_uint32, ctypes.c_int,
                                  u8p, u64p, f32p, u32p]
        lib.om_render.restype = ctypes.c_int
        lib.om_render_trace.argtypes = lib.om_render.argtypes + [f32p]
        lib.om_render_trace.restype = ctypes.c_int
        lib.om_render_costs.argtypes = lib.om_render.argtypes[:9] + [u32p]
        lib.om_render_costs.restype = ctypes.c_int
        lib.om_shade_trace.argtypes = [u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_int, u32p, ctypes.c_uint32, f32p, u8p]
        lib.om_shade_trace.restype = ctypes.c_int
        lib.om_scene_de.argtypes = [u8p, ctypes.c_uint32, ctypes.c_int, f32p, ctypes.c_uint32, f32p,
                                    f32p, u64p]
        lib.om_scene_de.restype = ctypes.c_int
        lib.om_render_census.argtypes = lib.om_render_trace.argtypes + [u64p, f32p]
        lib.om_render_census.restype = ctypes.c_int
        lib.om_scene_de_census.argtypes = lib.om_scene_de.argtypes + [u64p, f32p]
        lib.om_scene_de_census.restype = ctypes.c_int
        lay = (ctypes.c_uint32 * 3)()
        lib.om_census_layout(ctypes.byref(lay, 0), ctypes.byref(lay, 4), ctypes.byref(lay, 8))
        assert tuple(lay) == (len(CENSUS_COUNTS), len(CENSUS_EXTREMES), CENSUS_MAXIMA), tuple(lay)
        lib.om_math.argtypes = [ctypes.c_int, ctypes.c_int, f32p, f32p, ctypes.c_uint32, f32p]
        lib.om_math.restype = ctypes.c_int
        lib.om_srgb_thresholds.argtypes = [f32p]
        lib.om_srgb_thresholds.restype = None
        lib.om_encode_srgb.argtypes = [f32p, ctypes.c_uint32, u8p]
        lib.om_encode_srgb.restype = ctypes.c_int
        lib.om_srgb_decode.argtypes = [f32p]
        lib.om_srgb_decode.restype = None
        lib.om_blit.argtypes = [u8p, ctypes.c_uint32, ctypes.c_uint32, u8p, ctypes.c_uint32, ctypes.c_uint32,
                                ctypes.c_uint32]
        lib.om_blit.restype = ctypes.c_int
        lib.om_frame_info.argtypes = [u8p, ctypes.c_uint32, ctypes.c_int, f32p]
        lib.om_frame_info.restype = ctypes.c_int
        _lib = lib
    return _lib


def _params_buf(params):
    b = params.to_bytes() if hasattr(params, "to_bytes") else bytes(params)
    assert len(b) == 96
    return np.frombuffer(b, dtype=np.uint8).copy()


def render(params, width, height, max_steps, flags=0, mode=MODE_FRM, rows=None, threads=None,
           linear=False, info=False, trace=False, census=False):
    """Render rows (default all) -> dict(rgba=[n,W,4] u8, counters=[8] u64, ...); info: the
    per-pixel INFO_* bits | primary steps << 8; trace: [n,W,len(TRACE_FIELDS)] f32; census: the
    domain census of the rendered rows, a dict over CENSUS_COUNTS (int) and CENSUS_EXTREMES (float)."""
    lib = load()
    pb = _params_buf(params)
    if rows is None:
        nrows, rows_arr, rows_ptr = height, None, None
    else:
        rows_arr = np.ascontiguousarray(rows, dtype=np.uint32)
        nrows, rows_ptr = len(rows_arr), rows_arr.ctypes.data
    threads = threads or os.cpu_count() or 1
    rgba = np.zeros((nrows, width, 4), dtype=np.uint8)
    counters = np.zeros(8, dtype=np.uint64)
    lin = np.zeros((nrows, width, 3), dtype=np.float32) if linear else None
    inf = np.zeros((nrows, width), dtype=np.uint32) if info else None
    tr = np.zeros((nrows, width, len(TRACE_FIELDS)), dtype=np.float32) if trace else None
    args = (pb.ctypes.data, width, height, max_steps, flags, mode, rows_ptr, nrows, threads,
            rgba.ctypes.data, counters.ctypes.data,
            lin.ctypes.data if linear else None, inf.ctypes.data if info else None,
            tr.ctypes.data if trace else None)
    if census:
        cn, cx = _census_arrays()
        rc = lib.om_render_census(*args, cn.ctypes.data, cx.ctypes.data)
    else:
        rc = lib.om_render_trace(*args)
    if rc != 0:
        raise RuntimeError(f"om_render failed ({rc})")
    out = {"rgba": rgba, "counters": counters}
    if linear:
        out["linear"] = lin
    if info:
        out["info"] = inf
    if trace:
        out["trace"] = tr
    if census:
        out["census"] = _census_dict(cn, cx)
    return out


def render_costs(params, width, height, max_steps, flags=0, mode=MODE_FRM, rows=None, threads=None):
    """The scheduling cost of every pixel of the rows (default all) -> [n, W] uint32: Mandelbulb
    loop bodies over all of the pixel's DEs, DE evaluations for every other family and the sphere
    (om_render_costs; what libfrm's cost keys are 16 log2(cost + 1) of)."""
    lib = load()
    pb = _params_buf(params)
    if rows is None:
        nrows, rows_arr, rows_ptr = height, None, None
    else:
        rows_arr = np.ascontiguousarray(rows, dtype=np.uint32)
        nrows, rows_ptr = len(rows_arr), rows_arr.ctypes.data
    out = np.zeros((nrows, width), dtype=np.uint32)
    rc = lib.om_render_costs(pb.ctypes.data, width, height, max_steps, flags, mode, rows_ptr, nrows,
                             threads or os.cpu_count() or 1, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"om_render_costs failed ({rc})")
    return out


def _census_arrays():
    return np.zeros(len(CENSUS_COUNTS), dtype=np.uint64), np.zeros(len(CENSUS_EXTREMES), dtype=np.float32)


def _census_dict(cn, cx):
    d = {k: int(v) for k, v in zip(CENSUS_COUNTS, cn)}
    d.update({k: float(v) for k, v in zip(CENSUS_EXTREMES, cx)})
    return d


def merge_census(a, b):
    """The census of two runs together (counts add; extremes take the max / min)."""
    out = {k: a[k] + b[k] for k in CENSUS_COUNTS}
    out.update({k: max(a[k], b[k]) for k in CENSUS_EXTREMES[:CENSUS_MAXIMA]})
    out.update({k: min(a[k], b[k]) for k in CENSUS_EXTREMES[CENSUS_MAXIMA:]})
    return out


def shade_trace(params, width, height, max_steps, xs, ys, trace, flags=0, mode=MODE_FRM):
    """RGBA8 of pixels (xs[i], ys[i]) shaded (fragment.wgsl:336-346, builtins of `mode`) from
    the given traces ([n, len(TRACE_FIELDS)]) instead of their own march results."""
    lib = load()
    xy = np.ascontiguousarray(np.stack([xs, ys], axis=-1), dtype=np.uint32)
    tr = np.ascontiguousarray(trace, dtype=np.float32).reshape(-1, len(TRACE_FIELDS))
    out = np.zeros((len(tr), 4), dtype=np.uint8)
    rc = lib.om_shade_trace(_params_buf(params).ctypes.data, width, height, max_steps, flags, mode,
                            xy.ctypes.data, len(tr), tr.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise ValueError("om_shade_trace")
    return out


def scene_de(params, points, flags=0, mode=MODE_FRM):
    lib = load()
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = pts.shape[0]
    d = np.zeros(n, dtype=np.float32)
    col = np.zeros((n, 3), dtype=np.float32)
    cnt = np.zeros(2, dtype=np.uint64)
    lib.om_scene_de(_params_buf(params).ctypes.data, flags, mode, pts.ctypes.data, n, d.ctypes.data,
                    col.ctypes.data, cnt.ctypes.data)
    return d, col, cnt


def scene_de_census(params, points, flags=0, mode=MODE_FRM):
    """scene_de plus the domain census of the evaluations: (d, col, cnt, census)."""
    lib = load()
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = pts.shape[0]
    d = np.zeros(n, dtype=np.float32)
    col = np.zeros((n, 3), dtype=np.float32)
    cnt = np.zeros(2, dtype=np.uint64)
    cn, cx = _census_arrays()
    rc = lib.om_scene_de_census(_params_buf(params).ctypes.data, flags, mode, pts.ctypes.data, n, d.ctypes.data,
                                col.ctypes.data, cnt.ctypes.data, cn.ctypes.data, cx.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"om_scene_de_census failed ({rc})")
    return d, col, cnt, _census_dict(cn, cx)


def math_fn(name, a, b=None, mode=MODE_FRM):
    lib = load()
    a = np.ascontiguousarray(a, dtype=np.float32)
    bb = None if b is None else np.ascontiguousarray(np.broadcast_to(b, a.shape), dtype=np.float32)
    out = np.zeros_like(a)
    rc = lib.om_math(MATH_FN[name], mode, a.ctypes.data, None if bb is None else bb.ctypes.data,
                     a.size, out.ctypes.data)
    if rc != 0:
        raise ValueError(name)
    return out


def srgb_thresholds():
    out = np.zeros(256, dtype=np.float32)
    load().om_srgb_thresholds(out.ctypes.data)
    return out


def encode_srgb(c):
    c = np.ascontiguousarray(c, dtype=np.float32)
    out = np.zeros(c.shape, dtype=np.uint8)
    load().om_encode_srgb(c.ctypes.data, c.size, out.ctypes.data)
    return out


def frame_info(params, flags=0, mode=MODE_FRM):
    out = np.zeros(8, dtype=np.float32)
    load().om_frame_info(_params_buf(params).ctypes.data, flags, mode, out.ctypes.data)
    return {"family": int(out[0]), "mb_power": float(out[1]), "menger_cross": float(out[2]),
            "menger_scale": float(out[3]), "koch_normal_z": float(out[4]),
            "origin": tuple(float(v) for v in out[5:8])}


def srgb_decode():
    out = np.zeros(256, dtype=np.float32)
    load().om_srgb_decode(out.ctypes.data)
    return out


def blit(rgba, out_width, out_height, flags=1):
    """Presentation resample of an RGBA8 sRGB frame [H, W, 4] (om_blit): flags 1 = sRGB output,
    2 = BGRA byte order."""
    src = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = src.shape[:2]
    out = np.zeros((out_height, out_width, 4), dtype=np.uint8)
    rc = load().om_blit(src.ctypes.data, w, h, out.ctypes.data, out_width, out_height, flags)
    if rc != 0:
        raise ValueError("om_blit")
    return out
