"""What any correct implementation of the presentation blit must output, given tests/blit_reference.py:
the cases, the sources and the rules, shared by tests/test_blit_reference.py (the f32 oracle on the
CPU) and tests/test_gpu_blit.py (blit_kernel). The rules depend on no evaluation order, so the f32
oracle, the kernel and the float64 reference may differ in rounding but not in meaning.

Coordinate slack. An f32 implementation knows a sample's coordinate only approximately. With
e = 2^-24 (half an ulp, relative) and n the texture's size along the axis, the chain
    q = (2i + 1) / d      one division of exact integers, q <= 2:                 error <= 2e
    s = q - 1 (or 1 - q)  one addition, |s| <= 1:                                 error <= e
    s + 1                 one addition, result <= 2:                              error <= 2e
    * 0.5                 exact; the sum so far halves:                           u:  2.5e
    1 - (...)             along y only (v = 1 - ...), result <= 1:                v:  3.5e
    * n                   scales the error by n and rounds a value <= n:          (3.5e or 4.5e) n
    - 0.5                 linear only, rounds a value <= n:                       + e n
    t - floor(t)          linear only, exact but for t in (-1, 0), where it rounds a value <= 1: + e
leaves at most 4.5 e n on a nearest coordinate and 5.5 e n + e <= 6.5 e n on a linear weight. K is
the next power of two, 8: ex = 8 * 2^-24 * sw, ey = 8 * 2^-24 * sh.

Nearest. The output equals the stored bytes of one of the texels {floor(tx - ex), floor(tx + ex)} x
{floor(ty - ey), floor(ty + ey)}, clamped: at most four candidates. A pixel with more than one
candidate texel is ambiguous.

Linear. Every channel's code lies in [code(v - d), code(v + d)] with
    d = |dv/da| ex + |dv/dc| ey + 8 * 2^-24 * max(v, 2^-10):
the weight errors times the local slopes, plus the rounding of the arithmetic. All terms of the three
mixes are non-negative, so relative errors compose: the f32 decode of each tap, 1 - t, a product and
a sum per level of mixing, and the scaling by 255 of a unorm store, are seven roundings of e each; 8
covers them. The floor 2^-10 keeps the interval open where v is 0. A pixel whose interval holds more
than one code in any channel is undecided; no interval may span more than two codes.

Caps. The share of ambiguous or undecided pixels is computed from the reference alone and must stay
under the case's cap: a case that leaves too many pixels open checks too little. Cases that minify an
axis by an even integer sample exactly on texel borders, so every pixel is ambiguous: they are
declared ties and only the candidate rule (and the GPU's bit-exact comparison with the oracle) holds.
"""
import functools
from collections import namedtuple

import numpy as np

import blit_reference as ref

K = 8
EPS = 2.0 ** -24
FLAGS = (0, 1, 2, 3)  # FRM_BLIT_SRGB = 1, FRM_BLIT_BGRA = 2
SOURCES = ("random", "extremes", "ramp")

MAGNIFY_CAP = 0.12
MINIFY_CAP = 0.07

Case = namedtuple("Case", "sw sh dw dh cap tie cap_srgb")


def _case(sw, sh, dw, dh, cap, tie=False, cap_srgb=None):
    return Case(sw, sh, dw, dh, cap, tie, cap if cap_srgb is None else cap_srgb)


# cap: the largest share of undecided / ambiguous pixels over every source and flag value (cap_srgb:
# over the FRM_BLIT_SRGB ones). The measured shares are in DESIGN.md "Presentation blit". Output
# sizes cross the kernel's block edges: columns at 15, 16, 17, rows at 63, 64, 65 (16 x 64 a block).
CASES = {
    # linear: no axis minified
    "mag-7x5-33x65": _case(7, 5, 33, 65, MAGNIFY_CAP),
    "mag-64x48-200x129": _case(64, 48, 200, 129, MAGNIFY_CAP),
    "mag-3x2-200x150": _case(3, 2, 200, 150, MAGNIFY_CAP),
    "mag-16x9-48x27": _case(16, 9, 48, 27, MAGNIFY_CAP),      # odd integer factor 3
    "mag-16x9-17x10": _case(16, 9, 17, 10, MAGNIFY_CAP),
    "mag-256x255-511x300": _case(256, 255, 511, 300, MAGNIFY_CAP),
    "mag-1x1-33x65": _case(1, 1, 33, 65, 0.0),                # both taps are the one texel
    "mag-1x9-1x70": _case(1, 9, 1, 70, MAGNIFY_CAP),
    "mag-2x1-32768x1": _case(2, 1, 32768, 1, MAGNIFY_CAP),
    "mag-1x2-1x32768": _case(1, 2, 1, 32768, MAGNIFY_CAP),
    "same-64x48": _case(64, 48, 64, 48, MAGNIFY_CAP, cap_srgb=0.0),  # sRGB surface: the source itself
    "same-1x1": _case(1, 1, 1, 1, 0.0),
    # nearest: an axis minified
    "min-257x131-16x9": _case(257, 131, 16, 9, 0.0),
    "min-63x45-21x15": _case(63, 45, 21, 15, 0.0),            # ratio 3: the middle texel
    "mix-64x48-192x16": _case(64, 48, 192, 16, 0.0),          # x magnified, y minified
    "mix-64x48-21x144": _case(64, 48, 21, 144, MINIFY_CAP),   # y magnified, x minified
    "min-64x48-63x47": _case(64, 48, 63, 47, MINIFY_CAP),
    "min-130x33-16x63": _case(130, 33, 16, 63, 0.0),
    "min-130x33-17x64": _case(130, 33, 17, 64, MINIFY_CAP),
    "min-130x33-15x65": _case(130, 33, 15, 65, 0.34),         # 13/3 texels a pixel: every third column
    "min-32768x1-77x1": _case(32768, 1, 77, 1, MINIFY_CAP),
    "min-1x32768-1x77": _case(1, 32768, 1, 77, MINIFY_CAP),
    "min-7x5-1x1": _case(7, 5, 1, 1, 0.0),
    "min-5x7-1x3": _case(5, 7, 1, 3, 0.0),
    "tie-64x48-32x24": _case(64, 48, 32, 24, None, tie=True),
    "tie-mix-64x48-128x24": _case(64, 48, 128, 24, None, tie=True),
}
MIXED = ("mix-64x48-192x16", "mix-64x48-21x144", "tie-mix-64x48-128x24")  # one axis each way


def _seed(name, sw, sh):
    return [SOURCES.index(name), sw, sh]


@functools.lru_cache(maxsize=None)
def source(name, sw, sh):
    """A seeded sw x sh RGBA8 source, read-only. random: uniform codes; extremes: codes from
    {0, 1, 254, 255}, one draw per channel and 2 x 2 texels (a draw per texel puts a full-range
    edge, the steepest slope there is, under every pixel: at 256 texels a side that alone leaves
    14.5 % of the pixels undecided, above the magnify cap); ramp: the codes 0..255 in turn along
    the rows, through one permutation per channel. The alpha is random everywhere: the blit
    ignores it."""
    rng = np.random.default_rng(_seed(name, sw, sh))
    img = np.empty((sh, sw, 4), np.uint8)
    if name == "random":
        img[..., :3] = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    elif name == "extremes":
        draw = rng.integers(0, 4, (sh // 2 + 1, sw // 2 + 1, 3))  # the first row and column stand alone
        img[..., :3] = np.array([0, 1, 254, 255], np.uint8)[draw.repeat(2, axis=0).repeat(2, axis=1)[1:sh + 1, 1:sw + 1]]
    elif name == "ramp":
        k = (np.arange(sh * sw) % 256).reshape(sh, sw)
        for c in range(3):
            img[..., c] = rng.permutation(256).astype(np.uint8)[k]
    else:
        raise KeyError(name)
    img[..., 3] = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    img.setflags(write=False)
    return img


# nearest: cand [dh, dw, 4, 4] bytes; linear: lo, hi [dh, dw, 4] bytes (alpha 255 in both).
# open: the ambiguous / undecided pixels; span: the most codes an interval holds, minus one.
Expectation = namedtuple("Expectation", "linear image cand lo hi open share span")


@functools.lru_cache(maxsize=None)
def expectation(case_id, source_name, flags):
    """What the rules allow for a case, a source and a flag value, from the reference alone."""
    c = CASES[case_id]
    src = source(source_name, c.sw, c.sh)
    ex, ey = K * EPS * c.sw, K * EPS * c.sh
    image = ref.blit(src, c.dw, c.dh, flags)
    if ref.is_linear(c.sw, c.sh, c.dw, c.dh):
        v, da, dc = ref.linear_terms(src, c.dw, c.dh)
        d = np.abs(da) * ex + np.abs(dc) * ey + 8 * EPS * np.maximum(v, 2.0 ** -10)
        lo3, hi3 = ref.store(v - d, flags), ref.store(v + d, flags)
        span = int((hi3.astype(np.int64) - lo3).max())
        lo, hi = ref.surface_bytes(lo3, flags), ref.surface_bytes(hi3, flags)
        e = Expectation(True, image, None, lo, hi, (lo != hi).any(axis=-1), None, span)
    else:
        cand, ambiguous = ref.nearest_candidates(src, c.dw, c.dh, flags, ex, ey)
        e = Expectation(False, image, cand, None, None, ambiguous, None, 0)
    for a in e:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return e._replace(share=float(e.open.mean()))


def cap(case_id, flags):
    c = CASES[case_id]
    return c.cap_srgb if flags & ref.SRGB else c.cap


def violations(out, e):
    """The pixels [n, 2] (y, x) of `out` [dh, dw, 4] that break the rules of expectation e."""
    out = np.asarray(out)
    assert out.dtype == np.uint8 and out.shape == e.image.shape, (out.dtype, out.shape, e.image.shape)
    if e.linear:
        ok = ((e.lo <= out) & (out <= e.hi)).all(axis=-1)
    else:
        ok = (out[:, :, None, :] == e.cand).all(axis=-1).any(axis=-1)
    return np.argwhere(~ok)


def describe(out, e, bad, limit=4):
    """A few of the violating pixels, for an assertion message."""
    lines = []
    for y, x in bad[:limit]:
        allowed = (e.lo[y, x].tolist(), e.hi[y, x].tolist()) if e.linear else e.cand[y, x].tolist()
        lines.append(f"(x={x}, y={y}): got {out[y, x].tolist()}, allowed {allowed}")
    return f"{len(bad)} pixels break the rules; " + "; ".join(lines)
