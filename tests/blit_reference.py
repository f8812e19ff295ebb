"""The presentation blit (include/frm.h frm_present, frm_blit) restated in plain numpy float64, from the
definition of the sampler the reference draws its render texture through (persistent_graphics.rs:55-64
and blit.wgsl: clamp to edge, linear magnification, nearest minification, an Rgba8UnormSrgb texture)
in this file's own words.

It shares nothing with oracle/frm_oracle.c's om_blit or with blit_kernel: nothing is imported from
`oracle` or `frm`, nothing is loaded through ctypes, no table is read. Its only import from the suite
is f64_reference.encode, the float64 sRGB store that tests/test_f64_reference.py pins.

The definition, for a source of sw x sh texels drawn on dw x dh pixels (row 0 at the top):
  * pixel (x, y) samples the texture at tx = (x + 1/2) / dw * sw, ty = (y + 1/2) / dh * sh, in texel
    units (texel i covers [i, i + 1), its centre is i + 1/2);
  * a texel's code k is linear light s / 12.92 for s = k / 255 <= 0.04045, else ((s + 0.055) / 1.055)^2.4;
  * the filter is linear when no axis is minified (sw <= dw and sh <= dh), otherwise nearest on both;
  * nearest: texel (floor(tx), floor(ty)), clamped to the texture;
  * linear: along x, i0 = floor(tx - 1/2), weight a = tx - 1/2 - i0 of texel i0 + 1 against texel i0,
    both clamped to [0, sw - 1]; the same along y with weight c; horizontal mixes first, then vertical;
  * an sRGB surface (FRM_BLIT_SRGB) stores f64_reference.encode(value), a unorm surface
    floor(255 * clamp(value, 0, 1) + 1/2); alpha is 255 whatever the source's; FRM_BLIT_BGRA swaps
    the first and third byte.

Besides the image it hands tests/blit_cases.py what its rules need: the texels a nearest sample may
fall on when its coordinates are only known to +-(ex, ey), and a linear sample's float64 value with
its partial derivatives in the two weights.
"""
import numpy as np

from f64_reference import encode

SRGB, BGRA = 1, 2  # FRM_BLIT_SRGB, FRM_BLIT_BGRA


def decode_table():
    """Linear light of the 256 sRGB codes, float64."""
    s = np.arange(256, dtype=np.float64) / 255.0
    return np.where(s <= 0.04045, s / 12.92, np.power((s + 0.055) / 1.055, 2.4))


def sample_positions(n_src, n_dst):
    """Texture coordinate, in texels, of each of n_dst pixel centres along one axis."""
    return (np.arange(n_dst, dtype=np.float64) + 0.5) / n_dst * n_src


def is_linear(sw, sh, dw, dh):
    return sw <= dw and sh <= dh


def store(value, flags):
    """The stored code of each linear-light value (any shape) on the surface `flags` describes."""
    if flags & SRGB:
        return encode(value)
    return np.floor(255.0 * np.clip(value, 0.0, 1.0) + 0.5).astype(np.uint8)


def surface_bytes(rgb_codes, flags):
    """[h, w, 3] codes in R, G, B order -> [h, w, 4] bytes in the surface's order, alpha 255."""
    out = np.empty(rgb_codes.shape[:-1] + (4,), np.uint8)
    out[..., :3] = rgb_codes[..., ::-1] if flags & BGRA else rgb_codes
    out[..., 3] = 255
    return out


def _light(src):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 4
    return decode_table()[src[..., :3]]


def linear_terms(src, dw, dh):
    """A linear sample per pixel: (v, dv_da, dv_dc), each float64 [dh, dw, 3]: the filtered value and
    its partial derivatives in the horizontal weight a and the vertical weight c."""
    L = _light(src)
    sh, sw = L.shape[:2]
    px, py = sample_positions(sw, dw) - 0.5, sample_positions(sh, dh) - 0.5
    i0, j0 = np.floor(px), np.floor(py)
    a, c = (px - i0)[None, :, None], (py - j0)[:, None, None]
    x0, x1 = np.clip(i0, 0, sw - 1).astype(np.int64), np.clip(i0 + 1, 0, sw - 1).astype(np.int64)
    y0, y1 = np.clip(j0, 0, sh - 1).astype(np.int64), np.clip(j0 + 1, 0, sh - 1).astype(np.int64)
    t00, t10 = L[y0][:, x0], L[y0][:, x1]
    t01, t11 = L[y1][:, x0], L[y1][:, x1]
    top = t00 + (t10 - t00) * a
    bottom = t01 + (t11 - t01) * a
    v = top + (bottom - top) * c
    dv_da = (t10 - t00) + ((t11 - t01) - (t10 - t00)) * c
    dv_dc = bottom - top
    return v, dv_da, dv_dc


def nearest_texels(sw, sh, dw, dh, ex=0.0, ey=0.0):
    """The texel columns and rows a nearest sample may fall on when its coordinates are known to
    +-ex, +-ey: (cols [dw, 2], rows [dh, 2]), clamped. With no slack both entries are the texel."""
    tx, ty = sample_positions(sw, dw), sample_positions(sh, dh)
    cols = np.clip(np.stack([np.floor(tx - ex), np.floor(tx + ex)], axis=1), 0, sw - 1).astype(np.int64)
    rows = np.clip(np.stack([np.floor(ty - ey), np.floor(ty + ey)], axis=1), 0, sh - 1).astype(np.int64)
    return cols, rows


def nearest_candidates(src, dw, dh, flags, ex=0.0, ey=0.0):
    """(candidates uint8 [dh, dw, 4, 4], ambiguous bool [dh, dw]): the stored bytes of the up to four
    texels {floor(tx -+ ex)} x {floor(ty -+ ey)}, and where those are more than one texel."""
    L = _light(src)
    sh, sw = L.shape[:2]
    cols, rows = nearest_texels(sw, sh, dw, dh, ex, ey)
    stored = surface_bytes(store(L, flags), flags)  # every texel's output bytes
    cand = np.stack([stored[rows[:, j]][:, cols[:, i]] for j in (0, 1) for i in (0, 1)], axis=2)
    ambiguous = (rows[:, 0] != rows[:, 1])[:, None] | (cols[:, 0] != cols[:, 1])[None, :]
    return cand, ambiguous


def blit(src, dw, dh, flags):
    """The blit of src [sh, sw, 4] uint8 onto dw x dh pixels -> uint8 [dh, dw, 4]."""
    sh, sw = np.asarray(src).shape[:2]
    if is_linear(sw, sh, dw, dh):
        return surface_bytes(store(linear_terms(src, dw, dh)[0], flags), flags)
    return nearest_candidates(src, dw, dh, flags)[0][:, :, 0]
