"""Expected values of adaptive supersampling (include/frm.h frm_set_adaptive, frm_refine): the numpy
restatement of the pinned semantics. Integer arithmetic only, so it is exact.

With F1 the plain frame and FS the fully supersampled one (tests/ssaa_reference.py box_resolve of the
S x frame), for output pixel (X, Y):

    window   = F1[max(Y-1, 0) .. min(Y+1, H-1)][max(X-1, 0) .. min(X+1, W-1)]     # clipped 3 x 3
    range_c  = max(window.c) - min(window.c)        for c in R, G, B (8-bit sRGB codes; alpha ignored)
    refined  = max(range_R, range_G, range_B) >= threshold          # threshold 0: all, 256: none
    A[Y][X]  = FS[Y][X] if refined else F1[Y][X];  alpha 255
"""
import numpy as np


def edge_mask(rgba, threshold):
    """rgba: [H, W, 4] uint8 -> [H, W] bool, True where the pixel is refined."""
    rgba = np.asarray(rgba, dtype=np.uint8)
    assert rgba.ndim == 3 and rgba.shape[2] == 4 and 0 <= threshold <= 256
    c = rgba[..., :3].astype(np.int32)
    h, w = c.shape[:2]
    # clamp-to-edge padding repeats texels of the clipped window, which changes neither max nor min
    pad = np.pad(c, ((1, 1), (1, 1), (0, 0)), mode="edge")
    hi = np.full_like(c, -1)
    lo = np.full_like(c, 256)
    for dy in range(3):
        for dx in range(3):
            win = pad[dy:dy + h, dx:dx + w]
            hi = np.maximum(hi, win)
            lo = np.minimum(lo, win)
    contrast = (hi - lo).max(axis=2)
    return contrast >= threshold


def compose(plain, ssaa, mask):
    """The adaptive frame: `ssaa` where mask, `plain` elsewhere, alpha 255."""
    plain, ssaa = np.asarray(plain, dtype=np.uint8), np.asarray(ssaa, dtype=np.uint8)
    assert plain.shape == ssaa.shape and mask.shape == plain.shape[:2]
    out = np.where(mask[..., None], ssaa, plain)
    out[..., 3] = 255
    return out
