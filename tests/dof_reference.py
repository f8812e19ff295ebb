"""Expected values of the depth of field (include/frm.h frm_set_depth_of_field, frm_depth_of_field,
frm_dof_coc): the numpy float32 restatement of the pinned sequence. It shares no code with frm.

Inputs:

- A frame S of W x H RGBA8 sRGB texels.
- A depth plane Z of W x H f32 values.
- A, the aperture: the blur radius, in pixels, of a point at infinity. Finite, >= 0.
- F, the focus distance. Finite, > 0.
- R, the largest radius: an integer in 0..FRM_MAX_DOF_RADIUS, with FRM_MAX_DOF_RADIUS = 16.
- D, the blit's sRGB decode table.
- kPi = f32(pi).

All arithmetic is f32 with no contraction, and every division is an IEEE division.

Per pixel q (depends on q alone):

    c = A * fabsf(1.0f - F / Z[q])      (thin lens; Z = +inf gives c = A; Z = 0 gives +inf, or NaN when A = 0)
    if (!(c >= 0.0f)) c = 0.0f          (NaN: in focus)
    if (c > (float)R) c = (float)R
    a = c * c;   w = 1.0f / (kPi * a + 1.0f)

Per output pixel p: Start with sw = sr = sg = sb = 0.0f. Loop dy from -R to R, outer, top to bottom.
Loop dx from -R to R, inner, left to right. Let q = p + (dx, dy). Skip q when it lies outside the
frame: the window is clipped, not clamped.

    use_p = (Z[q] > Z[p]) && (c[p] < c[q])       (a sample behind p spreads no wider than p's own circle:
    a_e = use_p ? a[p] : a[q]                      no background bleeding onto a sharper foreground)
    w_e = use_p ? w[p] : w[q]
    if ((float)(dx*dx + dy*dy) <= a_e):
        sw = sw + w_e
        sr = sr + w_e * D[S[q].r]                  (one multiply, one add; likewise g, b)

Then:

    out[p] = encode(sr / sw), encode(sg / sw), encode(sb / sw), 255

encode is the sRGB store. The source alpha is ignored. Here D = oracle.srgb_decode() and encode =
oracle.encode_srgb, as panorama_reference.project takes them.
"""
import numpy as np

MAX_RADIUS = 16  # FRM_MAX_DOF_RADIUS
PI = np.float32(np.pi)  # kPi
# The GPU tests' kernel shapes (W, H, R): a frame smaller than the window, partial tiles at three
# radii, more than two 16 x 16 tiles each way plus a partial one, and a single pixel.
SHAPES = ((5, 3, 4), (37, 19, 1), (37, 19, 3), (37, 19, 16), (41, 35, 16), (1, 1, 16))
SIX_COLOURS = ((255, 0, 0), (0, 255, 255), (0, 255, 0), (255, 0, 255), (0, 0, 255), (255, 255, 0))


def coc(aperture, focus, radius, depth):
    """c of every depth (any shape), float32."""
    A, F, Rf = np.float32(aperture), np.float32(focus), np.float32(int(radius))
    z = np.asarray(depth, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = A * np.abs(np.float32(1.0) - F / z)
        c = np.where(c >= np.float32(0.0), c, np.float32(0.0))  # NaN: in focus
        c = np.where(c > Rf, Rf, c)
    assert c.dtype == np.float32
    return c


def area_weight(c):
    """(a, w) of c."""
    a = c * c
    w = np.float32(1.0) / (PI * a + np.float32(1.0))
    assert a.dtype == np.float32 and w.dtype == np.float32
    return a, w


def gather(src, depth, aperture, focus, radius, oracle, return_sums=False):
    """src: [H, W, 4] uint8 sRGB texels, depth: [H, W] float32 -> the blurred frame [H, W, 4] uint8
    (return_sums: the float32 sums (sw [H, W], s [H, W, 3]) instead)."""
    src = np.asarray(src, dtype=np.uint8)
    H, W = src.shape[:2]
    R = int(radius)
    assert src.shape == (H, W, 4) and 0 <= R <= MAX_RADIUS
    Z = np.asarray(depth, dtype=np.float32)
    assert Z.shape == (H, W)
    c = coc(aperture, focus, R, Z)
    a, w = area_weight(c)
    lin = oracle.srgb_decode().astype(np.float32)[src[..., :3]]  # [H, W, 3]
    sw = np.zeros((H, W), np.float32)
    s = np.zeros((H, W, 3), np.float32)
    zero = np.float32(0.0)
    for dy in range(-R, R + 1):
        # rows p with 0 <= p + dy < H
        p0, p1 = max(0, -dy), min(H, H - dy)
        if p0 >= p1:
            continue
        for dx in range(-R, R + 1):
            x0, x1 = max(0, -dx), min(W, W - dx)
            if x0 >= x1:
                continue
            P = (slice(p0, p1), slice(x0, x1))
            Q = (slice(p0 + dy, p1 + dy), slice(x0 + dx, x1 + dx))
            with np.errstate(invalid="ignore"):
                use_p = (Z[Q] > Z[P]) & (c[P] < c[Q])
                a_e = np.where(use_p, a[P], a[Q])
                w_e = np.where(use_p, w[P], w[Q])
                ok = np.float32(dx * dx + dy * dy) <= a_e
            sw[P] = np.where(ok, sw[P] + w_e, sw[P])
            s[P] = np.where(ok[..., None], s[P] + w_e[..., None] * lin[Q], s[P])
            assert a_e.dtype == np.float32 and w_e.dtype == np.float32
    assert sw.dtype == np.float32 and s.dtype == np.float32 and np.all(sw > zero)
    if return_sums:
        return sw, s
    out = np.empty((H, W, 4), np.uint8)
    out[..., :3] = oracle.encode_srgb(np.ascontiguousarray(s / sw[..., None]))
    out[..., 3] = 255
    return out


def test_depths(rng, W, H):
    """The GPU tests' depth planes: random in [0.5, 6], 30 % +inf, and planted 0, NaN and negative
    values (where the frame has room for them)."""
    z = rng.uniform(0.5, 6.0, size=(H, W)).astype(np.float32)
    z[rng.random((H, W)) < 0.3] = np.inf
    flat = z.reshape(-1)
    for k, v in enumerate((0.0, np.nan, -1.5, -0.0)):
        if flat.size > 2 * k + 1:
            flat[(flat.size * (2 * k + 1)) // 9 % flat.size] = v
    return z


test_depths.__test__ = False  # (not a test: pytest imports this module)


def six_colour_frame(W, H):
    """Vertical stripes of the six colours, alpha 255."""
    f = np.empty((H, W, 4), np.uint8)
    f[..., :3] = np.asarray(SIX_COLOURS, np.uint8)[(np.arange(W) * 6) // max(W, 1)][None, :, :]
    f[..., 3] = 255
    return f
