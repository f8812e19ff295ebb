"""The two float32 identities the persistent march kernel's full service pass relies on
(frm_render_kernels.h FRM_TAP_OFFSET, kTapStore), checked bit for bit in numpy float32:

* x + (-0.0) has the bits of x for every x that is not a NaN, both zeros and the denormals
  included, and a NaN stays a NaN: a lane that is no normal tap may add -0.0f to its sample point
  instead of selecting the point without an offset;
* the normal's three sums formed at the fourth tap from the four stored tap distances equal the
  sums carried from tap to tap (fragment.wgsl's accumulation as the kernel states it: tap 0 sets
  the sum to s_0 * d, taps 1..3 add s_k * d, with s_0..s_3 = (+--), (--+), (-+-), (+++)).

Both sides of the second identity are written out operation by operation in float32."""
import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
MIN_NORMAL = 2.0 ** -126
DENORMALS = [2.0 ** -149, 2.0 ** -140, 2.0 ** -127, (2.0 ** 23 - 1) * 2.0 ** -149]
SIGNS = [(1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1)]  # s_k of tap k = 0..3, per component


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def random_encodings(rng, n):
    """n random float32 bit patterns (every class: NaNs, infinities, denormals, zeros)."""
    return rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(F32)


def random_finite(rng, n):
    x = random_encodings(rng, n + n // 64 + 64)
    return x[np.isfinite(x)][:n]


def test_adding_negative_zero_keeps_the_bits():
    specials = [0.0, MIN_NORMAL, 1.0, FLT_MAX, np.inf] + DENORMALS
    x = np.array(specials + [-v for v in specials], F32)
    assert (bits(x)[: len(specials)] >> 31 == 0).all() and (bits(x)[len(specials):] >> 31 == 1).all()
    x = np.concatenate([x, random_encodings(np.random.default_rng(12), 100000)])
    with np.errstate(invalid="ignore"):
        y = x + F32(-0.0)
    assert y.dtype == F32
    nan = np.isnan(x)
    assert nan.any() and (~nan).sum() > 90000
    assert np.array_equal(bits(y)[~nan], bits(x)[~nan])
    assert np.isnan(y[nan]).all()
    # the other zero would not do: -0 + +0 is +0
    assert bits(F32(-0.0) + F32(0.0)) == 0 and bits(F32(-0.0) + F32(-0.0)) == 0x80000000


def running_sums(d):
    """The sums as the pass carried them: d[:, k] is tap k's distance; -> [n, 3]."""
    out = []
    for c in range(3):
        s = F32(SIGNS[0][c]) * d[:, 0]              # tap 0 sets the sum (a product by +-1: exact)
        for k in (1, 2, 3):
            term = d[:, k] if SIGNS[k][c] > 0 else -d[:, k]   # the select of +-d
            s = s + term                                      # one f32 addition per tap
        out.append(s)
    return np.stack(out, axis=-1)


def stored_sums(d):
    """The sums formed at the fourth tap from the stored distances d0, d1, d2 and the tap's own d3."""
    d0, d1, d2, d3 = (d[:, k] for k in range(4))
    x = ((d0 + -d1) + -d2) + d3
    y = ((-d0 + -d1) + d2) + d3
    z = ((-d0 + d1) + -d2) + d3
    return np.stack([x, y, z], axis=-1)


def same_sums(d):
    d = np.ascontiguousarray(d, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = running_sums(d), stored_sums(d)
    assert a.dtype == F32 and b.dtype == F32
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(bits(a)[~nan], bits(b)[~nan])
    return a


def test_tap_sums_of_random_distances():
    rng = np.random.default_rng(34)
    same_sums(random_finite(rng, 400000).reshape(-1, 4))
    # distances of the size the march meets (around MIN_DISTANCE), where the sums cancel
    same_sums((5e-7 * (1.0 + 1e-3 * rng.standard_normal((100000, 4)))).astype(F32))


def test_tap_sums_with_equal_distances_give_the_same_zeros():
    rng = np.random.default_rng(56)
    v = random_finite(rng, 20000)
    w = random_finite(rng, 20000)
    quads = [np.stack(q, axis=-1) for q in (
        (v, v, v, v), (v, v, w, w), (v, w, v, w), (v, w, w, v), (v, -v, w, -w), (v, w, -v, -w),
        (v, v, v, w), (w, v, v, v), (0 * v, 0 * v, 0 * w, 0 * w), (0 * v, -0 * v, v, v), (v, v, 0 * v, -0 * v))]
    zeros = np.array([[a, b, c, d] for a in (0.0, -0.0) for b in (0.0, -0.0) for c in (0.0, -0.0) for d in (0.0, -0.0)], F32)
    sums = same_sums(np.concatenate(quads + [zeros]))
    z = sums[sums == 0]
    assert (bits(z) == 0).any() and (bits(z) == 0x80000000).any()  # exact zeros of both signs arose


def test_tap_sums_with_inf_and_nan():
    vals = np.array([np.inf, -np.inf, np.nan, 1.0, -2.5, 0.0, -0.0, FLT_MAX, -FLT_MAX, 5e-7], F32)
    grid = np.stack(np.meshgrid(vals, vals, vals, vals, indexing="ij"), axis=-1).reshape(-1, 4)
    sums = same_sums(grid)
    assert np.isnan(sums).any() and np.isinf(sums).any()
