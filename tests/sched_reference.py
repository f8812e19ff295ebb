"""Independent references for the persistent kernel's pixel scheduler (csrc/frm_sched.hip, DESIGN.md
section 3 "The scheduler: keys, order, resample"): the 8-bit cost key of a pixel, the properties
of a fetch order, the stable order of the sort path and the resample of a key map on a resize.
Pure numpy and integers: nothing here imports the library or the oracle, and nothing shares code
with the kernels.

The key. The device computes (uint8) min(255.0f, 16.0f * __log2f((float)c + 1.0f)): the hardware
log2 (1 ulp) of an exactly represented c + 1 (c < 2^24 below saturation), then one product. For a
key below 255 the logarithm is below 16 (an ulp of at most 2^-20), so 16 x its error is at most
2^-16, and the product (below 256: half an ulp is 2^-17; by 16 it is in fact exact) adds at most
2^-17: 1.5 x 2^-16 in all, inside the 1.5 x 2^-15 the band is sized for. With delta = 2^-12 (more
than 5 times that size), a cost whose
exact 16 log2(c + 1) lies within delta of an integer may take either neighbouring key; every
other cost has exactly one key. c + 1 = 2^k is the integer 16 k itself, where a logarithm one
ulp low would give 16 k - 1: the MI355X returns k exactly (10 631 such pixels over the cases of
sched_cases.py, launch by launch, none at 16 k - 1), so those costs, c = 0 among them, have the
one key 16 k.
"""
import numpy as np

DELTA = 2.0 ** -12
KEY_SCALE = 16.0
SATURATION_COST = 62757  # the smallest cost whose float64 key is 255: 16 log2(62758) = 255.00001
SATURATED_COST = 62902   # the cost the saturating cases are asked to pass (16 log2 = 255.05: 255 for certain)


def key_of(cost):
    """(key, lo, hi) uint8 arrays of cost's shape: key = floor(min(255, 16 log2(cost + 1))) in
    float64, and the inclusive range [lo, hi] of the keys the device may record (lo = hi = key
    except within DELTA of an integer)."""
    c = np.asarray(cost, dtype=np.uint64).astype(np.float64)
    v = KEY_SCALE * np.log2(c + 1.0)
    fl = np.floor(v)
    lo = np.where(v - fl < DELTA, fl - 1.0, fl)        # just above (or on) an integer: it or the one below
    hi = np.where(fl + 1.0 - v < DELTA, fl + 1.0, fl)  # just below an integer: either side
    n = np.asarray(cost, dtype=np.uint64) + np.uint64(1)
    lo = np.where((n & (n - np.uint64(1))) == 0, fl, lo)  # c + 1 = 2^k: the logarithm is exact
    clip = lambda a: np.clip(a, 0.0, 255.0).astype(np.uint8)
    return clip(fl), clip(lo), clip(hi)


def in_band(cost):
    """Costs whose key is not unique: 16 log2(cost + 1) within DELTA of an integer without being
    one (cost + 1 is no power of two)."""
    _, lo, hi = key_of(cost)
    return lo != hi


def keys_allowed(got, cost):
    """Per element: the recorded key lies in key_of(cost)'s allowed range."""
    g = np.asarray(got, dtype=np.int64)
    _, lo, hi = key_of(cost)
    return (g >= lo.astype(np.int64)) & (g <= hi.astype(np.int64))


def check_order(order, keys):
    """None if `order` is a permutation of 0..npix-1 along which keys never increase, else a
    sentence saying what is wrong."""
    order = np.asarray(order, dtype=np.int64)
    keys = np.asarray(keys, dtype=np.int64)
    n = keys.size
    if order.size != n:
        return f"the order has {order.size} entries for {n} pixels"
    if n == 0:
        return None
    if order.min() < 0 or order.max() >= n:
        return f"entries outside 0..{n - 1}: min {order.min()}, max {order.max()}"
    seen = np.bincount(order, minlength=n)
    if np.any(seen != 1):
        return (f"not a permutation: {int((seen == 0).sum())} pixels missing (first {int(np.argmax(seen == 0))}), "
                f"{int((seen > 1).sum())} repeated (first {int(np.argmax(seen > 1))})")
    k = keys[order]
    up = np.nonzero(k[1:] > k[:-1])[0]
    if up.size:
        i = int(up[0])
        return f"keys rise along the order at position {i}: {k[i]} then {k[i + 1]} ({up.size} rises)"
    return None


def stable_order(keys):
    """The order a stable descending sort of (key, pixel index) pairs gives: descending key, equal
    keys by ascending pixel index."""
    k = np.asarray(keys, dtype=np.int64)
    return np.argsort(255 - k, kind="stable").astype(np.uint32)


def footprint(i, s, d):
    """Source interval [a, b) of destination index i when s source pixels are resampled to d: the
    covered pixels [floor(i s / d), ceil((i + 1) s / d)), widened by one on both sides, clipped to
    the map, at most 8 from its first pixel. Integers only."""
    first = (i * s) // d
    end = -((-(i + 1) * s) // d)
    a = max(first - 1, 0)
    b = min(end + 1, s, a + 8)
    return a, b


def rescale(keys, sw, sh, dw, dh):
    """The key map a resized whole frame starts from: every destination pixel takes the largest key
    of its footprint (footprint() along each axis). keys: sw * sh values, row-major; returns the
    dw * dh values, row-major."""
    src = np.asarray(keys, dtype=np.uint8).reshape(sh, sw)
    cols = np.empty((sh, dw), dtype=np.uint8)
    for x in range(dw):
        a, b = footprint(x, sw, dw)
        cols[:, x] = src[:, a:b].max(axis=1)
    out = np.empty((dh, dw), dtype=np.uint8)
    for y in range(dh):
        a, b = footprint(y, sh, dh)
        out[y] = cols[a:b].max(axis=0)
    return out.reshape(-1)
