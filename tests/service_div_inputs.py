"""Operands for the division ended by v_div_fixup (frm_fast.h div_fix) and for the last tap's
guarded normalize: plain float32 arrays, every pair inside the stated domain of one of the service
pass's two divisions, the values v_div_fixup supplies, and vectors inside and just outside the
normalize guard. Shared by the CPU and GPU halves of test_gpu_service_div.py."""
from dataclasses import dataclass

import numpy as np

from edge_cases import _ulps


@dataclass(frozen=True)
class Domain:
    """a in {+-0} U +-[2^a_lo, 2^a_hi], b in [2^b_lo, 2^b_hi] (b > 0), and b = +0 if b_zero."""
    name: str
    a_lo: int
    a_hi: int
    b_lo: int
    b_hi: int
    b_zero: bool = False

    def contains(self, a, b):
        a = np.abs(np.asarray(a, np.float32).astype(np.float64))
        bb = np.asarray(b, np.float32)
        b64 = bb.astype(np.float64)
        a_ok = (a == 0) | ((a >= 2.0 ** self.a_lo) & (a <= 2.0 ** self.a_hi))
        b_ok = (b64 >= 2.0 ** self.b_lo) & (b64 <= 2.0 ** self.b_hi)
        if self.b_zero:
            b_ok |= bb.view(np.uint32) == 0  # exactly +0
        return a_ok & b_ok


# the distance's num / dr and the shadow closeness's de / t ("Operand ranges of
# the two divisions")
WIDE = Domain("wide", -24, 100, 0, 100)
CLOSE = Domain("close", -100, 40, -21, 10, b_zero=True)
# the last tap's normalize: components of at least 2^-62 by a length in [2^-48, 2^63] (frm_scene.h
# normalize_wide; the rectangle is wider than |component| <= length allows)
NORMALIZE = Domain("normalize", -62, 63, -48, 63)


def _inside(lo, hi, ks=range(4)):
    """The values within 3 encodings of each end of [2^lo, 2^hi], inside it."""
    return np.concatenate([_ulps(2.0 ** lo, list(ks)), _ulps(2.0 ** hi, [-k for k in ks])])


def random_pairs(dom, n=200000, seed=21):
    """n pairs log-uniform over the domain, 2 % of the numerators +-0."""
    rng = np.random.default_rng(seed)
    a = np.clip(np.exp2(rng.uniform(dom.a_lo, dom.a_hi, n)), 2.0 ** dom.a_lo, 2.0 ** dom.a_hi)
    a = (a * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    z = rng.random(n) < 0.02
    a[z] = np.where(rng.random(z.sum()) < 0.5, np.float32(0.0), np.float32(-0.0))
    b = np.clip(np.exp2(rng.uniform(dom.b_lo, dom.b_hi, n)), 2.0 ** dom.b_lo, 2.0 ** dom.b_hi).astype(np.float32)
    return a, b


def end_pairs(dom):
    """Every pair of values within 3 encodings of the domain's ends (both signs of a, +-0): the
    extreme quotients 2^a_hi / 2^b_lo and 2^a_lo / 2^b_hi among them."""
    va = _inside(dom.a_lo, dom.a_hi)
    va = np.concatenate([va, -va, np.array([0.0, -0.0], np.float32)])
    vb = _inside(dom.b_lo, dom.b_hi)
    if dom.b_zero:
        vb = np.concatenate([vb, np.array([0.0], np.float32)])
    a, b = (g.ravel() for g in np.meshgrid(va, vb))
    return a.copy(), b.copy()


def mantissa_pairs(dom, per=8, seed=22):
    """Divisors with an all-zeros and an all-ones mantissa at every exponent of the domain, each
    against `per` random numerators."""
    rng = np.random.default_rng(seed)
    es = np.arange(dom.b_lo, dom.b_hi)
    zeros = np.exp2(es.astype(np.float64)).astype(np.float32)
    ones = _ulps_each(np.exp2(es + 1.0).astype(np.float32), -1)
    b = np.repeat(np.concatenate([zeros, ones, np.float32([2.0 ** dom.b_hi])]), per)
    a, _ = random_pairs(dom, len(b), seed=int(rng.integers(1 << 30)))
    return a, b


def _ulps_each(x, k):
    return (np.asarray(x, np.float32).view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(np.float32)


def power_of_two_quotient_pairs(dom, n=4000, seed=23):
    """Numerators that put the quotient within 3 encodings of a power of two (4 after the
    numerator's own rounding): a = RN(q b) for q = 2^k moved by -3..3 encodings (b random over the
    domain, k random over what keeps a inside it)."""
    rng = np.random.default_rng(seed)
    _, b = random_pairs(dom, n, seed=seed + 1)
    eb = np.floor(np.log2(b.astype(np.float64)))
    k = np.floor(rng.uniform(dom.a_lo - eb + 1, dom.a_hi - eb - 1)).astype(np.int64)
    q0 = np.ldexp(np.ones(n), k).astype(np.float32) * rng.choice([-1.0, 1.0], n).astype(np.float32)
    a = np.concatenate([(_ulps_each(q0, j).astype(np.float64) * b.astype(np.float64)).astype(np.float32)
                        for j in range(-3, 4)])
    b = np.tile(b, 7)
    keep = dom.contains(a, b)
    return a[keep], b[keep]


def all_pairs(dom):
    parts = [random_pairs(dom), end_pairs(dom), mantissa_pairs(dom), power_of_two_quotient_pairs(dom)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _waves(a_in, b_in, a_out, b_out, seed):
    """64-lane waves (eval_math's blocks are four consecutive waves): for every outside pair one
    wave of inside pairs with that pair in a random lane, then one wave of inside pairs alone, so
    the fallback and the fast path run beside each other."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for k in range(len(a_out)):
        idx = rng.integers(0, len(a_in), 128)
        wa, wb = a_in[idx].copy(), b_in[idx].copy()
        lane = int(rng.integers(0, 64))
        wa[lane], wb[lane] = a_out[k], b_out[k]
        a.append(wa)
        b.append(wb)
    return np.concatenate(a), np.concatenate(b)


F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)


def fixup_special_pairs():
    """The cross product of the values div_fixup supplies the quotient for (zeros, infinities,
    NaN) with themselves and with ordinary operands of both domains."""
    v = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -3.0, 2.0 ** -21, 2.0 ** 10, 2.0 ** 100, 2.0 ** -24,
                  -2.0 ** 40, 2.0 ** -100], F32)
    a, b = (g.ravel() for g in np.meshgrid(v, v))
    return a.copy(), b.copy()


def normalize_inputs(seed=41):
    """(x, y) of the vectors (x, y, y) for the last tap's normalize, in whole waves: ordinary sums
    of four distances, lengths at both ends of sqrt_rsq's range, components at the 2^-62 bound,
    and waves with a lane outside the guard (zero vector, zero or tiny component, inf, NaN,
    overflowing and underflowing dot products)."""
    rng = np.random.default_rng(seed)
    n = 64 * 512
    mag = np.exp2(rng.uniform(-47, 62, n))
    x = (mag * rng.uniform(0.05, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    y = (mag * rng.uniform(0.05, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    x[: n // 2] = (rng.uniform(-4e-6, 4e-6, n // 2)).astype(F32)  # the taps' sums: +-4 de around MIN_DISTANCE
    y[: n // 2] = (rng.uniform(-4e-6, 4e-6, n // 2)).astype(F32)
    # the ends: dot = x^2 + 2 y^2 around 2^-96 and 2^126, components around 2^-62
    ex = np.concatenate([_ulps(2.0 ** -48, range(-3, 4)), _ulps(2.0 ** 62, range(-3, 4)), _ulps(2.0 ** -62, range(-3, 4))])
    ey = np.concatenate([_ulps(2.0 ** -49, range(-3, 4)), _ulps(2.0 ** 62, range(-3, 4)), _ulps(2.0 ** -62, range(-3, 4))])
    gx, gy = (g.ravel() for g in np.meshgrid(np.concatenate([ex, -ex]), np.concatenate([ey, -ey])))
    out_x = np.array([0.0, 0.0, 1.0, -0.0, 2.0 ** -63, 1.0, np.inf, 1.0, np.nan, 1.0, 2.0 ** 64, 2.0 ** -60, 2.0 ** -80,
                      3e38, 1e-45], F32)
    out_y = np.array([0.0, 1.0, 0.0, -0.0, 1.0, 2.0 ** -63, 1.0, -np.inf, 1.0, np.nan, 2.0 ** 64, 2.0 ** -60, 2.0 ** -80,
                      3e38, 1e-45], F32)
    mx, my = _waves(x[n // 2: n // 2 + 4096], y[n // 2: n // 2 + 4096], out_x, out_y, seed + 1)
    mx2, my2 = _waves(x[:4096], y[:4096], out_x, out_y, seed + 2)
    return (np.concatenate([x, gx.astype(F32), mx, mx2]), np.concatenate([y, gy.astype(F32), my, my2]))
