"""frm_fast.h div_fix (the correctly rounded reciprocal, one Markstein correction and v_div_fixup)
against `/` bit for bit on the operand domains of the service pass's two divisions (the distance's
num / dr and the shadow closeness's de / t) and on the special values; and the
last tap's guarded normalize, inside and just outside its guard, against normalize(). The CPU half
pins the inputs: the oracle's `/` equals numpy's float32 `/` on them, the generated pairs lie
inside the stated domains and the end cases are present."""
import numpy as np
import pytest

import service_div_inputs as sd
from helpers import same_bits

DOMAINS = [sd.WIDE, sd.CLOSE, sd.NORMALIZE]
IDS = [d.name for d in DOMAINS]


@pytest.fixture(scope="module")
def gpu(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


_PAIRS = {}


def pairs(dom):
    if dom.name not in _PAIRS:
        a, b = sd.all_pairs(dom)
        a.setflags(write=False)
        b.setflags(write=False)
        _PAIRS[dom.name] = (a, b)
    return _PAIRS[dom.name]


def mismatches(got, ref, a, b, what):
    bad = ~((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref)))
    return bad, f"{what}: {bad.sum()} mismatches, e.g. a={a[bad][:3]} b={b[bad][:3]} gpu={got[bad][:3]} cpu={ref[bad][:3]}"


def numpy_div(a, b):
    with np.errstate(all="ignore"):
        return (a / b).astype(np.float32)


# ---- CPU half ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dom", DOMAINS, ids=IDS)
def test_pairs_lie_inside_the_stated_domain(dom):
    a, b = pairs(dom)
    assert a.dtype == np.float32 and b.dtype == np.float32 and len(a) == len(b) > 200000
    assert dom.contains(a, b).all()
    for part in (sd.random_pairs, sd.end_pairs, sd.mantissa_pairs, sd.power_of_two_quotient_pairs):
        pa, pb = part(dom)
        assert len(pa) and dom.contains(pa, pb).all(), part.__name__
    ra, _ = sd.random_pairs(dom)
    zeros = ra == 0
    assert 0.015 < zeros.mean() < 0.025 and np.signbit(ra[zeros]).any() and not np.signbit(ra[zeros]).all()


@pytest.mark.parametrize("dom", DOMAINS, ids=IDS)
def test_end_cases_are_present(dom):
    a, b = sd.end_pairs(dom)
    have = set(zip(a.view(np.uint32).tolist(), b.view(np.uint32).tolist()))

    def bits(x):
        return int(np.float32(x).view(np.uint32))

    for ea in (dom.a_lo, dom.a_hi):
        for eb in (dom.b_lo, dom.b_hi):
            assert (bits(2.0 ** ea), bits(2.0 ** eb)) in have and (bits(-(2.0 ** ea)), bits(2.0 ** eb)) in have
    assert (bits(0.0), bits(2.0 ** dom.b_hi)) in have and (bits(-0.0), bits(2.0 ** dom.b_lo)) in have
    if dom.b_zero:
        assert (bits(2.0 ** dom.a_lo), 0) in have and (bits(0.0), 0) in have and (bits(-0.0), 0) in have
    q = numpy_div(a, b).astype(np.float64)
    fin = np.isfinite(q) & (q != 0)
    assert np.abs(q[fin]).max() == 2.0 ** (dom.a_hi - dom.b_lo) and np.abs(q[fin]).min() == 2.0 ** (dom.a_lo - dom.b_hi)
    ma, mb = sd.mantissa_pairs(dom)
    mant = mb.view(np.uint32) & 0x7FFFFF
    expo = (mb.view(np.uint32) >> 23).astype(np.int64) - 127
    for e in range(dom.b_lo, dom.b_hi):
        assert (mant[expo == e] == 0).any() and (mant[expo == e] == 0x7FFFFF).any(), e
    pa, pb = sd.power_of_two_quotient_pairs(dom)
    pq = np.abs(numpy_div(pa, pb))
    near = np.minimum(pq.view(np.uint32) & 0x7FFFFF, 0x800000 - (pq.view(np.uint32) & 0x7FFFFF))
    assert (near <= 4).all() and (near == 0).any() and len(pa) > 20000


@pytest.mark.parametrize("which", IDS + ["special"])
def test_oracle_div_equals_numpy(oracle, which):
    a, b = sd.fixup_special_pairs() if which == "special" else pairs(DOMAINS[IDS.index(which)])
    assert same_bits(oracle.math_fn("div", a, b), numpy_div(a, b))


# ---- GPU half ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dom", DOMAINS, ids=IDS)
def test_div_fix_bit_exact_on_its_domain(gpu, oracle, dom):
    a, b = pairs(dom)
    bad, msg = mismatches(gpu.eval_math("div_fix", a, b), oracle.math_fn("div", a, b), a, b, "div_fix")
    assert not bad.any(), msg


@pytest.mark.gpu
def test_div_fix_special_values(gpu, oracle):
    """Zeros, infinities and NaN in either operand come from v_div_fixup, per lane: 0 / 0, x / 0,
    x / inf, NaN, and the sign of a zero quotient."""
    a, b = sd.fixup_special_pairs()
    bad, msg = mismatches(gpu.eval_math("div_fix", a, b), oracle.math_fn("div", a, b), a, b, "div_fix")
    assert not bad.any(), msg


@pytest.mark.gpu
@pytest.mark.parametrize("comp", ["x", "y"])
def test_normalize_guard(gpu, comp):
    """The last tap's normalize of (x, y, y) through its guard equals normalize() (the correctly
    rounded sqrt and three divisions, which the frames pin against the oracle)."""
    x, y = sd.normalize_inputs()
    got = gpu.eval_math(f"normalize_guarded_{comp}", x, y)
    ref = gpu.eval_math(f"normalize_{comp}", x, y)
    bad, msg = mismatches(got, ref, x, y, f"normalize {comp}")
    assert not bad.any(), msg
    assert np.isfinite(ref).mean() > 0.95
