"""The builtin input sets of tests/builtin_cases.py on the CPU. (i) A census from numpy alone: each
builtin's sets reach every branch, clamp end, tie and special operand they are built for, so the
GPU test (test_gpu_builtins_whole_type.py) cannot silently test nothing. (ii) The oracle against
float64 over those sets wherever WGSL or frm_math.h states a bound. (iii) Where no bound exists
the oracle's bits are recorded (tests/golden/builtin_specials.json) and DESIGN.md section 2 shows
them. (iv) The x86-64 build of frm_math.h equals the oracle bit for bit on every set."""
import ctypes
import json
import os

import numpy as np
import pytest

import builtin_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "builtin_specials.json")
HR_FN = {"sin": 0, "cos": 1, "acos": 2, "atan2": 3, "log": 4, "log2": 5, "exp2": 6, "pow": 7}


def ulps(got, ref):
    """|got - ref| in units of the float32 spacing at ref (2^-149 at and below the subnormals)."""
    return np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


# ---- (i) the census --------------------------------------------------------------------------------
def test_whole_type_holds_every_sign_and_exponent_field():
    w = bc.whole_type()
    b = bc.bits_of(w)
    assert len(w) == 2 * 256 * (len(bc.FIXED_MANTISSAS) + bc.RANDOM_MANTISSAS) == 530432
    field, mant = b >> np.uint32(23), b & np.uint32(0x7FFFFF)
    assert np.array_equal(np.unique(field), np.arange(512))
    for f in (0, 1, 127, 254, 255, 256, 511):
        m = mant[field == f]
        assert len(m) == 1036 and set(bc.FIXED_MANTISSAS) <= set(m.tolist()) and len(np.unique(m)) > 1000
    assert np.isnan(w).sum() == 2 * 1035 and np.isinf(w).sum() == 2 and (w == 0).sum() == 2
    for v in (np.sqrt(2.0), np.sqrt(0.5)):
        assert int(np.float32(v).view(np.uint32)) & 0x7FFFFF == bc.SQRT2_MANT


@pytest.mark.parametrize("name", bc.NAMES)
def test_sets_reach_their_strata(name):
    for label, a, b in bc.sets(name):
        assert a.dtype == np.float32 and 0 < len(a) <= bc.MAX_SET, (label, len(a))
        assert (b is None) == (name not in bc.BINARY) and (b is None or (b.dtype == np.float32 and len(b) == len(a)))
    st = bc.strata(name)
    for label, count, least in st:
        print(f"{name}: {label}: {count} (at least {least})")
    missed = [(label, count, least) for label, count, least in st if count < least]
    assert not missed, f"{name}: the sets miss {missed}"


def test_thinned_pairs_and_parity_point():
    t = bc.thinned()
    assert len(t) == 444 and len(np.unique(bc.bits_of(t))) == 444
    assert len(bc.get_set("atan2", "thinned_cross")[0]) == 444 * 444 >= 150000
    # the parity point: x * kInvPiHi is within one float32 spacing of 2^24, and above 2^20
    x = np.float64(bc.PARITY_X)
    assert abs(x * bc.INV_PI_HI - 2.0 ** 24) <= 2.0 and x > 2.0 ** 20
    assert 1e6 < 2.0 ** 20  # the value test_builtin_bit_exact calls "large" stays in the first branch


# ---- (ii) the oracle against float64 ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["sin", "cos"])
def test_sin_cos_within_wgsl_bound_up_to_2p20(oracle, name):
    """Absolute error <= 2^-11 for every |x| <= 2^20 of the sets: the header claims an exact j
    there, so the bound WGSL states for [-pi, pi] holds on the whole first branch."""
    a, _ = bc.union(name)
    a = a[np.abs(a) <= np.float32(2.0 ** 20)]
    assert len(a) > 1_000_000
    ref = (np.sin if name == "sin" else np.cos)(a.astype(np.float64))
    err = np.abs(oracle.math_fn(name, a).astype(np.float64) - ref)
    print(f"{name}: {len(a)} inputs, max abs error {err.max():.3g} at x = {a[np.argmax(err)]!r}")
    assert err.max() <= 2.0 ** -11


@pytest.mark.parametrize("name", ["log", "log2"])
def test_log_of_subnormals_within_3_ulp(oracle, name):
    a, _ = bc.union(name)
    a = a[(a > 0) & (a < np.float32(2.0 ** -126))]
    assert len(a) >= 20000
    ref = (np.log if name == "log" else np.log2)(a.astype(np.float64))
    e = ulps(oracle.math_fn(name, a), ref)
    print(f"{name}: {len(a)} subnormal inputs, max error {e.max():.3g} ulp at x = {a[np.argmax(e)]!r}")
    assert e.max() <= 3


def test_exp2_subnormal_results_within_wgsl_bound(oracle):
    """Where the float64 result is subnormal in float32: within 3 + 2|x| units of 2^-149."""
    a, _ = bc.union("exp2")
    with np.errstate(all="ignore"):
        x = a.astype(np.float64)
        ref = np.exp2(x)
    sel = (ref > 0) & (ref < 2.0 ** -126)
    assert sel.sum() >= 100000
    err = np.abs(oracle.math_fn("exp2", a[sel]).astype(np.float64) - ref[sel]) / 2.0 ** -149
    print(f"exp2: {sel.sum()} subnormal results, max error {err.max():.3g} units of 2^-149 at x = {a[sel][np.argmax(err)]!r}")
    assert np.all(err <= 3 + 2 * np.abs(x[sel]))


def test_acos_within_4096_ulp_on_the_domain(oracle):
    a, _ = bc.union("acos")
    a = a[np.abs(a) <= 1]
    assert len(a) >= 100000
    e = ulps(oracle.math_fn("acos", a), np.arccos(a.astype(np.float64)))
    print(f"acos: {len(a)} inputs of [-1, 1], max error {e.max():.3g} ulp at t = {a[np.argmax(e)]!r}")
    assert e.max() <= 4096


def test_atan2_within_4096_ulp_where_defined(oracle):
    """Finite operands with max(|x|, |y|) >= 2^-126, wherever the float64 result is a normal
    float32. Nothing else is left out; most stratified pairs have extreme ratios, so what is
    asserted is that at least 100 k pairs stay in."""
    y, x = bc.union("atan2")
    with np.errstate(all="ignore"):
        y64, x64 = y.astype(np.float64), x.astype(np.float64)
        ref = np.arctan2(y64, x64)
        sel = np.isfinite(y64) & np.isfinite(x64) & (np.maximum(np.abs(x64), np.abs(y64)) >= 2.0 ** -126)
        sel &= (np.abs(ref) >= 2.0 ** -126)
    assert sel.sum() >= 100000, sel.sum()
    e = ulps(oracle.math_fn("atan2", y[sel], x[sel]), ref[sel])
    k = np.argmax(e)
    print(f"atan2: {sel.sum()} of {len(y)} pairs, max error {e.max():.3g} ulp at y = {y[sel][k]!r}, x = {x[sel][k]!r}")
    assert e.max() <= 4096


# ---- (iii) recorded, not judged ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", bc.NAMES)
def test_oracle_reproduces_the_recorded_specials(oracle, golden, name):
    rec = golden["builtins"][name]
    a, b = bc.specials(name)
    hexes = lambda v: [f"{int(u):08x}" for u in v]  # noqa: E731
    assert rec["a"] == hexes(bc.bits_of(a)), "the list of specials changed: record the file again"
    assert (b is None) == ("b" not in rec) and (b is None or rec["b"] == hexes(bc.bits_of(b)))
    got = hexes(bc.canonical_bits(oracle.math_fn(name, a, b)))
    bad = [i for i, (g, w) in enumerate(zip(got, rec["out"])) if g != w]
    assert not bad, (f"{name}: {len(bad)} specials differ, e.g. a={a[bad[0]]!r} b={None if b is None else b[bad[0]]!r} "
                     f"oracle=0x{got[bad[0]]} recorded=0x{rec['out'][bad[0]]}")


def test_specials_hold_the_non_finite_and_tiny_operands():
    """Every builtin's list holds zeros of both signs, an infinity and a NaN in each operand, and a
    subnormal in the first."""
    for name in bc.NAMES:
        a, b = bc.specials(name)
        for v in (a, b):
            if v is None:
                continue
            assert np.isnan(v).any() and np.isinf(v).any() and (bc.bits_of(v) == 0x80000000).any() and (bc.bits_of(v) == 0).any()
        assert ((bc.mag_bits(a) > 0) & (bc.mag_bits(a) < 0x00800000)).any(), name
    assert 300 <= sum(len(bc.specials(n)[0]) for n in bc.NAMES) <= 1000


def test_recorded_semantics_named_by_the_issue(golden):
    """What the record says in words (frm semantics v3; recorded here, not changed)."""
    def out(name, a, b=None):
        rec = golden["builtins"][name]
        ka = f"{int(np.float32(a).view(np.uint32)):08x}"
        kb = None if b is None else f"{int(np.float32(b).view(np.uint32)):08x}"
        i = [i for i, h in enumerate(rec["a"]) if h == ka and (b is None or rec["b"][i] == kb)][0]
        return bc.f32(np.array([int(rec["out"][i], 16)]))[0]

    assert np.isnan(out("atan2", 2.0 ** -129, 2.0 ** -129)) and np.isnan(out("atan2", 2.0 ** -149, 0.0))
    # minNum / maxNum drop the NaN: atan2(1, NaN) is atan2(1, 1), pi / 4 to 2 ulp
    assert out("atan2", 1.0, np.nan) == out("atan2", 1.0, 1.0) and abs(float(out("atan2", 1.0, 1.0)) - np.pi / 4) < 2e-7
    assert abs(float(out("sin", 1e10))) > 1e19 and out("sin", 1e30) == np.inf and out("cos", 1e30) == np.inf
    assert np.isnan(out("pow", -2.0, 2.0)) and np.isnan(out("pow", 0.0, 0.0)) and np.isnan(out("pow", 1.0, np.inf))
    assert np.isnan(out("acos", 1.0000001)) and np.isnan(out("acos", -2.0))


def test_design_md_shows_the_recorded_table(golden):
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    assert "Builtins outside the hot path's ranges" in text
    missing = [line for line in bc.design_table(golden) if line not in text]
    assert not missing, f"DESIGN.md lacks rows of `make_builtin_specials.py --table`: {missing[:3]}"


def test_subnormal_atan2_pairs_are_nan_up_to_2pm128(oracle):
    """The atan2 NaN region, from the sets: every pair of finite operands with 0 < max(|x|, |y|)
    <= 2^-128 gives NaN (RN(1 / max) is inf there: 0 * inf, or inf - inf in the polynomial), and no
    pair of finite operands with a larger maximum does."""
    y, x = bc.union("atan2")
    mx = np.maximum(bc.mag_bits(y), bc.mag_bits(x))
    fin = mx < 0x7F800000
    t128 = int(np.float32(2.0 ** -128).view(np.uint32))
    got = oracle.math_fn("atan2", y, x)
    low = fin & (mx > 0) & (mx <= t128)
    assert low.sum() >= 100 and (mx == t128).sum() >= 6 and np.isnan(got[low]).all()
    assert not np.isnan(got[fin & (mx > t128)]).any()


# ---- (iv) the host build ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,label", bc.set_ids(), ids=[f"{n}-{l}" for n, l in bc.set_ids()])
def test_host_build_equals_oracle(host_replay, oracle, name, label):
    a, b = bc.get_set(name, label)
    out = np.zeros_like(a)
    rc = host_replay.hr_math(HR_FN[name], ctypes.c_void_p(a.ctypes.data), None if b is None else ctypes.c_void_p(b.ctypes.data),
                             ctypes.c_uint32(a.size), ctypes.c_void_p(out.ctypes.data))
    assert rc == 0
    ref = oracle.math_fn(name, a, b)
    assert not bc.mismatches(out, ref).any(), bc.report(name, label, a, b, out, ref, who="host")
