"""The eight frm builtins on the device over all of float32: Renderer.eval_math equals the CPU
oracle bit for bit (NaN matches NaN, the sign of zero counts) on every input set of
tests/builtin_cases.py: the second branch of sincos_ and its parity rule, frexpf on
subnormals, ldexpf at the clamp ends and with subnormal results, rint's ties, atan2's reciprocal
where it overflows or goes subnormal, NaN through minNum / maxNum, acos outside [-1, 1], pow of
negative, zero and infinite bases. These are the places where the device lowering of frexpf,
ldexpf, rintf, fminf, fmaxf, the float to int conversion or denormal handling can differ from
x86-64 while the source is the same. tests/test_builtin_census.py proves on the CPU that the sets
reach those places and that the x86-64 build agrees with the oracle there. The fast paths
(frm_fast.h) keep their own domain tests in test_gpu_de.py.

One difference was found this way: the device's fminf / fmaxf drop a signalling NaN as they drop
a quiet one, where IEEE minNum / maxNum and the oracle answer NaN (5,148 of the 197,136 atan2
pairs: atan2(0, sNaN) was 0). The device's atan2_ now tests its operands for one."""
import numpy as np
import pytest

import builtin_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


_SET_IDS = bc.set_ids()


@pytest.mark.parametrize("name,label", _SET_IDS, ids=[f"{n}-{l}" for n, l in _SET_IDS])
def test_builtin_equals_oracle_on_the_set(gpu, oracle, name, label):
    a, b = bc.get_set(name, label)
    assert len(a) <= bc.MAX_SET
    got = gpu.eval_math(name, a, b)
    ref = oracle.math_fn(name, a, b)
    assert not bc.mismatches(got, ref).any(), bc.report(name, label, a, b, got, ref)


@pytest.mark.parametrize("name", bc.NAMES)
def test_builtin_equals_oracle_on_the_recorded_specials(gpu, oracle, name):
    a, b = bc.specials(name)
    got = gpu.eval_math(name, a, b)
    ref = oracle.math_fn(name, a, b)
    assert not bc.mismatches(got, ref).any(), bc.report(name, "specials", a, b, got, ref)


@pytest.mark.parametrize("name", ["sqrt", "div"])
def test_sqrt_and_div_on_the_whole_type(gpu, oracle, name):
    """sqrt on every element of whole_type() (negative operands and NaN included); div on
    whole_type() against a seeded permutation of itself and against the thinned operands."""
    a = bc.whole_type()
    if name == "sqrt":
        b = None
    else:
        b = a[np.random.default_rng(9).permutation(len(a))]
        t = bc.thinned()
        ta, tb = (g.ravel() for g in np.meshgrid(t, t, indexing="ij"))
        a, b = np.concatenate([a, ta]), np.concatenate([b, tb])
    got = gpu.eval_math(name, a, b)
    ref = oracle.math_fn(name, a, b)
    assert not bc.mismatches(got, ref).any(), bc.report(name, "whole_type", a, b, got, ref)
