"""The tame Mandelbulb body's two shortcuts that lean on mb_tame()'s admission test (frm_scene.h):
atan2_tame_nz takes the sign of x from x's own sign bit, since no component of an admitted wave
is a zero, and the z sign goes onto pow(r, P) with an or, since that product is positive. Both must
give the oracle's bits: atan2_tame_nz over its whole stated domain (both magnitudes in
[2^-60, 2^40], every sign combination), and the body over whole waves of points of every sign
pattern at powers 4, 8 and 9, with waves in which one lane holds a zero of either sign (the wave
then takes the exact body)."""
import numpy as np
import pytest

import edge_cases as ec
import frm
from helpers import params_for, same_bits

pytestmark = pytest.mark.gpu

LO, HI = 2.0 ** -60, 2.0 ** 40


def _near(x, ks):
    """float32 x moved by each of ks encodings."""
    b = np.float32(x).view(np.uint32).astype(np.int64)
    return (b + np.asarray(ks, np.int64)).astype(np.uint32).view(np.float32)


def atan2_nz_inputs():
    """(y, x) float32 magnitudes in [2^-60, 2^40], then every sign combination of each pair."""
    rng = np.random.default_rng(26)
    n = 50000  # x 4 sign combinations = 200 k pairs
    y = np.clip(np.exp2(rng.uniform(-60, 40, n)), LO, HI).astype(np.float32)
    x = np.clip(np.exp2(rng.uniform(-60, 40, n)), LO, HI).astype(np.float32)
    # |x| = |y| over the range, and ratios within 3 encodings of 1 (both sides)
    eq = np.clip(np.exp2(rng.uniform(-60, 40, 2000)), LO, HI).astype(np.float32)
    ks = np.arange(-3, 4)
    base = eq[:700]
    base = base[(base > 2 * LO) & (base < HI / 2)]
    near_y = np.concatenate([_near(v, ks) for v in base])
    near_x = np.repeat(base, len(ks))
    # both ends of the range against each other, against 1 and against their neighbours inside it
    ends = np.concatenate([_near(LO, np.arange(0, 4)), _near(HI, np.arange(-3, 1)), np.float32([1.0])])
    ey, ex = (g.ravel() for g in np.meshgrid(ends, ends))
    my = np.concatenate([y, eq, near_y, ey])
    mx = np.concatenate([x, eq, near_x, ex])
    assert my.min() >= LO and mx.min() >= LO and my.max() <= HI and mx.max() <= HI
    ys = np.concatenate([sy * my for sy in (1, -1) for _ in (1, -1)]).astype(np.float32)
    xs = np.concatenate([sx * mx for _ in (1, -1) for sx in (1, -1)]).astype(np.float32)
    return ys, xs


def test_atan2_tame_nz_bit_exact_on_its_domain(gpu_renderer_factory, oracle):
    y, x = atan2_nz_inputs()
    assert y.size >= 200000 and (y == x).sum() >= 2000 and (np.abs(y) == np.abs(x)).sum() >= 8000
    with gpu_renderer_factory() as r:
        got = r.eval_math("atan2_tame_nz", y, x)
        also = r.eval_math("atan2_tame", y, x)
    ref = oracle.math_fn("atan2", y, x)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not np.isnan(ref).any()
    assert not bad.any(), f"{bad.sum()} mismatches, e.g. y={y[bad][:3]} x={x[bad][:3]} gpu={got[bad][:3]} cpu={ref[bad][:3]}"
    assert np.array_equal(also.view(np.uint32), ref.view(np.uint32))  # the form that also takes zeros


def body_points():
    """64 x 200 points of [-1.3, 1.3]^3, lane by lane: 100 waves of random signs, 96 waves of one
    sign pattern each (12 per pattern), and 4 waves of random signs in which lane 5 has a zero:
    x = -0, x = +0, y = -0, z = -0."""
    rng = np.random.default_rng(9)
    mag = rng.uniform(2.0 ** -20, 1.3, size=(200, 64, 3))
    sign = rng.choice([-1.0, 1.0], size=(200, 64, 3))
    for k in range(96):
        sign[100 + k] = [1.0 if (k % 8) >> b & 1 else -1.0 for b in range(3)]
    pts = (mag * sign).astype(np.float32)
    for wave, (comp, zero) in zip(range(196, 200), [(0, -0.0), (0, 0.0), (1, -0.0), (2, -0.0)]):
        pts[wave, 5, comp] = zero
    return pts


@pytest.mark.parametrize("time", [ec.P4_TIME, ec.P8, ec.P9_TIME], ids=["power4", "power8", "power9"])
def test_body_over_whole_waves_of_every_sign_pattern(gpu_renderer_factory, oracle, time):
    pts = body_points()
    patterns = {tuple(s) for s in np.signbit(pts[100:196, 0]).tolist()}
    assert len(patterns) == 8 and all(len(set(map(tuple, np.signbit(w).tolist()))) == 1 for w in pts[100:196])
    assert np.signbit(pts[196, 5, 0]) and pts[196, 5, 0] == 0 and (pts[:196] != 0).all()
    flat = pts.reshape(-1, 3)
    for iters in (1, 12):
        p = params_for(18, iters, time, 64, 64)
        with gpu_renderer_factory() as r:
            r.update_parameters_buffer(p)
            d, col = r.eval_scene(flat)
        rd, rcol, _ = oracle.scene_de(p, flat)
        bad = ~((d.view(np.uint32) == rd.view(np.uint32)) | (np.isnan(d) & np.isnan(rd)))
        assert not bad.any(), f"N={iters}: {bad.sum()} DE mismatches, first in wave {int(np.argmax(bad)) // 64}"
        assert same_bits(col, rcol)
