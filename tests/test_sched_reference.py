"""CPU side of the scheduler tests (no GPU): the oracle's per-pixel costs against its own work
counters, the references of sched_reference.py pinned by properties that share no code with them,
and a census of sched_cases.py, so that a GPU case cannot silently test nothing."""
from fractions import Fraction
from math import ceil, floor

import numpy as np
import pytest

import frm
import sched_cases as S
import sched_reference as R


# ---- oracle costs --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_costs_sum_to_the_work_counters(oracle, case):
    """Sum of the per-pixel costs = the frame's Mandelbulb bodies, or its DE evaluations (primary +
    shadow steps + normal taps): counters the oracle keeps on other lines of its code."""
    ref = S.reference(oracle, case)
    w, h = case.render_size
    c = [int(v) for v in ref["counters"]]
    assert ref["cost"].shape == (h, w) and ref["cost"].dtype == np.uint32
    want = c[5] if case.mandelbulb else c[2] + c[3] + c[4]
    assert int(ref["cost"].sum(dtype=np.uint64)) == want
    if not case.mandelbulb:
        assert c[5] == 0
        assert ref["cost"].min() >= 1  # every pixel evaluates step 0


@pytest.mark.parametrize("name", ["mandelbulb_n12", "menger0_n5", "size_127x97", "saturating"])
def test_costs_of_a_row_subset(oracle, name):
    case = S.BY_NAME[name]
    w, h = case.render_size
    rows = np.array(sorted({0, h // 3, h - 1}) + [h // 2], dtype=np.uint32)  # not in order
    sub = oracle.render_costs(case.params(), w, h, case.max_steps, flags=case.flags, rows=rows)
    assert np.array_equal(sub, S.reference(oracle, case)["cost"][rows])


def test_costs_of_band_rows(oracle):
    """The rows of each simulated rank's bands (the GPU band test's reference)."""
    b = S.BANDS
    case = S.BY_NAME["mandelbulb_n12"]
    p = S.SchedCase("bands", 18, 12, S.P8, b["width"], b["height"]).params()
    whole = oracle.render_costs(p, b["width"], b["height"], case.max_steps)
    seen = []
    for rk in range(b["ranks"]):
        rows = S.band_rows_of(b["height"], b["band_rows"], rk, b["ranks"])
        seen += list(rows)
        assert np.array_equal(oracle.render_costs(p, b["width"], b["height"], case.max_steps, rows=rows), whole[rows])
    assert sorted(seen) == list(range(b["height"]))
    assert len(S.band_rows_of(b["height"], b["band_rows"], 1, 2)) == 21  # the short last band is rank 1's


# ---- key_of --------------------------------------------------------------------------------------
def test_key_of_small_costs_and_the_ends():
    key, lo, hi = R.key_of(np.array([0, 1, 2, 3, 4, 62755, 62756, 62757, 62758, 62902, 10 ** 6, 2 ** 32 - 1]))
    # 16 log2(62757) = 254.99999 and 16 log2(62758) = 255.00001: both within delta of 255
    assert list(key) == [0, 16, 25, 32, 37, 254, 254, 255, 255, 255, 255, 255]
    assert list(lo) == [0, 16, 25, 32, 37, 254, 254, 254, 255, 255, 255, 255]  # 2 and 4 are powers of two: exact
    assert list(hi) == [0, 16, 25, 32, 37, 254, 255, 255, 255, 255, 255, 255]
    assert R.SATURATION_COST == 62757 and R.key_of([R.SATURATED_COST])[1][0] == 255


def test_key_of_band_census():
    """The costs below R.SATURATED_COST whose key is not unique: 29, the smallest 4870 (the last
    two, 62756 and 62757, around 255 itself); both neighbours are allowed there, one key anywhere
    else, the powers of two (c + 1 = 2 .. 2^15, key 16 k) included."""
    c = np.arange(0, R.SATURATED_COST, dtype=np.uint64)
    key, lo, hi = R.key_of(c)
    assert np.all((lo <= key) & (key <= hi)) and np.all(hi.astype(int) - lo <= 1)
    band = R.in_band(c)
    assert int(band.sum()) == 29 and int(c[band][0]) == 4870
    pow2 = np.array([2 ** k - 1 for k in range(0, 16)])
    assert np.array_equal(lo[pow2], 16 * np.arange(0, 16)) and np.array_equal(hi[pow2], 16 * np.arange(0, 16))
    # against exact integer arithmetic: key >= k  <=>  (c + 1)^16 >= 2^k
    for cost in (1, 2, 5, 99, 4869, 4870, 4871, 30000, 62756, 62757):
        exact = max(k for k in range(0, 256) if (cost + 1) ** 16 >= 2 ** k)
        k0, l0, h0 = (int(v[0]) for v in R.key_of([cost]))
        assert l0 <= exact <= h0 and (k0 == exact or l0 != h0), cost


def test_keys_allowed_is_strict_outside_the_band():
    cost = np.array([0, 0, 100, 100, 100, 3, 3, 3, 4870, 4870, 4870])
    got = np.array([0, 1, 106, 105, 107, 32, 31, 33, 195, 196, 197])
    _, lo, hi = R.key_of([4870])
    assert (int(lo[0]), int(hi[0])) == (195, 196)
    assert list(R.keys_allowed(got, cost)) == [True, False, True, False, False, True, False, False, True, True, False]


# ---- check_order / stable_order ------------------------------------------------------------------
def test_check_order_sees_each_fault():
    keys = np.array([3, 9, 9, 0, 7], dtype=np.uint8)
    assert R.check_order([1, 2, 4, 0, 3], keys) is None
    assert R.check_order([2, 1, 4, 0, 3], keys) is None          # ties in any order
    assert "rise" in R.check_order([1, 4, 2, 0, 3], keys)
    assert "rise" in R.check_order([3, 0, 4, 2, 1], keys)        # ascending
    assert "permutation" in R.check_order([1, 2, 4, 0, 0], keys)  # one pixel twice, one dropped
    assert "outside" in R.check_order([1, 2, 4, 0, 5], keys)
    assert "entries" in R.check_order([1, 2, 4, 0], keys)
    assert R.check_order([0], np.array([5])) is None


def test_stable_order_by_hand():
    keys = np.array([3, 9, 9, 0, 7, 9, 0], dtype=np.uint8)
    assert list(R.stable_order(keys)) == [1, 2, 5, 4, 0, 3, 6]
    assert R.check_order(R.stable_order(keys), keys) is None
    assert list(R.stable_order(np.full(5, 17, np.uint8))) == [0, 1, 2, 3, 4]
    rng = np.random.default_rng(5)
    k = rng.integers(0, 256, 5000).astype(np.uint8)
    o = R.stable_order(k)
    assert R.check_order(o, k) is None
    same = k[o][1:] == k[o][:-1]
    assert np.all(o[1:][same] > o[:-1][same])  # equal keys stay in pixel order


# ---- rescale -------------------------------------------------------------------------------------
# an upscale, a downscale, a ratio above 8 (the cap), portrait to landscape, 1 x 1 both ways, and a
# ratio between 6 and 8 where the widening is what the cap cuts
RESCALE_PAIRS = [((12, 7), (20, 11)), ((20, 11), (8, 5)), ((50, 30), (4, 3)), ((9, 16), (16, 9)),
                 ((1, 1), (5, 4)), ((5, 4), (1, 1)), ((30, 22), (4, 3))]
RESCALE_IDS = [f"{s[0]}x{s[1]}_to_{d[0]}x{d[1]}" for s, d in RESCALE_PAIRS]


def _contains(i, s, d, t):
    """Whether source index t lies in destination index i's widened, capped footprint, from the
    definition with exact fractions (no code shared with sched_reference.footprint)."""
    first, end = floor(Fraction(i * s, d)), ceil(Fraction((i + 1) * s, d))
    a = max(first - 1, 0)
    return a <= t < min(end + 1, s) and t - a < 8


@pytest.mark.parametrize("pair", RESCALE_PAIRS, ids=RESCALE_IDS)
def test_rescale_constant_map_stays_constant(pair):
    (sw, sh), (dw, dh) = pair
    out = R.rescale(np.full(sw * sh, 77, np.uint8), sw, sh, dw, dh)
    assert out.shape == (dw * dh,) and out.dtype == np.uint8 and np.all(out == 77)


@pytest.mark.parametrize("pair", RESCALE_PAIRS, ids=RESCALE_IDS)
def test_rescale_single_hot_texel(pair):
    (sw, sh), (dw, dh) = pair
    texels = {(0, 0), (sw - 1, sh - 1), (sw // 2, sh // 3), (sw - 1, 0), (sw // 3, sh - 1), (min(7, sw - 1), min(8, sh - 1))}
    for tx, ty in sorted(texels):
        src = np.zeros((sh, sw), np.uint8)
        src[ty, tx] = 200
        got = R.rescale(src.reshape(-1), sw, sh, dw, dh).reshape(dh, dw)
        want = np.array([[200 if _contains(x, sw, dw, tx) and _contains(y, sh, dh, ty) else 0 for x in range(dw)]
                         for y in range(dh)], np.uint8)
        assert np.array_equal(got, want), (tx, ty)
        if sw <= 8 * dw and sh <= 8 * dh and sw // dw <= 6 and sh // dh <= 6:
            assert got.max() == 200  # within the cap every texel reaches some pixel


@pytest.mark.parametrize("pair", [p for p in RESCALE_PAIRS if max(p[0][0] / p[1][0], p[0][1] / p[1][1]) <= 6],
                         ids=[i for p, i in zip(RESCALE_PAIRS, RESCALE_IDS) if max(p[0][0] / p[1][0], p[0][1] / p[1][1]) <= 6])
def test_rescale_never_below_the_covered_maximum(pair):
    """Ratio <= 6: the unwidened footprint (at most ceil(6) + 1 = 7 pixels with the one before it)
    fits under the cap, so no pixel starts below the largest key it covers."""
    (sw, sh), (dw, dh) = pair
    rng = np.random.default_rng(sw * 1000 + dw)
    src = rng.integers(0, 256, (sh, sw)).astype(np.uint8)
    got = R.rescale(src.reshape(-1), sw, sh, dw, dh).reshape(dh, dw)
    for y in range(dh):
        y0, y1 = floor(Fraction(y * sh, dh)), ceil(Fraction((y + 1) * sh, dh))
        for x in range(dw):
            x0, x1 = floor(Fraction(x * sw, dw)), ceil(Fraction((x + 1) * sw, dw))
            assert got[y, x] >= src[y0:y1, x0:x1].max(), (x, y)


def test_rescale_identity_size_is_a_3x3_maximum():
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, (6, 7)).astype(np.uint8)
    got = R.rescale(src.reshape(-1), 7, 6, 7, 6).reshape(6, 7)
    pad = np.pad(src, 1)
    want = np.max([pad[dy:dy + 6, dx:dx + 7] for dy in range(3) for dx in range(3)], axis=0)
    assert np.array_equal(got, want)


# ---- case census ---------------------------------------------------------------------------------
def test_key_range_cases_are_what_they_claim(oracle):
    cost = {n: S.reference(oracle, S.BY_NAME[n])["cost"] for n in ("all_zero", "inside_p9_n200", "saturating", "all_saturated")}
    assert cost["all_zero"].max() == 0
    assert int(S.reference(oracle, S.BY_NAME["all_zero"])["counters"][6]) > 0  # DEs ran, and bailed out at entry
    assert np.all(cost["inside_p9_n200"] == 5 * 201)
    sat = cost["saturating"] >= R.SATURATED_COST
    assert 1 <= int(sat.sum()) < sat.size // 4
    assert len(np.unique(R.key_of(cost["saturating"])[0])) > 20
    assert cost["all_saturated"].min() >= R.SATURATED_COST


def test_step0_cases_are_what_they_claim(oracle):
    info = {n: oracle.frame_info(S.BY_NAME[n].params()) for n in ("origin_neg_zero", "origin_pos_zero")}
    ox = {n: np.float32(v["origin"][0]) for n, v in info.items()}
    assert ox["origin_neg_zero"] == 0 and np.signbit(ox["origin_neg_zero"])
    assert ox["origin_pos_zero"] == 0 and not np.signbit(ox["origin_pos_zero"])
    a, b = (S.reference(oracle, S.BY_NAME[n]) for n in ("origin_neg_zero", "origin_pos_zero"))
    assert np.array_equal(a["cost"], b["cost"]) and np.array_equal(a["rgba"], b["rgba"])
    assert a["cost"].max() > 1000 and int(a["counters"][1]) > 0
    # the camera inside geometry hits at step 0 in every pixel; max_steps 1 runs exactly one primary DE
    hit = S.reference(oracle, S.BY_NAME["hit_at_step0"])
    assert int(hit["counters"][1]) == 33 * 19 and int(hit["counters"][2]) == 33 * 19
    one = S.reference(oracle, S.BY_NAME["max_steps_1"])
    assert int(one["counters"][2]) == 33 * 19 and int(one["counters"][1]) == 0


@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_band_share_is_small(oracle, case):
    """At most 0.5 % of a case's pixels have a cost whose key is not unique (powers of two not
    counted): the key test is exact almost everywhere."""
    cost = S.reference(oracle, case)["cost"]
    share = float(R.in_band(cost).mean())
    print(f"{case.name}: {int(R.in_band(cost).sum())} of {cost.size} pixels in the band")
    assert share <= 0.005


def test_cases_cover_the_block_sizes():
    npix = sorted(c.render_size[0] * c.render_size[1] for c in S.CASES)
    for n in (1, 64, 4095, 4096, 4097):
        assert n in npix
    assert any(n > 3 * 4096 and n % 4096 for n in npix) and max(npix) < 20000
    assert frm.FRM_MAX_BATCH >= len(S.BATCH_POSES)
