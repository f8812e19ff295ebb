"""The edge cases of tests/edge_cases.py on the CPU: (i) the oracle's domain census shows that
each case reaches the events it is named for (decided by the reference alone, so a GPU case
cannot silently test nothing), and (ii) the product's per-pixel source compiled for the CPU
(tests/native) equals the oracle there bit for bit. Plus the oracle's own `/` and sqrt against
numpy's float32 over the whole type, and a search for the edges no input here reaches."""
import numpy as np
import pytest

import edge_cases as ec
from helpers import hr_render, hr_scene_de, same_bits


@pytest.mark.parametrize("case", ec.CASES, ids=ec.CASE_IDS)
def test_frame_case_reaches_its_events(oracle, case):
    census = ec.reference(oracle, case)["census"]
    print(case.name, {k: v for k, v in census.items() if v})
    assert 32 <= case.width <= 64 and 18 <= case.height <= 36 and 64 <= case.max_steps <= 128 and case.iters <= 219
    missing = [e for e in case.events if census[e] < 1]
    assert not missing, f"{case.name} never meets {missing}"
    present = [e for e in case.absent if census[e] != 0]
    assert not present, f"{case.name} meets {present}"


@pytest.mark.parametrize("case", ec.CASES, ids=ec.CASE_IDS)
def test_frame_case_host_replay_equals_oracle(host_replay, oracle, case):
    ref = ec.reference(oracle, case)
    img, c = hr_render(host_replay, case.params(), case.width, case.height, case.max_steps)
    assert np.array_equal(img, ref["rgba"]), f"{np.any(img != ref['rgba'], axis=-1).sum()} pixels differ"
    assert np.array_equal(c, ref["counters"])


def test_extreme_cameras_do_what_they_are_for(oracle):
    """From the oracle alone: on scene 0 the subnormal, inf and NaN cameras each hit at least one
    pixel and march shadow rays; every far camera of every scene ends each ray after its one step
    at t = 0; the inf and NaN cameras run all N + 1 Mandelbulb bodies per pixel without a bailout."""
    assert len(ec.CAMERA_CASES) == 28 and all(c.camera[1:] == (0.0, 0.0) for c in ec.CAMERA_CASES)
    for case in ec.CAMERA_CASES:
        pixels, hits, primary, shadow, _, bodies, bailouts = (int(v) for v in ec.reference(oracle, case)["counters"][:7])
        tag = case.name.split("_", 1)[1]
        print(case.name, pixels, hits, primary, shadow, bodies, bailouts)
        assert pixels == case.width * case.height == 627
        if case.scene == 0 and not tag.startswith("far"):
            assert hits >= 1 and shadow >= 1, case.name
        if tag.startswith("far"):
            assert hits == 0 and shadow == 0 and primary == pixels, case.name
        if case.scene == 18 and tag in ("inf", "nan"):
            assert bodies == pixels * (case.iters + 1) and bailouts == 0, case.name


def test_census_changes_no_output_and_is_thread_independent(oracle):
    case = ec.CASES[ec.CASE_IDS.index("mb_inside")]
    p = case.params()
    plain = oracle.render(p, case.width, case.height, case.max_steps, trace=True, linear=True, info=True)
    runs = [oracle.render(p, case.width, case.height, case.max_steps, trace=True, linear=True, info=True, census=True,
                          threads=t) for t in (1, 3, 8)]
    for r in runs:
        assert r["census"] == runs[0]["census"]
        for k in ("rgba", "counters", "info"):
            assert np.array_equal(r[k], plain[k]), k
        assert same_bits(r["trace"], plain["trace"]) and same_bits(r["linear"], plain["linear"])
    rows = oracle.render(p, case.width, case.height, case.max_steps, rows=[3, 4], census=True)["census"]
    assert rows["primary_divs"] == 2 * case.width  # one step-0 division per pixel of the two rows


def test_axis_aligned_rays_keep_exact_zero_components(oracle):
    """The odd-sized frame's centre column and row march along x = 0 or y = 0; the even twin has
    no such ray and meets zero components only at the camera origin's own sample."""
    odd = ec.reference(oracle, ec.CASES[ec.CASE_IDS.index("mb_axis_odd")])["census"]
    even = ec.reference(oracle, ec.CASES[ec.CASE_IDS.index("mb_axis_even")])["census"]
    assert odd["mb_comp_zero"] / (33 * 19) > 2 * even["mb_comp_zero"] / (32 * 18)


@pytest.mark.parametrize("case", ec.POINT_CASES, ids=ec.POINT_CASE_IDS)
def test_point_case_reaches_its_events_and_host_replay_matches(host_replay, oracle, case):
    pts = ec.point_set(case.points)
    assert pts.shape == (4096, 3)
    p = case.params()
    d, col, cnt, census = oracle.scene_de_census(p, pts)
    print(case.name, {k: v for k, v in census.items() if v})
    d0, col0, cnt0 = oracle.scene_de(p, pts)
    assert same_bits(d, d0) and same_bits(col, col0) and np.array_equal(cnt, cnt0)
    missing = [e for e in case.events if census[e] < 1]
    assert not missing, f"{case.name} never meets {missing}"
    present = [e for e in case.absent if census[e] != 0]
    assert not present, f"{case.name} meets {present}"
    # the census agrees with the results it describes
    if case.scene != 18:
        assert census["de_nan"] == int(np.isnan(d).sum()) and census["de_inf"] == int(np.isinf(d).sum())
        assert census["de_zero"] == int((d == 0).sum())
    hd, hcol = hr_scene_de(host_replay, p, pts)
    assert same_bits(hd, d), f"{np.sum(~((hd.view(np.uint32) == d.view(np.uint32)) | (np.isnan(hd) & np.isnan(d))))} DEs differ"
    assert same_bits(hcol, col)


def test_tame_boundary_points_lie_on_their_sides(oracle):
    """The shell and component points of the Mandelbulb point set: with one body per point
    (N = 0), every `below` point has r < 2^-13 or a nonzero component under 2^-60, no `above`
    point has, and the points within an ulp of the shell fall on both sides."""
    below, above, edge = ec.tame_boundary_points()
    p = ec.params_for(18, 0, ec.P9_TIME, 8, 8)
    cb = oracle.scene_de_census(p, below)[3]
    ca = oracle.scene_de_census(p, above)[3]
    ce = oracle.scene_de_census(p, edge)[3]
    assert cb["mb_bodies"] == len(below) and cb["mb_r_small"] + cb["mb_comp_tiny"] == len(below)
    assert cb["mb_r_small"] > 0 and cb["mb_comp_tiny"] > 0
    assert ca["mb_bodies"] == len(above) and ca["mb_r_small"] + ca["mb_comp_tiny"] + ca["mb_comp_zero"] == 0
    assert 0 < ce["mb_r_small"] < len(edge)
    far = ec.far_below_points()
    cf = oracle.scene_de_census(p, far)[3]
    assert cf["mb_r_small"] == len(far) and cf["mb_comp_tiny"] + cf["mb_comp_zero"] == 0
    assert np.abs(far).min() >= 2.0 ** -60 and np.linalg.norm(far.astype(np.float64), axis=1).max() < 2.0 ** -15.9


def _bits_equal(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def test_oracle_div_is_ieee_division_over_the_whole_type(oracle):
    """The oracle's `/` equals numpy's float32 division (the float64 quotient rounded once) on
    the arrays the GPU's div is compared with, and those arrays hold what they are for."""
    a, b = ec.div_whole_type_inputs()
    assert len(a) == len(b) >= 400000 + len(ec.DIV_SPECIALS) ** 2
    with np.errstate(all="ignore"):
        want = a / b
    got = oracle.math_fn("div", a, b)
    bad = ~_bits_equal(got, want)
    assert not bad.any(), f"{bad.sum()} mismatches, e.g. {a[bad][:3]} / {b[bad][:3]}"
    fin = np.isfinite(a) & np.isfinite(b)
    tiny = np.finfo(np.float32).tiny
    assert ((want != 0) & (np.abs(want) < tiny)).sum() >= 1000              # subnormal quotients
    assert (np.isinf(want) & fin).sum() >= 1000                              # overflowing quotients
    ab = np.abs(b[fin & (b != 0)])
    assert ((ab < 2.0 ** -125) | (ab > 2.0 ** 125)).sum() >= 1000            # divisors outside rcp's range
    with np.errstate(all="ignore"):
        q = np.abs(a.astype(np.float64) / np.where(b == 0, np.nan, b).astype(np.float64))
        half = np.mod(q * 2.0 ** 149, 1.0) == 0.5
    assert (half & (q < 2.0 ** -126)).sum() >= 100                           # exact ties between subnormals


def test_oracle_sqrt_is_ieee_sqrt_over_the_whole_type(oracle):
    a = ec.sqrt_whole_type_inputs()
    with np.errstate(all="ignore"):
        want = np.sqrt(a)
    got = oracle.math_fn("sqrt", a)
    bad = ~_bits_equal(got, want)
    assert not bad.any(), f"{bad.sum()} mismatches, e.g. {a[bad][:3]}"
    assert ((a > 0) & (a < np.finfo(np.float32).tiny)).sum() >= 20000


def test_div_tame_edge_inputs_straddle_the_domain_ends():
    a, b = ec.div_tame_edge_inputs()
    for v in (a, b):
        m = np.abs(v)
        assert (m < np.float32(2.0 ** -60)).any() and (m == np.float32(2.0 ** -60)).any() and (m > np.float32(2.0 ** 40)).any()
    q = a.astype(np.float64) / b.astype(np.float64)
    assert np.any(q == 2.0 ** 100) and np.any(q == 2.0 ** -100)


# ---- the rarest edges ----------------------------------------------------------------------------
RARE = ("mb_dr_ge_2p125", "mb_dr_inf", "mb_de_subnormal")


def test_search_for_the_rare_mandelbulb_edges(oracle):
    """|dr| >= 2^125, dr = inf and a subnormal Mandelbulb DE are met by no ordinary camera or
    random point at N <= 64. This seeded search (P in {4, 8, 9}, N in {12, 64, 200, 219}: 32 k
    random points of the cube and 16 k of a 2^-3..2^-70 shell around the origin) is what found the
    deep points of edge_cases.py (power 9, N >= 200). Every rare event it meets must be named by a
    case of the table, so that a GPU test covers it; powers 4 and 8 and N <= 64 meet none."""
    rng = np.random.default_rng(125)
    cube = rng.uniform(-1.2, 1.2, (32768, 3)).astype(np.float32)
    shell = rng.normal(size=(16384, 3))
    shell = (shell / np.linalg.norm(shell, axis=1)[:, None] * np.exp2(-rng.uniform(3, 70, 16384))[:, None]).astype(np.float32)
    named = {e for c in ec.CASES + ec.POINT_CASES for e in c.events}
    for time in (ec.P4_TIME, ec.P8, ec.P9_TIME):
        for iters in (12, 64, 200, 219):
            p = ec.params_for(18, iters, time, 8, 8)
            c = oracle.merge_census(oracle.scene_de_census(p, cube)[3], oracle.scene_de_census(p, shell)[3])
            met = {e: c[e] for e in RARE if c[e]}
            print(f"t={time} N={iters}", met, "max finite |dr|", c["mb_dr_max_finite"], "min |DE|", c["mb_de_min_nonzero"])
            assert set(met) <= named, f"the search met {met}: add a case for it"
            if iters <= 64:
                assert not met
