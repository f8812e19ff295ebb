"""The limit cases of tests/limit_cases.py on the CPU: the oracle alone shows that each case
reaches what it is named for, so a GPU case of test_gpu_limits.py cannot silently test nothing.
Deep marches: hit and miss pixels in every frame, hits of 2^13 (cube), 2^16 (Sierpinski, Koch) and
2^21 (two cube rows, the Mandelbulb crawl) steps and more, every bit 13..21 of the step count set in
one cube hit and clear in another, and at least 8 misses of exactly FRM_MAX_STEPS_LIMIT steps in the
stalled and crawling frames. FRM_MAX_DIMENSION: the aspect (1, 1) frames have hits and misses in
both halves of the long axis. FRM_MAX_NUM_ITERATIONS: from inside the Mandelbulb all 384 distance
estimators of the frame run all 65537 bodies and none bails out, from P1 all bail out, and from two
cameras on the set's boundary both happen in one frame, within each pixel's lane. Each test prints
its figures (pytest -s shows them)."""
import os
import re

import numpy as np
import pytest

import limit_cases as lc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frm.h")


def test_limits_are_the_headers():
    text = open(HEADER).read()
    value = lambda name: int(re.search(rf"#define {name} (\d+)u", text).group(1))
    assert lc.MAX_STEPS == value("FRM_MAX_STEPS_LIMIT") == (1 << 22) - 1
    assert lc.MAX_DIM == value("FRM_MAX_DIMENSION")
    assert lc.MAX_ITERS == value("FRM_MAX_NUM_ITERATIONS")
    assert lc.BIG_STRIDE >= 1 << 32 and lc.BIG_STRIDE % 4 == 0 and lc.BIG_STRIDE < 16 << 30  # "below 16 GiB"


@pytest.mark.parametrize("case", lc.DEEP_CASES, ids=lc.DEEP_IDS)
def test_deep_case_reaches_its_depth(frm_lib, oracle, case):
    ref = lc.deep_reference(oracle, case)
    c = lc.step_census(ref)
    print(f"{case.name}: hits {c['hits']} misses {c['misses']} hit steps {c['min_hit_steps']}..{c['max_hit_steps']} "
          f"bits set {c['ones']:#x} clear {c['zeros']:#x} full-length marches {c['full']} "
          f"primary_steps {int(ref['counters'][2])}")
    assert (case.width, case.height, case.max_steps) == (8, 8, lc.MAX_STEPS)
    assert c["hits"] >= 1 and c["misses"] >= 1  # the full and the lean service pass both run
    assert c["hits"] == int(ref["counters"][1])
    assert c["max_hit_steps"] >= case.min_hit_steps
    if case.kind == "graze":
        assert c["max_hit_steps"] >= 1 << 13
    else:
        assert c["full"] >= 8
        assert c["full"] == ref["census"]["primary_end_steps"]  # the oracle's own count of such marches
        hit = (ref["info"] & 1) != 0
        assert int(ref["counters"][2]) >= c["full"] * lc.MAX_STEPS + int((ref["info"] >> 8)[hit].sum())
    tr = ref["trace"].reshape(-1, 10)
    assert np.array_equal(tr[:, 1].astype(np.int64), (ref["info"].ravel() >> 8))  # a float holds every count exactly


def test_cube_grazes_cover_the_high_step_bits(frm_lib, oracle):
    """Over the cube cases, each of the bits 13..21 of a pixel record's step field is 1 in some hit
    pixel's count and 0 in another's: a field narrowed from above, or a flag moved into it, changes a
    count that the trace and the ambient-occlusion byte show."""
    cs = [lc.step_census(lc.deep_reference(oracle, case)) for case in lc.CUBE_GRAZES]
    span = sum(1 << b for b in lc.STEP_BITS)
    ones = np.bitwise_or.reduce([c["ones"] for c in cs])
    zeros = np.bitwise_or.reduce([c["zeros"] for c in cs])
    print(f"cube grazes: bits set {int(ones):#x} clear {int(zeros):#x} of {span:#x}")
    assert len(cs) >= 4 and ones == span and zeros == span
    assert sum(c["max_hit_steps"] >= 1 << 21 for c in cs) >= 1


@pytest.mark.parametrize("family", ["sier", "koch16", "koch17", "mb"])
def test_every_family_has_a_deep_hit(frm_lib, oracle, family):
    best = max(lc.step_census(lc.deep_reference(oracle, c))["max_hit_steps"] for c in lc.DEEP_CASES
               if c.name.startswith(family))
    print(f"{family}: deepest hit {best} steps")
    assert best >= 1 << 16


def test_second_frames_of_the_deep_batches(frm_lib, oracle):
    """The other frames of the multi-frame launches, which ride beside a deep one: P1 under the case's
    aspect (64 near-identical rays), and the Mandelbulb crawl's camera at power 9 (every pixel hits
    at step 0). They differ from the deep frame, and are cheap."""
    for name in lc.BATCH_CAMERA_CASES:
        ref = lc.deep_reference(oracle, lc.deep_case(name), camera=lc.P1)
        c = lc.step_census(ref)
        print(f"{name} from P1: hits {c['hits']} misses {c['misses']} hit steps {c['min_hit_steps']}..{c['max_hit_steps']}")
        assert int(ref["counters"][2]) < 1 << 16
    mb = lc.deep_case("mb_crawl")
    assert lc.MB_CRAWL_TIMES[0] == mb.time
    p = [oracle.frame_info(mb.params(time=t))["mb_power"] for t in lc.MB_CRAWL_TIMES]
    ref = lc.deep_reference(oracle, mb, time=lc.MB_CRAWL_TIMES[1])
    c = lc.step_census(ref)
    print(f"mb_crawl at powers {p}: the second has hits {c['hits']} hit steps {c['min_hit_steps']}..{c['max_hit_steps']}")
    assert p[0] == 8.0 and abs(p[1] - 9.0) < 1e-5 and c["hits"] == 64 and c["max_hit_steps"] == 0


@pytest.mark.parametrize("case", lc.DIM_CASES, ids=lc.DIM_IDS)
def test_dimension_case_sweeps_the_object(frm_lib, oracle, case):
    ref = lc.dim_reference(oracle, case)
    hit = ((ref["info"] & 1) != 0).ravel()
    halves = [hit[:lc.MAX_DIM // 2], hit[lc.MAX_DIM // 2:]]
    print(f"{case.name}: hits {[int(h.sum()) for h in halves]} misses {[int((~h).sum()) for h in halves]} per half")
    assert max(case.width, case.height) == lc.MAX_DIM and case.width * case.height == lc.MAX_DIM
    if case.unit_aspect:
        for h in halves:
            assert h.any() and not h.all()


@pytest.mark.parametrize("case", lc.ITER_CASES, ids=lc.ITER_IDS)
def test_iteration_case_runs_the_whole_loop(frm_lib, oracle, case):
    ref = lc.iter_reference(oracle, case)
    counters = [int(c) for c in ref["counters"][:7]]
    census = ref["census"]
    print(f"{case.name}: counters {counters} DEs {census['mb_dists'] or census['de_evals']}")
    assert case.iters == lc.MAX_ITERS and case.params().num_iterations == lc.MAX_ITERS
    dists, bodies, bailouts = census["mb_dists"], counters[5], counters[6]
    if case.name == "mb_inside":
        # All 64 rays start at one point of the set: step 0 hits, and the hit's four normal taps and one
        # shadow step are the same six points for every pixel. None of the 384 DEs bails out, each
        # leaves by the count after N + 1 bodies. (At N = 12 this camera's frame also has bailouts;
        # at N = 65536 a frame's bailouts come from mb_p1, and from the launch of both cameras.)
        assert dists == 6 * 64 and bailouts == 0 and bodies == dists * (lc.MAX_ITERS + 1)
        print(f"mb_inside: {dists} of {dists} DEs ran all {lc.MAX_ITERS + 1} bodies")
    if case.name == "mb_p1":
        assert bailouts > 0 and bailouts == dists  # every DE of the outside camera bails out
    if case.name in ("mb_pole", "mb_edge"):
        # each DE ends one way: those that did not bail out left by the count, after N + 1 bodies each
        count_exits = dists - bailouts
        print(f"{case.name}: {count_exits} count exits and {bailouts} bailouts in {dists} DEs")
        assert count_exits >= 64 and bailouts >= 64 and bodies >= count_exits * (lc.MAX_ITERS + 1)
        assert counters[1] == 64  # every pixel hits, so both exits occur within each pixel's lane
        if case.name == "mb_edge":
            assert counters[2] > 64  # some pixels march past step 0: the lanes of the wave differ
