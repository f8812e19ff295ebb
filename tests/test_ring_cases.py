"""CPU census of the ring loops (tests/ring_cases.py), from the oracle alone. A ring frame that is
never marched or never shaded keeps the bytes its slot's earlier frame left, so a loop exposes it only
if the oracle's frame k differs from frame k - 1 and from frame k - slots, for both ring sizes. That
is asserted here as a condition of the tables, for every loop of test_gpu_ring_edges.py that relies
on it; a GPU loop can therefore not pass by showing an earlier frame. The Python restatement of the
eligibility rule is held to the in / out split of the eligibility tests and to all 69 edge frames,
and the sizes to the ring's three boundaries."""
import time

import numpy as np
import pytest

import edge_cases as ec
import ring_cases as rc
from test_gpu_edges import mixed_frame_size

SLOTS = [rc.slots_for(f) for f in rc.FIFS]


def _images(oracle, frames, w, h, steps, flags=0):
    return [rc.reference(oracle, p, w, h, steps, flags) for p in frames]


def test_ring_sizes():
    assert SLOTS == [2, 4] and rc.slots_for(1) == 0 and rc.slots_for(8) == 4


@pytest.mark.parametrize("case", ec.CASES, ids=ec.CASE_IDS)
def test_edge_loop_neighbours_differ(oracle, case):
    frames = rc.edge_loop(case)
    assert frames[1].to_bytes() == frames[4].to_bytes() == case.params().to_bytes()
    imgs = _images(oracle, frames, case.width, case.height, case.max_steps)
    assert np.array_equal(imgs[1], ec.reference(oracle, case)["rgba"])
    for slots in SLOTS:
        assert rc.neighbours_differ(imgs, slots) is None, f"{case.name}, {slots} slots"
    # A and B belong to the case's generation (ring_same_gen) unless the table says why not
    for p in (frames[0], frames[2]):
        assert p.scene_index == case.scene and tuple(p.aspect_scale) == tuple(frames[1].aspect_scale)
        assert p.num_iterations == rc.OTHER_N.get(case.name, case.iters)
        assert case.mandelbulb or p.time == case.time


def test_other_n_is_needed(oracle):
    """The cases of OTHER_N show one image from every pose at their own N."""
    for name in rc.OTHER_N:
        case = ec.CASES[ec.CASE_IDS.index(name)]
        imgs = [rc.reference(oracle, rc.params_for(case.scene, case.iters, case.time, case.width, case.height, pose=pose),
                             case.width, case.height, case.max_steps) for pose in ("P0", "P1", "P2")]
        assert all(np.array_equal(i, imgs[0]) for i in imgs), name


def test_all_edge_cases_are_ring_frames():
    assert len(ec.CASES) == 69
    for case in ec.CASES:
        assert case.max_steps <= 100 and case.iters <= 219
        for fif in rc.FIFS:
            assert rc.edge_loop_eligible(case, fif) == 5, case.name


def test_eligibility_rule():
    split = {name: rc.eligible(steps, n, pixels=rc.EDGE_W * rc.EDGE_H, frames_in_flight=2, flags=flags)
             for name, flags, steps, n, _, _ in rc.ELIGIBILITY_EDGE}
    assert split == {name: served for name, _, _, _, _, served in rc.ELIGIBILITY_EDGE}
    assert split == {"menger_4096_n254": True, "menger_4096_n255": False, "bulb_16_n65534": True,
                     "bulb_16_n65536": False, "bulb_8_n65534": True, "bulb_8_n65536": True,
                     "sphere_524288": True, "sphere_524289": False}
    # each in / out pair straddles the budget exactly
    assert 2 * 4096 * (254 + 2) == rc.TRIP_BUDGET == 2 * 16 * (65534 + 2) == 2 * 524288 * 2
    for name, flags, steps, n, p, _ in rc.ELIGIBILITY_EDGE:
        assert p.num_iterations == n
    ok = dict(pixels=64, frames_in_flight=2)
    assert rc.eligible(64, 12, **ok)
    assert not rc.eligible(64, 12, pixels=64, frames_in_flight=1)
    assert not rc.eligible(64, 12, flags=rc.SIMPLE, **ok)
    assert not rc.eligible(64, 12, group=True, **ok)
    assert not rc.eligible(64, 12, stats=True, **ok)
    assert not rc.eligible(64, 12, reloaded=True, **ok)
    assert not rc.eligible(64, 12, ring=False, **ok)
    assert not rc.eligible(64, 12, pixels=(1 << 28) + 1, frames_in_flight=2)
    assert rc.eligible(64, 12, pixels=1 << 28, frames_in_flight=8)
    for mode in ("supersampled", "adaptive", "shutter", "panorama", "dof"):
        assert not rc.eligible(64, 12, mode=mode, **ok)


def test_eligibility_edge_renders_in_seconds_and_differs(oracle):
    """The oracle renders the costliest frames of the eligibility tests in seconds, and the two frames
    of each test differ."""
    for name, flags, steps, n, p, _ in rc.ELIGIBILITY_EDGE:
        t0 = time.perf_counter()
        o = flags & rc.SPHERE
        imgs = _images(oracle, [p, rc.edge_pair(p)], rc.EDGE_W, rc.EDGE_H, steps, o)
        print(f"{name}: {time.perf_counter() - t0:.2f} s")
        assert np.array_equal(imgs[0], imgs[1]) == (name in rc.BLACK_PAIRS), name


def test_sizes_cover_the_boundaries():
    npix = [w * h for w, h in rc.SIZES]
    assert any(n % 64 for n in npix)
    assert rc.TASK_PIXELS - 1 in npix and rc.TASK_PIXELS in npix and rc.TASK_PIXELS + 128 in npix
    assert any(n % rc.TASK_PIXELS == 0 for n in npix)            # on a task boundary
    assert any(n % rc.TASK_PIXELS == rc.TASK_PIXELS - 1 for n in npix)  # one below it
    assert any(0 < n - rc.TASK_PIXELS < rc.TASK_PIXELS and n % 64 == 0 for n in npix)  # a second task of whole chunks
    assert any(n > rc.TASK_PIXELS and n % 64 for n in npix)      # a second task that ends inside a chunk
    assert 1 in npix and 64 in npix and 65 in npix
    assert sorted(rc.RESIZE_ORDER) == sorted(rc.SIZES)
    cap = 0
    smaller = 0
    for w, h in rc.RESIZE_ORDER:
        smaller += w * h < cap
        cap = max(cap, w * h)
    assert smaller == len(rc.SIZES) - 2  # every size but the first two runs in buffers larger than its frame


@pytest.mark.parametrize("scene,iters", rc.SIZE_SCENES)
@pytest.mark.parametrize("size", rc.SIZES, ids=rc.SIZE_IDS)
def test_size_loop_neighbours_differ(oracle, size, scene, iters):
    w, h = size
    imgs = _images(oracle, rc.size_frames(scene, iters, w, h), w, h, rc.SIZE_STEPS)
    for slots in SLOTS:
        assert rc.neighbours_differ(imgs, slots) is None


def test_size_loop_of_the_other_families_differ(oracle):
    w, h = 130, 9
    frames = rc.size_frames(18, 8, w, h)
    assert rc.neighbours_differ(_images(oracle, frames, w, h, rc.SIZE_STEPS, flags=1), 2) is None


def _mixed_sizes():
    return [mixed_frame_size(rc.MIXED_CUS), (160, 90)]


MIXED_SLOTS = rc.slots_for(3)  # the mixed loops run with three frames in flight only


@pytest.mark.parametrize("time_iters", rc.MIXED_TIMES, ids=rc.MIXED_IDS)
def test_mixed_rounds_neighbours_differ(oracle, time_iters):
    """At N = 0 the Mandelbulb's one body leaves every pixel of every camera black (the GPU loop there
    can only show that the ring serves such frames; what the batch test pins at N = 0 are counters,
    which ring frames do not have): asserted, so that the exception is a checked fact."""
    t, iters = time_iters
    for w, h in _mixed_sizes():
        ps = ec.mixed_params(t, w, h, iters) + [rc.mixed_separator(t, w, h, iters)]
        five = _images(oracle, ps, w, h, rc.MIXED_STEPS)
        imgs = [five[i] for i in rc.MIXED_ORDER]
        if iters == 0:
            assert all(np.array_equal(i, five[0]) for i in five) and not five[0][..., :3].any()
        else:
            assert np.array_equal(five[1], five[3])  # why two bare rounds cannot meet the condition
            assert rc.neighbours_differ(imgs, MIXED_SLOTS) is None, (w, h)


def test_mixed_power_round_neighbours_differ(oracle):
    for w, h in _mixed_sizes():
        ps = rc.mixed_power_params(w, h) + [rc.mixed_separator(ec.P8, w, h)]
        five = _images(oracle, ps, w, h, rc.MIXED_STEPS)
        imgs = [five[i] for i in rc.MIXED_ORDER]
        assert rc.neighbours_differ(imgs, MIXED_SLOTS) is None, (w, h)
    assert sorted(rc.MIXED_ORDER[:4]) == sorted(rc.MIXED_ORDER[5:]) == [0, 1, 2, 3] and rc.MIXED_ORDER[4] == 4


def test_moving_loops_neighbours_differ(oracle):
    """The ticket, grid-id and long loops of section 6: the 35 distinct frames of the long loop, and
    its seam (frame 35 is frame 0 again)."""
    w, h = rc.SMALL_W, rc.SMALL_H
    frames = rc.moving(rc.LONG_LOOP, w, h, distinct=rc.LONG_DISTINCT)
    assert len({p.to_bytes() for p in frames}) == rc.LONG_DISTINCT
    assert rc.LONG_LOOP > rc.FRAME_TABLES and rc.GRID_ROUNDS > rc.GRID_IDS
    imgs = _images(oracle, frames, w, h, 64)
    for slots in SLOTS:
        assert rc.neighbours_differ(imgs, slots) is None
    # the ticket loops fetch frame k after 2 * slots - 1 further posts, from an image that frame
    # k - 2 * slots wrote before: every frame of the moving sequence differs from every other one (its
    # prefixes are the first-read, grid-id and generation-change loops, and section 5's plain frames)
    longest = 2 * rc.ticket_bound(max(SLOTS)) + 3
    for (w, h), n in (((rc.SMALL_W, rc.SMALL_H), longest), ((128, 72), 3), ((160, 90), 2 * max(SLOTS)), ((48, 24), 12)):
        frames = rc.moving(n, w, h)
        assert [p.to_bytes() for p in frames[:3]] == [p.to_bytes() for p in rc.moving(3, w, h)]
        imgs = _images(oracle, frames, w, h, 64)
        assert len({i.tobytes() for i in imgs}) == n, (w, h)


def test_ticket_bound():
    """ring_render's image choice, replayed: frame k's image is next posted into by frame k + 2 * slots."""
    for slots in SLOTS:
        image = lambda k: ((k - 1) % slots, ((k - 1) // slots) & 1)
        for k in range(1, 40):
            later = [j for j in range(k + 1, k + 40) if image(j) == image(k)]
            assert later[0] == k + rc.ticket_bound(slots) + 1
    # include/frm.h: a ticket holds until frames_in_flight further renders
    for fif in range(2, 9):
        assert rc.ticket_bound(rc.slots_for(fif)) + 1 >= fif
