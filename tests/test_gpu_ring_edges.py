"""The resident frame ring at the suite's hard frames (tests/ring_cases.py has the tables and the
helper, tests/test_ring_cases.py their census). frm_render(ctx, NULL) on a FRM_RING=1 context runs
march_persistent<..., RES = true> and the service waves of frm_ring_kernels.h: step 0 per pixel, no
lean pass, no tap store, lanes of up to four frames in one wave, a second copy of the shading and of
the ranking, and bookkeeping modulo the slots, the image parities, 8 grid ids and 64 table entries.
Every ring frame's RGBA8 bytes must equal oracle.render of its own Parameters, and every test reads,
from the totals line a context prints when it is destroyed under FRM_RING_DEBUG, how many frames
the ring served, and compares that with the count ring_cases.eligible (the rule restated) gives: a
frame that silently took the ordinary path fails its test.

  1  all 69 frames of edge_cases.CASES between ordinary frames of their generation, 2 and 4 slots
  2  the four cameras of ec.MIXED_CAMERAS posted without waiting: lanes of several frames in a wave
  3  sizes at npix % 64, at the 16384-pixel shade / rank task and one pixel and two chunks past it,
     on fresh contexts and as resizes of one; the sphere extension and the hardware-math family
  4  both sides of the eligibility budget, and the contexts and calls that stay out of the ring
  5  leaving the ring for every frame mode and re-entering it
  6  ticket lifetime, tickets across a generation change, the first asynchronous read's copy, more
     grids than grid ids, more frames than table entries"""
import numpy as np
import pytest

import adaptive_reference as ada
import dof_reference as dof
import edge_cases as ec
import frm
import panorama_reference as pano
import ring_cases as rc
import shutter_reference as shutter
import ssaa_reference as ssaa
from frm import _lib
from reload_cases import assert_frame
from test_gpu_edges import _mixed_refs, mixed_frame_size
from test_gpu_shutter import sub_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _ring_env(monkeypatch):
    rc.set_env(monkeypatch)


def _check(oracle, frames, got, w, h, steps, what, flags=0):
    assert len(got) == len(frames)
    for k, (p, g) in enumerate(zip(frames, got)):
        assert_frame(g.reshape(h, w, 4), rc.reference(oracle, p, w, h, steps, flags), f"{what} frame {k}")


# ---- 1. the 69 edge frames ------------------------------------------------------------------------------

_EDGE_CTX = {}  # (max_steps, frames in flight) -> [context, posts expected, cases run]


def _edge_ctx(max_steps, fif):
    key = (max_steps, fif)
    if key not in _EDGE_CTX:
        _EDGE_CTX[key] = [rc.open_ring(max_steps, fif), 0, 0]
    return _EDGE_CTX[key]


@pytest.mark.parametrize("fif", rc.FIFS, ids=["2slots", "4slots"])
@pytest.mark.parametrize("case", ec.CASES, ids=ec.CASE_IDS)
def test_edge_case_between_ordinary_frames(frm_lib, oracle, case, fif):
    """[A, case, B, A, case] posted back to back (ring_cases.edge_loop), read with a lag of slots - 1
    frames. The contexts are shared per (max_steps, frames in flight), so consecutive cases are
    generation changes too; test_edge_loops_posted_counts closes them and checks their totals."""
    entry = _edge_ctx(case.max_steps, fif)
    r = entry[0]
    frames = rc.edge_loop(case)
    r.resize(case.width, case.height)
    entry[1] += rc.edge_loop_eligible(case, fif)
    entry[2] += 1
    got = rc.run_loop(r, frames, rc.slots_for(fif) - 1)
    _check(oracle, frames, got, case.width, case.height, case.max_steps, case.name)


def test_edge_loops_posted_counts(frm_lib, capfd):
    """Every frame of every edge loop run so far was a ring frame."""
    assert _EDGE_CTX, "no edge loop ran before this test"
    try:
        for key in sorted(_EDGE_CTX):
            r, want, cases = _EDGE_CTX[key]
            posted, grids = rc.close_and_count(r, capfd)
            assert want == 5 * cases
            assert posted == want and grids >= 1, key
    finally:
        for r, _, _ in _EDGE_CTX.values():
            r.close()
        _EDGE_CTX.clear()


# ---- 2. lanes of several frames in one wave ----------------------------------------------------------------

def _mixed_size(size):
    import torch

    if size == "160x90":
        return 160, 90
    return mixed_frame_size(torch.cuda.get_device_properties(0).multi_processor_count)


def _run_mixed(oracle, capfd, ps, refs, w, h):
    frames = [ps[i] for i in rc.MIXED_ORDER]
    r = rc.open_ring(rc.MIXED_STEPS, 3)
    try:
        r.resize(w, h)
        got = rc.run_loop(r, frames, 3)
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    for k, g in enumerate(got):
        assert_frame(g, refs[rc.MIXED_ORDER[k]], f"frame {k} (camera {rc.MIXED_ORDER[k]})")
    want = sum(rc.eligible(rc.MIXED_STEPS, p.num_iterations, pixels=w * h, frames_in_flight=3) for p in frames)
    assert posted == want == len(rc.MIXED_ORDER)


@pytest.mark.parametrize("size", ["device", "160x90"])
@pytest.mark.parametrize("time,iters", rc.MIXED_TIMES, ids=rc.MIXED_IDS)
def test_mixed_cameras_posted_without_waiting(frm_lib, oracle, capfd, time, iters, size):
    """Ordinary P1, the origin (every lane NaN after one body), ordinary P2 and the r < 2^-13 camera,
    two rounds of them with an ordinary P0 frame between (ring_cases.MIXED_ORDER), on a ring of four
    slots; the pixels of frame k - 3 are fetched after frame k was posted, so the host never waits
    for the ring to run dry. A ring march wave claims from the oldest frame it has not drained and
    moves to frame f + 1 when frame f's queue is empty for it (ring_claim) while its other lanes
    still march pixels of frame f: each lane reads its own frame's camera rows, origin and power from
    the wave's LDS copy, and mb_step's tame ballot, mb_length's length_wide ballot and the pass's
    plain_log ballot see lanes of a degenerate frame beside lanes of an ordinary one. The device-sized
    frame (test_gpu_edges.mixed_frame_size) has about as many 64-pixel chunks as the grid has waves, so
    a wave that refills its free lanes finds frame f's queue empty and takes a chunk of frame f + 1,
    which the host has posted already; at 160 x 90 only a few waves hold pixels at all. It is this
    construction that produces the mixing; nothing observes it: the oracle cannot, and a ring frame
    has no counters.
    What is asserted is that each frame equals the oracle's bytes and that the ring served all nine."""
    w, h = _mixed_size(size)
    ps = ec.mixed_params(time, w, h, iters) + [rc.mixed_separator(time, w, h, iters)]
    refs = [x["rgba"] for x in _mixed_refs(oracle, time, w, h, rc.MIXED_STEPS, iters)]
    refs.append(rc.reference(oracle, ps[4], w, h, rc.MIXED_STEPS))
    _run_mixed(oracle, capfd, ps, refs, w, h)


@pytest.mark.parametrize("size", ["device", "160x90"])
def test_mixed_cameras_with_a_power_per_frame(frm_lib, oracle, capfd, size):
    """The same loop with the four frames at powers 8, 9, 4 and 8.6: lanes of one wave then differ in
    lane_power too (cam_o[3]), the degenerate lanes beside lanes of every power."""
    w, h = _mixed_size(size)
    ps = rc.mixed_power_params(w, h) + [rc.mixed_separator(ec.P8, w, h)]
    refs = [rc.reference(oracle, p, w, h, rc.MIXED_STEPS) for p in ps]
    _run_mixed(oracle, capfd, ps, refs, w, h)


# ---- 3. sizes at the ring's own boundaries -----------------------------------------------------------------

@pytest.mark.parametrize("scene,iters", rc.SIZE_SCENES, ids=["mandelbulb", "menger"])
@pytest.mark.parametrize("size", rc.SIZES, ids=rc.SIZE_IDS)
def test_size_on_a_fresh_context(frm_lib, oracle, capfd, size, scene, iters):
    w, h = size
    frames = rc.size_frames(scene, iters, w, h)
    r = rc.open_ring(rc.SIZE_STEPS, 2)
    try:
        r.resize(w, h)
        got = rc.run_loop(r, frames, 1)
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    _check(oracle, frames, got, w, h, rc.SIZE_STEPS, f"{w}x{h}")
    assert posted == sum(rc.eligible(rc.SIZE_STEPS, iters, pixels=w * h, frames_in_flight=2) for _ in frames) == 3


@pytest.mark.parametrize("fif", rc.FIFS, ids=["2slots", "4slots"])
@pytest.mark.parametrize("scene,iters", rc.SIZE_SCENES, ids=["mandelbulb", "menger"])
def test_sizes_as_resizes_of_one_context(frm_lib, oracle, capfd, scene, iters, fif):
    """Every resize is a new generation; from the third size on the slot buffers are larger than the
    frame (npix < R.cap: a slot's records, keys and order start at s * npix of the new size)."""
    lag = rc.slots_for(fif) - 1
    got = {}
    r = rc.open_ring(rc.SIZE_STEPS, fif)
    try:
        for w, h in rc.RESIZE_ORDER:
            r.resize(w, h)
            got[w, h] = rc.run_loop(r, rc.size_frames(scene, iters, w, h), lag)
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    for (w, h), g in got.items():
        _check(oracle, rc.size_frames(scene, iters, w, h), g, w, h, rc.SIZE_STEPS, f"{w}x{h}")
    assert posted == 3 * len(rc.RESIZE_ORDER)


def test_sphere_extension_at_130x9(frm_lib, oracle, capfd):
    w, h = 130, 9
    frames = rc.size_frames(18, 8, w, h)
    r = rc.open_ring(rc.SIZE_STEPS, 2, rc.PERSISTENT | rc.SPHERE)
    try:
        r.resize(w, h)
        got = rc.run_loop(r, frames, 1)
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    _check(oracle, frames, got, w, h, rc.SIZE_STEPS, "sphere", flags=1)
    assert posted == 3


def test_hardware_math_family_at_130x9(frm_lib, oracle, capfd):
    """FRM_FLAG_HW_MATH (kMandelbulbHw) is not bit-exact with the oracle by design
    (test_gpu_hw_math.py), so this one family is compared with the same context's per-frame grid (a
    stats render, which stays out of the ring): the ring's instantiation must give the same bytes.
    Not all three frames are the oracle's (as test_gpu_hw_math.py asserts differ_any > 0): it is not
    the bit-exact family that ran."""
    w, h = 130, 9
    frames = rc.size_frames(18, 8, w, h)
    r = rc.open_ring(rc.SIZE_STEPS, 2, rc.PERSISTENT | frm.FRM_FLAG_HW_MATH)
    try:
        r.resize(w, h)
        got = rc.run_loop(r, frames, 1)
        grid = []
        for p in frames:
            r.update_parameters_buffer(p)
            r.render(stats=True)
            grid.append(r.read_frame())
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    for k, (g, want) in enumerate(zip(got, grid)):
        assert_frame(g, want, f"frame {k}")
    assert not all(np.array_equal(g, rc.reference(oracle, p, w, h, rc.SIZE_STEPS)) for g, p in zip(got, frames))
    assert posted == 3


# ---- 4. the eligibility edge -------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", rc.ELIGIBILITY_EDGE, ids=rc.EDGE_IDS)
def test_eligibility_budget_both_sides(frm_lib, oracle, capfd, entry):
    """2 * max_steps * (N + 2) <= 2^21 exactly and one past it: both render the oracle's frames, the
    first through the ring and the second through the per-frame grid."""
    name, flags, steps, n, p, served = entry
    w, h = rc.EDGE_W, rc.EDGE_H
    frames = [p, rc.edge_pair(p), p]
    r = rc.open_ring(steps, 2, flags)
    try:
        r.resize(w, h)
        got = rc.run_loop(r, frames, 1)
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    _check(oracle, frames, got, w, h, steps, name, flags=flags & rc.SPHERE)
    want = sum(rc.eligible(steps, q.num_iterations, pixels=w * h, frames_in_flight=2, flags=flags) for q in frames)
    assert want == (3 if served else 0)
    assert posted == want


STAY_OUT = {"one_frame_in_flight": dict(fif=1), "simple_kernel": dict(flags=rc.SIMPLE),
            "group": dict(devices=[0, 0]), "stats": dict(stats=True)}


@pytest.mark.parametrize("why", list(STAY_OUT))
def test_frames_that_stay_out_of_the_ring(frm_lib, oracle, capfd, why):
    kw = STAY_OUT[why]
    fif, flags, devices, stats = kw.get("fif", 2), kw.get("flags", rc.PERSISTENT), kw.get("devices"), kw.get("stats", False)
    w, h = rc.EDGE_W, rc.EDGE_H
    frames = rc.size_frames(18, 8, w, h)
    r = rc.open_ring(rc.SIZE_STEPS, fif, flags, devices=devices)
    try:
        r.resize(w, h)
        if stats:
            got = []
            for p in frames:
                r.update_parameters_buffer(p)
                r.render(stats=True)
                got.append(r.read_frame())
        else:
            got = rc.run_loop(r, frames, fif - 1)
    finally:
        posted, grids = rc.close_and_count(r, capfd, contexts=None if devices else 1)
    _check(oracle, frames, got, w, h, rc.SIZE_STEPS, why)
    want = sum(rc.eligible(rc.SIZE_STEPS, 8, pixels=w * h, frames_in_flight=fif, flags=flags, group=bool(devices),
                           stats=stats) for _ in frames)
    assert posted == want == 0 and grids == 0


# ---- 5. leaving and re-entering the ring ---------------------------------------------------------------------

def test_every_frame_mode_between_ring_frames(frm_lib, oracle, capfd):
    """Two ring frames, then each frame mode set, rendered once and unset, with two ring frames after
    each: every plain frame is the oracle's, every mode frame its built-in test's reference, and the
    ring served exactly the plain frames."""
    w, h, steps, n = 48, 24, 64, 14
    plain = rc.moving(12, w, h)
    lens = (6.0, 1.8, 8)
    subs = sub_frames("mandelbulb", 3, w, h)
    mode_p = plain[5]
    got_plain, got_mode = [], {}
    r = rc.open_ring(steps, 2)
    try:
        r.resize(w, h)
        got_plain += rc.run_loop(r, plain[0:2], 1)

        def mode_frame(name, on, off, render=None):
            on()
            r.update_parameters_buffer(mode_p)
            (render or (lambda: r.render(stats=False)))()
            got_mode[name] = r.read_frame()
            if name == "dof":
                got_mode["depth"] = r.read_depth()
            off()

        modes = [("supersampled", lambda: r.set_supersampling(2), lambda: r.set_supersampling(1), None),
                 ("adaptive", lambda: r.set_adaptive(2), lambda: r.set_adaptive(1), None),
                 ("shutter", lambda: None, lambda: None, lambda: r.render_shutter(subs, stats=False)),
                 ("panorama", lambda: r.set_panorama(n), lambda: r.set_panorama(0), None),
                 ("dof", lambda: r.set_depth_of_field(*lens), lambda: r.set_depth_of_field(0.0, 1.0, 0), None)]
        for k, (name, on, off, render) in enumerate(modes):
            mode_frame(name, on, off, render)
            got_plain += rc.run_loop(r, plain[2 + 2 * k:4 + 2 * k], 1)
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    _check(oracle, plain, got_plain, w, h, steps, "plain")
    f1 = rc.reference(oracle, mode_p, w, h, steps)
    fs = ssaa.box_resolve(oracle.render(mode_p, 2 * w, 2 * h, steps)["rgba"], 2, oracle)
    assert_frame(got_mode["supersampled"], fs, "supersampled")
    mask = ada.edge_mask(f1, frm.FRM_ADAPTIVE_DEFAULT_THRESHOLD)
    assert 0 < mask.sum() < w * h
    assert_frame(got_mode["adaptive"], ada.compose(f1, fs, mask), "adaptive")
    sub_imgs = np.stack([rc.reference(oracle, p, w, h, steps) for p in subs])
    assert_frame(got_mode["shutter"], shutter.accumulate(sub_imgs, 1, oracle), "shutter")
    faces = np.stack([oracle.render(q, n + 2, n + 2, steps)["rgba"] for q in pano.face_parameters(mode_p, n)])
    assert_frame(got_mode["panorama"], pano.project(faces, n, w, h, frm.equirect_tables(w, h), oracle), "panorama")
    want_dof = dof.gather(f1, got_mode["depth"], *lens, oracle)
    assert np.any(want_dof != f1)
    assert_frame(got_mode["dof"], want_dof, "depth of field")
    modes_of = ["plain"] * 2 + ["supersampled", "plain", "plain", "adaptive", "plain", "plain", "shutter", "plain", "plain",
                                "panorama", "plain", "plain", "dof", "plain", "plain"]
    assert posted == sum(rc.eligible(steps, 8, pixels=w * h, frames_in_flight=2, mode=m) for m in modes_of) == len(plain)


# ---- 6. tickets, images and ids --------------------------------------------------------------------------------

@pytest.mark.parametrize("fif", rc.FIFS, ids=["2slots", "4slots"])
def test_ticket_lifetime(frm_lib, oracle, capfd, fif):
    """A ring frame's ticket names the pinned image (slot, parity) its shading wrote; frame k + 2 slots
    is the next to post into that image (ring_cases.ticket_bound, which also shows that this is never
    less than include/frm.h's promise). So after 2 slots - 1 further posts, the last before the image
    is reused, the ticket of frame k still shows frame k, for the copied first frame and for every
    zero-copy one; one post later it has expired."""
    w, h, steps = rc.SMALL_W, rc.SMALL_H, 64
    slots = rc.slots_for(fif)
    bound = rc.ticket_bound(slots)
    frames = rc.moving(2 * bound + 3, w, h)
    assert len({p.to_bytes() for p in frames}) == len(frames)
    r = rc.open_ring(steps, fif)
    try:
        r.resize(w, h)
        tickets, got = [], {}
        for k, p in enumerate(frames):
            r.update_parameters_buffer(p)
            r.render(stats=False)
            tickets.append(r.read_frame_async())
            if k >= bound:
                got[k - bound] = r.frame_pixels(tickets[k - bound])
            if k > bound:
                with pytest.raises(frm.FrmError) as e:
                    r.frame_pixels(tickets[k - bound - 1])
                assert e.value.code == _lib.FRM_ERR_INVALID_ARGUMENT
        for k in range(len(frames) - bound, len(frames)):
            got[k] = r.frame_pixels(tickets[k])
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    _check(oracle, frames, [got[k] for k in range(len(frames))], w, h, steps, f"{slots} slots")
    assert posted == len(frames)


@pytest.mark.parametrize("fif", rc.FIFS, ids=["2slots", "4slots"])
def test_ticket_across_a_generation_change(frm_lib, oracle, capfd, fif):
    """A ticket taken at 128 x 72 outlives the resize to 160 x 90, whose larger images replace the
    ring's (ring_free_images retires the one the ticket names), and 2 slots frames of the new size."""
    steps = 64
    slots = rc.slots_for(fif)
    small = rc.moving(3, 128, 72)
    large = rc.moving(2 * slots, 160, 90)
    r = rc.open_ring(steps, fif)
    try:
        r.resize(128, 72)
        got_small = rc.run_loop(r, small[:2], 1)
        r.update_parameters_buffer(small[2])
        r.render(stats=False)
        kept = r.read_frame_async()
        r.resize(160, 90)
        got_large = rc.run_loop(r, large, slots - 1)
        old = r.frame_pixels(kept)
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    assert old.shape == (72, 128, 4)  # out_bytes = 128 * 72 * 4: the view reshapes to the ticket's own size
    assert_frame(old, rc.reference(oracle, small[2], 128, 72, steps), "the kept ticket")
    _check(oracle, small[:2], got_small, 128, 72, steps, "128x72")
    _check(oracle, large, got_large, 160, 90, steps, "160x90")
    assert posted == 3 + 2 * slots


def test_first_asynchronous_read_copies(frm_lib, oracle, capfd):
    """Three ring frames posted with no readback carry no image; the first frm_read_frame_async then
    waits for the last and copies it (ring_read_async), and every later frame is zero-copy."""
    w, h, steps = rc.SMALL_W, rc.SMALL_H, 64
    frames = rc.moving(7, w, h)
    r = rc.open_ring(steps, 2)
    try:
        r.resize(w, h)
        for p in frames[:3]:
            r.update_parameters_buffer(p)
            r.render(stats=False)
        first = r.frame_pixels(r.read_frame_async())
        got = rc.run_loop(r, frames[3:], 1)
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    _check(oracle, frames[2:], [first] + got, w, h, steps, "from the copied frame on")
    assert posted == len(frames)


def test_more_grids_than_grid_ids(frm_lib, oracle, capfd):
    """Twelve rounds of one ring frame and frm_synchronize: each round's grid closes, so the thirteenth
    id's grid_stop word is the fifth's (id % 8)."""
    w, h, steps = rc.SMALL_W, rc.SMALL_H, 64
    frames = rc.moving(rc.GRID_ROUNDS, w, h)
    got = []
    r = rc.open_ring(steps, 2)
    try:
        r.resize(w, h)
        for p in frames:
            r.update_parameters_buffer(p)
            r.render(stats=False)
            t = r.read_frame_async()
            r.synchronize()
            got.append(r.frame_pixels(t))
    finally:
        posted, grids = rc.close_and_count(r, capfd)
    _check(oracle, frames, got, w, h, steps, "round")
    assert posted == rc.GRID_ROUNDS
    assert grids >= rc.GRID_ROUNDS > rc.GRID_IDS


@pytest.mark.parametrize("fif", rc.FIFS, ids=["2slots", "4slots"])
def test_long_loop_past_the_frame_tables(frm_lib, oracle, capfd, fif):
    """70 frames: seq % 64 wraps. 35 distinct frames, each rendered once by the oracle."""
    w, h, steps = rc.SMALL_W, rc.SMALL_H, 64
    frames = rc.moving(rc.LONG_LOOP, w, h, distinct=rc.LONG_DISTINCT)
    r = rc.open_ring(steps, fif)
    try:
        r.resize(w, h)
        got = rc.run_loop(r, frames, rc.slots_for(fif) - 1)
    finally:
        posted, _ = rc.close_and_count(r, capfd)
    _check(oracle, frames, got, w, h, steps, "long loop")
    assert posted == rc.LONG_LOOP
