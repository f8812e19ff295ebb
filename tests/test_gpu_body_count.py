"""The Mandelbulb body loop's count-down (frm_render_kernels.h count_down): a lane holds the
bodies its DE has left, one subtract-with-borrow per iteration takes 1 from the computing lanes
and its borrow-out is the mask of count exits, and the service pass derives the DE's bodies
(N - left, N + 1 after a count exit) for the pixel's cost and the bailout counter. Frames whose
DEs exit by count at the first body (N = 0), the second (N = 1), the third and the last (N = 12,
200), beside DEs that bail out before it, from P1 and from a camera inside the
set; 64x36 (a row is one chunk) and 130x9 (rows straddle chunks, a short last chunk). Bytes, the
seven work counters and the cost keys must equal the live oracle's: as a single launch, with the
wave counters started below a carry (FRM_DEBUG_COUNTER_START), as a 4-frame launch with a power
per frame (the per-lane-power instantiation), and with hardware math (no oracle: the simple
kernel's bytes and counters, and keys that do not depend on the fetch order).
FRM_FLAG_PERSISTENT_KERNEL throughout: auto picks the simple kernel at these sizes."""
import numpy as np
import pytest

import edge_cases as ec
import frm
from helpers import params_for
from test_gpu_edges import counters_of
from test_gpu_sched import check_keys

pytestmark = pytest.mark.gpu

PERSISTENT = frm.FRM_FLAG_PERSISTENT_KERNEL
ENV = "FRM_DEBUG_COUNTER_START"
FIRST = 2 ** 32 - 1  # the first event of every wave counter carries
STEPS = 64
INSIDE = ((0.0, 0.0, -1.0), 0.0, 0.0)  # inside the set: hits at step 0, DEs that run all N + 1 bodies
CAMERAS = {"p1": ec.P1, "inside": INSIDE}
SIZES = [(64, 36), (130, 9)]
ITERS = [0, 1, 2, 12, 200]
ANIM_TIMES = [ec.P8, ec.P9_TIME, ec.P4_TIME, ec.P8 + 0.5]
CASES = [(w, h, cam, n) for (w, h) in SIZES for cam in CAMERAS for n in ITERS]
IDS = [f"{w}x{h}_{cam}_n{n}" for (w, h, cam, n) in CASES]

_REFS = {}


def _params(cam, n, w, h, time=ec.P8):
    p = params_for(18, n, time, w, h)
    p.update_camera(frm.Camera(*CAMERAS[cam]))
    return p


def _ref(oracle, cam, n, w, h, time=ec.P8):
    """The oracle's frame and per-pixel costs, rendered once per session (read-only)."""
    key = (cam, n, w, h, time)
    if key not in _REFS:
        p = _params(cam, n, w, h, time)
        ref = oracle.render(p, w, h, STEPS)
        ref["cost"] = oracle.render_costs(p, w, h, STEPS)
        _REFS[key] = ref
    return _REFS[key]


def _want(refs):
    return [sum(int(ref["counters"][i]) for ref in refs) for i in range(7)]


def _des(ref):
    c = ref["counters"]
    return int(c[2]) + int(c[3]) + int(c[4])  # primary + shadow + normal-tap DEs


def test_the_frames_exit_both_ways(oracle):
    """What the cases are chosen for, from the oracle's counters: every N has frames whose DEs
    exit by count (all of them at N = 0 and 1: the first and second body), every N >= 2 has
    frames with bailouts, and frames mix the two."""
    for n in ITERS:
        refs = [_ref(oracle, cam, n, w, h) for (w, h, cam, m) in CASES if m == n]
        count_exits = [_des(ref) - int(ref["counters"][6]) for ref in refs]
        bails = [int(ref["counters"][6]) for ref in refs]
        assert max(count_exits) > 0, f"N={n}: no count exit"
        if n >= 2:
            assert max(bails) > 0, f"N={n}: no bailout"
            assert any(c > 0 and b > 0 for c, b in zip(count_exits, bails)), f"N={n}: no mixed frame"
        for ref, c in zip(refs, count_exits):  # a count exit ran N + 1 bodies
            assert int(ref["counters"][5]) >= (n + 1) * c


@pytest.mark.parametrize("start", [0, FIRST], ids=["start0", "start2p32-1"])
@pytest.mark.parametrize("w,h,cam,n", CASES, ids=IDS)
def test_single_launch(frm_lib, oracle, monkeypatch, w, h, cam, n, start):
    """Two launches of one frame (row-major, then in the ranked order)."""
    ref = _ref(oracle, cam, n, w, h)
    monkeypatch.setenv(ENV, str(start))
    with frm.Renderer(device=0, max_steps=STEPS, flags=PERSISTENT) as r:
        r.resize(w, h)
        r.update_parameters_buffer(_params(cam, n, w, h))
        for launch in range(2):
            what = f"start {start} launch {launch}"
            st = r.render(stats=True)
            diff = np.any(r.read_frame() != ref["rgba"], axis=-1)
            assert not diff.any(), f"{what}: {diff.sum()} pixels differ"
            assert counters_of(st) == _want([ref]), what
            check_keys(r.pixel_keys(), ref["cost"], what)


@pytest.mark.parametrize("w,h,cam,n", CASES, ids=IDS)
def test_batch_with_a_power_per_frame(frm_lib, oracle, w, h, cam, n):
    """Four frames of one camera at four times in one launch: each lane counts down from the same
    N under its own frame's power. The keys are the last frame's costs."""
    import torch

    ps = [_params(cam, n, w, h, t) for t in ANIM_TIMES]
    refs = [_ref(oracle, cam, n, w, h, t) for t in ANIM_TIMES]
    fb = w * h * 4
    out = torch.zeros(len(ps) * fb, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    with frm.Renderer(device=0, max_steps=STEPS, flags=PERSISTENT) as r:
        r.resize(w, h)
        for launch in range(2):
            counters.zero_()
            out.zero_()
            r.render_bands_batch(ps, out.data_ptr(), dst_bytes=out.numel(), frame_stride=fb, band_rows=h, first_band=0,
                                 band_stride=1, stream=0, dev_counters=counters.data_ptr())
            torch.cuda.synchronize()
            img = out.cpu().numpy().reshape(len(ps), h, w, 4)
            for k, ref in enumerate(refs):
                diff = np.any(img[k] != ref["rgba"], axis=-1)
                assert not diff.any(), f"launch {launch} frame {k}: {diff.sum()} pixels differ"
            got = [int(v) for v in counters.cpu().tolist()][:7]
            assert got == _want(refs), f"launch {launch}"
            check_keys(r.pixel_keys(), refs[-1]["cost"], f"launch {launch}")


@pytest.mark.parametrize("w,h,cam,n", CASES, ids=IDS)
def test_hw_math_counters_and_keys(frm_lib, monkeypatch, w, h, cam, n):
    """FRM_FLAG_HW_MATH has no oracle: the persistent kernel's counters (and bytes) equal the simple
    kernel's, which counts its bodies upwards in a plain loop, and its keys are the same whatever
    the fetch order and the counters' start value."""
    p = _params(cam, n, w, h)
    with frm.Renderer(device=0, max_steps=STEPS, flags=frm.FRM_FLAG_HW_MATH | frm.FRM_FLAG_SIMPLE_KERNEL) as r:
        r.resize(w, h)
        r.update_parameters_buffer(p)
        st = r.render(stats=True)
        want, frame = counters_of(st), r.read_frame().copy()
    keys = []
    for start in (0, FIRST):
        monkeypatch.setenv(ENV, str(start))
        with frm.Renderer(device=0, max_steps=STEPS, flags=frm.FRM_FLAG_HW_MATH | PERSISTENT) as r:
            r.resize(w, h)
            r.update_parameters_buffer(p)
            for launch in range(2):
                st = r.render(stats=True)
                assert counters_of(st) == want, f"start {start} launch {launch}"
                assert np.array_equal(r.read_frame(), frame), f"start {start} launch {launch}"
                keys.append(r.pixel_keys().copy())
    assert all(np.array_equal(k, keys[0]) for k in keys[1:])
    assert keys[0].size == w * h and (keys[0] > 0).any() == (want[5] > 0)
