"""The persistent march kernel's work counters across a carry (frm_render_kernels.h WaveCounter):
each wave keeps a counter's low 32 bits in one SGPR and bumps the high word in a cold branch.
A small frame never counts 2^32 of anything, so FRM_DEBUG_COUNTER_START (read by the launcher at
every launch) starts every wave's counters just below the carry and the flush takes the value
off again in 64 bits: 2^32 - 1 makes the first event of every counter carry, 2^32 - 37 a later
one. The frames are unchanged by it: every frame equals the oracle's bytes and the launch's seven
counters the oracle's sums (hardware math, which has no oracle: the run with start value 0).
FRM_FLAG_PERSISTENT_KERNEL throughout: auto picks the simple kernel at these sizes."""
import math

import numpy as np
import pytest

import edge_cases as ec
import frm
from helpers import params_for
from test_gpu_edges import counters_of

pytestmark = pytest.mark.gpu

PERSISTENT = frm.FRM_FLAG_PERSISTENT_KERNEL
ENV = "FRM_DEBUG_COUNTER_START"
FIRST = 2 ** 32 - 1  # the first event of every counter carries
MID = 2 ** 32 - 37   # the carry falls inside the frame
W, H, ITERS, STEPS = 96, 64, 12, 64
AWAY = (ec.P1[0], math.pi, 0.0)        # P1's position, looking away from the bulb: no pixel hits
INSIDE = ((0.0, 0.0, -1.0), 0.0, 0.0)  # inside the set (edge_cases mb_inside): hits at step 0
ANIM_TIMES = [ec.P8, ec.P9_TIME, ec.P4_TIME]
INFO_HIT = 1

_REFS = {}


def _params(camera=ec.P1, time=ec.P8, w=W, h=H, scene=18, iters=ITERS):
    p = params_for(scene, iters, time, w, h)
    p.update_camera(frm.Camera(*camera))
    return p


def _ref(oracle, camera=ec.P1, time=ec.P8, w=W, h=H, scene=18, iters=ITERS, steps=STEPS):
    """The oracle's frame with its per-pixel info, rendered once per session (read-only)."""
    key = (camera, time, w, h, scene, iters, steps)
    if key not in _REFS:
        _REFS[key] = oracle.render(_params(camera, time, w, h, scene, iters), w, h, steps, info=True)
    return _REFS[key]


def _want(refs):
    return [sum(int(ref["counters"][i]) for ref in refs) for i in range(7)]


def _single(monkeypatch, p, ref, start, w=W, h=H, steps=STEPS, flags=PERSISTENT, launches=2):
    """`launches` renders of one frame (the first in row-major order, the next scheduled)."""
    monkeypatch.setenv(ENV, str(start))
    with frm.Renderer(device=0, max_steps=steps, flags=flags) as r:
        r.resize(w, h)
        r.update_parameters_buffer(p)
        for launch in range(launches):
            st = r.render(stats=True)
            diff = np.any(r.read_frame() != ref["rgba"], axis=-1)
            assert not diff.any(), f"start {start} launch {launch}: {diff.sum()} pixels differ"
            got = counters_of(st)
            print(f"start {start} launch {launch}: {got}")
            assert got == _want([ref]), f"start {start} launch {launch}"


def _batch(monkeypatch, ps, refs, start, w=W, h=H, steps=STEPS):
    import torch

    monkeypatch.setenv(ENV, str(start))
    fb = w * h * 4
    out = torch.zeros(len(ps) * fb, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    with frm.Renderer(device=0, max_steps=steps, flags=PERSISTENT) as r:
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
                assert not diff.any(), f"start {start} launch {launch} frame {k}: {diff.sum()} pixels differ"
            got = [int(v) for v in counters.cpu().tolist()][:7]
            print(f"start {start} launch {launch}: {got}")
            assert got == _want(refs), f"start {start} launch {launch}"


@pytest.mark.parametrize("start", [0, FIRST, MID], ids=["0", "2p32-1", "2p32-37"])
def test_mandelbulb_single_frame(frm_lib, oracle, monkeypatch, start):
    ref = _ref(oracle)
    assert all(c > 37 for c in _want([ref])), "every counter must pass the mid-frame carry"
    _single(monkeypatch, _params(), ref, start)


@pytest.mark.parametrize("start", [0, FIRST, MID], ids=["0", "2p32-1", "2p32-37"])
def test_mandelbulb_batch_of_three(frm_lib, oracle, monkeypatch, start):
    """Three frames of one power in one launch (MULTI): the waves' counts sum over the frames."""
    _batch(monkeypatch, [_params()] * 3, [_ref(oracle)] * 3, start)


@pytest.mark.parametrize("start", [0, FIRST, MID], ids=["0", "2p32-1", "2p32-37"])
def test_mandelbulb_animated_batch(frm_lib, oracle, monkeypatch, start):
    """The same camera at three times, so three powers: the per-lane-power instantiation (ANIM)."""
    _batch(monkeypatch, [_params(time=t) for t in ANIM_TIMES], [_ref(oracle, time=t) for t in ANIM_TIMES], start)


def test_hw_math_counters_equal_start_zero(frm_lib, monkeypatch):
    """FRM_FLAG_HW_MATH has no oracle bytes: the counters (and the bytes) of the runs started below a
    carry equal those of the run started at 0."""
    flags = frm.FRM_FLAG_HW_MATH | PERSISTENT
    runs = {}
    for start in (0, FIRST, MID):
        monkeypatch.setenv(ENV, str(start))
        with frm.Renderer(device=0, max_steps=STEPS, flags=flags) as r:
            r.resize(W, H)
            r.update_parameters_buffer(_params())
            runs[start] = []
            for _ in range(2):
                st = r.render(stats=True)
                runs[start].append((counters_of(st), r.read_frame().copy()))
        print(f"start {start}: {[c for c, _ in runs[start]]}")
    assert runs[0][0][0] == runs[0][1][0] and all(c > 37 for c in runs[0][0][0])
    for start in (FIRST, MID):
        for launch in range(2):
            assert runs[start][launch][0] == runs[0][launch][0], f"start {start} launch {launch}"
            assert np.array_equal(runs[start][launch][1], runs[0][launch][1]), f"start {start} launch {launch}"


@pytest.mark.parametrize("start", [0, FIRST], ids=["0", "2p32-1"])
def test_menger(frm_lib, oracle, monkeypatch, start):
    """A fixed-trip family (counters without the lean pass; its bodies and bailouts stay 0)."""
    w, h = 64, 48
    iters = frm.Parameters().num_iterations
    ref = _ref(oracle, w=w, h=h, scene=0, iters=iters)
    assert int(ref["counters"][1]) > 0 and int(ref["counters"][3]) > 0
    _single(monkeypatch, _params(w=w, h=h, scene=0, iters=iters), ref, start, w=w, h=h)


def test_all_misses(frm_lib, oracle, monkeypatch):
    """No pixel hits, so every pass is lean: the lean path's primary count crosses the carry."""
    ref = _ref(oracle, camera=AWAY)
    assert int(ref["counters"][1]) == 0 and not (ref["info"] & INFO_HIT).any() and int(ref["counters"][2]) > 0
    _single(monkeypatch, _params(AWAY), ref, FIRST)


def test_camera_inside_the_set(frm_lib, oracle, monkeypatch):
    """Pixels hit at step 0, so the waves' first pass takes the full path: its hit and shadow
    counts cross the carry."""
    ref = _ref(oracle, camera=INSIDE)
    hit = (ref["info"] & INFO_HIT) != 0
    assert (hit & ((ref["info"] >> 8) == 0)).any(), "no pixel hits at step 0"
    assert int(ref["counters"][1]) > 0 and int(ref["counters"][3]) > 0
    _single(monkeypatch, _params(INSIDE), ref, FIRST)


def test_two_launches_in_flight(frm_lib, oracle, monkeypatch):
    """Two contexts, each with a launch of its own frame and counters on its own stream, neither
    waited for before both are queued: each launch's counters are its own frame's."""
    import torch

    monkeypatch.setenv(ENV, str(FIRST))
    cams = [ec.P1, AWAY]
    refs = [_ref(oracle, camera=c) for c in cams]
    assert _want([refs[0]]) != _want([refs[1]])
    fb = W * H * 4
    outs = [torch.zeros(fb, dtype=torch.uint8, device="cuda") for _ in cams]
    counters = [torch.zeros(8, dtype=torch.int64, device="cuda") for _ in cams]
    streams = [torch.cuda.Stream() for _ in cams]
    torch.cuda.synchronize()
    rs = [frm.Renderer(device=0, max_steps=STEPS, flags=PERSISTENT) for _ in cams]
    try:
        for r in rs:
            r.resize(W, H)
        for launch in range(2):
            for c in counters:
                c.zero_()
            torch.cuda.synchronize()
            for r, cam, out, cnt, s in zip(rs, cams, outs, counters, streams):
                r.render_bands_batch([_params(cam)], out.data_ptr(), dst_bytes=out.numel(), frame_stride=fb, band_rows=H,
                                     first_band=0, band_stride=1, stream=s.cuda_stream, dev_counters=cnt.data_ptr())
            torch.cuda.synchronize()
            for k, ref in enumerate(refs):
                img = outs[k].cpu().numpy().reshape(H, W, 4)
                assert np.array_equal(img, ref["rgba"]), f"launch {launch} context {k}"
                got = [int(v) for v in counters[k].cpu().tolist()][:7]
                print(f"launch {launch} context {k}: {got}")
                assert got == _want([ref]), f"launch {launch} context {k}"
    finally:
        for r in rs:
            r.close()
