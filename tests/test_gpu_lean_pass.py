"""The persistent march kernel's lean service pass (frm_render_kernels.h kLeanPass): a pass in
which every live lane of the wave is a primary ray and no consuming lane hits skips the shadow
closeness, the tap sums and the phase updates. Every wave starts all-primary, so every GPU test
crosses lean -> full; the frames here pin what those do not: frames that never leave the lean
pass (and end pixels on its first pass), waves that return to it after their hit pixels drain,
the pass in which a lean wave meets its first hit, the multi-frame and per-lane-power
instantiations with lean-only and mixed frames in one launch, and the hardware-math one.
Bytes and the seven work counters must equal the live oracle's (hardware math: the simple
kernel's). FRM_FLAG_PERSISTENT_KERNEL throughout: auto picks the simple kernel at these sizes."""
import math

import numpy as np
import pytest

import edge_cases as ec
import frm
from helpers import params_for
from test_gpu_edges import WAVES_PER_CU, counters_of, mixed_frame_size

pytestmark = pytest.mark.gpu

PERSISTENT = frm.FRM_FLAG_PERSISTENT_KERNEL
INFO_HIT = 1
AWAY = (ec.P1[0], math.pi, 0.0)  # P1's position, looking away from the bulb: no pixel hits
P0 = frm.POSES["P0"]

_REFS = {}


def _camera_params(camera, w, h, time=ec.P8):
    p = params_for(18, 12, time, w, h)
    p.update_camera(frm.Camera(*camera))
    return p


def _ref(oracle, camera, w, h, steps, time=ec.P8):
    """The oracle's frame with its per-pixel info, rendered once per session (read-only)."""
    key = (camera, w, h, steps, time)
    if key not in _REFS:
        _REFS[key] = oracle.render(_camera_params(camera, w, h, time), w, h, steps, info=True)
    return _REFS[key]


def _want(ref):
    return [int(c) for c in ref["counters"][:7]]


def _render_launches(p, ref, w, h, steps, launches, flags=PERSISTENT):
    with frm.Renderer(device=0, max_steps=steps, flags=flags) as r:
        r.resize(w, h)
        r.update_parameters_buffer(p)
        for launch in range(launches):  # the first in row-major order, the others scheduled
            st = r.render(stats=True)
            diff = np.any(r.read_frame() != ref["rgba"], axis=-1)
            assert not diff.any(), f"launch {launch}: {diff.sum()} pixels differ"
            assert counters_of(st) == _want(ref), f"launch {launch}"


@pytest.mark.parametrize("steps", [256, 1, 2])
@pytest.mark.parametrize("w,h", [(64, 36), (8, 8)], ids=["64x36", "8x8_one_chunk"])
def test_all_lean_frame(frm_lib, oracle, w, h, steps):
    """No pixel hits, so no wave ever leaves the lean pass; at max_steps 1 and 2 a pixel ends on
    its first lean pass (8x8 is a single chunk: one wave, whose refills find the queue empty)."""
    ref = _ref(oracle, AWAY, w, h, steps)
    assert int(ref["counters"][1]) == 0 and not (ref["info"] & INFO_HIT).any()
    _render_launches(_camera_params(AWAY, w, h), ref, w, h, steps, launches=2)


def _mixed_single():
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    w, h = mixed_frame_size(cus, frames=1)
    assert w * h // 64 >= 2 * cus * WAVES_PER_CU
    return w, h


def test_full_to_lean_inside_a_wave(frm_lib, oracle):
    """P1 with at least twice as many chunks as resident waves: every wave claims several chunks,
    and from the second launch on the longest-first order ends in chunks of miss pixels only, so
    waves whose hit pixels have drained go back to the lean pass."""
    steps = 64
    w, h = _mixed_single()
    ref = _ref(oracle, ec.P1, w, h, steps)
    hit = (ref["info"] & INFO_HIT) != 0
    psteps = ref["info"] >> 8
    assert 0 < hit.sum() <= w * h // 2
    assert (~hit & (psteps >= 2)).sum() >= w * h // 4
    _render_launches(_camera_params(ec.P1, w, h), ref, w, h, steps, launches=3)


def _one_hit_camera(oracle, w, h, steps):
    """P1 stepped outward (distance x 1.25 per step) until 1..64 pixels hit."""
    (x, y, z), yaw, pitch = ec.P1
    for _ in range(16):
        cam = ((x, y, z), yaw, pitch)
        n = int((_ref(oracle, cam, w, h, steps)["info"] & INFO_HIT).astype(bool).sum())
        if 1 <= n <= 64:
            return cam
        assert n > 64, "the bulb vanished between two camera steps"
        x, y, z = 1.25 * x, 1.25 * y, 1.25 * z
    raise AssertionError("no camera with 1..64 hit pixels")


def test_one_hit_among_misses(frm_lib, oracle):
    """A few hit pixels in rows of misses. The frame is 64 wide, so a row is one chunk of the
    row-major launch: the wave that meets a hit (de <= kMinDistance in a lean pass) carries
    mostly primary rays that miss, and goes back to the lean pass when the hit pixels end."""
    w, h, steps = 64, 36, 256
    cam = _one_hit_camera(oracle, w, h, steps)
    ref = _ref(oracle, cam, w, h, steps)
    hit = (ref["info"] & INFO_HIT) != 0
    assert 1 <= hit.sum() <= 64 and int(ref["counters"][1]) == hit.sum()
    per_row = hit.sum(axis=1)
    assert (per_row[per_row > 0] < w // 2).all()  # every row with a hit is mostly misses
    _render_launches(_camera_params(cam, w, h), ref, w, h, steps, launches=2)


BATCH_CAMERAS = [ec.P1, AWAY, P0, ec.P2]
BATCH_TIMES = {"uniform_power": [ec.P8] * 4, "per_frame_powers": [ec.P8, ec.P9_TIME, ec.P4_TIME, ec.P8 + 0.5]}


@pytest.mark.parametrize("powers", list(BATCH_TIMES))
def test_batch_of_lean_and_mixed_frames(frm_lib, oracle, powers):
    """One frm_render_bands_batch launch of four frames (P1, the camera turned away, P0, P2) whose
    chunks interleave in the queue, so the same waves take chunks of the frame that never hits and
    of the mixed ones; with one power (MULTI) and with a power per frame (ANIM). Each frame equals
    the oracle's bytes and the launch's counters the frames' sums, over two launches."""
    import torch

    steps = 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    w, h = mixed_frame_size(cus)
    times = BATCH_TIMES[powers]
    ps = [_camera_params(c, w, h, t) for c, t in zip(BATCH_CAMERAS, times)]
    refs = [_ref(oracle, c, w, h, steps, t) for c, t in zip(BATCH_CAMERAS, times)]
    assert int(refs[1]["counters"][1]) == 0 and int(refs[0]["counters"][1]) > 0
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
                assert not diff.any(), f"launch {launch} frame {k}: {diff.sum()} pixels differ"
            got = [int(v) for v in counters.cpu().tolist()][:7]
            assert got == [sum(int(ref["counters"][i]) for ref in refs) for i in range(7)], f"launch {launch}"


def test_hw_math_persistent_equals_simple(frm_lib):
    """FRM_FLAG_HW_MATH has no oracle: on the frame of test_full_to_lean_inside_a_wave the
    persistent kernel (three launches) gives the simple kernel's bytes and counters."""
    steps = 64
    w, h = _mixed_single()
    p = _camera_params(ec.P1, w, h)
    with frm.Renderer(device=0, max_steps=steps, flags=frm.FRM_FLAG_HW_MATH | frm.FRM_FLAG_SIMPLE_KERNEL) as r:
        r.resize(w, h)
        r.update_parameters_buffer(p)
        st = r.render(stats=True)
        ref = {"rgba": r.read_frame().copy(), "counters": counters_of(st)}
    assert 0 < ref["counters"][1] <= w * h // 2
    _render_launches(p, ref, w, h, steps, launches=3, flags=frm.FRM_FLAG_HW_MATH | PERSISTENT)
