"""The persistent march kernel's full service pass after round 12 (frm_render_kernels.h
FRM_PASS_MASKS, kTapStore, FRM_TAP_OFFSET): passes in which refilling, primary, tap and shadow
lanes meet. FRM_BLOCKS_PER_CU=1 (read at every launch) leaves one wave per CU, so a frame of
3 x 64 x CU-count pixels gives every wave several chunks: its lanes hold pixels in every phase while
others refill. Bytes and the seven work counters must equal the live oracle's over three launches
(the first row-major, the others in the scheduled order); hardware math, which has no oracle, must
equal the simple kernel. FRM_FLAG_PERSISTENT_KERNEL throughout: auto picks the simple kernel at
these sizes.

The odd-sized frames put a pixel on the optical axis: with the camera on a coordinate axis and
looking along it, that pixel's ray has two exact-zero direction components and origin components,
so ray_at returns zeros in the start-DE block that also offsets taps (the -0.0f of FRM_TAP_OFFSET
meets +-0), and on the sphere the symmetric taps cancel to exact-zero sum components."""
import math

import numpy as np
import pytest

import edge_cases as ec
import f64_reference as ref64
import frm
from helpers import params_for
from test_gpu_edges import counters_of

pytestmark = pytest.mark.gpu

PERSISTENT = frm.FRM_FLAG_PERSISTENT_KERNEL
INFO_HIT = 1
ON_AXIS = ((0.0, 0.0, -2.5), 0.0, 0.0)  # on the z axis, looking along it at the bulb
BATCH_CAMERAS = [ec.P1, ON_AXIS, ec.P2]
BATCH_TIMES = {"uniform_power": [ec.P8] * 3, "per_frame_powers": [ec.P8, ec.P9_TIME, ec.P4_TIME]}

_REFS = {}


@pytest.fixture(autouse=True)
def one_wave_per_cu(monkeypatch):
    monkeypatch.setenv("FRM_BLOCKS_PER_CU", "1")


def frame_size(odd=False, frames=1):
    """The smallest 4:3 frame, its width a multiple of 64 (or both sides odd), at which `frames`
    frames hold at least three 64-pixel chunks per wave of a one-wave-per-CU launch."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pixels = -(-3 * 64 * cus // frames)
    h = math.isqrt(pixels * 3 // 4) + 1
    if odd:
        h |= 1
        w = -(-pixels // h) | 1
    else:
        w = -(-pixels // h // 64) * 64
    assert frames * (w * h // 64) >= 3 * cus
    return w, h


def params(scene, camera, w, h, time=ec.P8, iters=12):
    p = params_for(scene, iters, time, w, h)
    p.update_camera(frm.Camera(*camera))
    return p


def reference(oracle, scene, camera, w, h, steps, time=ec.P8, flags=0):
    """The oracle's frame with its per-pixel info, rendered once per session (read-only)."""
    key = (scene, camera, w, h, steps, time, flags)
    if key not in _REFS:
        ref = oracle.render(params(scene, camera, w, h, time), w, h, steps, flags=flags, info=True)
        hit = (ref["info"] & INFO_HIT) != 0
        assert hit.any() and not hit.all(), "the frame needs hit and miss pixels"
        _REFS[key] = ref
    return _REFS[key]


def render_launches(p, ref, w, h, steps, flags=PERSISTENT, launches=3):
    with frm.Renderer(device=0, max_steps=steps, flags=flags) as r:
        r.resize(w, h)
        r.update_parameters_buffer(p)
        for launch in range(launches):  # the first in row-major order, the others scheduled
            st = r.render(stats=True)
            diff = np.any(r.read_frame() != ref["rgba"], axis=-1)
            assert not diff.any(), f"launch {launch}: {diff.sum()} pixels differ"
            assert counters_of(st) == [int(c) for c in ref["counters"][:7]], f"launch {launch}"


@pytest.mark.parametrize("steps", [256, 64])
def test_headline_scene(frm_lib, oracle, steps):
    w, h = frame_size()
    assert w % 64 == 0
    ref = reference(oracle, 18, ec.P1, w, h, steps)
    render_launches(params(18, ec.P1, w, h), ref, w, h, steps)


def axis_ray(p, w, h):
    """The centre pixel's ray in float32 (the camera of tests/f64_reference.py): origin, direction."""
    o, d = ref64.camera_rays(ref64.decode(p.to_bytes()), w, h, dtype=np.float32, xs=[w // 2], ys=[h // 2])
    return o, d[0]


@pytest.mark.parametrize("scene_flags", [0, frm.FRM_FLAG_SCENE_SPHERE], ids=["mandelbulb", "sphere"])
def test_odd_frame_with_a_ray_along_an_axis(frm_lib, oracle, scene_flags):
    steps = 64
    w, h = frame_size(odd=True)
    assert w % 2 == 1 and h % 2 == 1
    p = params(18, ON_AXIS, w, h)
    o, d = axis_ray(p, w, h)
    assert o[0] == 0 and o[1] == 0 and d[0] == 0 and d[1] == 0 and d[2] == 1  # exact zeros, head-on
    ref = reference(oracle, 18, ON_AXIS, w, h, steps, flags=scene_flags)
    assert ref["info"][h // 2, w // 2] & INFO_HIT  # the axis pixel runs its taps
    render_launches(p, ref, w, h, steps, flags=PERSISTENT | scene_flags)


@pytest.mark.parametrize("powers", list(BATCH_TIMES))
def test_batch_of_three_cameras(frm_lib, oracle, powers):
    """One frm_render_bands_batch launch of three frames with different cameras, with one power
    (the MULTI instantiation) and with three (ANIM): each frame the oracle's bytes, the launch's
    counters the frames' sums."""
    import torch

    steps = 64
    w, h = frame_size(frames=3)
    times = BATCH_TIMES[powers]
    ps = [params(18, c, w, h, t) for c, t in zip(BATCH_CAMERAS, times)]
    refs = [reference(oracle, 18, c, w, h, steps, t) for c, t in zip(BATCH_CAMERAS, times)]
    fb = w * h * 4
    out = torch.zeros(len(ps) * fb, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    with frm.Renderer(device=0, max_steps=steps, flags=PERSISTENT) as r:
        r.resize(w, h)
        for launch in range(3):
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
    steps = 64
    w, h = frame_size()
    p = params(18, ec.P1, w, h)
    with frm.Renderer(device=0, max_steps=steps, flags=frm.FRM_FLAG_HW_MATH | frm.FRM_FLAG_SIMPLE_KERNEL) as r:
        r.resize(w, h)
        r.update_parameters_buffer(p)
        st = r.render(stats=True)
        ref = {"rgba": r.read_frame().copy(), "counters": counters_of(st)}
    assert 0 < ref["counters"][1] < w * h  # hit and miss pixels
    render_launches(p, ref, w, h, steps, flags=frm.FRM_FLAG_HW_MATH | PERSISTENT)
