"""Buffers that follow the frame size, grown again after their first allocation: a context walks
48x27 -> 96x54 -> 48x27 -> 128x72 (every upward step exceeds the buffers' 25 % headroom, the step
down keeps the larger blocks) with frames in flight and a frame of readback latency. Each slot's
framebuffers, records and scheduling arrays, the resolved images of a supersampled context, the
refine list of an adaptive one, a group's band and gather buffers and the presentation outputs are
then released and re-allocated in stream order while earlier frames are still being read back.
Every frame equals the oracle's render (plain, group) or the frame of a fresh context created at
that size (supersampled, adaptive: their first-allocation path is pinned to the oracle by
test_gpu_supersample.py and test_gpu_adaptive.py)."""
import numpy as np
import pytest

import frm
from helpers import params_for

pytestmark = pytest.mark.gpu

SIZES = ((48, 27), (96, 54), (48, 27), (128, 72))
MAX_STEPS = 128
FIF = 2
POSES = ("P0", "P1", "P2")
_oracle_frames = {}


def frame_params(w, h):
    return [params_for(18, 6, frm.POWER8_TIME + 0.3 * k, w, h, pose=POSES[k % 3]) for k in range(FIF + 1)]


def oracle_frames(oracle, w, h):
    """The oracle's renders of frame_params(w, h), computed once for the cases that share them."""
    if (w, h) not in _oracle_frames:
        _oracle_frames[w, h] = [oracle.render(p, w, h, MAX_STEPS)["rgba"] for p in frame_params(w, h)]
    return _oracle_frames[w, h]


def renderer(**kw):
    return frm.Renderer(max_steps=MAX_STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, frames_in_flight=FIF, **kw)


def render_loop(r, w, h):
    """FIF + 1 frames at w x h in the drop-in loop: render, start the readback, take the frame before."""
    r.resize(w, h)
    held, got = [], []
    for p in frame_params(w, h):
        r.update_parameters_buffer(p)
        r.render(stats=False)
        held.append(r.read_frame_async())
        if len(held) > 1:
            got.append(r.frame_pixels(held.pop(0)))
    return got + [r.frame_pixels(t) for t in held]


def fresh_frames(w, h, **kw):
    with renderer(**kw) as one:
        return render_loop(one, w, h)


def test_regrow_plain_and_present(frm_lib, oracle):
    """Every frame of the walk is the oracle's; the last frame of each size presented at twice the
    frame size (frm_present's and frm_present_async's outputs grow at every upward step) is the
    presentation of a fresh context at that size."""
    with renderer() as r:
        for w, h in SIZES:
            for k, (g, ref) in enumerate(zip(render_loop(r, w, h), oracle_frames(oracle, w, h))):
                assert np.array_equal(g, ref), f"{w}x{h} frame {k}"
            with renderer() as one:
                render_loop(one, w, h)
                want = one.present(2 * w, 2 * h, srgb=False, bgra=True)
            assert np.array_equal(r.present(2 * w, 2 * h, srgb=False, bgra=True), want), f"{w}x{h} present"
            t = r.present_async(2 * w, 2 * h, srgb=False, bgra=True)
            assert np.array_equal(r.frame_pixels(t), want), f"{w}x{h} present_async"


@pytest.mark.parametrize("setting", [{"supersampling": 2}, {"adaptive": (2, 16)}], ids=["supersampled", "adaptive"])
def test_regrow_resolved(frm_lib, setting):
    with renderer(**setting) as r:
        for w, h in SIZES:
            for k, (g, ref) in enumerate(zip(render_loop(r, w, h), fresh_frames(w, h, **setting))):
                assert np.array_equal(g, ref), f"{w}x{h} frame {k}"


def test_regrow_group(frm_lib, oracle):
    with renderer(devices=[0, 0]) as r:
        for w, h in SIZES:
            for k, (g, ref) in enumerate(zip(render_loop(r, w, h), oracle_frames(oracle, w, h))):
                assert np.array_equal(g, ref), f"{w}x{h} frame {k}"
