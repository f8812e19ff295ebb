"""GPU parity at the numerically delicate inputs of tests/edge_cases.py: degenerate cameras
(NaN, -inf and 0 / 0 closeness, r < 2^-13 at every body), the Mandelbulb power's two ends, deep
points whose dr passes 2^125 or overflows, Koch and Menger at the iteration counts where their
scales overflow or their distances go subnormal, and subnormal, far, infinite and NaN camera
positions on four scenes. tests/test_edge_census.py proves on the CPU,
from the oracle's census alone, that every case reaches the events it is named for; here both
march kernels must equal the oracle on them, bytes, work counters and (Mandelbulb) traces."""
import math

import numpy as np
import pytest

import edge_cases as ec
import frm

pytestmark = pytest.mark.gpu

KERNELS = [frm.FRM_FLAG_PERSISTENT_KERNEL, frm.FRM_FLAG_SIMPLE_KERNEL]


def counters_of(st):
    return [st["pixels"], st["hit_pixels"], st["primary_steps"], st["shadow_steps"],
            st["normal_evals"], st["fractal_bodies"], st["fractal_bailouts"]]


@pytest.mark.parametrize("kernel_flags", KERNELS, ids=["persistent", "simple"])
@pytest.mark.parametrize("case", ec.CASES, ids=ec.CASE_IDS)
def test_edge_case_bytes_and_counters(frm_lib, oracle, case, kernel_flags):
    """RGBA8 bytes and the seven work counters equal the oracle's. The persistent kernel renders
    the frame twice: the second launch fetches its pixels in the order scheduled from the first."""
    ref = ec.reference(oracle, case)
    want = [int(c) for c in ref["counters"][:7]]
    with frm.Renderer(device=0, max_steps=case.max_steps, flags=kernel_flags) as r:
        r.resize(case.width, case.height)
        r.update_parameters_buffer(case.params())
        for launch in range(2 if kernel_flags == frm.FRM_FLAG_PERSISTENT_KERNEL else 1):
            st = r.render(stats=True)
            img = r.read_frame()
            diff = np.any(img != ref["rgba"], axis=-1)
            assert not diff.any(), f"{case.name} launch {launch}: {diff.sum()} pixels differ"
            assert counters_of(st) == want, f"{case.name} launch {launch}"


@pytest.mark.parametrize("case", ec.MANDELBULB_CASES, ids=[c.name for c in ec.MANDELBULB_CASES])
def test_edge_case_trace(frm_lib, oracle, case):
    """frm_debug_trace after a persistent-kernel frame equals the oracle's trace bit for bit on
    hit pixels (NaN equal to NaN). This pins the shadow closeness as a float: -inf and NaN on the
    degenerate cameras, an ordinary quotient at the power's ends, beyond what an sRGB byte shows."""
    ref = ec.reference(oracle, case)["trace"].reshape(case.height, case.width, 10)
    with frm.Renderer(device=0, max_steps=case.max_steps, flags=frm.FRM_FLAG_PERSISTENT_KERNEL) as r:
        r.resize(case.width, case.height)
        r.update_parameters_buffer(case.params())
        r.render(stats=True)
        tr = r.trace()
    hit = ref[..., 0] != 0
    assert np.array_equal(tr[..., 0] != 0, hit)
    a, b = tr[hit], ref[hit]
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert same.all(), f"{case.name}: {np.sum(~same.all(axis=-1))} hit pixels differ, fields {sorted(set(np.nonzero(~same)[1].tolist()))}"


WAVES_PER_CU = 32  # the persistent kernel's ceiling of one-wave workgroups per CU (frm_ctx.h)


def mixed_frame_size(cus, frames=4):
    """The smallest 16:9-ish frame at which `frames` frames hold at least twice as many 64-pixel
    chunks as the device has resident waves."""
    pixels = -(-2 * cus * WAVES_PER_CU * 64 // frames)
    h = math.isqrt(pixels * 9 // 16) + 1
    return -(-pixels // h), h


_MIXED_REFS = {}


def _mixed_refs(oracle, time, w, h, steps, iters=12):
    key = (time, w, h, steps, iters)
    if key not in _MIXED_REFS:
        _MIXED_REFS[key] = [oracle.render(p, w, h, steps) for p in ec.mixed_params(time, w, h, iters)]
    return _MIXED_REFS[key]


@pytest.mark.parametrize("time,iters", [(ec.P8, 12), (ec.P9_TIME, 12), (ec.P8, 0)], ids=["power8", "power9", "power8_n0"])
def test_mixed_waves_in_one_batch_launch(frm_lib, oracle, time, iters):
    """One frm_render_bands_batch launch of four frames whose cameras differ: ordinary P1, the
    origin (every lane's |z|^2 is 0: length_wide, a non-normal magnitude at the distance, DE =
    NaN), ordinary P2, and (1e-5, -2e-5, 3e-5) (every body has r < 2^-13: never tame). The frame
    size gives the launch at least twice as many 64-pixel chunks as the device has resident waves,
    so every wave claims several chunks and refills its free lanes from the queue, in which the
    four frames' chunks are interleaved: lanes that just started a pixel of a degenerate frame then
    run beside lanes still marching an ordinary one, and mb_step's tame ballot, mb_length's
    length_wide ballot and the service pass's plain_log ballot see both kinds in one wave.
    It is this construction, not a measurement, that makes tame and non-tame lanes share waves:
    the oracle cannot observe the mixing, and no counter of the kernel reports it. What is asserted
    is that each frame equals the oracle's bytes and the launch's counters the frames' sums, over
    two consecutive launches (the second in scheduled order). At N = 0 the origin frame's dr
    stays 1, so its NaN distance comes from the logarithm of the zero magnitude alone: a wave whose
    plain_log ballot ignored such a lane would give 0 there."""
    import torch

    steps = 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    w, h = mixed_frame_size(cus)
    ps = ec.mixed_params(time, w, h, iters)
    assert len(ps) * w * h // 64 >= 2 * cus * WAVES_PER_CU
    refs = _mixed_refs(oracle, time, w, h, steps, iters)
    fb = w * h * 4
    out = torch.zeros(len(ps) * fb, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    with frm.Renderer(device=0, max_steps=steps, flags=frm.FRM_FLAG_PERSISTENT_KERNEL) as r:
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


def test_extreme_cameras_in_one_batch_launch(frm_lib, oracle):
    """The seven extreme cameras of scene 0 (subnormal, four far ones, inf, NaN) as the frames of
    one frm_render_bands_batch launch: the far frames' rays all end at step 0 beside the inf
    camera's, whose pixels march 18,304 shadow steps with an infinite origin. Each frame equals the
    oracle's bytes and the launch's counters the frames' sums, over two launches."""
    import torch

    cases = [c for c in ec.CAMERA_CASES if c.scene == 0]
    assert len(cases) == 7
    w, h, steps = cases[0].width, cases[0].height, cases[0].max_steps
    ps = ec.camera_batch_params(0)
    refs = [ec.reference(oracle, c) for c in cases]
    fb = w * h * 4
    out = torch.zeros(len(ps) * fb, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    with frm.Renderer(device=0, max_steps=steps, flags=frm.FRM_FLAG_PERSISTENT_KERNEL) as r:
        r.resize(w, h)
        for launch in range(2):
            counters.zero_()
            out.zero_()
            r.render_bands_batch(ps, out.data_ptr(), dst_bytes=out.numel(), frame_stride=fb, band_rows=h, first_band=0,
                                 band_stride=1, stream=0, dev_counters=counters.data_ptr())
            torch.cuda.synchronize()
            img = out.cpu().numpy().reshape(len(ps), h, w, 4)
            for c, ref in zip(cases, refs):
                diff = np.any(img[cases.index(c)] != ref["rgba"], axis=-1)
                assert not diff.any(), f"launch {launch} {c.name}: {diff.sum()} pixels differ"
            got = [int(v) for v in counters.cpu().tolist()][:7]
            assert got == [sum(int(ref["counters"][i]) for ref in refs) for i in range(7)], f"launch {launch}"


def test_mixed_frame_size_rule():
    assert mixed_frame_size(256) == (681, 385)
    for cus in (1, 64, 104, 256, 304):
        w, h = mixed_frame_size(cus)
        assert 4 * w * h // 64 >= 2 * cus * WAVES_PER_CU > 4 * (w - 1) * (h - 1) // 64


def test_cameras_changing_per_frame_with_frames_in_flight(frm_lib, oracle):
    """The four cameras as consecutive single frames through one context with two frames in
    flight (each slot's schedule comes from another camera's frame), each read back and compared."""
    w, h, steps = 160, 90, 64
    ps = ec.mixed_params(ec.P8, w, h)
    refs = _mixed_refs(oracle, ec.P8, w, h, steps)
    with frm.Renderer(device=0, max_steps=steps, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, frames_in_flight=2) as r:
        r.resize(w, h)
        for k in range(2 * len(ps)):
            r.update_parameters_buffer(ps[k % len(ps)])
            r.render(stats=False)
            assert np.array_equal(r.read_frame(), refs[k % len(ps)]["rgba"]), f"frame {k}"
        for k in (1, 3):  # a stats render waits for the frames in flight and counts only itself
            r.update_parameters_buffer(ps[k])
            st = r.render(stats=True)
            assert counters_of(st) == [int(c) for c in refs[k]["counters"][:7]], f"frame {k}"
            assert np.array_equal(r.read_frame(), refs[k]["rgba"])
