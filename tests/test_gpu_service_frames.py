"""Frames whose service passes meet operands on both sides of a wave-uniform guard of the pass
(the last tap's normalize_wave, the distance's plain_log; frm_scene.h, frm_render_kernels.h), wave
by wave and within waves: an ordinary Mandelbulb camera beside cameras at deep points (dr >= 2^125,
dr = inf, DE = +-0, tap sums far below 2^-62, the 0 / 0 closeness) and the origin (DE = NaN), in one batch
launch with uniform and with per-frame powers, as single frames with their traces, and with two
frames in flight; Menger, Koch and Sierpinski frames whose closeness quotient is subnormal,
infinite or NaN. Bytes, work counters and traces must equal the oracle's."""
import numpy as np
import pytest

import edge_cases as ec
import frm
from helpers import params_for
from test_gpu_edges import WAVES_PER_CU, counters_of, mixed_frame_size

pytestmark = pytest.mark.gpu

STEPS = 40
ORIGIN = ((0.0, 0.0, 0.0), 0.0, 0.0)
# ordinary P1; dr >= 2^125 at N = 200 and inf at N = 219; dr = inf and DE = 0 at N = 200; DE = NaN
CAMERAS = [ec.P1, (ec.DEEP_A, 0.0, 0.0), (ec.DEEP_B, 0.0, 0.0), ORIGIN]


def camera_params(times, iters, w, h, cameras=CAMERAS, scene=18):
    out = []
    for (pos, yaw, pitch), t in zip(cameras, times):
        p = params_for(scene, iters, t, w, h)
        p.update_camera(frm.Camera(pos, yaw, pitch))
        out.append(p)
    return out


_REFS = {}


def refs_for(oracle, key, ps, w, h, steps, trace=False):
    """The oracle's frames of a parameter list (rendered once per session; not written to)."""
    key = (key, w, h, steps, trace)
    if key not in _REFS:
        _REFS[key] = [oracle.render(p, w, h, steps, trace=trace) for p in ps]
    return _REFS[key]


def run_batch(r, ps, refs, w, h, launches=2):
    import torch

    fb = w * h * 4
    out = torch.zeros(len(ps) * fb, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    for launch in range(launches):
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


BATCHES = {
    # uniform power 9, N = 200: the deep cameras' huge and infinite dr beside P1's ordinary one
    "deep_n200": ([ec.P9_TIME] * 4, 200),
    # per-frame powers (the ANIM instantiation): P1 at power 8, the deep cameras at power 9
    "deep_n200_anim": ([ec.P8, ec.P9_TIME, ec.P9_TIME, ec.P8], 200),
    # N = 0: dr stays 1 everywhere and the origin's NaN distance comes from the magnitude alone
    "n0": ([ec.P9_TIME] * 4, 0),
    "n0_anim": ([ec.P8, ec.P9_TIME, ec.P9_TIME, ec.P8], 0),
}


@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_launch_mixes_domains_in_waves(frm_lib, oracle, name):
    """One frm_render_bands_batch launch of the four cameras, sized (test_gpu_edges.mixed_frame_size)
    so that every wave claims several chunks of the interleaved frames and refills its free lanes
    from another frame's pixels: the guards' ballots see lanes inside and outside their domains
    in one wave (the deep cameras' distances, and so their tap sums, are tiny where P1's are
    ordinary). Two launches, the second in scheduled order."""
    import torch

    times, iters = BATCHES[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    w, h = mixed_frame_size(cus)
    assert len(CAMERAS) * w * h // 64 >= 2 * cus * WAVES_PER_CU
    ps = camera_params(times, iters, w, h)
    refs = refs_for(oracle, name, ps, w, h, STEPS)
    with frm.Renderer(device=0, max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL) as r:
        r.resize(w, h)
        run_batch(r, ps, refs, w, h)


def same_trace(tr, ref):
    hit = ref[..., 0] != 0
    if not np.array_equal(tr[..., 0] != 0, hit):
        return False
    a, b = tr[hit], ref[hit]
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("iters", [200, 219, 0])
def test_single_frames_bytes_counters_and_traces(frm_lib, oracle, iters):
    """The four cameras as single frames (the deep cameras' rays leave the deep point, so a frame's
    waves hold lanes on both sides of the guards): bytes, counters and the trace, which
    pins the normal and the shadow closeness as floats."""
    w, h = 96, 54
    ps = camera_params([ec.P9_TIME] * 4, iters, w, h)
    refs = refs_for(oracle, ("single", iters), ps, w, h, STEPS, trace=True)
    with frm.Renderer(device=0, max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL) as r:
        r.resize(w, h)
        for k, (p, ref) in enumerate(zip(ps, refs)):
            r.update_parameters_buffer(p)
            st = r.render(stats=True)
            assert np.array_equal(r.read_frame(), ref["rgba"]), f"camera {k}"
            assert counters_of(st) == [int(c) for c in ref["counters"][:7]], f"camera {k}"
            assert same_trace(r.trace(), ref["trace"].reshape(h, w, 10)), f"camera {k}"


def test_two_frames_in_flight(frm_lib, oracle):
    """The cameras as consecutive frames of one context with two in flight, each scheduled from
    another camera's costs."""
    w, h = 96, 54
    ps = camera_params([ec.P9_TIME] * 4, 200, w, h)
    refs = refs_for(oracle, ("single", 200), ps, w, h, STEPS, trace=True)
    with frm.Renderer(device=0, max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, frames_in_flight=2) as r:
        r.resize(w, h)
        for k in range(2 * len(ps)):
            r.update_parameters_buffer(ps[k % len(ps)])
            r.render(stats=False)
            assert np.array_equal(r.read_frame(), refs[k % len(ps)]["rgba"]), f"frame {k}"
        for k in (1, 2):
            r.update_parameters_buffer(ps[k])
            st = r.render(stats=True)
            assert counters_of(st) == [int(c) for c in refs[k]["counters"][:7]], f"frame {k}"


# the closeness quotient is subnormal (Menger from N = 80), +-inf or NaN (Koch at N >= 211), and the
# distance exactly 0 (Sierpinski N = 31): DESIGN section 3, "edge, Koch / Menger / Sierpinski"
OTHER = [(0, 80, 1.0), (4, 82, 1.0), (16, 217, 1.0), (17, 214, 1.0), (15, 31, 0.5)]
OTHER_CAMERAS = [ec.P1, ec.P2, frm.POSES["P0"]]


@pytest.mark.parametrize("scene,iters,time", OTHER, ids=[f"scene{s}_n{n}" for s, n, _ in OTHER])
def test_other_families_batch_and_in_flight(frm_lib, oracle, scene, iters, time):
    w, h, steps = 96, 54, 64
    ps = camera_params([time] * 3, iters, w, h, OTHER_CAMERAS, scene)
    refs = refs_for(oracle, ("other", scene, iters), ps, w, h, steps)
    with frm.Renderer(device=0, max_steps=steps, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, frames_in_flight=2) as r:
        r.resize(w, h)
        run_batch(r, ps, refs, w, h)
        for k in range(2 * len(ps)):
            r.update_parameters_buffer(ps[k % len(ps)])
            r.render(stats=False)
            assert np.array_equal(r.read_frame(), refs[k % len(ps)]["rgba"]), f"frame {k}"
        r.update_parameters_buffer(ps[0])
        st = r.render(stats=True)
        assert counters_of(st) == [int(c) for c in refs[0]["counters"][:7]]
