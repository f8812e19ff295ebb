"""GPU parity at the four hard limits of include/frm.h, on the cases of tests/limit_cases.py
(tests/test_limit_census.py proves on the CPU that each reaches what it is named for):

1. FRM_MAX_STEPS_LIMIT: 8 x 8 frames whose marches run up to 4194303 steps: hits after 2e5 to 4.19e6
   steps along a flat face of the cube, the Sierpinski and the Koch tetrahedra and on the Mandelbulb's
   r = 8 shell, misses that run every step (stalled far from the cube and the sphere, crawling around
   the Mandelbulb). Both march kernels, the trace, launches of several frames, and the 2 x 2 samples of
   a 4 x 4 frame through the supersampled and the adaptive path.
2. FRM_MAX_DIMENSION: frames of 32768 x 1 and 1 x 32768 through frm_render, the trace, the
   asynchronous readbacks, bands and their reassembly, a launch of three frames, supersampling and
   adaptive sampling at factor 4 from 8192, and a shutter frame.
3. FRM_MAX_NUM_ITERATIONS: every family at N = 65536 (inside the Mandelbulb every distance estimator
   runs all 65537 bodies).
4. Frame and rank strides of 4 GiB + 64 bytes in frm_render_bands_batch, frm_accumulate and
   frm_unshuffle_bands.

Every assertion is exact: RGBA8 bytes and the seven work counters equal the oracle's, traces equal
the oracle's bit for bit on hit pixels (NaN equal to NaN). The persistent kernel renders twice on one
context, so its second launch runs in scheduled order. Nothing here uses the resident ring. Each
render prints its kernel time (pytest -s)."""
import ctypes

import numpy as np
import pytest

import adaptive_reference as ada
import frm
import limit_cases as lc
import shutter_reference as shutter
import ssaa_reference as ssaa
from frm import _lib

pytestmark = pytest.mark.gpu

PERSISTENT, SIMPLE = frm.FRM_FLAG_PERSISTENT_KERNEL, frm.FRM_FLAG_SIMPLE_KERNEL
KERNELS = [PERSISTENT, SIMPLE]
KERNEL_IDS = ["persistent", "simple"]
COUNTERS = ("pixels", "hit_pixels", "primary_steps", "shadow_steps", "normal_evals", "fractal_bodies",
            "fractal_bailouts")


def counters_of(st):
    return [st[c] for c in COUNTERS]


def want_counters(*refs):
    return [sum(int(ref["counters"][i]) for ref in refs) for i in range(7)]


def launches(flags):
    return 2 if flags & PERSISTENT else 1


def assert_frame(img, ref_rgba, what):
    diff = np.any(img != ref_rgba, axis=-1)
    assert not diff.any(), f"{what}: {diff.sum()} pixels differ, first at {tuple(np.argwhere(diff)[0])}"


def assert_trace(tr, ref_trace, what):
    ref = ref_trace.reshape(tr.shape)
    hit = ref[..., 0] != 0
    assert np.array_equal(tr[..., 0] != 0, hit), what
    a, b = tr[hit], ref[hit]
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert same.all(), (f"{what}: {np.sum(~same.all(axis=-1))} hit pixels differ, fields "
                        f"{sorted(set(np.nonzero(~same)[1].tolist()))}, steps {a[~same.all(axis=-1)][:4, 1]} "
                        f"for {b[~same.all(axis=-1)][:4, 1]}")


def render_and_compare(r, ref, flags, what):
    for launch in range(launches(flags)):
        st = r.render(stats=True)
        print(f"{what} launch {launch}: kernel {st['kernel_ms']:.1f} ms")
        assert_frame(r.read_frame(), ref["rgba"], f"{what} launch {launch}")
        assert counters_of(st) == want_counters(ref), f"{what} launch {launch}"


def batch_and_compare(r, params, refs, w, h, what, n_launches=2):
    """One frm_render_bands_batch launch of whole frames, each compared, and the summed counters."""
    import torch
    fb = w * h * 4
    out = torch.zeros(len(params) * fb, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    for launch in range(n_launches):
        out.zero_()
        counters.zero_()
        r.render_bands_batch(params, out.data_ptr(), dst_bytes=out.numel(), frame_stride=fb, band_rows=h, first_band=0,
                             band_stride=1, stream=0, dev_counters=counters.data_ptr())
        torch.cuda.synchronize()
        img = out.cpu().numpy().reshape(len(params), h, w, 4)
        for k, ref in enumerate(refs):
            assert_frame(img[k], ref["rgba"], f"{what} launch {launch} frame {k}")
        assert [int(v) for v in counters.cpu().tolist()][:7] == want_counters(*refs), f"{what} launch {launch}"


# ---- 1. deep marches -------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("case", lc.DEEP_CASES, ids=lc.DEEP_IDS)
def test_deep_march_bytes_and_counters(frm_lib, oracle, case, flags):
    """The ambient-occlusion term (1 - steps / max_steps)^100 puts a hit's step count into its bytes,
    primary_steps sums the counts of all 64 pixels."""
    ref = lc.deep_reference(oracle, case)
    with frm.Renderer(device=0, max_steps=case.max_steps, flags=flags | case.flags) as r:
        r.resize(case.width, case.height)
        r.update_parameters_buffer(case.params())
        render_and_compare(r, ref, flags, case.name)


@pytest.mark.parametrize("case", lc.DEEP_CASES, ids=lc.DEEP_IDS)
def test_deep_march_trace(frm_lib, oracle, case):
    """frm_debug_trace after a persistent-kernel frame: the step count of every hit as a number (a
    float holds counts below 2^24 exactly), with its normal, shadow result and colour."""
    ref = lc.deep_reference(oracle, case)
    with frm.Renderer(device=0, max_steps=case.max_steps, flags=PERSISTENT | case.flags) as r:
        r.resize(case.width, case.height)
        r.update_parameters_buffer(case.params())
        r.render(stats=True)
        assert_trace(r.trace(), ref["trace"], case.name)


@pytest.mark.parametrize("name", lc.BATCH_CAMERA_CASES)
def test_deep_march_in_a_launch_of_two_cameras(frm_lib, oracle, name):
    """The multi-frame instantiation: the case's camera and P1 (under the case's aspect) in one launch."""
    case = lc.deep_case(name)
    refs = [lc.deep_reference(oracle, case), lc.deep_reference(oracle, case, camera=lc.P1)]
    params = [case.params(), case.params(camera=lc.P1)]
    with frm.Renderer(device=0, max_steps=case.max_steps, flags=PERSISTENT) as r:
        r.resize(case.width, case.height)
        batch_and_compare(r, params, refs, case.width, case.height, name)


def test_mandelbulb_crawl_in_a_launch_of_two_times(frm_lib, oracle):
    """The per-lane-power instantiation: the crawl at power 8 beside the same camera's frame at power 9,
    whose pixels all hit at step 0."""
    case = lc.deep_case("mb_crawl")
    refs = [lc.deep_reference(oracle, case, time=t) for t in lc.MB_CRAWL_TIMES]
    params = [case.params(time=t) for t in lc.MB_CRAWL_TIMES]
    with frm.Renderer(device=0, max_steps=case.max_steps, flags=PERSISTENT) as r:
        r.resize(case.width, case.height)
        batch_and_compare(r, params, refs, case.width, case.height, "mb_crawl times")


@pytest.mark.parametrize("flags", KERNELS, ids=KERNEL_IDS)
def test_deep_march_supersampled(frm_lib, oracle, flags):
    """frm_set_supersampling(2) on a 4 x 4 output renders the case's 8 x 8 frame and resolves it."""
    case = lc.deep_case(lc.SUPERSAMPLED_CASE)
    ref = lc.deep_reference(oracle, case)
    want = {"rgba": ssaa.box_resolve(ref["rgba"], 2, oracle), "counters": ref["counters"]}
    with frm.Renderer(device=0, max_steps=case.max_steps, flags=flags, supersampling=2) as r:
        r.resize(4, 4)
        assert (r.render_width, r.render_height) == (8, 8)
        r.update_parameters_buffer(case.params(4, 4))
        render_and_compare(r, want, flags, f"{case.name} supersampled")


@pytest.mark.parametrize("flags", KERNELS, ids=KERNEL_IDS)
def test_deep_march_adaptive(frm_lib, oracle, flags):
    """frm_set_adaptive(2, 0): refine_samples marches on its own; threshold 0 refines every pixel, so
    the bytes are the supersampled frame's and the counters the 4 x 4 frame's plus the 8 x 8 frame's."""
    case = lc.deep_case(lc.SUPERSAMPLED_CASE)
    hi, lo = lc.deep_reference(oracle, case), lc.deep_reference(oracle, case, width=4, height=4)
    want = ada.compose(lo["rgba"], ssaa.box_resolve(hi["rgba"], 2, oracle), np.ones((4, 4), bool))
    with frm.Renderer(device=0, max_steps=case.max_steps, flags=flags, adaptive=(2, 0)) as r:
        r.resize(4, 4)
        r.update_parameters_buffer(case.params(4, 4))
        for launch in range(launches(flags)):
            st = r.render(stats=True)
            print(f"{case.name} adaptive launch {launch}: kernel {st['kernel_ms']:.1f} ms")
            assert_frame(r.read_frame(), want, f"launch {launch}")
            assert counters_of(st) == want_counters(lo, hi), f"launch {launch}"


# ---- 2. frames at FRM_MAX_DIMENSION ----------------------------------------------------------------

UNIT_CASES = [c for c in lc.DIM_CASES if c.unit_aspect]
UNIT_IDS = [c.name for c in UNIT_CASES]


@pytest.mark.parametrize("flags", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("case", lc.DIM_CASES, ids=lc.DIM_IDS)
def test_dimension_frame(frm_lib, oracle, case, flags):
    """frm_render at 32768 x 1 and 1 x 32768; on the persistent kernel also the trace and the two
    asynchronous readbacks (frm_present_async at the same size with FRM_BLIT_SRGB gives the frame)."""
    ref = lc.dim_reference(oracle, case)
    w, h = case.width, case.height
    with frm.Renderer(device=0, max_steps=lc.DIM_STEPS, flags=flags) as r:
        r.resize(w, h)
        r.update_parameters_buffer(case.params())
        render_and_compare(r, ref, flags, case.name)
        assert_frame(r.frame_pixels(r.read_frame_async()), ref["rgba"], "read_frame_async")
        assert_frame(r.frame_pixels(r.present_async(w, h, srgb=True)), ref["rgba"], "present_async")
        if flags & PERSISTENT:
            assert_trace(r.trace(), ref["trace"], case.name)


def local_rows(height, band_rows, first, stride):
    out = ctypes.c_uint32(0)
    assert frm.load().frm_band_rows_for(height, band_rows, first, stride, ctypes.byref(out)) == 0
    return out.value


BAND_SPLITS = [  # width, height, band_rows, ranks
    (1, lc.MAX_DIM, 1, 16),           # 32768 bands of one pixel, 2048 per rank
    (1, lc.MAX_DIM, lc.MAX_DIM, 1),   # one band
    (1, lc.MAX_DIM, 20000, 2),        # a short last band: 20000 and 12768 rows (in a slot of 20000)
    (lc.MAX_DIM, 1, 1, 1),
    (lc.MAX_DIM, 1, 1, 2),            # one band: rank 1 gets no rows
]


@pytest.mark.parametrize("flags", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("scene", list(lc.DIM_SCENES))
@pytest.mark.parametrize("width,height,band_rows,ranks", BAND_SPLITS,
                         ids=[f"{w}x{h}-rows{b}-ranks{n}" for w, h, b, n in BAND_SPLITS])
def test_dimension_bands_reassemble(frm_lib, oracle, width, height, band_rows, ranks, scene, flags):
    """frm_render_bands per rank (first_band = rank, band_stride = ranks) and frm_unshuffle_bands."""
    import torch
    case = lc.dim_case(f"{scene}_{'wide' if width > 1 else 'tall'}_unit")
    ref = lc.dim_reference(oracle, case)
    rows = [local_rows(height, band_rows, k, ranks) for k in range(ranks)]  # whole bands: a short last band keeps its slot
    assert height <= sum(rows) < height + band_rows
    rank_stride = max(rows) * width * 4
    gathered = torch.zeros(ranks * rank_stride, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    out = torch.zeros(width * height * 4, dtype=torch.uint8, device="cuda")
    with frm.Renderer(device=0, max_steps=lc.DIM_STEPS, flags=flags) as r:
        r.resize(width, height)
        r.update_parameters_buffer(case.params())
        for launch in range(launches(flags)):
            counters.zero_()
            for k in range(ranks):  # a rank without rows makes the call too: it launches nothing and succeeds
                r.render_bands(gathered.data_ptr() + k * rank_stride, rows[k] * width * 4, band_rows, k, ranks, 0,
                               counters.data_ptr())
            out.zero_()
            r.unshuffle_bands(gathered.data_ptr(), rank_stride, out.data_ptr(), out.numel(), band_rows, ranks)
            torch.cuda.synchronize()
            assert_frame(out.cpu().numpy().reshape(height, width, 4), ref["rgba"], f"launch {launch}")
            assert [int(v) for v in counters.cpu().tolist()][:7] == want_counters(ref), f"launch {launch}"


@pytest.mark.parametrize("case", UNIT_CASES, ids=UNIT_IDS)
def test_dimension_launch_of_three_poses(frm_lib, oracle, case):
    poses = ("P0", "P1", "P2")
    refs = [lc.dim_reference(oracle, case, pose=p) for p in poses]
    with frm.Renderer(device=0, max_steps=lc.DIM_STEPS, flags=PERSISTENT) as r:
        r.resize(case.width, case.height)
        batch_and_compare(r, [case.params(pose=p) for p in poses], refs, case.width, case.height, case.name)


def quarter(case):
    """The output size whose factor-4 render is 32768 long (and 4 across)."""
    return (lc.MAX_DIM // 4, 1) if case.width > 1 else (1, lc.MAX_DIM // 4)


@pytest.mark.parametrize("case", UNIT_CASES, ids=UNIT_IDS)
def test_dimension_supersampled(frm_lib, oracle, case):
    """frm_set_supersampling(4) at 8192 x 1 and 1 x 8192 renders 32768 x 4 and 4 x 32768; one pixel
    more is refused."""
    ow, oh = quarter(case)
    hi = lc.dim_reference(oracle, case, out_size=(ow, oh), factor=4, costs=True)
    want = {"rgba": ssaa.box_resolve(hi["rgba"], 4, oracle), "counters": hi["counters"]}
    with frm.Renderer(device=0, max_steps=lc.DIM_STEPS, flags=PERSISTENT, supersampling=4) as r:
        r.resize(ow, oh)
        assert max(r.render_width, r.render_height) == lc.MAX_DIM
        r.update_parameters_buffer(case.params(ow, oh))
        render_and_compare(r, want, PERSISTENT, f"{case.name} supersampled")
        with pytest.raises(frm.FrmError) as e:
            r.resize(ow + (ow > 1), oh + (oh > 1))  # 8193 x 1, 1 x 8193
        assert e.value.code == _lib.FRM_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("case", UNIT_CASES, ids=UNIT_IDS)
def test_dimension_adaptive(frm_lib, oracle, case):
    """frm_set_adaptive(4, T) at 8192 x 1 and 1 x 8192: the frame, the edge mask and the work counters.
    T = 16: F1's counters plus those of the refined pixels' samples. At 1 x 8192 a refined pixel is four
    whole rows of the 4 x 32768 frame, so the oracle's render of those rows gives all seven. At
    8192 x 1 the oracle's per-sample outputs summed over the refined blocks give pixels, hit_pixels,
    normal_evals and primary_steps, and from the scheduling cost fractal_bodies for the Mandelbulb (its
    cost is bodies) and shadow_steps for the Menger sponge (its cost is DE evaluations; its
    fractal_bodies and fractal_bailouts are 0): as test_gpu_adaptive.py, the wide Mandelbulb's
    shadow_steps and fractal_bailouts have no per-sample oracle output at this threshold.
    T = 0 refines every pixel: all seven are F1's plus the whole factor-4 frame's, in both shapes."""
    ow, oh = quarter(case)
    lo = lc.dim_reference(oracle, case, out_size=(ow, oh))
    hi = lc.dim_reference(oracle, case, out_size=(ow, oh), factor=4, costs=True)
    fs = ssaa.box_resolve(hi["rgba"], 4, oracle)
    hit = (hi["info"] & 1).astype(np.int64)
    c1, cs = want_counters(lo), want_counters(hi)
    with frm.Renderer(device=0, max_steps=lc.DIM_STEPS, flags=PERSISTENT, adaptive=(4, 16)) as r:
        r.resize(ow, oh)
        r.update_parameters_buffer(case.params(ow, oh))
        for T in (16, 0):
            r.set_adaptive(4, T)
            mask = ada.edge_mask(lo["rgba"], T)
            refined = int(mask.sum())
            want = ada.compose(lo["rgba"], fs, mask)
            over = lambda v: int(v.astype(np.int64).reshape(oh, 4, ow, 4).sum(axis=(1, 3))[mask].sum())
            hits, primary, cost = over(hit), over((hi["info"] >> 8).astype(np.int64) + hit), over(hi["cost"])
            if T == 0:
                assert refined == ow * oh
                seven = [a + b for a, b in zip(c1, cs)]
            elif oh > 1:
                assert 0 < refined < ow * oh
                rows = (4 * np.nonzero(mask[:, 0])[0][:, None] + np.arange(4)).ravel()
                part = oracle.render(case.params(ow, oh), 4 * ow, 4 * oh, lc.DIM_STEPS, rows=rows)
                seven = [a + b for a, b in zip(c1, want_counters(part))]
            else:
                assert 0 < refined < ow * oh
                seven = None
            for launch in range(2):
                st = r.render(stats=True)
                what = f"threshold {T} launch {launch}"
                assert_frame(r.read_frame(), want, what)
                assert np.array_equal(r.refine_mask(), mask), what
                assert st["pixels"] == ow * oh + 16 * refined, what
                assert st["hit_pixels"] == c1[1] + hits and st["normal_evals"] == c1[4] + 4 * hits, what
                assert st["primary_steps"] == c1[2] + primary, what
                if case.scene == 18:
                    assert st["fractal_bodies"] == c1[5] + cost, what
                else:
                    assert st["shadow_steps"] == c1[3] + cost - primary - 4 * hits, what
                    assert st["fractal_bodies"] == 0 and st["fractal_bailouts"] == 0, what
                if seven is not None:
                    assert counters_of(st) == seven, what


@pytest.mark.parametrize("scene", list(lc.DIM_SCENES))
def test_dimension_shutter(frm_lib, oracle, scene):
    """frm_render_shutter with 3 sub-frames (an orbiting camera, advancing time) at 32768 x 1."""
    case = lc.dim_case(f"{scene}_wide_unit")
    cam = frm.Camera(*lc.P1)
    cam.raw.orbit_angle_per_second, cam.raw.lock_yaw_mode = 2.0, 1
    timing = frm.Timing()
    timing.raw.time_factor = 4.0
    subs = frm.shutter_parameters(case.params(), cam, timing, 0, 0.2, 3, 1.0)
    rs = [oracle.render(p, case.width, case.height, lc.DIM_STEPS) for p in subs]
    assert np.any(rs[0]["rgba"] != rs[2]["rgba"])
    want = {"rgba": shutter.accumulate(np.stack([x["rgba"] for x in rs]), 1, oracle),
            "counters": np.sum([x["counters"] for x in rs], axis=0)}
    with frm.Renderer(device=0, max_steps=lc.DIM_STEPS, flags=PERSISTENT) as r:
        r.resize(case.width, case.height)
        for launch in range(2):
            st = r.render_shutter(subs, stats=True)
            assert_frame(r.read_frame(), want["rgba"], f"launch {launch}")
            assert counters_of(st) == want_counters(want), f"launch {launch}"


# ---- 3. FRM_MAX_NUM_ITERATIONS rendered ------------------------------------------------------------

@pytest.mark.parametrize("flags", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("case", lc.ITER_CASES, ids=lc.ITER_IDS)
def test_max_iterations_frame(frm_lib, oracle, case, flags):
    ref = lc.iter_reference(oracle, case)
    with frm.Renderer(device=0, max_steps=lc.ITER_STEPS, flags=flags) as r:
        r.resize(case.width, case.height)
        r.update_parameters_buffer(case.params())
        render_and_compare(r, ref, flags, case.name)


@pytest.mark.parametrize("case", lc.ITER_CASES, ids=lc.ITER_IDS)
def test_max_iterations_launch_of_two(frm_lib, oracle, case):
    """The case's camera and another in one launch; for the camera inside the Mandelbulb the other is
    P1, so lanes that leave every DE by the count run beside lanes that bail out."""
    other = lc.P1 if case.name == "mb_inside" else lc.ITER_SECOND_CAMERA
    refs = [lc.iter_reference(oracle, case), lc.iter_reference(oracle, case, camera=other)]
    with frm.Renderer(device=0, max_steps=lc.ITER_STEPS, flags=PERSISTENT) as r:
        r.resize(case.width, case.height)
        batch_and_compare(r, [case.params(), case.params(camera=other)], refs, case.width, case.height, case.name)


# ---- 4. strides of 4 GiB and more ------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_buffer(frm_lib):
    """One uninitialised allocation of 4 GiB + 1 MiB, of which the tests touch a few KiB."""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 16 << 30:
        print(f"skipped: {free >> 20} MiB of device memory free, the 4 GiB stride tests ask for 16 GiB")
        pytest.skip(f"{free >> 20} MiB of device memory free (16 GiB asked)")
    buf = torch.empty(lc.BIG_BUFFER_BYTES, dtype=torch.uint8, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


def stride_params(pose, w=lc.STRIDE_W, h=lc.STRIDE_H):
    return lc.params_for(18, 8, lc.P8, w, h, pose=pose)


def put(buf, offset, array):
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(array).reshape(-1))
    buf[offset:offset + flat.numel()].copy_(flat)


def test_batch_frame_stride_over_4gib(big_buffer, oracle):
    """Two frames 2^32 + 64 bytes apart. A stride cut to 32 bits would put frame 1 at byte 64, inside
    frame 0; the 64 bytes before frame 1 and the 64 after frame 0 keep their sentinel."""
    import torch
    w, h, fb = lc.STRIDE_W, lc.STRIDE_H, lc.STRIDE_W * lc.STRIDE_H * 4
    poses = ("P1", "P2")
    refs = [oracle.render(stride_params(p), w, h, lc.STRIDE_STEPS) for p in poses]
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    with frm.Renderer(device=0, max_steps=lc.STRIDE_STEPS, flags=PERSISTENT) as r:
        r.resize(w, h)
        for launch in range(2):
            big_buffer[:fb + 64] = 0xA5
            big_buffer[lc.BIG_STRIDE - 64:lc.BIG_STRIDE + fb + 64] = 0xA5
            counters.zero_()
            r.render_bands_batch([stride_params(p) for p in poses], big_buffer.data_ptr(), dst_bytes=big_buffer.numel(),
                                 frame_stride=lc.BIG_STRIDE, band_rows=h, first_band=0, band_stride=1, stream=0,
                                 dev_counters=counters.data_ptr())
            torch.cuda.synchronize()
            for k, ref in enumerate(refs):
                got = big_buffer[k * lc.BIG_STRIDE:k * lc.BIG_STRIDE + fb].cpu().numpy().reshape(h, w, 4)
                assert_frame(got, ref["rgba"], f"launch {launch} frame {k}")
                after = big_buffer[k * lc.BIG_STRIDE + fb:k * lc.BIG_STRIDE + fb + 64]
                assert bool((after == 0xA5).all()), f"launch {launch}: bytes after frame {k}"
            assert bool((big_buffer[lc.BIG_STRIDE - 64:lc.BIG_STRIDE] == 0xA5).all()), f"launch {launch}: bytes before frame 1"
            assert [int(v) for v in counters.cpu().tolist()][:7] == want_counters(*refs), f"launch {launch}"


@pytest.mark.parametrize("S", [1, 2])
def test_accumulate_frame_stride_over_4gib(big_buffer, oracle, S):
    """frm_accumulate of two frames 2^32 + 64 bytes apart, at factor 1 and 2 (sources of S x the size)."""
    import torch
    w, h = lc.STRIDE_W, lc.STRIDE_H
    frames = np.stack([oracle.render(stride_params(p, w, h), S * w, S * h, lc.STRIDE_STEPS)["rgba"] for p in ("P1", "P2")])
    assert np.any(frames[0] != frames[1])
    fb = frames[0].size
    big_buffer[:fb + 128] = 0xA5  # what a stride cut to 32 bits would read as frame 1 is not frame 1
    for k in range(2):
        put(big_buffer, k * lc.BIG_STRIDE, frames[k])
    dst = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    with frm.Renderer(device=0, max_steps=lc.STRIDE_STEPS) as r:
        r.accumulate(big_buffer.data_ptr(), big_buffer.numel(), lc.BIG_STRIDE, 2, w, h, S, divisor=2 * S * S,
                     dst_ptr=dst.data_ptr(), dst_bytes=dst.numel())
        r.synchronize()
    assert_frame(dst.cpu().numpy().reshape(h, w, 4), shutter.accumulate(frames, S, oracle), f"factor {S}")


def test_unshuffle_rank_stride_over_4gib(big_buffer, oracle):
    """Two ranks' bands of 5 rows (the last band 4), rendered 2^32 + 64 bytes apart and reassembled."""
    import torch
    w, h, band_rows = lc.STRIDE_W, lc.STRIDE_H, 5
    p = stride_params("P1")
    ref = oracle.render(p, w, h, lc.STRIDE_STEPS)
    rows = [local_rows(h, band_rows, k, 2) for k in range(2)]
    assert rows == [15, 10]  # rank 0's last band has 4 rows and a slot of 5
    big_buffer[:16 * w * 4] = 0xA5
    out = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    with frm.Renderer(device=0, max_steps=lc.STRIDE_STEPS, flags=PERSISTENT) as r:
        r.resize(w, h)
        r.update_parameters_buffer(p)
        for k in range(2):
            r.render_bands(big_buffer.data_ptr() + k * lc.BIG_STRIDE, rows[k] * w * 4, band_rows, k, 2)
        r.unshuffle_bands(big_buffer.data_ptr(), lc.BIG_STRIDE, out.data_ptr(), out.numel(), band_rows, 2)
        r.synchronize()
    torch.cuda.synchronize()
    assert_frame(out.cpu().numpy().reshape(h, w, 4), ref["rgba"], "reassembled")
