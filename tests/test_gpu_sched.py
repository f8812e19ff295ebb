"""What the pixel scheduler is for, on the GPU (DESIGN.md section 3 "The scheduler: keys, order,
resample"): the cost keys a persistent launch records against the oracle's per-pixel costs, the
fetch order it ranks for the next launch (the default, fused path), the order the sort path
(FRM_SCHED=sort: also every first launch, resize, injected key map and reloaded kernel) fetches by
against a stable sort of the keys it started from, the resample of the keys on a resize texel by
texel, and the keys a slot borrows from another. Frames are rendered into zeroed buffers, so a
pixel the order dropped cannot hide behind the previous frame's bytes."""
import ctypes

import numpy as np
import pytest

import frm
from frm import _lib

import sched_cases as S
import sched_reference as R
from test_gpu_reload import copy_sources

pytestmark = pytest.mark.gpu

PERSISTENT = frm.FRM_FLAG_PERSISTENT_KERNEL


def open_renderer(case, inflight=1):
    r = frm.Renderer(device=0, max_steps=case.max_steps, flags=case.flags | PERSISTENT, frames_in_flight=inflight,
                     supersampling=case.supersampling)
    r.resize(case.width, case.height)
    r.update_parameters_buffer(case.params())
    return r


class Target:
    """A zeroed device frame and counters for whole-frame launches through frm_render_bands."""

    def __init__(self, width, height):
        import torch

        self.w, self.h = width, height
        self.buf = torch.zeros(width * height * 4, dtype=torch.uint8, device="cuda")
        self.counters = torch.zeros(8, dtype=torch.int64, device="cuda")

    def launch(self, r):
        self.buf.zero_()
        self.counters.zero_()
        r.render_bands(self.buf.data_ptr(), self.buf.numel(), self.h, 0, 1, 0, self.counters.data_ptr())
        r.synchronize()

    def check(self, ref, what):
        img = self.buf.cpu().numpy().reshape(self.h, self.w, 4)
        bad = int(np.any(img != ref["rgba"], axis=-1).sum())
        assert bad == 0, f"{what}: {bad} pixels differ from the oracle"
        got = [int(v) for v in self.counters.cpu().tolist()][:7]
        assert got == [int(v) for v in ref["counters"][:7]], what


def check_keys(keys, cost, what):
    """The recorded keys lie in key_of(cost)'s allowed set at every pixel; prints how many costs
    had an exact logarithm or two allowed keys."""
    cost = np.asarray(cost).reshape(-1)
    assert keys.shape == cost.shape, f"{what}: {keys.shape[0]} keys for {cost.shape[0]} pixels"
    ok = R.keys_allowed(keys, cost)
    key, lo, hi = R.key_of(cost)
    if not ok.all():
        i = int(np.argmax(~ok))
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} keys outside the allowed set; pixel {i}: "
                             f"cost {int(cost[i])}, key {int(keys[i])}, allowed {int(lo[i])}..{int(hi[i])}")
    band = R.in_band(cost)
    n = cost.astype(np.uint64) + np.uint64(1)
    pow2 = (n & (n - np.uint64(1))) == 0
    print(f"KEYS {what}: power-of-two costs {int(pow2.sum())}, band costs {int(band.sum())} "
          f"(not the float64 key: {int((band & (keys != key)).sum())})")


def check_ranked_order(r, keys, what):
    order, ranked = r.pixel_order()
    assert ranked == 1, f"{what}: the launch did not rank its keys"
    err = R.check_order(order, keys)
    assert err is None, f"{what}: {err}"
    return order


# ---- keys and the fused order (the default) --------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_keys_and_fused_order(frm_lib, oracle, case):
    """Two identical launches (the second fetches in the order the first ranked): bytes and counters
    equal the oracle's, every key lies in the allowed set of the oracle's cost, and the ranked order
    is a permutation along which the keys just read never increase."""
    ref = S.reference(oracle, case)
    w, h = case.render_size
    with open_renderer(case) as r:
        tgt = None if case.supersampling > 1 else Target(w, h)  # a supersampled context renders no bands
        for launch in range(2):
            what = f"{case.name} launch {launch}"
            if tgt:
                tgt.launch(r)
                tgt.check(ref, what)
            else:
                st = r.render(stats=True)
                assert [st[k] for k in ("pixels", "hit_pixels", "primary_steps", "shadow_steps", "normal_evals",
                                        "fractal_bodies", "fractal_bailouts")] == [int(v) for v in ref["counters"][:7]]
            keys = r.pixel_keys()
            check_keys(keys, ref["cost"], what)
            check_ranked_order(r, keys, what)


def test_neg_zero_origin_records_the_same_keys(frm_lib, oracle):
    """The frame whose origin has a -0 component runs step 0 per pixel, its +0 twin once per frame
    (KernelArgs::first_info): the seeded cost equals the counted one, key for key."""
    got = {}
    for name in ("origin_neg_zero", "origin_pos_zero"):
        case = S.BY_NAME[name]
        with open_renderer(case) as r:
            tgt = Target(*case.render_size)
            tgt.launch(r)
            tgt.check(S.reference(oracle, case), name)
            got[name] = r.pixel_keys()
    assert np.array_equal(got["origin_neg_zero"], got["origin_pos_zero"])


def test_batch_keys_are_the_last_frames(frm_lib, oracle):
    """A launch of 3 poses: keys and order are those of its last frame, in both launches."""
    import torch

    base = S.BY_NAME["mandelbulb_n12"]
    w, h = base.width, base.height
    ps = [S.params_for(base.scene, base.iters, base.time, w, h, pose=pz) for pz in S.BATCH_POSES]
    refs = [oracle.render(p, w, h, base.max_steps) for p in ps]
    cost = oracle.render_costs(ps[-1], w, h, base.max_steps)
    fb = w * h * 4
    out = torch.zeros(len(ps) * fb, dtype=torch.uint8, device="cuda")
    with frm.Renderer(device=0, max_steps=base.max_steps, flags=PERSISTENT) as r:
        r.resize(w, h)
        for launch in range(2):
            out.zero_()
            r.render_bands_batch(ps, out.data_ptr(), dst_bytes=out.numel(), frame_stride=fb, band_rows=h, first_band=0,
                                 band_stride=1)
            r.synchronize()
            img = out.cpu().numpy().reshape(len(ps), h, w, 4)
            for k, ref in enumerate(refs):
                assert np.array_equal(img[k], ref["rgba"]), f"launch {launch} frame {k}"
            keys = r.pixel_keys()
            check_keys(keys, cost, f"batch launch {launch}")
            check_ranked_order(r, keys, f"batch launch {launch}")


def test_band_keys_are_in_local_pixel_order(frm_lib, oracle):
    """Two simulated ranks' interleaved bands (a short last band): each rank's keys are its own rows'
    costs in local pixel order, and its order a permutation of exactly those pixels."""
    import torch

    b = S.BANDS
    w, h, br, ranks = b["width"], b["height"], b["band_rows"], b["ranks"]
    case = S.SchedCase("bands", 18, 12, S.P8, w, h)
    p = case.params()
    ref = oracle.render(p, w, h, case.max_steps)
    cost = oracle.render_costs(p, w, h, case.max_steps)
    for rk in range(ranks):
        rows = S.band_rows_of(h, br, rk, ranks)
        reserved = -(-len(rows) // br) * br  # a band buffer holds whole bands
        buf = torch.zeros(reserved * w * 4, dtype=torch.uint8, device="cuda")
        with open_renderer(case) as r:
            for launch in range(2):
                buf.zero_()
                r.render_bands(buf.data_ptr(), buf.numel(), br, rk, ranks, 0)
                r.synchronize()
                img = buf.cpu().numpy().reshape(reserved, w, 4)[:len(rows)]
                assert np.array_equal(img, ref["rgba"][rows]), f"rank {rk} launch {launch}"
                keys = r.pixel_keys()
                check_keys(keys, cost[rows], f"rank {rk} launch {launch}")
                order = check_ranked_order(r, keys, f"rank {rk} launch {launch}")
                assert order.size == len(rows) * w


def test_two_frames_in_flight_rank_each_slot(frm_lib, oracle):
    """Two slots, four launches: every launch ranks the keys of its own slot."""
    case = S.BY_NAME["mandelbulb_n12"]
    ref = S.reference(oracle, case)
    with open_renderer(case, inflight=2) as r:
        tgt = Target(*case.render_size)
        for launch in range(4):
            tgt.launch(r)
            tgt.check(ref, f"launch {launch}")
            keys = r.pixel_keys()
            check_keys(keys, ref["cost"], f"inflight launch {launch}")
            check_ranked_order(r, keys, f"inflight launch {launch}")


# ---- the sort path -------------------------------------------------------------------------------
SORT_CASES = ["mandelbulb_n12", "menger0_n5", "size_1x1", "size_65x63", "size_64x64", "size_4097x1", "size_127x97",
              "all_zero", "saturating"]


def expect_sorted_order(r, keys_before, what):
    order, ranked = r.pixel_order()
    assert ranked == 0, f"{what}: the sort path reports a ranked order"
    want = R.stable_order(keys_before)
    assert order.shape == want.shape, what
    bad = np.nonzero(order != want)[0]
    assert bad.size == 0, (f"{what}: the order differs from the stable sort at {bad.size} of {order.size} positions, "
                           f"first {int(bad[0])}: pixel {int(order[bad[0]])}, expected {int(want[bad[0]])}")


@pytest.mark.parametrize("name", SORT_CASES)
def test_sort_path_order_is_the_stable_sort(frm_lib, oracle, monkeypatch, name):
    """FRM_SCHED=sort: a geometry's first launch fetches in pixel order; the second by the stable
    descending sort of the first one's keys (SortPairsDescending over (key, pixel index))."""
    monkeypatch.setenv("FRM_SCHED", "sort")
    case = S.BY_NAME[name]
    ref = S.reference(oracle, case)
    npix = case.render_size[0] * case.render_size[1]
    with open_renderer(case) as r:
        tgt = Target(*case.render_size)
        tgt.launch(r)
        tgt.check(ref, f"{name} first")
        order, ranked = r.pixel_order()
        assert ranked == 0 and np.array_equal(order, np.arange(npix, dtype=np.uint32))
        keys1 = r.pixel_keys()
        check_keys(keys1, ref["cost"], f"{name} sort first")
        tgt.launch(r)
        tgt.check(ref, f"{name} second")
        expect_sorted_order(r, keys1, f"{name} second")
        check_keys(r.pixel_keys(), ref["cost"], f"{name} sort second")


def injected_maps(keys):
    rng = np.random.default_rng(11)
    last = np.zeros_like(keys)
    last[-1] = 255
    return {"all_equal": np.full_like(keys, 93), "reversed": 255 - keys,
            "random": rng.integers(0, 256, keys.size).astype(np.uint8),
            "two_values": (rng.integers(0, 2, keys.size) * 255).astype(np.uint8), "last_pixel": last}


@pytest.mark.parametrize("name", ["mandelbulb_n12", "size_127x97"])
def test_sort_path_injected_keys(frm_lib, oracle, monkeypatch, name):
    """Injected key maps: the next launch fetches by their stable sort, renders the oracle's bytes
    and records its own costs' keys again."""
    monkeypatch.setenv("FRM_SCHED", "sort")
    case = S.BY_NAME[name]
    ref = S.reference(oracle, case)
    with open_renderer(case) as r:
        tgt = Target(*case.render_size)
        tgt.launch(r)
        keys = r.pixel_keys()
        for label, inj in injected_maps(keys).items():
            r.set_pixel_keys(inj)
            tgt.launch(r)
            tgt.check(ref, f"{name} {label}")
            expect_sorted_order(r, inj, f"{name} {label}")
            check_keys(r.pixel_keys(), ref["cost"], f"{name} injected {label}")


RESIZES = [((96, 54), (160, 90)),   # the buffers grow
           ((160, 90), (64, 36)),   # in place, through the sort's second half
           ((96, 54), (130, 9)),
           ((200, 120), (16, 9)),   # ratio 12.5: the 8 x 8 cap
           ((40, 30), (1, 1)),
           ((1, 1), (40, 30))]


@pytest.mark.parametrize("src,dst", RESIZES, ids=[f"{s[0]}x{s[1]}_to_{d[0]}x{d[1]}" for s, d in RESIZES])
def test_resize_resamples_the_keys_texel_by_texel(frm_lib, oracle, monkeypatch, src, dst):
    """Random bytes injected at the old size: the first frame of the new size fetches by the stable
    sort of their resample. Any wrong key of rescale_keys_kernel moves its pixel in a stable sort."""
    monkeypatch.setenv("FRM_SCHED", "sort")
    (sw, sh), (dw, dh) = src, dst
    a = S.SchedCase("resize_src", 18, 12, S.P8, sw, sh)
    b = S.SchedCase("resize_dst", 18, 12, S.P8, dw, dh)
    p = b.params()
    ref = oracle.render(p, dw, dh, b.max_steps)
    cost = oracle.render_costs(p, dw, dh, b.max_steps)
    inj = np.random.default_rng(sw * 131 + dw).integers(0, 256, sw * sh).astype(np.uint8)
    with open_renderer(a) as r:
        Target(sw, sh).launch(r)
        r.set_pixel_keys(inj)
        r.resize(dw, dh)
        r.update_parameters_buffer(p)
        tgt = Target(dw, dh)
        tgt.launch(r)
        tgt.check(ref, "resized frame")
        expect_sorted_order(r, R.rescale(inj, sw, sh, dw, dh), f"{sw}x{sh} -> {dw}x{dh}")
        check_keys(r.pixel_keys(), cost, f"resize {sw}x{sh} -> {dw}x{dh}")


def test_second_slot_borrows_the_first_slots_keys(frm_lib, oracle, monkeypatch):
    """Two frames in flight: slot 1's first launch has no history of its own and fetches by the stable
    sort of the keys slot 0 recorded."""
    monkeypatch.setenv("FRM_SCHED", "sort")
    case = S.BY_NAME["mandelbulb_n12"]
    ref = S.reference(oracle, case)
    with open_renderer(case, inflight=2) as r:
        tgt = Target(*case.render_size)
        tgt.launch(r)
        keys0 = r.pixel_keys()
        check_keys(keys0, ref["cost"], "slot 0")
        assert len(np.unique(keys0)) > 20  # an order that tells these keys from any constant map
        tgt.launch(r)  # slot 1
        tgt.check(ref, "slot 1 first launch")
        expect_sorted_order(r, keys0, "slot 1 first launch")


def test_reloaded_kernels_sort_and_report_unranked(frm_lib, oracle, tmp_path):
    """Runtime-reloaded kernels do not rank: every launch sorts the keys the last one recorded."""
    case = S.BY_NAME["mandelbulb_n12"]
    ref = S.reference(oracle, case)
    npix = case.width * case.height
    with open_renderer(case) as r:
        r.reload(str(copy_sources(tmp_path, "csrc")))
        tgt = Target(*case.render_size)
        tgt.launch(r)
        tgt.check(ref, "reloaded first")
        order, ranked = r.pixel_order()
        assert ranked == 0 and np.array_equal(order, np.arange(npix, dtype=np.uint32))
        keys1 = r.pixel_keys()
        check_keys(keys1, ref["cost"], "reloaded first")
        tgt.launch(r)
        tgt.check(ref, "reloaded second")
        expect_sorted_order(r, keys1, "reloaded second")


# ---- errors of frm_debug_pixel_order ---------------------------------------------------------------
def test_pixel_order_errors(frm_lib, oracle):
    case = S.BY_NAME["size_65x63"]
    npix = case.width * case.height
    L = frm_lib
    with open_renderer(case) as r:
        with pytest.raises(frm.FrmError) as e:  # no persistent launch yet
            r.pixel_order()
        assert e.value.code == _lib.FRM_ERR_INVALID_ARGUMENT
        with pytest.raises(frm.FrmError) as e:
            r.pixel_keys()
        assert e.value.code == _lib.FRM_ERR_INVALID_ARGUMENT
        r.render(stats=False)
        full, ranked = r.pixel_order()
        assert full.size == npix and ranked == 1
        big, _ = r.pixel_order(n=npix + 1000)  # the count is the launch's pixels, not the capacity offered
        assert np.array_equal(big, full)
        part, ranked = r.pixel_order(n=100)    # a short buffer: n entries, and the count says so
        assert ranked == 1 and np.array_equal(part, full[:100])
        out = np.zeros(4, np.uint32)
        flag = ctypes.c_uint32()
        assert L.frm_debug_pixel_order(r.ctx, None, 4, ctypes.byref(flag)) == -_lib.FRM_ERR_INVALID_ARGUMENT
        assert L.frm_debug_pixel_order(r.ctx, out.ctypes.data, 4, None) == -_lib.FRM_ERR_INVALID_ARGUMENT
        # a smaller geometry in the same buffers: the count follows the last launch, not the capacity
        r.resize(16, 9)
        r.update_parameters_buffer(S.SchedCase("small", 18, 12, S.P8, 16, 9).params())
        r.render(stats=False)
        small, _ = r.pixel_order(n=npix)
        assert small.size == 16 * 9 and R.check_order(small, r.pixel_keys()) is None
    with frm.Renderer(max_steps=64, flags=PERSISTENT, devices=[0, 0]) as g:  # a group context
        g.resize(32, 18)
        g.update_parameters_buffer(S.SchedCase("group", 18, 12, S.P8, 32, 18).params())
        g.render(stats=False)
        with pytest.raises(frm.FrmError) as e:
            g.pixel_order()
        assert e.value.code == _lib.FRM_ERR_UNSUPPORTED
