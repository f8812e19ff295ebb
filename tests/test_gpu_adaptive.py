"""Adaptive supersampling on the GPU (include/frm.h frm_set_adaptive, frm_refine): the edge pass on
raw texels, adaptive frames and their work counters against the oracle's plain and S x frames
composed by tests/adaptive_reference.py, the presentation paths, frames in flight (one device and a
three-rank group) across setting changes, and the error codes. Everything is bit-exact."""
import ctypes

import numpy as np
import pytest

import adaptive_reference as ada
import frm
import ssaa_reference as ssaa
from frm import _lib
from helpers import params_for

pytestmark = pytest.mark.gpu

COUNTERS = ("pixels", "hit_pixels", "primary_steps", "shadow_steps", "normal_evals", "fractal_bodies",
            "fractal_bailouts")
W, H, STEPS = 33, 17, 128
SCENES = {"mandelbulb": (18, 6), "menger": (3, 3)}  # scene, num_iterations (pose P1)
DEFAULT_T = frm.FRM_ADAPTIVE_DEFAULT_THRESHOLD


def counters_of(st):
    return [st[c] for c in COUNTERS]


@pytest.fixture(scope="module")
def frame_refs(oracle):
    """(scene name, S) -> the oracle's view of one frame, each render done once: the parameters, the
    plain frame F1 and its counters, and of the (S W) x (S H) frame the resolved image FS, the
    counters and, per sample, the hit bit, the primary DE evaluations and the scheduling cost."""
    cache = {}

    def get(name, S):
        if (name, S) not in cache:
            scene, iters = SCENES[name]
            p = params_for(scene, iters, frm.POWER8_TIME, W, H)
            lo = cache.get((name, 1)) or oracle.render(p, W, H, STEPS)
            cache[(name, 1)] = lo
            hi = oracle.render(p, S * W, S * H, STEPS, info=True)
            hit = (hi["info"] & oracle.INFO_HIT).astype(np.int64)
            ref = {
                "p": p,
                "f1": lo["rgba"],
                "c1": [int(c) for c in lo["counters"][:7]],
                "fs": ssaa.box_resolve(hi["rgba"], S, oracle),
                "cs": [int(c) for c in hi["counters"][:7]],
                "hit": hit,
                "primary": (hi["info"] >> 8).astype(np.int64) + hit,  # march steps, + the hit's evaluation
                "cost": oracle.render_costs(p, S * W, S * H, STEPS).astype(np.int64),
            }
            for v in ref.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            cache[(name, S)] = ref
        return cache[(name, S)]

    return get


def over_blocks(per_sample, mask, S):
    """Sum of a per-sample quantity of the S x frame over the S x S blocks of the refined pixels."""
    return int(per_sample.reshape(mask.shape[0], S, mask.shape[1], S).sum(axis=(1, 3))[mask].sum())


# ---- 1. the edge pass on raw texels, through frm_refine ---------------------------------------------

RAW_STEPS = 32
THRESHOLDS = (0, 1, 40, 255, 256)
RAW_SIZES = {(1, 1): 4, (67, 5): 3, (1, 70): 2, (130, 33): 2}  # w, h -> the factor used at that size


def raw_params(w, h):
    return params_for(3, 1, frm.POWER8_TIME, w, h)  # a cheap scene: Menger, one iteration


@pytest.fixture(scope="module")
def raw_renderer(gpu_renderer_factory):
    with gpu_renderer_factory(max_steps=RAW_STEPS) as r:
        yield r


@pytest.fixture(scope="module")
def raw_refs(oracle):
    cache = {}

    def get(w, h, S):
        if (w, h, S) not in cache:
            img = ssaa.box_resolve(oracle.render(raw_params(w, h), S * w, S * h, RAW_STEPS)["rgba"], S, oracle)
            img.setflags(write=False)
            cache[(w, h, S)] = img
        return cache[(w, h, S)]

    return get


def random_texels(w, h, seed):
    """Random texels with structure at several contrasts: blocks of one random colour, a sprinkle of
    per-texel noise below 45 codes, alpha random throughout."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, size=((h + 6) // 7, (w + 4) // 5, 3), dtype=np.uint8)
    img = np.empty((h, w, 4), np.uint8)
    img[..., :3] = np.repeat(np.repeat(blocks, 7, axis=0), 5, axis=1)[:h, :w]
    noise = rng.integers(0, 45, size=(h, w, 3), dtype=np.uint8) * (rng.random((h, w, 1)) < 0.3)
    img[..., :3] = np.clip(img[..., :3].astype(np.int32) + noise, 0, 255).astype(np.uint8)
    img[..., 3] = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    if w * h > 1:  # and one pair at the largest contrast there is
        img[0, 0, :3] = 0
        img[(0, 1) if w > 1 else (1, 0)][:3] = 255
    return img


def gpu_refine(r, src_img, S, T, params, offset=False, counters=False):
    """frm_refine of src_img [h, w, 4] from a torch device tensor; offset: the source starts 4 bytes
    into its allocation (only 4-byte aligned). Returns the frame (and the counters added)."""
    import torch
    h, w = src_img.shape[:2]
    flat = torch.from_numpy(np.ascontiguousarray(src_img).reshape(-1))
    buf = torch.zeros(flat.numel() + 4, dtype=torch.uint8, device="cuda")
    src = buf[4:] if offset else buf[:flat.numel()]
    src.copy_(flat)
    assert src.data_ptr() % 16 == (4 if offset else 0)
    dst = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(_lib.FRM_NUM_COUNTERS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    r.refine(src.data_ptr(), src.numel(), w, h, S, T, dst.data_ptr(), dst.numel(), params=params,
             dev_counters=cnt.data_ptr() if counters else 0)
    r.synchronize()
    out = dst.cpu().numpy().reshape(h, w, 4)
    return (out, cnt.cpu().numpy()[:7].tolist()) if counters else out


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "plus4"])
@pytest.mark.parametrize("w,h", list(RAW_SIZES))
def test_refine_random_texels(raw_renderer, raw_refs, w, h, offset):
    S = RAW_SIZES[(w, h)]
    src = random_texels(w, h, 100 * w + h)
    fs = raw_refs(w, h, S)
    opaque = src.copy()
    opaque[..., 3] = 255
    counts = []
    for T in THRESHOLDS:
        mask = ada.edge_mask(src, T)
        counts.append(int(mask.sum()))
        got, cnt = gpu_refine(raw_renderer, src, S, T, raw_params(w, h), offset, counters=True)
        assert np.array_equal(got, ada.compose(opaque, fs, mask)), f"threshold {T}"
        assert cnt[0] == S * S * counts[-1], f"threshold {T}"  # the refined samples, and only those
    assert counts[0] == w * h and counts[-1] == 0
    if w * h > 1:  # the thresholds in between split this frame
        assert w * h > counts[2] > counts[3] > 0


def test_refine_uses_the_context_parameters_when_none_are_given(raw_renderer, raw_refs):
    w, h, S = 67, 5, 3
    src = random_texels(w, h, 7)
    opaque = src.copy()
    opaque[..., 3] = 255
    raw_renderer.update_parameters_buffer(raw_params(w, h))
    got = gpu_refine(raw_renderer, src, S, 40, None)
    assert np.array_equal(got, ada.compose(opaque, raw_refs(w, h, S), ada.edge_mask(src, 40)))
    one = gpu_refine(raw_renderer, src, 1, 40, None)  # factor 1: every sample is the pixel itself
    assert np.array_equal(one, opaque)


# ---- 2. frames and counters ------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, frm.FRM_FLAG_PERSISTENT_KERNEL], ids=["default-kernel", "persistent"])
@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("name", list(SCENES))
def test_adaptive_frame_and_counters(frm_lib, frame_refs, name, S, flags):
    """Counters checked: at threshold 0 and 256 all seven (F1's plus the S x frame's; F1's alone). At
    threshold 16, from the oracle's per-sample outputs over the refined blocks: pixels, hit_pixels,
    normal_evals (4 per hit) and primary_steps (info) for both scenes; fractal_bodies for the
    Mandelbulb (its cost is bodies); shadow_steps for the Menger sponge (its cost is primary + shadow
    + normal evaluations), whose fractal_bodies and fractal_bailouts stay 0. The Mandelbulb's
    shadow_steps and fractal_bailouts have no per-sample oracle output and are left to 0 and 256."""
    ref = frame_refs(name, S)
    f1, fs, c1, cs = ref["f1"], ref["fs"], ref["c1"], ref["cs"]
    with frm.Renderer(max_steps=STEPS, flags=flags, adaptive=(S, 0)) as r:
        assert r.adaptive == (S, 0) and r.supersampling == 1
        r.resize(W, H)
        assert (r.width, r.height, r.render_width, r.render_height) == (W, H, W, H)
        r.update_parameters_buffer(ref["p"])
        for T in (0, DEFAULT_T, 256):
            r.set_adaptive(S, T)
            mask = ada.edge_mask(f1, T)
            R = int(mask.sum())
            want = ada.compose(f1, fs, mask)
            for k in range(2):  # the second frame runs in the scheduled order; the list order differs
                st = r.render(stats=True)
                got = counters_of(st)
                assert np.array_equal(r.read_frame(), want), f"threshold {T}, frame {k}"
                assert np.array_equal(r.refine_mask(), mask), f"threshold {T}, frame {k}"
                assert st["pixels"] == W * H + S * S * R
                assert st["march_steps"] == st["primary_steps"] + st["shadow_steps"]
                if T == 0:
                    assert R == W * H and got == [a + b for a, b in zip(c1, cs)], f"frame {k}"
                elif T == 256:
                    assert R == 0 and got == c1, f"frame {k}"
                else:
                    assert 0 < R < W * H
                    hits = over_blocks(ref["hit"], mask, S)
                    primary = over_blocks(ref["primary"], mask, S)
                    cost = over_blocks(ref["cost"], mask, S)
                    assert st["hit_pixels"] == c1[1] + hits
                    assert st["normal_evals"] == c1[4] + 4 * hits
                    assert st["primary_steps"] == c1[2] + primary
                    if name == "mandelbulb":
                        assert st["fractal_bodies"] == c1[5] + cost
                    else:
                        assert st["shadow_steps"] == c1[3] + cost - primary - 4 * hits
                        assert st["fractal_bodies"] == 0 and st["fractal_bailouts"] == 0


def test_factor_one_is_the_plain_frame(frm_lib, frame_refs):
    ref = frame_refs("mandelbulb", 2)
    with frm.Renderer(max_steps=STEPS) as r:
        assert r.adaptive == (1, DEFAULT_T)
        r.set_adaptive(1, 0)  # off, whatever the threshold
        r.resize(W, H)
        r.update_parameters_buffer(ref["p"])
        st = r.render(stats=True)
        assert counters_of(st) == ref["c1"]
        assert np.array_equal(r.read_frame(), ref["f1"])


# ---- 3. presentation -----------------------------------------------------------------------------

def test_presentation_reads_the_adaptive_frame(frm_lib, oracle, frame_refs):
    ref = frame_refs("mandelbulb", 2)
    want = ada.compose(ref["f1"], ref["fs"], ada.edge_mask(ref["f1"], DEFAULT_T))
    assert not np.array_equal(want, ref["f1"]) and not np.array_equal(want, ref["fs"])
    with frm.Renderer(max_steps=STEPS, adaptive=2) as r:
        assert r.adaptive == (2, DEFAULT_T)
        r.resize(W, H)
        r.update_parameters_buffer(ref["p"])
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), want)
        for ow, oh in ((50, 30), (20, 10)):  # magnifying, minifying
            for srgb, bgra, flags in ((True, False, 1), (False, True, 2)):
                got = r.present(ow, oh, srgb=srgb, bgra=bgra)
                assert np.array_equal(got, oracle.blit(want, ow, oh, flags)), (ow, oh, flags)
                t = r.present_async(ow, oh, srgb=srgb, bgra=bgra)
                assert np.array_equal(r.frame_pixels(t), got), (ow, oh, flags)
        assert np.array_equal(r.present(W, H, srgb=True), want)  # same size + FRM_BLIT_SRGB
        assert np.array_equal(r.frame_pixels(r.read_frame_async()), want)


# ---- 4. frames in flight ---------------------------------------------------------------------------

LW, LH, LSTEPS = 48, 27, 256
SETTINGS = [(2, 16), (2, 16), (3, 16), (3, 64), (1, 64), (1, 64)]  # frame k's (factor, threshold); 1: off


def loop_params():
    return [params_for((18, 0, 15)[k % 3], 6, frm.POWER8_TIME + 0.3 * k, LW, LH, pose=("P0", "P1", "P2")[k % 3])
            for k in range(6)]


@pytest.fixture(scope="module")
def loop_refs(oracle):
    """(frame k, S, T) -> the composed oracle frame of the moving loop, each render done once."""
    frames = loop_params()
    renders, cache = {}, {}

    def render(k, S):
        if (k, S) not in renders:
            img = oracle.render(frames[k], S * LW, S * LH, LSTEPS)["rgba"]
            renders[(k, S)] = ssaa.box_resolve(img, S, oracle) if S > 1 else img
        return renders[(k, S)]

    def get(k, S, T):
        if (k, S, T) not in cache:
            f1 = render(k, 1)
            img = ada.compose(f1, render(k, S), ada.edge_mask(f1, T)) if S > 1 else f1
            img.setflags(write=False)
            cache[(k, S, T)] = img
        return cache[(k, S, T)]

    return get


def run_loop(r, fif, settings):
    """The drop-in loop with a frame of presentation latency; settings[k] is frame k's."""
    held, got = [], []
    for k, p in enumerate(loop_params()):
        if r.adaptive != settings[k]:
            r.set_adaptive(*settings[k])  # tickets issued before keep their frames
        r.update_parameters_buffer(p)
        r.render(stats=False)
        held.append(r.read_frame_async())
        if len(held) > fif - 1:
            got.append(r.frame_pixels(held.pop(0)))
    got += [r.frame_pixels(t) for t in held]
    return got


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one-device", "group3"])
@pytest.mark.parametrize("fif", [1, 2, 3])
def test_moving_loop_with_setting_changes(frm_lib, loop_refs, fif, devices):
    with frm.Renderer(max_steps=LSTEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, frames_in_flight=fif,
                      devices=devices, adaptive=SETTINGS[0]) as r:
        r.resize(LW, LH)
        got = run_loop(r, fif, SETTINGS)
        assert r.adaptive == SETTINGS[-1]
    for k, g in enumerate(got):
        assert g.shape == (LH, LW, 4)
        assert np.array_equal(g, loop_refs(k, *SETTINGS[k])), f"frame {k} (factor, threshold {SETTINGS[k]})"
    # the loop's frames tell the settings apart: frame 3 at threshold 64 is not frame 3 at 16 or off
    assert not np.array_equal(loop_refs(3, 3, 64), loop_refs(3, 3, 16))
    assert not np.array_equal(loop_refs(3, 3, 64), loop_refs(3, 1, 64))


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one-device", "group3"])
def test_group_and_single_counters_agree_with_the_oracle(frm_lib, frame_refs, devices):
    ref = frame_refs("menger", 2)
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, devices=devices, adaptive=(2, 0)) as r:
        r.resize(W, H)
        r.update_parameters_buffer(ref["p"])
        st = r.render(stats=True)
        assert counters_of(st) == [a + b for a, b in zip(ref["c1"], ref["cs"])]
        assert np.array_equal(r.read_frame(), ref["fs"])


def test_async_readback_refuses_after_a_setting_change(frm_lib, frame_refs):
    ref = frame_refs("mandelbulb", 2)
    f1 = ref["f1"]
    want = ada.compose(f1, ref["fs"], ada.edge_mask(f1, DEFAULT_T))
    with frm.Renderer(max_steps=STEPS, frames_in_flight=2, adaptive=2) as r:
        r.resize(W, H)
        r.update_parameters_buffer(ref["p"])
        r.render(stats=False)
        t = r.read_frame_async()
        r.set_adaptive(2, DEFAULT_T)  # no change: the frame stays readable
        t2 = r.read_frame_async()
        r.set_adaptive(2, 64)  # as frm_resize: no frame under the new setting yet
        with pytest.raises(frm.FrmError) as e:
            r.read_frame_async()
        assert e.value.code == _lib.FRM_ERR_NOT_READY
        assert np.array_equal(r.frame_pixels(t2), want)
        r.render(stats=False)
        assert np.array_equal(r.frame_pixels(r.read_frame_async()), ada.compose(f1, ref["fs"], ada.edge_mask(f1, 64)))
        assert t != t2


# ---- 5. errors -------------------------------------------------------------------------------------

def current(r):
    f, t = ctypes.c_uint32(), ctypes.c_uint32()
    assert r._lib.frm_get_adaptive(r.ctx, ctypes.byref(f), ctypes.byref(t)) == _lib.FRM_OK
    return f.value, t.value


def raises_code(code, fn, *args, **kw):
    with pytest.raises(frm.FrmError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


def test_adaptive_errors(frm_lib, tmp_path):
    import torch
    INV, UNS = _lib.FRM_ERR_INVALID_ARGUMENT, _lib.FRM_ERR_UNSUPPORTED
    with frm.Renderer(max_steps=64) as r:
        assert current(r) == (1, DEFAULT_T)
        r.set_adaptive(2, 40)
        for bad in ((0, 40), (5, 40), (2, 257), (3, 2 ** 31)):
            raises_code(INV, r.set_adaptive, *bad)
            assert current(r) == (2, 40) and r.adaptive == (2, 40)
        # 2 x 20000 exceeds FRM_MAX_DIMENSION: the size is refused, then set with adaptive off
        raises_code(INV, r.resize, 20000, 8)
        raises_code(INV, r.resize, 8, 20000)
        r.set_adaptive(1)
        r.resize(10000, 8)
        r.set_adaptive(3, 40)
        raises_code(INV, r.set_adaptive, 4, 40)  # samples on a frame 40000 texels wide
        assert current(r) == (3, 40)
        # adaptive and supersampling exclude each other, whichever comes second
        r.resize(32, 32)
        raises_code(UNS, r.set_supersampling, 2)
        assert r.supersampling == 1 and current(r) == (3, 40)
        r.set_supersampling(1)  # off stays allowed
        r.set_adaptive(1)
        r.set_supersampling(2)
        raises_code(UNS, r.set_adaptive, 2, 40)
        assert current(r) == (1, DEFAULT_T) and r.adaptive == (1, DEFAULT_T)
        r.set_adaptive(1, 40)  # off stays allowed
        r.set_supersampling(1)
        # the band entry points and frm_reload of an adaptive context
        r.set_adaptive(2)
        r.update_parameters_buffer(params_for(18, 4, frm.POWER8_TIME, 32, 32))
        buf = torch.empty(2 * 32 * 32 * 4, dtype=torch.uint8, device="cuda")
        out = torch.empty(32 * 32 * 4, dtype=torch.uint8, device="cuda")
        raises_code(UNS, r.render_bands, buf.data_ptr(), buf.numel(), 16, 0, 1)
        raises_code(UNS, r.render_bands_batch, [params_for(18, 4, frm.POWER8_TIME, 32, 32)] * 2, buf.data_ptr(),
                    dst_bytes=buf.numel(), frame_stride=32 * 32 * 4, band_rows=32, first_band=0, band_stride=1)
        raises_code(UNS, r.unshuffle_bands, buf.data_ptr(), 32 * 32 * 4, out.data_ptr(), out.numel(), 16, 1)
        raises_code(UNS, r.reload, str(tmp_path))
        raises_code(_lib.FRM_ERR_NOT_READY, r.refine_mask)  # no adaptive frame yet
        r.reload(None)  # the built-in kernels: nothing to refuse
        r.set_adaptive(1)
        r.render_bands(buf.data_ptr(), buf.numel(), 16, 0, 1)  # and plainly again
        r.synchronize()
    with frm.Renderer(max_steps=64) as r:
        # frm_refine: a 4 x 4 frame needs 64 source and 64 destination bytes
        src = torch.zeros(64 + 16, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(64 + 16, dtype=torch.uint8, device="cuda")
        s, d = src.data_ptr(), dst.data_ptr()
        p = params_for(3, 1, frm.POWER8_TIME, 4, 4)
        raises_code(_lib.FRM_ERR_NOT_READY, r.refine, s, 64, 4, 4, 2, 16, d, 64)  # NULL params, none set
        raises_code(_lib.FRM_ERR_BUFFER_TOO_SMALL, r.refine, s, 64, 4, 4, 2, 16, d, 63, params=p)
        raises_code(_lib.FRM_ERR_BUFFER_TOO_SMALL, r.refine, s, 63, 4, 4, 2, 16, d, 64, params=p)
        raises_code(INV, r.refine, s + 1, 64, 4, 4, 2, 16, d, 64, params=p)
        raises_code(INV, r.refine, s, 64, 4, 4, 2, 16, d + 1, 64, params=p)
        raises_code(INV, r.refine, s, 64, 4, 4, 0, 16, d, 64, params=p)
        raises_code(INV, r.refine, s, 64, 4, 4, 5, 16, d, 64, params=p)
        raises_code(INV, r.refine, s, 64, 4, 4, 2, 257, d, 64, params=p)
        raises_code(INV, r.refine, s, 64, 0, 4, 2, 16, d, 64, params=p)
        raises_code(INV, r.refine, s, 64, 4, 4, 2, 16, s + 16, 64, params=p)  # overlap
        raises_code(INV, r.refine, 0, 64, 4, 4, 2, 16, d, 64, params=p)
        raises_code(INV, r.refine, s, 64, 4, 4, 2, 16, 0, 64, params=p)
        raises_code(INV, r.refine, s, 64, 4, 4, 2, 16, d, 64, params=p, dev_counters=d + 4)  # misaligned words
        r.refine(s, 64, 4, 4, 2, 16, d, 64, params=p)  # and the valid call
        r.synchronize()
        assert dst[:64].cpu().numpy().reshape(4, 4, 4)[..., 3].min() == 255


# ---- 6. hardware math (consistency only) -----------------------------------------------------------

@pytest.mark.parametrize("S", [2, 3, 4])
def test_hw_math_threshold_zero_equals_the_supersampled_frame(frm_lib, S):
    """FRM_FLAG_HW_MATH has no oracle: this compares two paths of the code under test with each
    other (every pixel refined by refine_samples against frm_set_supersampling's render + resolve),
    not either of them with a reference."""
    p = params_for(18, 6, frm.POWER8_TIME, W, H)
    frames = []
    for kw in ({"adaptive": (S, 0)}, {"supersampling": S}):
        with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_HW_MATH, **kw) as r:
            r.resize(W, H)
            r.update_parameters_buffer(p)
            st = r.render(stats=True)
            frames.append((r.read_frame(), counters_of(st)))
    (a, ca), (b, cb) = frames
    assert np.array_equal(a, b)
    assert ca[0] == cb[0] + W * H and ca[1] > cb[1]  # the plain frame's work on top
