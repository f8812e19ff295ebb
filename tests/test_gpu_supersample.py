"""Supersampled anti-aliasing on the GPU (include/frm.h frm_set_supersampling, frm_resolve): the
resolve kernel on raw texels and on the summation-order fixture, supersampled frames and their work
counters against the oracle's render of the internal frame resolved by tests/ssaa_reference.py, the
presentation paths, frames in flight (single device and a three-rank group) across factor changes,
and the error codes. Everything is bit-exact."""
import ctypes
import os

import numpy as np
import pytest

import frm
import ssaa_reference as ref
from frm import _lib
from helpers import params_for

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssaa_order_cases.npz")
COUNTERS = ("pixels", "hit_pixels", "primary_steps", "shadow_steps", "normal_evals", "fractal_bodies",
            "fractal_bailouts")
W, H, STEPS = 33, 17, 128
SCENES = {"mandelbulb": (18, 6), "menger": (3, 3)}  # scene, num_iterations (pose P1)


@pytest.fixture(scope="module")
def renderer(gpu_renderer_factory):
    with gpu_renderer_factory(max_steps=STEPS) as r:
        yield r


@pytest.fixture(scope="module")
def frame_refs(oracle):
    """(scene name, S) -> (Parameters, resolved frame, counters): each oracle render done once."""
    cache = {}

    def get(name, S):
        if (name, S) not in cache:
            scene, iters = SCENES[name]
            p = params_for(scene, iters, frm.POWER8_TIME, W, H)
            r = oracle.render(p, S * W, S * H, STEPS)
            img = ref.box_resolve(r["rgba"], S, oracle)
            img.setflags(write=False)
            cache[(name, S)] = (p, img, [int(c) for c in r["counters"][:7]])
        return cache[(name, S)]

    return get


def gpu_resolve(r, hi, S, offset=False):
    """frm_resolve of hi [S*h, S*w, 4] from a torch device tensor; offset: the source starts 4 bytes
    into its allocation (only 4-byte aligned)."""
    import torch
    h, w = hi.shape[0] // S, hi.shape[1] // S
    flat = torch.from_numpy(np.ascontiguousarray(hi).reshape(-1))
    buf = torch.zeros(flat.numel() + 4, dtype=torch.uint8, device="cuda")
    src = buf[4:] if offset else buf[:flat.numel()]
    src.copy_(flat)
    assert src.data_ptr() % 16 == (4 if offset else 0)
    dst = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.resolve(src.data_ptr(), src.numel(), w, h, S, dst.data_ptr(), dst.numel())
    r.synchronize()
    return dst.cpu().numpy().reshape(h, w, 4)


# ---- 1. the kernel on raw texels ---------------------------------------------------------------

@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "plus4"])
@pytest.mark.parametrize("w,h", [(1, 1), (67, 5), (1, 70), (130, 33)])
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_resolve_random_texels(renderer, oracle, S, w, h, offset):
    rng = np.random.default_rng(1000 * S + 10 * w + h)
    hi = rng.integers(0, 256, size=(S * h, S * w, 4), dtype=np.uint8)  # alpha included: it is ignored
    got = gpu_resolve(renderer, hi, S, offset)
    assert np.array_equal(got, ref.box_resolve(hi, S, oracle))


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "plus4"])
@pytest.mark.parametrize("S", ref.FACTORS)
def test_resolve_order_fixture(renderer, oracle, S, offset):
    """One fixture case per output pixel, the block's codes in all three channels: the kernel's sum
    gives the pinned code where a pairwise, column-major, float64, reciprocal or pre-scaled one would not."""
    cases = np.load(FIXTURE)
    blocks, pinned = cases[f"blocks_{S}"], cases[f"pinned_{S}"]
    n = len(blocks)
    hi = np.empty((S, S * n, 4), np.uint8)
    hi[..., :3] = blocks.transpose(1, 0, 2).reshape(S, S * n)[..., None]
    hi[..., 3] = np.random.default_rng(S).integers(0, 256, size=(S, S * n), dtype=np.uint8)
    assert np.array_equal(ref.box_resolve(hi, S, oracle)[0, :, 0], pinned)  # the tiling itself
    got = gpu_resolve(renderer, hi, S, offset)
    for c in range(3):
        assert np.array_equal(got[0, :, c], pinned), f"channel {c}"
    assert np.all(got[..., 3] == 255)


# ---- 2. frames ---------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, frm.FRM_FLAG_PERSISTENT_KERNEL], ids=["default-kernel", "persistent"])
@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(SCENES))
def test_supersampled_frame_and_counters(frm_lib, frame_refs, name, S, flags):
    p, want, counters = frame_refs(name, S)
    with frm.Renderer(max_steps=STEPS, flags=flags, supersampling=S) as r:
        assert r.supersampling == S
        r.resize(W, H)
        assert (r.width, r.height, r.render_width, r.render_height) == (W, H, S * W, S * H)
        r.update_parameters_buffer(p)
        for k in range(2):  # the second frame runs in the scheduled order
            st = r.render(stats=True)
            assert [st[c] for c in COUNTERS] == counters, f"frame {k}"
            assert st["pixels"] == S * S * W * H
            assert np.array_equal(r.read_frame(), want), f"frame {k}"


def test_factor_one_is_the_plain_frame(frm_lib, oracle, frame_refs):
    p, want, _ = frame_refs("mandelbulb", 1)
    assert np.array_equal(want, oracle.render(p, W, H, STEPS)["rgba"])
    with frm.Renderer(max_steps=STEPS) as r:
        r.set_supersampling(1)
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), want)


# ---- 3. presentation -----------------------------------------------------------------------------

def test_presentation_reads_the_resolved_frame(frm_lib, oracle, frame_refs):
    p, want, _ = frame_refs("mandelbulb", 2)
    with frm.Renderer(max_steps=STEPS, supersampling=2) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
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


def loop_params():
    return [params_for((18, 0, 15)[k % 3], 6, frm.POWER8_TIME + 0.3 * k, LW, LH, pose=("P0", "P1", "P2")[k % 3])
            for k in range(6)]


@pytest.fixture(scope="module")
def loop_refs(oracle):
    """(frame k, S) -> the resolved oracle frame of the moving loop, rendered once."""
    cache = {}
    frames = loop_params()

    def get(k, S):
        if (k, S) not in cache:
            img = ref.box_resolve(oracle.render(frames[k], S * LW, S * LH, LSTEPS)["rgba"], S, oracle)
            img.setflags(write=False)
            cache[(k, S)] = img
        return cache[(k, S)]

    return get


def run_loop(r, fif, factors):
    """The drop-in loop with a frame of presentation latency; factors[k] is frame k's factor."""
    frames = loop_params()
    held, got = [], []
    for k, p in enumerate(frames):
        if r.supersampling != factors[k]:
            r.set_supersampling(factors[k])  # tickets issued before keep their frames
        r.update_parameters_buffer(p)
        r.render(stats=False)
        held.append(r.read_frame_async())
        if len(held) > fif - 1:
            got.append(r.frame_pixels(held.pop(0)))
    got += [r.frame_pixels(t) for t in held]
    return got


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one-device", "group3"])
@pytest.mark.parametrize("fif", [1, 2, 3])
def test_moving_loop_with_latency(frm_lib, loop_refs, fif, devices):
    with frm.Renderer(max_steps=LSTEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, frames_in_flight=fif,
                      devices=devices, supersampling=2) as r:
        r.resize(LW, LH)
        got = run_loop(r, fif, [2] * 6)
    for k, g in enumerate(got):
        assert g.shape == (LH, LW, 4)
        assert np.array_equal(g, loop_refs(k, 2)), f"frame {k}"


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one-device", "group3"])
def test_factor_changes_mid_loop(frm_lib, loop_refs, devices):
    factors = [2, 2, 3, 3, 1, 1]
    with frm.Renderer(max_steps=LSTEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, frames_in_flight=3,
                      devices=devices, supersampling=2) as r:
        r.resize(LW, LH)
        got = run_loop(r, 3, factors)
        assert r.supersampling == 1 and (r.render_width, r.render_height) == (LW, LH)
    for k, g in enumerate(got):
        assert g.shape == (LH, LW, 4)
        assert np.array_equal(g, loop_refs(k, factors[k])), f"frame {k} (factor {factors[k]})"


def test_async_readback_refuses_after_a_factor_change(frm_lib, frame_refs):
    p, want, _ = frame_refs("mandelbulb", 2)
    with frm.Renderer(max_steps=STEPS, frames_in_flight=2, supersampling=2) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        t = r.read_frame_async()
        r.set_supersampling(3)  # as frm_resize: no frame of the new internal size yet
        with pytest.raises(frm.FrmError) as e:
            r.read_frame_async()
        assert e.value.code == _lib.FRM_ERR_NOT_READY
        assert np.array_equal(r.frame_pixels(t), want)  # the ticket keeps its frame
        r.render(stats=False)
        assert np.array_equal(r.frame_pixels(r.read_frame_async()), frame_refs("mandelbulb", 3)[1])


# ---- 5. errors -------------------------------------------------------------------------------------

def current_factor(r):
    out = ctypes.c_uint32()
    assert r._lib.frm_get_supersampling(r.ctx, ctypes.byref(out)) == _lib.FRM_OK
    return out.value


def raises_code(code, fn, *args, **kw):
    with pytest.raises(frm.FrmError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


def test_supersampling_errors(frm_lib):
    import torch
    with frm.Renderer(max_steps=64) as r:
        assert current_factor(r) == 1
        r.set_supersampling(2)
        for bad in (0, 5):
            raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.set_supersampling, bad)
            assert current_factor(r) == 2 and r.supersampling == 2
        # 2 x 20000 exceeds FRM_MAX_DIMENSION: the size is refused, then set with factor 1
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.resize, 20000, 8)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.resize, 8, 20000)
        r.set_supersampling(1)
        r.resize(10000, 8)
        r.set_supersampling(3)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.set_supersampling, 4)  # 40000 texels wide
        assert current_factor(r) == 3 and r.supersampling == 3
        # the band entry points of a supersampled context
        r.resize(32, 32)
        r.update_parameters_buffer(params_for(18, 4, frm.POWER8_TIME, 32, 32))
        buf = torch.empty(96 * 96 * 4, dtype=torch.uint8, device="cuda")
        raises_code(_lib.FRM_ERR_UNSUPPORTED, r.render_bands, buf.data_ptr(), buf.numel(), 16, 0, 1)
        r.set_supersampling(1)
        # frm_resolve: a 4 x 4 output at factor 2 needs 256 source and 64 destination bytes
        src = torch.zeros(256 + 16, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(64 + 16, dtype=torch.uint8, device="cuda")
        s, d = src.data_ptr(), dst.data_ptr()
        raises_code(_lib.FRM_ERR_BUFFER_TOO_SMALL, r.resolve, s, 256, 4, 4, 2, d, 63)
        raises_code(_lib.FRM_ERR_BUFFER_TOO_SMALL, r.resolve, s, 255, 4, 4, 2, d, 64)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.resolve, s + 1, 256, 4, 4, 2, d, 64)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.resolve, s, 256, 4, 4, 2, d + 1, 64)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.resolve, s, 256, 4, 4, 0, d, 64)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.resolve, s, 256, 4, 4, 5, d, 64)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.resolve, s, 256, 0, 4, 2, d, 64)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.resolve, s, 256, 4, 4, 2, s + 64, 64)  # overlap
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.resolve, 0, 256, 4, 4, 2, d, 64)
        r.resolve(s, 256, 4, 4, 2, d, 64)  # and the valid call
        r.synchronize()
        assert dst[:64].cpu().numpy().reshape(4, 4, 4)[..., 3].min() == 255
