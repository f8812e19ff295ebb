"""The presentation blit on the GPU (include/frm.h frm_blit, frm_present, frm_present_async): blit_kernel
on caller-owned texels equals the oracle's om_blit byte for byte on every case x source x flags of
tests/blit_cases.py, from a 16-byte and from a 4-byte aligned source; it keeps the float64 rules of
tests/blit_cases.py directly, so an error the kernel and the oracle shared would still show;
frm_present and frm_present_async are frm_blit of frm_read_frame's bytes; and frm_blit's error codes."""
import numpy as np
import pytest

import blit_cases as bc
import frm
from frm import _lib
from frm.parameters import Camera
from helpers import params_for

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes after the destination that the kernel must leave alone
STEPS = 128


@pytest.fixture(scope="module")
def renderer(gpu_renderer_factory):
    with gpu_renderer_factory(max_steps=STEPS) as r:
        yield r


def gpu_blit(r, src, dw, dh, flags, offset=False):
    """frm_blit of src [sh, sw, 4] from a torch device tensor onto dw x dh; offset: the source starts
    4 bytes into its allocation (only 4-byte aligned)."""
    import torch
    sh, sw = src.shape[:2]
    flat = torch.from_numpy(np.ascontiguousarray(src).reshape(-1).copy())
    buf = torch.zeros(flat.numel() + 4, dtype=torch.uint8, device="cuda")
    s = buf[4:] if offset else buf[:flat.numel()]
    s.copy_(flat)
    assert s.data_ptr() % 16 == (4 if offset else 0)
    n = dw * dh * 4
    dst = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.blit(s.data_ptr(), s.numel(), sw, sh, dst.data_ptr(), n, dw, dh, srgb=bool(flags & 1), bgra=bool(flags & 2))
    r.synchronize()
    out = dst.cpu().numpy()
    assert (out[n:] == 0xA5).all(), "the kernel wrote past its output"
    return out[:n].reshape(dh, dw, 4)


@pytest.fixture(scope="module")
def blits(renderer):
    """(case, source, flags) -> the kernel's output from an aligned source, each computed once."""
    cache = {}

    def get(case_id, name, flags):
        key = (case_id, name, flags)
        if key not in cache:
            c = bc.CASES[case_id]
            out = gpu_blit(renderer, bc.source(name, c.sw, c.sh), c.dw, c.dh, flags)
            out.setflags(write=False)
            cache[key] = out
        return cache[key]

    return get


# ---- 1. the kernel on raw texels -------------------------------------------------------------------

@pytest.mark.parametrize("case_id", list(bc.CASES))
def test_blit_equals_the_oracle(blits, oracle, case_id):
    c = bc.CASES[case_id]
    for name in bc.SOURCES:
        src = bc.source(name, c.sw, c.sh)
        for flags in bc.FLAGS:
            got = blits(case_id, name, flags)
            want = oracle.blit(src, c.dw, c.dh, flags)
            bad = np.argwhere((got != want).any(axis=-1))
            assert not len(bad), (name, flags, len(bad), bad[:4].tolist())
            if case_id == "same-64x48" and flags & 1:  # same size on an sRGB surface: the source itself
                order = [2, 1, 0] if flags & 2 else [0, 1, 2]
                assert np.array_equal(got[..., :3], src[..., order]) and (got[..., 3] == 255).all()


@pytest.mark.parametrize("case_id", list(bc.CASES))
def test_blit_from_a_source_four_bytes_into_its_allocation(renderer, blits, case_id):
    c = bc.CASES[case_id]
    for name in bc.SOURCES:
        for flags in bc.FLAGS:
            got = gpu_blit(renderer, bc.source(name, c.sw, c.sh), c.dw, c.dh, flags, offset=True)
            assert np.array_equal(got, blits(case_id, name, flags)), (name, flags)


@pytest.mark.parametrize("case_id", list(bc.CASES))
def test_blit_keeps_the_f64_rules(blits, case_id):
    c = bc.CASES[case_id]
    for name in bc.SOURCES:
        for flags in bc.FLAGS:
            e = bc.expectation(case_id, name, flags)
            assert e.span <= 1
            if not c.tie:
                assert e.share <= bc.cap(case_id, flags), (name, flags, e.share)
            got = blits(case_id, name, flags)
            bad = bc.violations(got, e)
            assert not len(bad), (name, flags, bc.describe(got, e, bad))
            decided = ~e.open
            assert np.array_equal(got[decided], e.image[decided]), (name, flags)


# ---- 2. frm_present is frm_blit of frm_read_frame ----------------------------------------------------

W, H = 160, 90


def frame_params(name):
    if name == "mandelbulb":  # mostly background
        return params_for(18, 6, frm.POWER8_TIME, W, H)
    p = params_for(0, 3, 0.0, W, H)  # the Menger sponge from just outside a face: it fills the view
    p.update_camera(Camera((0.0, 0.0, -0.56), 0.0, 0.0))
    return p


@pytest.mark.parametrize("S", [1, 2], ids=["plain", "supersampling2"])
@pytest.mark.parametrize("name", ["mandelbulb", "menger"])
def test_present_is_blit_of_the_read_back_frame(frm_lib, oracle, name, S):
    with frm.Renderer(max_steps=STEPS, supersampling=S) as r:
        r.resize(W, H)
        r.update_parameters_buffer(frame_params(name))
        r.render(stats=False)
        frame = r.read_frame()
        assert frame.shape == (H, W, 4)
        if name == "menger":
            colours, counts = np.unique(frame.reshape(-1, 4), axis=0, return_counts=True)
            assert counts.max() < 0.1 * W * H and len(colours) > 1000
        for ow, oh in ((97, 61), (320, 45)):  # minified; x magnified and y minified
            for flags in bc.FLAGS:
                srgb, bgra = bool(flags & 1), bool(flags & 2)
                want = gpu_blit(r, frame, ow, oh, flags)
                assert np.array_equal(r.present(ow, oh, srgb=srgb, bgra=bgra), want), (ow, oh, flags)
                t = r.present_async(ow, oh, srgb=srgb, bgra=bgra)
                assert np.array_equal(r.frame_pixels(t), want), (ow, oh, flags)
                assert np.array_equal(want, oracle.blit(frame, ow, oh, flags)), (ow, oh, flags)


# ---- 3. errors ---------------------------------------------------------------------------------------

def test_blit_error_codes(renderer):
    import torch
    r = renderer
    BAD, SMALL = _lib.FRM_ERR_INVALID_ARGUMENT, _lib.FRM_ERR_BUFFER_TOO_SMALL
    # a 4 x 4 source onto 8 x 2 pixels: 64 bytes each
    src = torch.zeros(64 + 64 + 16, dtype=torch.uint8, device="cuda")
    dst = torch.full((64 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s, d = src.data_ptr(), dst.data_ptr()
    big = 32768 + 1  # FRM_MAX_DIMENSION + 1

    def code(sp, sb, sw, sh, dp, db, ow, oh, flags=1):
        return r._lib.frm_blit(r.ctx, sp, sb, sw, sh, dp, db, ow, oh, flags, None)

    assert code(None, 64, 4, 4, d, 64, 8, 2) == BAD
    assert code(s, 64, 4, 4, None, 64, 8, 2) == BAD
    assert code(s, 64, 0, 4, d, 64, 8, 2) == BAD
    assert code(s, 64, 4, 0, d, 64, 8, 2) == BAD
    assert code(s, 1 << 40, big, 1, d, 64, 8, 2) == BAD
    assert code(s, 1 << 40, 1, big, d, 64, 8, 2) == BAD
    assert code(s, 64, 4, 4, d, 64, 0, 2) == BAD
    assert code(s, 64, 4, 4, d, 64, 8, 0) == BAD
    assert code(s, 64, 4, 4, d, 1 << 40, big, 1) == BAD
    assert code(s, 64, 4, 4, d, 1 << 40, 1, big) == BAD
    assert code(s, 64, 4, 4, d, 64, 8, 2, flags=4) == BAD
    assert b"flags" in r._lib.frm_last_error(r.ctx)
    assert code(s + 1, 64, 4, 4, d, 64, 8, 2) == BAD
    assert code(s, 64, 4, 4, d + 2, 64, 8, 2) == BAD
    assert code(s, 63, 4, 4, d, 64, 8, 2) == SMALL
    assert code(s, 64, 4, 4, d, 63, 8, 2) == SMALL
    assert code(s, 64, 4, 4, s + 60, 64, 8, 2) == BAD  # the output starts inside the source
    assert code(s + 60, 64, 4, 4, s, 64, 8, 2) == BAD  # the source starts inside the output
    r.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()  # no refused call wrote anything
    assert code(s, 64, 4, 4, s + 64, 64, 8, 2) == _lib.FRM_OK  # adjacent, not overlapping
    assert code(s, 64, 4, 4, d, 64, 8, 2) == _lib.FRM_OK
    r.synchronize()
    out = dst.cpu().numpy()
    assert (out[:64].reshape(2, 8, 4) == np.array([0, 0, 0, 255], np.uint8)).all() and (out[64:] == 0xA5).all()
    with pytest.raises(frm.FrmError) as e:
        r.blit(s, 63, 4, 4, d, 64, 8, 2)
    assert e.value.code == SMALL


def test_blit_on_a_caller_stream_and_a_group_context(frm_lib, blits):
    """Asynchronous on the caller's stream, and on a group context (its devices[0])."""
    import torch
    c = bc.CASES["mag-7x5-33x65"]
    src = torch.from_numpy(np.ascontiguousarray(bc.source("random", c.sw, c.sh)).reshape(-1).copy()).cuda()
    n = c.dw * c.dh * 4
    with frm.Renderer(max_steps=STEPS, devices=[0, 0]) as r:
        stream = torch.cuda.Stream()
        dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r.blit(src.data_ptr(), src.numel(), c.sw, c.sh, dst.data_ptr(), n, c.dw, c.dh, srgb=True,
               stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(dst.cpu().numpy().reshape(c.dh, c.dw, 4), blits("mag-7x5-33x65", "random", 1))
        dst.zero_()
        torch.cuda.synchronize()
        r.blit(src.data_ptr(), src.numel(), c.sw, c.sh, dst.data_ptr(), n, c.dw, c.dh, srgb=False, bgra=True)
        r.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy().reshape(c.dh, c.dw, 4), blits("mag-7x5-33x65", "random", 2))
