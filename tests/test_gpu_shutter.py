"""Motion blur on the GPU (include/frm.h frm_render_shutter, frm_accumulate): the accumulation
kernel on raw texels and on the summation-order fixture, chunks carried through the f32
accumulator, blurred frames and their work counters against the oracle's renders of every sub-frame
combined by tests/shutter_reference.py, the presentation paths, frames in flight, and the error
codes. Everything is bit-exact."""
import os

import numpy as np
import pytest

import frm
import shutter_reference as ref
from frm import _lib
from helpers import params_for

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shutter_order_cases.npz")
COUNTERS = ("pixels", "hit_pixels", "primary_steps", "shadow_steps", "normal_evals", "fractal_bodies",
            "fractal_bailouts")
W, H, STEPS = 33, 17, 128
# scene, num_iterations (pose P1): the Mandelbulb's sub-frames differ in power and share a launch on
# the persistent kernel, so do the Menger's; the animated Menger's cross size follows the time, so
# each of its sub-frames gets a launch of its own
SCENES = {"mandelbulb": (18, 6), "menger": (3, 3), "menger-animated": (4, 3)}
DT, SHUTTER, ORBIT, TIME_FACTOR = 0.2, 1.0, 2.0, 4.0  # a wide shutter: the sub-frames differ visibly
PAD = {"packed": 0, "plus4": 0, "padded": 48, "padded4": 4}  # bytes between two frames
LAYOUTS = list(PAD)  # plus4: the source starts 4 bytes into its allocation (only 4-byte aligned);
# padded: a stride that keeps every frame 16-byte aligned; padded4: one that does not


@pytest.fixture(scope="module")
def renderer(gpu_renderer_factory):
    with gpu_renderer_factory(max_steps=STEPS) as r:
        yield r


def sub_frames(name, T, w=W, h=H):
    """T sub-frames of an orbiting camera (yaw locked inwards) and advancing time from pose P1."""
    scene, iters = SCENES[name]
    p = params_for(scene, iters, frm.POWER8_TIME, w, h)
    cam = frm.Camera(*frm.POSES["P1"])
    cam.raw.orbit_angle_per_second = ORBIT
    cam.raw.lock_yaw_mode = 1
    timing = frm.Timing()
    timing.raw.time_factor = TIME_FACTOR
    subs = frm.shutter_parameters(p, cam, timing, 0, DT, T, SHUTTER)
    assert len(subs) == T and subs[0].to_bytes() == p.to_bytes()
    return subs


@pytest.fixture(scope="module")
def shutter_refs(oracle):
    """(scene name, S, T, w, h) -> (sub-frame Parameters, the oracle's sub-frames, the blurred frame,
    the summed counters): each oracle render done once."""
    cache = {}

    def get(name, S, T, w=W, h=H):
        key = (name, S, T, w, h)
        if key not in cache:
            subs = sub_frames(name, T, w, h)
            rs = [oracle.render(p, S * w, S * h, STEPS) for p in subs]
            frames = np.stack([r["rgba"] for r in rs])
            frames.setflags(write=False)
            img = ref.accumulate(frames, S, oracle)
            img.setflags(write=False)
            counters = [sum(int(r["counters"][c]) for r in rs) for c in range(7)]
            cache[key] = (subs, frames, img, counters)
        return cache[key]

    return get


def gpu_accumulate(r, frames, S, layout="packed", acc=None, divisor=None, dst=True):
    """frm_accumulate of frames [T, S*h, S*w, 4] from a torch device tensor laid out as `layout`.
    acc: None, or a float32 torch tensor [h*w*4] on the device (read and updated in place); returns
    the frame [h, w, 4] (dst=True) or None."""
    import torch
    T, h, w = len(frames), frames.shape[1] // S, frames.shape[2] // S
    fb = frames[0].size
    lead, stride = (4 if layout == "plus4" else 0), fb + PAD[layout]
    host = np.full(lead + T * stride + 16, 171, np.uint8)  # the padding holds no zeros
    for k in range(T):
        host[lead + k * stride:lead + k * stride + fb] = np.ascontiguousarray(frames[k]).reshape(-1)
    buf = torch.from_numpy(host).cuda()
    src = buf[lead:lead + T * stride - PAD[layout]]  # the last frame needs no padding after it
    assert src.data_ptr() % 16 == lead
    out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda") if dst else None
    torch.cuda.synchronize()
    r.accumulate(src.data_ptr(), src.numel(), stride, T, w, h, S,
                 acc_ptr=0 if acc is None else acc.data_ptr(), acc_bytes=0 if acc is None else acc.numel() * 4,
                 divisor=T * S * S if divisor is None else divisor,
                 dst_ptr=out.data_ptr() if dst else 0, dst_bytes=out.numel() if dst else 0)
    r.synchronize()
    return out.cpu().numpy().reshape(h, w, 4) if dst else None


# ---- 1. the kernel on raw texels ---------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T", [1, 2, 3, 8, 32])
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_accumulate_random_texels(renderer, oracle, S, T, layout):
    for w, h in ((1, 1), (67, 5), (1, 70), (130, 33)):
        rng = np.random.default_rng(100000 * S + 1000 * T + 10 * w + h)
        frames = rng.integers(0, 256, size=(T, S * h, S * w, 4), dtype=np.uint8)  # alpha included: it is ignored
        got = gpu_accumulate(renderer, frames, S, layout)
        assert np.array_equal(got, ref.accumulate(frames, S, oracle)), (w, h)


# ---- 2. the order fixture through the kernel ---------------------------------------------------

@pytest.mark.parametrize("layout", ["packed", "plus4"])
@pytest.mark.parametrize("S,T", ref.SHAPES)
def test_accumulate_order_fixture(renderer, oracle, S, T, layout):
    """One fixture case per output pixel, the block's codes in all three channels: the kernel's sum
    gives the pinned code where a pairwise, float64 or texel-major one would not."""
    cases = np.load(FIXTURE)
    blocks, pinned = cases[f"blocks_{S}_{T}"], cases[f"pinned_{S}_{T}"]
    n = len(blocks)
    frames = np.empty((T, S, S * n, 4), np.uint8)
    frames[..., :3] = blocks.transpose(1, 2, 0, 3).reshape(T, S, S * n)[..., None]
    frames[..., 3] = np.random.default_rng(S + T).integers(0, 256, size=(T, S, S * n), dtype=np.uint8)
    assert np.array_equal(ref.accumulate(frames, S, oracle)[0, :, 0], pinned)  # the tiling itself
    got = gpu_accumulate(renderer, frames, S, layout)
    for c in range(3):
        assert np.array_equal(got[0, :, c], pinned), f"channel {c}"
    assert np.all(got[..., 3] == 255)


# ---- 3. chunking is invisible ------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 2, 3])
def test_chunks_through_the_accumulator(renderer, oracle, S):
    import torch
    T, w, h = 7, 67, 5
    frames = np.random.default_rng(S).integers(0, 256, size=(T, S * h, S * w, 4), dtype=np.uint8)
    want = ref.accumulate(frames, S, oracle)
    sums = ref.accumulate_sum(frames, S, oracle)
    one = gpu_accumulate(renderer, frames, S)
    assert np.array_equal(one, want)
    # 3 + 3 + 1 through a zeroed accumulator, the frame written by the last call only
    acc = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
    assert gpu_accumulate(renderer, frames[0:3], S, acc=acc, dst=False) is None
    assert gpu_accumulate(renderer, frames[3:6], S, acc=acc, dst=False) is None
    chunked = gpu_accumulate(renderer, frames[6:7], S, acc=acc, divisor=T * S * S)
    assert np.array_equal(chunked, one)
    a = acc.cpu().numpy().reshape(h, w, 4)
    assert np.array_equal(a[..., :3].view(np.uint32), sums.view(np.uint32)) and np.all(a[..., 3].view(np.uint32) == 0)
    # the whole sum in one call with both outputs
    acc2 = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
    both = gpu_accumulate(renderer, frames, S, acc=acc2)
    assert np.array_equal(both, one)
    a2 = acc2.cpu().numpy().reshape(h, w, 4)
    assert np.array_equal(a2.view(np.uint32), a.view(np.uint32))


# ---- 4. frames -------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, frm.FRM_FLAG_PERSISTENT_KERNEL], ids=["default-kernel", "persistent"])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("name", list(SCENES))
def test_shutter_frame_and_counters(frm_lib, shutter_refs, name, S, flags):
    subs, frames, want, counters = shutter_refs(name, S, 3)
    assert np.any(frames[0] != frames[2])  # the sub-frames move
    with frm.Renderer(max_steps=STEPS, flags=flags, supersampling=S) as r:
        r.resize(W, H)
        for k in range(2):  # the second frame runs in the scheduled order
            st = r.render_shutter(subs, stats=True)
            assert [st[c] for c in COUNTERS] == counters, f"frame {k}"
            assert st["pixels"] == 3 * S * S * W * H
            assert np.array_equal(r.read_frame(), want), f"frame {k}"


# ---- 5. forced chunks ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mandelbulb", "menger-animated"])
def test_forced_chunks_change_nothing(frm_lib, shutter_refs, monkeypatch, name):
    subs, _, want, counters = shutter_refs(name, 2, 5)
    monkeypatch.setenv("FRM_SHUTTER_CHUNK", "2")  # read by frm_create: chunks of 2 + 2 + 1
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, supersampling=2) as r:
        r.resize(W, H)
        for k in range(2):
            st = r.render_shutter(subs, stats=True)
            assert [st[c] for c in COUNTERS] == counters, f"frame {k}"
            assert np.array_equal(r.read_frame(), want), f"frame {k}"
    monkeypatch.delenv("FRM_SHUTTER_CHUNK")
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, supersampling=2) as r:
        r.resize(W, H)
        st = r.render_shutter(subs, stats=True)  # unchunked
        assert [st[c] for c in COUNTERS] == counters
        assert np.array_equal(r.read_frame(), want)


# ---- 6. one sub-frame, identical sub-frames ----------------------------------------------------------

@pytest.mark.parametrize("S", [1, 2])
def test_one_and_identical_sub_frames_are_the_plain_frame(frm_lib, S):
    p = sub_frames("mandelbulb", 2)[1]
    with frm.Renderer(max_steps=STEPS, supersampling=S) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        plain_stats = r.render(stats=True)
        plain = r.read_frame()
        st = r.render_shutter([p], stats=True)
        assert np.array_equal(r.read_frame(), plain)
        assert [st[c] for c in COUNTERS] == [plain_stats[c] for c in COUNTERS]
        st = r.render_shutter([p] * 4, stats=True)
        assert np.array_equal(r.read_frame(), plain)
        assert [st[c] for c in COUNTERS] == [4 * plain_stats[c] for c in COUNTERS]


# ---- 7. the context around a shutter frame ---------------------------------------------------------

def test_frames_in_flight_keep_their_tickets(frm_lib, oracle, shutter_refs):
    subs, frames, blurred, _ = shutter_refs("mandelbulb", 1, 3)
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, frames_in_flight=2) as r:
        r.resize(W, H)
        held, got, want = [], [], []
        for k in range(6):  # plain and blurred frames alternate, a frame of presentation latency
            if k % 2:
                r.render_shutter(subs, stats=False)
                want.append(blurred)
            else:
                r.update_parameters_buffer(subs[k // 2])
                r.render(stats=False)
                want.append(frames[k // 2])
            held.append(r.read_frame_async())
            if len(held) > 1:
                got.append(r.frame_pixels(held.pop(0)))
        got += [r.frame_pixels(t) for t in held]
    assert len(got) == 6
    for k in range(6):
        assert np.array_equal(got[k], want[k]), f"frame {k}"


def test_presentation_resize_and_a_plain_frame_afterwards(frm_lib, oracle, shutter_refs):
    subs, frames, want, _ = shutter_refs("mandelbulb", 2, 3)
    with frm.Renderer(max_steps=STEPS, supersampling=2) as r:
        r.resize(W, H)
        r.render_shutter(subs, stats=False)
        assert np.array_equal(r.read_frame(), want)
        for ow, oh, srgb, bgra, flags in ((50, 30, True, False, 1), (20, 10, False, True, 2)):
            got = r.present(ow, oh, srgb=srgb, bgra=bgra)
            assert np.array_equal(got, oracle.blit(want, ow, oh, flags)), (ow, oh, flags)
            assert np.array_equal(r.frame_pixels(r.present_async(ow, oh, srgb=srgb, bgra=bgra)), got)
        assert np.array_equal(r.frame_pixels(r.read_frame_async()), want)
        # another size between two shutter frames, no drain
        w2, h2 = 21, 12
        subs2, _, want2, counters2 = shutter_refs("mandelbulb", 2, 3, w2, h2)
        r.resize(w2, h2)
        st = r.render_shutter(subs2, stats=True)
        assert [st[c] for c in COUNTERS] == counters2
        assert np.array_equal(r.read_frame(), want2)
        r.resize(W, H)
        r.render_shutter(subs, stats=False)
        assert np.array_equal(r.read_frame(), want)
        # the context's parameters are the last sub-frame's; a plain render gives its plain bytes
        r.render(stats=False)
        last = ref.accumulate(frames[2:3], 2, oracle)
        assert np.array_equal(r.read_frame(), last)
        r.update_parameters_buffer(subs[0])
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), ref.accumulate(frames[0:1], 2, oracle))


# ---- 8. errors -------------------------------------------------------------------------------------

def raises_code(code, fn, *args, **kw):
    with pytest.raises(frm.FrmError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


def test_render_shutter_errors(frm_lib, shutter_refs):
    subs = sub_frames("mandelbulb", 3)
    want = shutter_refs("mandelbulb", 1, 3)[2]
    with frm.Renderer(max_steps=STEPS, devices=[0, 0]) as g:  # a group: one device listed twice
        g.resize(W, H)
        raises_code(_lib.FRM_ERR_UNSUPPORTED, g.render_shutter, subs)
    with frm.Renderer(max_steps=STEPS, adaptive=2) as a:
        a.resize(W, H)
        raises_code(_lib.FRM_ERR_UNSUPPORTED, a.render_shutter, subs)
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL) as r:
        raises_code(_lib.FRM_ERR_NOT_READY, r.render_shutter, subs)  # before resize
        r.resize(W, H)
        r.render_shutter(subs, stats=False)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.render_shutter, [])
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.render_shutter, [subs[0]] * 33)
        other_scene = frm.Parameters.from_bytes(subs[1].to_bytes())
        other_scene.scene_index = 3
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.render_shutter, [subs[0], other_scene])
        other_iters = frm.Parameters.from_bytes(subs[1].to_bytes())
        other_iters.num_iterations = 7
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.render_shutter, [subs[0], other_iters])
        other_aspect = frm.Parameters.from_bytes(subs[1].to_bytes())
        other_aspect.update_aspect(H, W)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.render_shutter, [subs[0], other_aspect])
        endless = frm.Parameters.from_bytes(subs[1].to_bytes())
        endless.num_iterations = 0xFFFFFFFF
        raises_code(_lib.FRM_ERR_UNSUPPORTED, r.render_shutter, [endless, endless])
        # the refusals changed nothing: the blurred frame is still shown, and not traceable
        assert np.array_equal(r.read_frame(), want)
        raises_code(_lib.FRM_ERR_NOT_READY, r.trace)
        r.render(stats=False)  # a plain persistent frame is
        assert r.trace().shape == (H, W, 10)


def test_accumulate_errors(frm_lib):
    import torch
    with frm.Renderer(max_steps=64) as r:
        # two 4 x 4 outputs at factor 2: 256 source bytes per frame, 256 of sums, 64 of frame
        src = torch.zeros(2 * 256 + 16, dtype=torch.uint8, device="cuda")
        acc = torch.zeros(64 + 4, dtype=torch.float32, device="cuda")
        dst = torch.zeros(64 + 16, dtype=torch.uint8, device="cuda")
        s, a, d = src.data_ptr(), acc.data_ptr(), dst.data_ptr()

        def call(src_ptr=s, src_bytes=512, stride=256, count=2, w=4, h=4, factor=2, acc_ptr=a, acc_bytes=256,
                 divisor=8, dst_ptr=d, dst_bytes=64):
            r.accumulate(src_ptr, src_bytes, stride, count, w, h, factor, acc_ptr=acc_ptr, acc_bytes=acc_bytes,
                         divisor=divisor, dst_ptr=dst_ptr, dst_bytes=dst_bytes)

        bad, small = _lib.FRM_ERR_INVALID_ARGUMENT, _lib.FRM_ERR_BUFFER_TOO_SMALL
        raises_code(bad, call, acc_ptr=0, dst_ptr=0)  # both outputs NULL
        raises_code(bad, call, src_ptr=0)
        raises_code(bad, call, acc_ptr=a + 4)  # 16-byte alignment of the sums
        raises_code(bad, call, src_ptr=s + 2)
        raises_code(bad, call, dst_ptr=d + 1)
        raises_code(bad, call, stride=258)
        raises_code(bad, call, stride=252)  # below a frame's bytes
        raises_code(bad, call, count=0)
        raises_code(bad, call, count=33, src_bytes=33 * 256)
        raises_code(bad, call, factor=0)
        raises_code(bad, call, factor=5)
        raises_code(bad, call, w=0)
        raises_code(bad, call, h=40000)
        raises_code(bad, call, divisor=0)
        raises_code(bad, call, dst_ptr=s + 256)  # overlaps the source
        raises_code(bad, call, acc_ptr=s + 256)
        raises_code(small, call, src_bytes=511)
        raises_code(small, call, acc_bytes=255)
        raises_code(small, call, dst_bytes=63)
        call()  # and the valid calls
        call(acc_ptr=0, acc_bytes=0)
        call(dst_ptr=0, dst_bytes=0, divisor=0)
        r.synchronize()
        assert dst[:64].cpu().numpy().reshape(4, 4, 4)[..., 3].min() == 255
        assert torch.count_nonzero(acc).item() == 0  # sums of code 0 texels
