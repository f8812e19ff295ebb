"""Panoramas on the GPU (include/frm.h frm_set_panorama, frm_project_equirect): the projection kernel
on raw texels against tests/panorama_reference.py, and the context mode against the oracle's renders
of the six faces projected by that reference: frames, work counters, the presentation paths, frames
in flight, mode and size changes, and the error codes. Everything is bit-exact."""
import ctypes

import numpy as np
import pytest

import frm
import panorama_reference as ref
from frm import _lib
from helpers import params_for

pytestmark = pytest.mark.gpu

COUNTERS = ("pixels", "hit_pixels", "primary_steps", "shadow_steps", "normal_evals", "fractal_bodies",
            "fractal_bailouts")
N, M, W, H, STEPS = 14, 16, 48, 24, 48
SCENES = {"mandelbulb": (18, 4), "menger": (3, 3)}  # scene, num_iterations
# pose P1 of the workloads looks at the set from outside, so one face sees it; "inside" stands in the
# Menger sponge's central void, and for the Mandelbulb (whose inside is black) in a fold of its
# surface: geometry on nearly every face
CAMERAS = {"P1": None, "inside": {"menger": ((0.1, 0.05, -0.1), 0.7, -0.4), "mandelbulb": ((0.3, 0.9, -0.4), 0.7, -0.4)}}


def parameters(scene_name, camera, w=W, h=H):
    scene, iters = SCENES[scene_name]
    p = params_for(scene, iters, frm.POWER8_TIME, w, h)
    cam = CAMERAS[camera] if isinstance(camera, str) else camera
    if isinstance(cam, dict):
        cam = cam[scene_name]
    if cam is not None:
        p.update_camera(frm.Camera(*cam))
    return p


@pytest.fixture(scope="module")
def pano_refs(oracle, frm_lib):
    """(scene, camera, n, w, h) -> (Parameters, the oracle's six faces, the panorama, the summed counters)."""
    cache = {}

    def get(scene_name, camera, n=N, w=W, h=H):
        key = (scene_name, camera, n, w, h)
        if key not in cache:
            p = parameters(scene_name, camera, w, h)
            rs = [oracle.render(q, n + 2, n + 2, STEPS) for q in ref.face_parameters(p, n)]
            faces = np.stack([r["rgba"] for r in rs])
            pano = ref.project(faces, n, w, h, frm.equirect_tables(w, h), oracle)
            for a in (faces, pano):
                a.setflags(write=False)
            counters = [sum(int(r["counters"][c]) for r in rs) for c in range(7)]
            cache[key] = (p, faces, pano, counters)
        return cache[key]

    return get


@pytest.fixture(scope="module")
def renderer(gpu_renderer_factory):
    with gpu_renderer_factory(max_steps=STEPS) as r:
        yield r


def gpu_project(r, faces, n, w, h, pad=0, stream=0):
    """frm_project_equirect of faces [6, n+2, n+2, 4] from a torch device tensor, `pad` bytes between faces."""
    import torch
    fb = faces[0].size
    stride = fb + pad
    host = np.full(6 * stride + 16, 171, np.uint8)  # the padding holds no zeros
    for f in range(6):
        host[f * stride:f * stride + fb] = np.ascontiguousarray(faces[f]).reshape(-1)
    buf = torch.from_numpy(host).cuda()
    src = buf[:6 * stride - pad]  # the last face needs no padding after it
    out = torch.zeros(h * w * 4 + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.project_equirect(src.data_ptr(), src.numel(), stride, n, out.data_ptr(), h * w * 4, w, h, stream=stream)
    if stream:
        torch.cuda.synchronize()
    r.synchronize()
    got = out.cpu().numpy()
    assert not got[h * w * 4:].any()  # nothing written past the frame
    return got[:h * w * 4].reshape(h, w, 4)


# ---- 1. the kernel on raw texels ---------------------------------------------------------------

@pytest.mark.parametrize("pad", [0, 52], ids=["packed", "padded"])
@pytest.mark.parametrize("n,w,h", ref.SHAPES)
def test_project_random_texels_and_six_colours(renderer, oracle, n, w, h, pad):
    tabs = frm.equirect_tables(w, h)
    m = n + 2
    rng = np.random.default_rng(10000 * n + 10 * w + h)
    faces = rng.integers(0, 256, size=(6, m, m, 4), dtype=np.uint8)  # alpha included: it is ignored
    want = ref.project(faces, n, w, h, tabs, oracle)
    got = gpu_project(renderer, faces, n, w, h, pad)
    assert np.array_equal(got, want)
    six = ref.constant_faces(n, ref.SIX_COLOURS)
    got = gpu_project(renderer, six, n, w, h, pad)
    assert np.array_equal(got, ref.project(six, n, w, h, tabs, oracle))
    face = ref.taps(n, w, h, tabs)[0]
    assert np.array_equal(got[..., :3], np.array(ref.SIX_COLOURS, np.uint8)[face])


def test_project_on_another_stream(renderer, oracle):
    import torch
    n, w, h = 5, 33, 17
    faces = np.random.default_rng(7).integers(0, 256, size=(6, n + 2, n + 2, 4), dtype=np.uint8)
    s = torch.cuda.Stream()
    got = gpu_project(renderer, faces, n, w, h, stream=s.cuda_stream)
    assert np.array_equal(got, ref.project(faces, n, w, h, frm.equirect_tables(w, h), oracle))


def raises_code(code, fn, *args, **kw):
    with pytest.raises(frm.FrmError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


def test_project_errors(frm_lib):
    import torch
    with frm.Renderer(max_steps=64) as r:
        # faces of n = 2: 4 x 4 texels = 64 bytes each; an 8 x 4 panorama = 128 bytes
        src = torch.zeros(6 * 64 + 64, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(128 + 16, dtype=torch.uint8, device="cuda")
        s, d = src.data_ptr(), dst.data_ptr()

        def call(src_ptr=s, src_bytes=384, stride=64, n=2, dst_ptr=d, dst_bytes=128, w=8, h=4):
            r.project_equirect(src_ptr, src_bytes, stride, n, dst_ptr, dst_bytes, w, h)

        bad, small = _lib.FRM_ERR_INVALID_ARGUMENT, _lib.FRM_ERR_BUFFER_TOO_SMALL
        raises_code(bad, call, src_ptr=0)
        raises_code(bad, call, dst_ptr=0)
        raises_code(bad, call, src_ptr=s + 2)
        raises_code(bad, call, dst_ptr=d + 1)
        raises_code(bad, call, stride=66, src_bytes=448)
        raises_code(bad, call, stride=60)  # below a face's bytes
        raises_code(bad, call, n=0)
        raises_code(bad, call, n=32767, src_bytes=1 << 40, stride=1 << 36)  # M above FRM_MAX_DIMENSION
        raises_code(bad, call, w=0)
        raises_code(bad, call, h=0)
        raises_code(bad, call, w=32769)
        raises_code(bad, call, h=40000)
        raises_code(bad, call, dst_ptr=s + 64)  # overlaps the faces
        raises_code(bad, call, src_ptr=d, src_bytes=384, dst_ptr=d + 64)
        raises_code(small, call, src_bytes=383)
        raises_code(small, call, stride=68, src_bytes=5 * 68 + 63)
        raises_code(small, call, dst_bytes=127)
        call()  # and the valid calls
        call(stride=68, src_bytes=5 * 68 + 64)
        r.synchronize()
        assert dst[:128].cpu().numpy().reshape(4, 8, 4)[..., 3].min() == 255
        assert not dst[128:].cpu().numpy().any()


# ---- 2. frames -------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [frm.FRM_FLAG_SIMPLE_KERNEL, frm.FRM_FLAG_PERSISTENT_KERNEL],
                         ids=["simple", "persistent"])
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_panorama_frame_and_counters(frm_lib, pano_refs, scene, camera, flags):
    p, faces, want, counters = pano_refs(scene, camera)
    if camera == "inside":
        assert sum(bool(np.any(faces[f, ..., :3])) for f in range(6)) >= 5  # geometry all round
    with frm.Renderer(max_steps=STEPS, flags=flags, panorama=N) as r:
        assert (r.render_width, r.render_height) == (M, M)
        r.resize(W, H)
        r.update_parameters_buffer(p)
        for k in range(2):  # the second frame runs in the scheduled order; the bytes stay
            st = r.render(stats=True)
            assert [st[c] for c in COUNTERS] == counters, f"frame {k}"
            assert st["pixels"] == 6 * M * M
            got = r.read_frame()
            assert got.shape == (H, W, 4) and np.array_equal(got, want), f"frame {k}"
        raises_code(_lib.FRM_ERR_NOT_READY, r.trace)  # no single frame to trace


def test_the_default_kernel_choice_gives_the_same_bytes(frm_lib, pano_refs):
    p, _, want, counters = pano_refs("mandelbulb", "P1")
    with frm.Renderer(max_steps=STEPS, panorama=N) as r:  # small faces: kernel_for picks the simple kernel
        assert r.kernel_for(M * M) == "simple"
        r.resize(W, H)
        r.update_parameters_buffer(p)
        st = r.render(stats=True)
        assert [st[c] for c in COUNTERS] == counters
        assert np.array_equal(r.read_frame(), want)


def test_frames_in_flight_keep_their_tickets(frm_lib, oracle, pano_refs):
    cams = [((0.1 + 0.05 * k, 0.05, -0.1 - 0.1 * k), 0.7 + 0.2 * k, -0.4 + 0.1 * k) for k in range(3)]
    refs = [pano_refs("menger", cam) for cam in cams]
    assert np.any(refs[0][2] != refs[1][2]) and np.any(refs[1][2] != refs[2][2])  # the camera moves
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, frames_in_flight=2, panorama=N) as r:
        r.resize(W, H)
        held, got = [], []
        for k in range(3):  # a frame of presentation latency
            r.update_parameters_buffer(refs[k][0])
            r.render(stats=False)
            held.append(r.read_frame_async())
            if len(held) > 1:
                got.append(r.frame_pixels(held.pop(0)))
        got += [r.frame_pixels(t) for t in held]
    assert len(got) == 3
    for k in range(3):
        assert np.array_equal(got[k], refs[k][2]), f"frame {k}"


def test_presentation_resize_and_switching_off(frm_lib, oracle, pano_refs):
    p, _, want, _ = pano_refs("mandelbulb", "inside")
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, panorama=N) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), want)
        for ow, oh, srgb, bgra, flags in ((100, 60, True, False, 1), (20, 10, False, True, 2)):
            got = r.present(ow, oh, srgb=srgb, bgra=bgra)
            assert np.array_equal(got, oracle.blit(want, ow, oh, flags)), (ow, oh, flags)
            assert np.array_equal(r.frame_pixels(r.present_async(ow, oh, srgb=srgb, bgra=bgra)), got)
        assert np.array_equal(r.frame_pixels(r.read_frame_async()), want)
        # another output size and another face size between two panoramas, no drain
        w2, h2, n2 = 21, 12, 6
        p2, _, want2, counters2 = pano_refs("mandelbulb", "inside", n2, w2, h2)
        r.resize(w2, h2)
        raises_code(_lib.FRM_ERR_NOT_READY, r.read_frame_async)  # no panorama of this size yet
        r.set_panorama(n2)
        r.update_parameters_buffer(p2)
        st = r.render(stats=True)
        assert [st[c] for c in COUNTERS] == counters2 and st["pixels"] == 6 * (n2 + 2) ** 2
        assert np.array_equal(r.read_frame(), want2)
        r.set_panorama(N)
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), want)
        # off: frm_render's plain frame of the same parameters, as the oracle renders it
        r.set_panorama(0)
        assert (r.render_width, r.render_height) == (W, H)
        raises_code(_lib.FRM_ERR_NOT_READY, r.read_frame_async)
        st = r.render(stats=True)
        plain = oracle.render(p, W, H, STEPS)
        assert np.array_equal(r.read_frame(), plain["rgba"])
        assert [st[c] for c in COUNTERS] == [int(c) for c in plain["counters"][:7]]
        assert r.trace().shape == (H, W, 10)  # a plain persistent frame is traceable again
        # and on again
        r.set_panorama(N)
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), want)


# ---- 3. what a panorama context refuses --------------------------------------------------------

def test_unsupported_pairings_leave_the_state(frm_lib, pano_refs):
    import torch
    unsupported = _lib.FRM_ERR_UNSUPPORTED
    p, _, want, _ = pano_refs("menger", "inside")
    with frm.Renderer(max_steps=STEPS, devices=[0, 0]) as g:  # a group: one device listed twice
        raises_code(unsupported, g.set_panorama, N)
        assert g.panorama == 0
        g.set_panorama(0)  # off stays allowed
    with frm.Renderer(max_steps=STEPS, supersampling=2) as s:
        raises_code(unsupported, s.set_panorama, N)
        s.resize(W, H)
        assert (s.render_width, s.render_height) == (2 * W, 2 * H)
    with frm.Renderer(max_steps=STEPS, adaptive=2) as a:
        raises_code(unsupported, a.set_panorama, N)
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL, panorama=N) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        buf = torch.zeros(6 * M * M * 4, dtype=torch.uint8, device="cuda")
        raises_code(unsupported, r.set_supersampling, 2)
        raises_code(unsupported, r.set_adaptive, 2)
        raises_code(unsupported, r.render_shutter, [p, p])
        raises_code(unsupported, r.render_bands, buf.data_ptr(), buf.numel(), 16, 0, 1)
        raises_code(unsupported, r.render_bands_batch, [p, p], buf.data_ptr(), dst_bytes=buf.numel(),
                    frame_stride=M * M * 4, band_rows=16, first_band=0, band_stride=1)
        raises_code(unsupported, r.unshuffle_bands, buf.data_ptr(), M * M * 4, buf.data_ptr() + M * M * 4, M * M * 4, 16, 1)
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.set_panorama, 32767)  # M above FRM_MAX_DIMENSION
        raises_code(_lib.FRM_ERR_INVALID_ARGUMENT, r.set_panorama, 8000)  # six faces above 1 GiB
        r.set_supersampling(1)  # the neutral settings stay allowed
        r.set_adaptive(1)
        n = ctypes.c_uint32()
        assert frm_lib.frm_get_panorama(r.ctx, ctypes.byref(n)) == 0 and n.value == N
        # the refusals changed nothing: the panorama is still shown, and the next one is the same
        assert np.array_equal(r.read_frame(), want)
        assert np.array_equal(r.frame_pixels(r.read_frame_async()), want)
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), want)
