"""Depth of field on the GPU (include/frm.h frm_depth_of_field, frm_read_depth, frm_set_depth_of_field):
the gather kernel on raw data against tests/dof_reference.py, the depth plane against the oracle's hit
mask and the float64 reference's hit distances, and the context mode against that reference applied to
the oracle's plain frame: frames, work counters, the presentation paths, frames in flight, mode and
size changes, and the error codes. Everything but the depth accuracy is bit-exact."""
import ctypes

import numpy as np
import pytest

import dof_reference as ref
import f64_reference as f64
import frm
from frm import _lib
from helpers import params_for

pytestmark = pytest.mark.gpu

COUNTERS = ("pixels", "hit_pixels", "primary_steps", "shadow_steps", "normal_evals", "fractal_bodies",
            "fractal_bailouts")
W, H, STEPS = 48, 36, 256
# name -> scene, num_iterations, camera position (identity rotation), context flags
CASES = {"sphere": (0, 0, (0.1, 0.05, -2.0), frm.FRM_FLAG_SCENE_SPHERE),
         "menger": (3, 3, (0.2, 0.3, -3.0), 0),
         "mandelbulb": (18, 4, (0.1, 0.2, -2.5), 0)}
# |t_gpu - t_64| <= DEPTH_RATIO * max |t_32 - t_64|: the ratio measured on the MI355X (DESIGN.md "Depth of
# field": sphere 2.235, menger 2.896, mandelbulb 0.798) rounded up to the next power of two. The GPU's
# fma ray points and pinned builtins round differently from numpy's f32, but at the same scale; the
# loosest rule the project has is 16, and a ratio above it would be a wrong t, not rounding.
DEPTH_RATIO = {"sphere": 4.0, "menger": 4.0, "mandelbulb": 1.0}
LENS = (6.0, 1.8, 8)  # aperture, focus, radius of the context tests


def parameters(name, w=W, h=H, pos=None):
    scene, iters, position, _ = CASES[name]
    p = params_for(scene, iters, frm.POWER8_TIME, w, h)
    p.update_camera(frm.Camera(pos or position, 0.0, 0.0))
    return p


def raises_code(code, fn, *args, **kw):
    with pytest.raises(frm.FrmError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


@pytest.fixture(scope="module")
def renderer(gpu_renderer_factory):
    with gpu_renderer_factory(max_steps=STEPS) as r:
        yield r


@pytest.fixture(scope="module")
def plain_refs(oracle, frm_lib):
    """(name, w, h, pos) -> (Parameters, the oracle's frame, its hit mask, its counters)."""
    cache = {}

    def get(name, w=W, h=H, pos=None):
        key = (name, w, h, pos)
        if key not in cache:
            p = parameters(name, w, h, pos)
            o = oracle.render(p, w, h, STEPS, flags=CASES[name][3], trace=True)
            hit = o["trace"][..., 0] > 0
            for a in (o["rgba"], hit):
                a.setflags(write=False)
            cache[key] = (p, o["rgba"], hit, [int(c) for c in o["counters"][:7]])
        return cache[key]

    return get


def gpu_gather(r, src, depth, aperture, focus, radius, stream=0):
    """frm_depth_of_field of src [H, W, 4] and depth [H, W] from torch device tensors, the destination
    padded with zeros that must stay."""
    import torch
    h, w = depth.shape
    n = h * w * 4
    s = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    z = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).cuda()
    out = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.depth_of_field(s.data_ptr(), n, z.data_ptr(), n, w, h, aperture, focus, radius, out.data_ptr(), n, stream=stream)
    if stream:
        torch.cuda.synchronize()
    r.synchronize()
    got = out.cpu().numpy()
    assert not got[n:].any()  # nothing written past the frame
    return got[:n].reshape(h, w, 4)


# ---- 1. the kernel on raw data -----------------------------------------------------------------

@pytest.mark.parametrize("w,h,radius", ref.SHAPES)
def test_gather_random_texels_and_six_colours(renderer, oracle, w, h, radius):
    rng = np.random.default_rng(10000 * w + 100 * h + radius)
    src = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)  # alpha included: it is ignored
    z = ref.test_depths(rng, w, h)
    for aperture, focus in ((7.5, 2.0), (30.0, 0.9)):
        assert np.array_equal(gpu_gather(renderer, src, z, aperture, focus, radius),
                              ref.gather(src, z, aperture, focus, radius, oracle)), (aperture, focus)
    six = ref.six_colour_frame(w, h)
    assert np.array_equal(gpu_gather(renderer, six, z, 7.5, 2.0, radius), ref.gather(six, z, 7.5, 2.0, radius, oracle))
    # no aperture, or no radius: the source's bytes with alpha 255
    plain = src.copy()
    plain[..., 3] = 255
    assert np.array_equal(gpu_gather(renderer, src, z, 0.0, 2.0, radius), plain)
    assert np.array_equal(gpu_gather(renderer, src, z, 7.5, 2.0, 0), plain)


def test_gather_regions_in_and_out_of_focus(renderer, oracle):
    """Blocks whose staged pixels are all sharp, all blurred, and mixed: the block's reach changes, the bytes
    are the reference's."""
    w, h, F = 70, 40, 2.0
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    z = np.full((h, w), F, np.float32)
    z[:, 40:] = np.inf
    z[20:, 30:50] = rng.uniform(0.5, 6.0, size=(20, 20)).astype(np.float32)
    for radius in (5, 16):
        assert np.array_equal(gpu_gather(renderer, src, z, 9.0, F, radius), ref.gather(src, z, 9.0, F, radius, oracle))


def test_gather_on_another_stream(renderer, oracle):
    import torch
    w, h, radius = 37, 19, 3
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    z = ref.test_depths(rng, w, h)
    s = torch.cuda.Stream()
    got = gpu_gather(renderer, src, z, 4.0, 1.5, radius, stream=s.cuda_stream)
    assert np.array_equal(got, ref.gather(src, z, 4.0, 1.5, radius, oracle))


def test_gather_errors(frm_lib):
    import torch
    with frm.Renderer(max_steps=64) as r:
        # an 8 x 4 frame: 128 bytes of texels, 128 bytes of depths
        src = torch.zeros(128 + 64, dtype=torch.uint8, device="cuda")
        dep = torch.ones(32 + 16, dtype=torch.float32, device="cuda")
        dst = torch.zeros(128 + 16, dtype=torch.uint8, device="cuda")
        s, z, d = src.data_ptr(), dep.data_ptr(), dst.data_ptr()

        def call(src_ptr=s, src_bytes=128, depth_ptr=z, depth_bytes=128, w=8, h=4, aperture=2.0, focus=1.0, radius=4,
                 dst_ptr=d, dst_bytes=128):
            r.depth_of_field(src_ptr, src_bytes, depth_ptr, depth_bytes, w, h, aperture, focus, radius, dst_ptr, dst_bytes)

        bad, small = _lib.FRM_ERR_INVALID_ARGUMENT, _lib.FRM_ERR_BUFFER_TOO_SMALL
        raises_code(bad, call, src_ptr=0)
        raises_code(bad, call, depth_ptr=0)
        raises_code(bad, call, dst_ptr=0)
        raises_code(bad, call, src_ptr=s + 2)
        raises_code(bad, call, depth_ptr=z + 2)
        raises_code(bad, call, dst_ptr=d + 1)
        raises_code(bad, call, w=0)
        raises_code(bad, call, h=0)
        raises_code(bad, call, w=32769)
        raises_code(bad, call, radius=17)
        for aperture in (-1.0, float("nan"), float("inf")):
            raises_code(bad, call, aperture=aperture)
        for focus in (0.0, -2.0, float("nan"), float("inf")):
            raises_code(bad, call, focus=focus)
        raises_code(bad, call, dst_ptr=s + 64)  # overlaps the source
        raises_code(bad, call, dst_ptr=z + 64)  # overlaps the depths
        raises_code(small, call, src_bytes=127)
        raises_code(small, call, depth_bytes=124)
        raises_code(small, call, dst_bytes=127)
        call()  # and the valid call
        r.synchronize()
        assert dst[:128].cpu().numpy().reshape(4, 8, 4)[..., 3].min() == 255
        assert not dst[128:].cpu().numpy().any()


# ---- 2. the depth plane --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def marches():
    """name -> (the float64 march of the case's rays, the yardstick max |t_32 - t_64|)."""
    cache = {}

    def get(name):
        if name not in cache:
            P = f64.decode(parameters(name).to_bytes())
            sphere = bool(CASES[name][3])
            o, d = f64.camera_rays(P, W, H)
            m64 = f64.march(P, o, d, STEPS, sphere_scene=sphere)
            o32, d32 = f64.camera_rays(P, W, H, dtype=np.float32)
            m32 = f64.march(P, o32, d32, STEPS, dtype=np.float32, sphere_scene=sphere)
            assert np.array_equal(m32["hit"], m64["hit"]) and m64["hit"].sum() >= 20  # the reference alone: 0
            both = m64["hit"]
            yard = float(np.abs(m32["distance"][both].astype(np.float64) - m64["distance"][both]).max())
            cache[name] = (m64, yard)
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_read_depth(frm_lib, plain_refs, marches, name):
    p, frame, hit, counters = plain_refs(name)
    flags = CASES[name][3]
    with frm.Renderer(max_steps=STEPS, flags=flags | frm.FRM_FLAG_PERSISTENT_KERNEL) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        raises_code(_lib.FRM_ERR_NOT_READY, r.read_depth)  # no frame yet
        st = r.render(stats=True)
        z = r.read_depth()
        assert np.array_equal(r.read_frame(), frame) and [st[c] for c in COUNTERS] == counters
    assert z.shape == (H, W) and z.dtype == np.float32
    assert np.array_equal(np.isfinite(z), hit)  # exact
    assert np.all(np.isposinf(z[~hit])) and np.all(z[hit] >= 0)
    m64, yard = marches(name)
    hit64 = m64["hit"].reshape(H, W)
    disagree = int((hit64 != hit).sum())
    both = hit64 & hit
    err = float(np.abs(z[both].astype(np.float64) - m64["distance"].reshape(H, W)[both]).max())
    print(f"depth {name}: hits {int(hit.sum())}, mask disagreements with float64 {disagree}, "
          f"max |t_gpu - t_64| {err:.3e}, yardstick max |t_32 - t_64| {yard:.3e}, ratio {err / yard:.3f}")
    assert disagree <= 0.01 * W * H
    assert err <= DEPTH_RATIO[name] * yard
    # the plane of a depth-of-field context, whatever kernel the frame's size would have chosen: the same
    with frm.Renderer(max_steps=STEPS, flags=flags, depth_of_field=LENS) as r:
        assert r.kernel_for(W * H) == "persistent"
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        assert np.array_equal(r.read_depth().view(np.uint32), z.view(np.uint32))


def test_read_depth_is_refused_where_the_trace_is(frm_lib, plain_refs):
    p = plain_refs("menger")[0]
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_SIMPLE_KERNEL) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        raises_code(_lib.FRM_ERR_NOT_READY, r.read_depth)  # no records
        raises_code(_lib.FRM_ERR_NOT_READY, r.trace)
    with frm.Renderer(max_steps=STEPS, devices=[0, 0]) as g:
        g.resize(W, H)
        g.update_parameters_buffer(p)
        g.render(stats=False)
        raises_code(_lib.FRM_ERR_UNSUPPORTED, g.read_depth)
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        out = np.zeros(W * H - 1, np.float32)
        assert frm_lib.frm_read_depth(r.ctx, out.ctypes.data, out.size) == _lib.FRM_ERR_BUFFER_TOO_SMALL
        assert frm_lib.frm_read_depth(r.ctx, None, W * H) == _lib.FRM_ERR_INVALID_ARGUMENT
        assert not out.any()
        r.render_shutter([p, p])
        raises_code(_lib.FRM_ERR_NOT_READY, r.read_depth)  # no single frame's depth


# ---- 3. the context mode ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["menger", "mandelbulb", "sphere"])
def test_frame_counters_and_presentation(frm_lib, oracle, plain_refs, name):
    p, frame, hit, counters = plain_refs(name)
    A, F, R = LENS
    with frm.Renderer(max_steps=STEPS, flags=CASES[name][3], depth_of_field=LENS) as r:
        assert r.dof == LENS
        r.resize(W, H)
        r.update_parameters_buffer(p)
        for k in range(2):  # the second frame runs in the scheduled order; the bytes stay
            st = r.render(stats=True)
            assert [st[c] for c in COUNTERS] == counters, f"frame {k}"  # the plain frame's
            z = r.read_depth()
            assert np.array_equal(np.isfinite(z), hit)
            want = ref.gather(frame, z, A, F, R, oracle)
            got = r.read_frame()
            assert got.shape == (H, W, 4) and np.array_equal(got, want), f"frame {k}"
        assert np.any(want[..., :3] != frame[..., :3])  # the lens does blur this frame
        for ow, oh, srgb, bgra, flags in ((100, 60, True, False, 1), (20, 10, False, True, 2)):
            shown = r.present(ow, oh, srgb=srgb, bgra=bgra)
            assert np.array_equal(shown, oracle.blit(want, ow, oh, flags)), (ow, oh, flags)
            assert np.array_equal(r.frame_pixels(r.present_async(ow, oh, srgb=srgb, bgra=bgra)), shown)
        assert np.array_equal(r.frame_pixels(r.read_frame_async()), want)
        # no aperture: the plain frame's bytes (the oracle's alpha is 255 already)
        r.set_depth_of_field(0.0, F, R)
        raises_code(_lib.FRM_ERR_NOT_READY, r.read_frame_async)  # no frame under the new lens yet
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), frame)
        assert np.array_equal(r.read_depth().view(np.uint32), z.view(np.uint32))


def test_frames_in_flight_with_the_lens_changing(frm_lib, oracle, plain_refs):
    poses = [(0.2 + 0.1 * k, 0.3, -3.0 + 0.2 * k) for k in range(4)]
    lenses = [(6.0, 1.8, 8), (3.0, 2.5, 8), (10.0, 3.0, 16), (6.0, 1.8, 2)]
    refs = [plain_refs("menger", W, H, pos) for pos in poses]
    with frm.Renderer(max_steps=STEPS, frames_in_flight=2, depth_of_field=lenses[0]) as r:
        r.resize(W, H)
        held, got, planes = [], [], []
        for k in range(4):  # a frame of presentation latency
            r.set_depth_of_field(*lenses[k])
            r.update_parameters_buffer(refs[k][0])
            r.render(stats=False)
            planes.append(r.read_depth())
            held.append(r.read_frame_async())
            if len(held) > 1:
                got.append(r.frame_pixels(held.pop(0)))
        got += [r.frame_pixels(t) for t in held]
    assert len(got) == 4
    for k in range(4):
        assert np.array_equal(np.isfinite(planes[k]), refs[k][2]), f"frame {k}"
        assert np.array_equal(got[k], ref.gather(refs[k][1], planes[k], *lenses[k], oracle)), f"frame {k}"
    assert np.any(got[0] != got[1]) and np.any(got[2] != got[3])


def test_switching_on_off_and_resizing(frm_lib, oracle, plain_refs):
    p, frame, hit, counters = plain_refs("mandelbulb")
    A, F, R = LENS
    with frm.Renderer(max_steps=STEPS) as r:  # off: small frames run on the simple kernel
        assert r.dof[2] == 0 and r.kernel_for(W * H) == "simple"
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), frame)
        raises_code(_lib.FRM_ERR_NOT_READY, r.read_depth)
        r.set_depth_of_field(*LENS)  # on
        assert r.kernel_for(W * H) == "persistent"
        raises_code(_lib.FRM_ERR_NOT_READY, r.read_frame_async)
        st = r.render(stats=True)
        z = r.read_depth()
        want = ref.gather(frame, z, A, F, R, oracle)
        assert np.array_equal(r.read_frame(), want) and [st[c] for c in COUNTERS] == counters
        a, f, n = ctypes.c_float(), ctypes.c_float(), ctypes.c_uint32()
        assert frm_lib.frm_get_depth_of_field(r.ctx, ctypes.byref(a), ctypes.byref(f), ctypes.byref(n)) == 0
        assert (a.value, round(f.value, 6), n.value) == (A, F, R)
        # another size, no drain
        w2, h2 = 31, 22
        p2, frame2, hit2, counters2 = plain_refs("mandelbulb", w2, h2)
        r.resize(w2, h2)
        raises_code(_lib.FRM_ERR_NOT_READY, r.read_frame_async)
        r.update_parameters_buffer(p2)
        st = r.render(stats=True)
        z2 = r.read_depth()
        assert z2.shape == (h2, w2) and np.array_equal(np.isfinite(z2), hit2)
        assert np.array_equal(r.read_frame(), ref.gather(frame2, z2, A, F, R, oracle))
        assert [st[c] for c in COUNTERS] == counters2
        # off: the plain frame again, on the kernel its size chooses
        r.set_depth_of_field(0.0, 1.0, 0)
        assert r.kernel_for(w2 * h2) == "simple"
        raises_code(_lib.FRM_ERR_NOT_READY, r.read_frame_async)
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), frame2)
        # and on again at the first size
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.set_depth_of_field(*LENS)
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), want)
        assert r.trace().shape == (H, W, 10)  # the records are a persistent frame's


def test_unsupported_pairings_leave_the_state(frm_lib, oracle, plain_refs, tmp_path):
    import torch
    unsupported, bad = _lib.FRM_ERR_UNSUPPORTED, _lib.FRM_ERR_INVALID_ARGUMENT
    p, frame, _, _ = plain_refs("menger")
    A, F, R = LENS
    with frm.Renderer(max_steps=STEPS, devices=[0, 0]) as g:  # a group: one device listed twice
        raises_code(unsupported, g.set_depth_of_field, *LENS)
        assert g.dof[2] == 0
        g.set_depth_of_field(0.0, 1.0, 0)  # off stays allowed
    with frm.Renderer(max_steps=STEPS, supersampling=2) as s:
        raises_code(unsupported, s.set_depth_of_field, *LENS)
        s.resize(W, H)
        assert (s.render_width, s.render_height) == (2 * W, 2 * H)
    with frm.Renderer(max_steps=STEPS, adaptive=2) as a:
        raises_code(unsupported, a.set_depth_of_field, *LENS)
        assert a.adaptive[0] == 2
    with frm.Renderer(max_steps=STEPS, panorama=6) as q:
        raises_code(unsupported, q.set_depth_of_field, *LENS)
        assert q.panorama == 6
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_SIMPLE_KERNEL) as k:
        raises_code(unsupported, k.set_depth_of_field, *LENS)
        k.resize(W, H)
        k.update_parameters_buffer(p)
        k.render(stats=False)
        assert np.array_equal(k.read_frame(), frame)
    with frm.Renderer(max_steps=STEPS, depth_of_field=LENS) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        want = ref.gather(frame, r.read_depth(), A, F, R, oracle)
        assert np.array_equal(r.read_frame(), want)
        buf = torch.zeros(2 * W * H * 4, dtype=torch.uint8, device="cuda")
        raises_code(unsupported, r.set_supersampling, 2)
        raises_code(unsupported, r.set_adaptive, 2)
        raises_code(unsupported, r.set_panorama, 6)
        raises_code(unsupported, r.render_shutter, [p, p])
        raises_code(unsupported, r.render_bands, buf.data_ptr(), buf.numel(), 16, 0, 1)
        raises_code(unsupported, r.render_bands_batch, [p, p], buf.data_ptr(), dst_bytes=buf.numel(),
                    frame_stride=W * H * 4, band_rows=16, first_band=0, band_stride=1)
        raises_code(unsupported, r.unshuffle_bands, buf.data_ptr(), W * H * 4, buf.data_ptr() + W * H * 4, W * H * 4, 16, 1)
        raises_code(unsupported, r.reload, str(tmp_path))  # refused before anything is compiled
        raises_code(bad, r.set_depth_of_field, A, F, 17)
        raises_code(bad, r.set_depth_of_field, -1.0, F, R)
        raises_code(bad, r.set_depth_of_field, float("nan"), F, R)
        raises_code(bad, r.set_depth_of_field, float("inf"), F, R)
        raises_code(bad, r.set_depth_of_field, A, 0.0, R)
        raises_code(bad, r.set_depth_of_field, A, float("inf"), R)
        raises_code(bad, r.set_depth_of_field, A, float("nan"), R)
        r.set_supersampling(1)  # the neutral settings stay allowed
        r.set_adaptive(1)
        r.set_panorama(0)
        r.reload(None)
        assert r.dof == LENS
        a, f, n = ctypes.c_float(), ctypes.c_float(), ctypes.c_uint32()
        assert frm_lib.frm_get_depth_of_field(r.ctx, ctypes.byref(a), ctypes.byref(f), ctypes.byref(n)) == 0
        assert (a.value, round(f.value, 6), n.value) == (A, F, R)
        # the refusals changed nothing: the frame is still shown, and the next one is the same
        assert np.array_equal(r.read_frame(), want)
        assert np.array_equal(r.frame_pixels(r.read_frame_async()), want)
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), want)


def test_reloaded_kernels_refuse_the_lens(frm_lib, plain_refs, oracle, tmp_path):
    """Runtime-reloaded kernels write the records themselves: no depth of field while they are active."""
    import os
    import shutil
    p, frame, _, counters = plain_refs("menger")
    A, F, R = LENS
    src = tmp_path / "csrc"
    shutil.copytree(os.path.join(os.path.dirname(os.path.abspath(frm.__file__)), "..", "csrc"), src)
    with frm.Renderer(max_steps=STEPS, flags=frm.FRM_FLAG_PERSISTENT_KERNEL) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        r.reload(str(src))
        raises_code(_lib.FRM_ERR_UNSUPPORTED, r.set_depth_of_field, *LENS)
        assert r.dof[2] == 0
        a, f, n = ctypes.c_float(7), ctypes.c_float(7), ctypes.c_uint32(7)
        assert frm_lib.frm_get_depth_of_field(r.ctx, ctypes.byref(a), ctypes.byref(f), ctypes.byref(n)) == 0
        assert n.value == 0
        r.set_depth_of_field(0.0, 1.0, 0)  # off stays allowed
        st = r.render(stats=True)  # the plain frame, by the reloaded kernels
        assert np.array_equal(r.read_frame(), frame) and [st[c] for c in COUNTERS] == counters
        r.reload(None)  # back on the built-in kernels the lens is accepted
        r.set_depth_of_field(*LENS)
        assert r.dof == LENS
        r.render(stats=False)
        assert np.array_equal(r.read_frame(), ref.gather(frame, r.read_depth(), A, F, R, oracle))
