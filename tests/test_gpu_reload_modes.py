"""The host paths that only a context with a runtime-reloaded module takes (reload_cases.py has the
harness): frm_render_bands_batch, frm_render_shutter and panoramas as one launch per frame with a
pinned slot (batch_shares_launch is false), launches that never rank (every one sorts again), the
module's own occupancy figure, one module per member of a group, and ring_eligible keeping reloaded
contexts out of the resident ring. Small frames; every frame equals the oracle's render of its own
parameters, and shutter, supersampled and panorama frames the float references of the built-in
tests (shutter_reference.py, ssaa_reference.py, panorama_reference.py).

Contexts are shared with test_gpu_reload_parity.py where the kernel flag and max_steps fit
(reload_cases.SHARED, RING_LOOP)."""
import numpy as np
import pytest

import edge_cases as ec
import frm
import panorama_reference as pano
import reload_cases as rc
import shutter_reference as shutter
import ssaa_reference as ssaa
from frm import _lib
from helpers import params_for
from reload_cases import PERSISTENT
from test_gpu_edges import counters_of
from test_gpu_lean_pass import BATCH_CAMERAS, BATCH_TIMES, _camera_params
from test_gpu_panorama import parameters as pano_parameters
from test_gpu_shutter import sub_frames

pytestmark = pytest.mark.gpu

STEPS = 64
W, H = 96, 54


@pytest.fixture(scope="module")
def ctx(tmp_path_factory, frm_lib):
    def get(flags, max_steps, **kw):
        return rc.context(tmp_path_factory, flags, max_steps, **kw)

    return get


# ---- frm_render_bands_batch: one launch per frame ---------------------------------------------------

@pytest.mark.parametrize("iters", [12, 0])
def test_batch_of_four_cameras(ctx, oracle, iters):
    """P1, the origin, P2 and the r < 2^-13 camera (ec.mixed_params), frames 208 bytes further apart
    than their size in a poisoned buffer."""
    ps = ec.mixed_params(ec.P8, W, H, iters)
    refs = [oracle.render(p, W, H, STEPS) for p in ps]
    rc.check_batch(ctx(PERSISTENT, STEPS), ps, refs, W, H, f"N = {iters}")


def test_batch_with_a_power_per_frame(ctx, oracle):
    times = BATCH_TIMES["per_frame_powers"]
    ps = [_camera_params(c, W, H, t) for c, t in zip(BATCH_CAMERAS, times)]
    assert len({p.to_bytes()[72:] for p in ps}) > 1  # the frames differ in more than their cameras
    refs = [oracle.render(p, W, H, STEPS) for p in ps]
    rc.check_batch(ctx(PERSISTENT, STEPS), ps, refs, W, H, "powers")


# ---- frm_render_bands + frm_unshuffle_bands -------------------------------------------------------------

def test_bands_of_three_ranks_reassemble(ctx, oracle):
    """Odd width, 11 bands of 5 rows and a last one of 2, over three ranks; three frames (the second
    and third sort by the keys of the one before)."""
    w, h = 131, 57
    p = params_for(18, 12, frm.POWER8_TIME, w, h)
    ref = oracle.render(p, w, h, STEPS)
    r = ctx(PERSISTENT, STEPS)
    r.resize(w, h)
    r.update_parameters_buffer(p)
    for frame in range(3):
        img, counters, _ = rc.render_by_bands(r, w, h, 5, 3)
        rc.assert_frame(img, ref["rgba"], f"frame {frame}")
        assert counters == rc.want_counters(ref), f"frame {frame}"


# ---- panorama and supersampling: the reloaded march, then the built-in projection / resolve -----------

def test_panorama_of_six_reloaded_faces(ctx, oracle):
    n, w, h = 14, 48, 24
    r = ctx(PERSISTENT, STEPS)
    r.set_panorama(n)
    try:
        r.resize(w, h)
        for scene, camera in (("mandelbulb", "inside"), ("menger", "inside")):
            p = pano_parameters(scene, camera, w, h)
            rs = [oracle.render(q, n + 2, n + 2, STEPS) for q in pano.face_parameters(p, n)]
            faces = np.stack([x["rgba"] for x in rs])
            assert sum(bool(np.any(faces[f, ..., :3])) for f in range(6)) >= 5  # geometry all round
            want = pano.project(faces, n, w, h, frm.equirect_tables(w, h), oracle)
            r.update_parameters_buffer(p)
            for k in range(2):
                st = r.render(stats=True)
                assert counters_of(st) == rc.want_counters(*rs), f"{scene} frame {k}"
                assert st["pixels"] == 6 * (n + 2) ** 2
                assert np.array_equal(r.read_frame(), want), f"{scene} frame {k}"
    finally:
        r.set_panorama(0)


def test_supersampled_reloaded_frame(ctx, oracle):
    w, h = 33, 17
    r = ctx(PERSISTENT, STEPS)
    r.set_supersampling(2)
    try:
        r.resize(w, h)
        for scene, iters in ((18, 6), (3, 3)):
            p = params_for(scene, iters, frm.POWER8_TIME, w, h)
            hi = oracle.render(p, 2 * w, 2 * h, STEPS)
            want = ssaa.box_resolve(hi["rgba"], 2, oracle)
            r.update_parameters_buffer(p)
            for k in range(2):
                st = r.render(stats=True)
                assert counters_of(st) == rc.want_counters(hi), f"scene {scene} frame {k}"
                assert np.array_equal(r.read_frame(), want), f"scene {scene} frame {k}"
    finally:
        r.set_supersampling(1)


# ---- frm_render_shutter ---------------------------------------------------------------------------------

SHUTTER_STEPS, SW, SH = 100, 33, 17  # 100 steps: the unchunked context also hosts the 100-step edge frames
_SHUTTER = {}


def shutter_frame(oracle, name):
    """(five sub-frame Parameters, the blurred frame at supersampling 2, the summed counters)."""
    if name not in _SHUTTER:
        subs = sub_frames(name, 5, SW, SH)
        rs = [oracle.render(p, 2 * SW, 2 * SH, SHUTTER_STEPS) for p in subs]
        img = shutter.accumulate(np.stack([x["rgba"] for x in rs]), 2, oracle)
        _SHUTTER[name] = (subs, img, rc.want_counters(*rs))
    return _SHUTTER[name]


@pytest.mark.parametrize("chunk", [None, "2"], ids=["unchunked", "chunks_of_2"])
def test_shutter_frames_keep_their_slots(ctx, oracle, chunk):
    """Five sub-frames at supersampling 2, each a launch of its own, on a context with two frames in
    flight: two consecutive shutter frames (Mandelbulb, animated Menger) are read back through their
    tickets after both were rendered, then each again with its counters."""
    env = (("FRM_SHUTTER_CHUNK", chunk),) if chunk else ()
    r = ctx(PERSISTENT, SHUTTER_STEPS, frames_in_flight=2, env=env)
    frames = [shutter_frame(oracle, name) for name in ("mandelbulb", "menger-animated")]
    assert np.any(frames[0][1] != frames[1][1])
    r.set_supersampling(2)
    try:
        r.resize(SW, SH)
        for rounds in range(2):
            tickets = []
            for subs, _, _ in frames:
                r.render_shutter(subs, stats=False)
                tickets.append(r.read_frame_async())
            for k, (t, (_, want, _)) in enumerate(zip(tickets, frames)):
                assert np.array_equal(r.frame_pixels(t), want), f"round {rounds} frame {k}"
        for k, (subs, want, counters) in enumerate(frames):
            st = r.render_shutter(subs, stats=True)
            assert counters_of(st) == counters, f"frame {k}"
            assert np.array_equal(r.read_frame(), want), f"frame {k}"
    finally:
        r.set_supersampling(1)


# ---- frames in flight ---------------------------------------------------------------------------------

def moving_loop(r, seq):
    """frm_render + frm_read_frame_async per (w, h, Parameters) with a frame of lag: the frames read."""
    held, got, size = [], [], None
    for w, h, p in seq:
        if (w, h) != size:
            r.resize(w, h)
            size = (w, h)
        r.update_parameters_buffer(p)
        r.render(stats=False)
        held.append((w, h, r.read_frame_async()))
        if len(held) > 1:
            hw, hh, t = held.pop(0)
            got.append(r.frame_pixels(t).reshape(hh, hw, 4))
    got += [r.frame_pixels(t).reshape(hh, hw, 4) for hw, hh, t in held]
    assert len(got) == len(seq)
    return got


LOOP_SIZES = [(W, H)] * 5 + [(80, 45)] * 4 + [(W, H)] * 3  # a resize in the middle of the loop, and back


def test_moving_loop_with_three_frames_in_flight(ctx, oracle):
    """Every frame of the loop is the oracle's render of its own parameters."""
    seq = [(w, h, params_for(18, 8, frm.POWER8_TIME + 0.37 * k, w, h, pose=("P0", "P1", "P2")[k % 3]))
           for k, (w, h) in enumerate(LOOP_SIZES)]
    got = moving_loop(ctx(PERSISTENT, 256, frames_in_flight=3), seq)
    for k, ((w, h, p), g) in enumerate(zip(seq, got)):
        rc.assert_frame(g, oracle.render(p, w, h, 256)["rgba"], f"frame {k}")


def test_moving_loop_stays_out_of_the_ring(ctx, oracle):
    """The loop again on a context created with FRM_RING=1. Its module is the wrong-kernel copy
    (mb_tame without its r term, reload_cases.py): the ring runs built-in kernels, so if
    ring_eligible let a reloaded context in, every frame would equal the oracle's. Every third frame
    stands at mb_tiny_r's camera, where the edit shows, and must differ from the oracle's; the frames
    between them, where it does not show, must equal it."""
    tiny = ec.CASES[ec.CASE_IDS.index("mb_tiny_r")]
    assert tiny.max_steps == STEPS
    seq = []
    for k, (w, h) in enumerate(LOOP_SIZES):
        p = tiny.params(w, h) if k % 3 == 1 else params_for(18, 12, ec.P8 + 0.37 * k, w, h, pose=("P0", "P1", "P2")[k % 3])
        seq.append((w, h, p))
    got = moving_loop(ctx(PERSISTENT, STEPS, **rc.RING_LOOP), seq)
    for k, ((w, h, p), g) in enumerate(zip(seq, got)):
        want = oracle.render(p, w, h, STEPS)["rgba"]
        if k % 3 == 1:
            assert np.any(g != want), f"frame {k}: the reloaded edit does not show"
        else:
            rc.assert_frame(g, want, f"frame {k}")


# ---- a group context: one module per member ---------------------------------------------------------------

def test_group_reload_is_all_or_none(ctx, oracle, tmp_path_factory):
    """devices = [0, 0, 0]: reloaded frames of 96 x 54 and 130 x 9 (fewer bands than ranks), back to
    the built-in kernels, then a copy that does not compile, which must leave every member rendering
    as before. That copy is the probe copy: its log also tells which of the three fallback branches
    the runtime compiler takes (printed: pytest -s)."""
    frames = []
    for w, h in ((W, H), (130, 9)):
        p = params_for(18, 8, frm.POWER8_TIME, w, h)
        frames.append((p, w, h, oracle.render(p, w, h, 128)))
    r = ctx(PERSISTENT, 128, devices=[0, 0, 0])

    def render_all(what):
        for p, w, h, ref in frames:
            rc.check_frame(r, p, w, h, ref, 2, f"{what} {w}x{h}")

    render_all("reloaded")
    rc.retire(r)
    with r:
        r.reload(None)
        render_all("built-in")
        with pytest.raises(frm.FrmError) as e:
            rc.reload(r, rc.source_copy(tmp_path_factory, "probe"))
        assert e.value.code == _lib.FRM_ERR_COMPILE and "FRM_PROBE" in str(e.value)
        for name, taken in rc.probe_answers(str(e.value)).items():  # a record, not an assertion: it depends on the torch build
            print(f"runtime compiler: {name} takes its {'fallback' if taken else 'builtin' if taken is False else '?'}")
        render_all("after the failed reload")


def test_compile_cap(ctx):
    print(f"frm_reload(dir) calls so far: {rc.reload_calls()}; compile seconds {[round(s, 2) for s in rc.compile_seconds]}")
    assert rc.reload_calls() <= rc.MAX_RELOADS
