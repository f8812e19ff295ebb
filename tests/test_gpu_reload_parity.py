"""Runtime-reloaded kernels on the suite's hard single frames (reload_cases.py has the harness).

A reloaded module is not the code the rest of the suite pins: another compiler builds it (inside a
torch process, torch's bundled hiprtc), preprocessor fallbacks may be taken, march_persistent runs in
its single-frame instantiation (MULTI = false, which no built-in launch uses), and step 0 runs on the
device for every pixel. Here both reloaded kernels render the edge frames (edge_cases.py), the
all-lean and mixed lean frames, the service-pass cameras with their traces, the frames at the limits
of frm.h (limit_cases.py) and two step-0 cameras; bytes and the seven work counters equal the live
oracle's, the persistent kernel twice per frame. Hardware math has no oracle: the reloaded
persistent kernel equals the reloaded simple one.

Source variants that only reload can reach: the three preprocessor fallbacks forced, and a copy with
a wrong mb_tame, which the edge frames must expose. (Which fallbacks the runtime compiler really
takes is read from the log of the copy that test_gpu_reload_modes fails to load on a group.)

Contexts are shared with test_gpu_reload_modes.py where the kernel flag and max_steps fit: the
100-step edge frames run on the shutter context (two frames in flight), the 256-step all-lean frames
on the plain loop's (three), and the wrong-kernel copy is the one the FRM_RING=1 loop runs on."""
import math

import numpy as np
import pytest

import edge_cases as ec
import frm
import limit_cases as lc
import reload_cases as rc
from reload_cases import PERSISTENT, SIMPLE
from test_gpu_edges import WAVES_PER_CU, counters_of, mixed_frame_size
from test_gpu_lean_pass import AWAY, INFO_HIT, _camera_params, _ref as lean_ref
from test_gpu_service_frames import camera_params, refs_for

pytestmark = pytest.mark.gpu

KERNELS = [PERSISTENT, SIMPLE]
KERNEL_IDS = ["persistent", "simple"]
STEPS = 64  # of every frame whose max_steps the tables leave open


@pytest.fixture(scope="module")
def ctx(tmp_path_factory, frm_lib):
    def get(flags, max_steps, **kw):
        kw = dict(rc.SHARED.get((flags, max_steps), {}), **kw)
        return rc.context(tmp_path_factory, flags, max_steps, **kw)

    return get


# ---- 1. the hard single frames ---------------------------------------------------------------------

@pytest.mark.parametrize("flags", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("case", ec.CASES, ids=ec.CASE_IDS)
def test_edge_case_bytes_and_counters(ctx, oracle, case, flags):
    """As test_gpu_edges.test_edge_case_bytes_and_counters; the cases of one max_steps (64, 100) share
    a context per kernel."""
    r = ctx(flags, case.max_steps)
    rc.check_frame(r, case.params(), case.width, case.height, ec.reference(oracle, case), rc.launches(flags), case.name)


@pytest.mark.parametrize("case", ec.MANDELBULB_CASES, ids=[c.name for c in ec.MANDELBULB_CASES])
def test_edge_case_trace(ctx, oracle, case):
    """The built-in trace kernel reads the records the reloaded single-frame march wrote."""
    r = ctx(PERSISTENT, case.max_steps)
    rc.check_frame(r, case.params(), case.width, case.height, ec.reference(oracle, case), 1, case.name, trace=True)


@pytest.mark.parametrize("steps", [256, 1, 2])
@pytest.mark.parametrize("w,h", [(64, 36), (8, 8)], ids=["64x36", "8x8_one_chunk"])
def test_all_lean_frame(ctx, oracle, w, h, steps):
    """kLeanPass is on for MULTI = false: frames that never leave the lean pass."""
    ref = lean_ref(oracle, AWAY, w, h, steps)
    assert int(ref["counters"][1]) == 0 and not (ref["info"] & INFO_HIT).any()
    rc.check_frame(ctx(PERSISTENT, steps), _camera_params(AWAY, w, h), w, h, ref, 2, f"away {w}x{h}")


def mixed_single():
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    w, h = mixed_frame_size(cus, frames=1)
    assert w * h // 64 >= 2 * cus * WAVES_PER_CU
    return w, h


def test_mixed_lean_frame(ctx, oracle):
    """P1 with twice as many chunks as resident waves, three launches: waves whose hit pixels have
    drained go back to the lean pass (test_gpu_lean_pass.test_full_to_lean_inside_a_wave)."""
    w, h = mixed_single()
    ref = lean_ref(oracle, ec.P1, w, h, STEPS)
    assert 0 < ((ref["info"] & INFO_HIT) != 0).sum() <= w * h // 2
    rc.check_frame(ctx(PERSISTENT, STEPS), _camera_params(ec.P1, w, h), w, h, ref, 3, "mixed lean")


def service_frames(oracle, iters, w=96, h=54):
    ps = camera_params([ec.P9_TIME] * 4, iters, w, h)
    return ps, refs_for(oracle, ("reload single", iters), ps, w, h, STEPS, trace=True)


@pytest.mark.parametrize("iters", [200, 0])
def test_service_pass_guards(ctx, oracle, iters):
    """P1, the two deep points and the origin as single frames with their traces (power 9)."""
    r = ctx(PERSISTENT, STEPS)
    for k, (p, ref) in enumerate(zip(*service_frames(oracle, iters))):
        rc.check_frame(r, p, 96, 54, ref, 2, f"camera {k}", trace=True)


LIMIT_FRAMES = ("cube_g1", "cube_g2", "cube_g3", "cube_g4", "cube_stall", "sphere_stall", "mb_crawl")


def test_limit_frames_cover_the_step_bits(oracle):
    """Between the four grazes every bit 13..21 of the packed step count is set in one hit pixel and
    clear in another, and the stalls and the crawl run marches of the full length (from the oracle's
    info alone: the frames below cannot silently test nothing)."""
    span = sum(1 << b for b in lc.STEP_BITS)
    ones = zeros = 0
    for name in LIMIT_FRAMES[:4]:
        census = lc.step_census(lc.deep_reference(oracle, lc.deep_case(name)))
        ones |= census["ones"]
        zeros |= census["zeros"]
    assert ones == span and zeros == span
    for name in LIMIT_FRAMES[4:]:
        assert lc.step_census(lc.deep_reference(oracle, lc.deep_case(name)))["full"] > 0


@pytest.mark.parametrize("name", LIMIT_FRAMES)
def test_limit_deep_march(ctx, oracle, name):
    case = lc.deep_case(name)
    assert case.max_steps == lc.MAX_STEPS
    r = ctx(PERSISTENT | case.flags, lc.MAX_STEPS)  # sphere_stall: FRM_FLAG_SCENE_SPHERE, a family and a context of its own
    rc.check_frame(r, case.params(), case.width, case.height, lc.deep_reference(oracle, case), 2, name)


@pytest.mark.parametrize("case", lc.DIM_CASES, ids=lc.DIM_IDS)
def test_limit_dimension(ctx, oracle, case):
    assert lc.DIM_STEPS == STEPS
    rc.check_frame(ctx(PERSISTENT, STEPS), case.params(), case.width, case.height, lc.dim_reference(oracle, case), 2,
                   case.name)


@pytest.mark.parametrize("name", ["mb_pole", "mb_edge"])
def test_limit_iterations(ctx, oracle, name):
    assert lc.ITER_STEPS == STEPS
    case = lc.ITER_CASES[lc.ITER_IDS.index(name)]
    assert case.iters == lc.MAX_ITERS
    rc.check_frame(ctx(PERSISTENT, STEPS), case.params(), case.width, case.height, lc.iter_reference(oracle, case), 2,
                   name)


NEG0 = ((-0.0, ec.P1[0][1], ec.P1[0][2]), ec.P1[1], ec.P1[2])  # the built-in path does not skip step 0 here


def step_zero_frames(oracle, w=96, h=54):
    assert ec.P1[0][0] == 0.0 and math.copysign(1.0, NEG0[0][0]) < 0
    frames = [(p, oracle.render(p, w, h, STEPS)) for p in (_camera_params(cam, w, h) for cam in (ec.P1, NEG0))]
    assert frames[0][0].to_bytes() != frames[1][0].to_bytes()  # the sign of the zero reaches the parameters
    return frames


@pytest.mark.parametrize("flags", KERNELS, ids=KERNEL_IDS)
def test_step_zero_on_the_device(ctx, oracle, flags):
    """The built-in path runs P1's step 0 once on the host and the -0.0 camera's per pixel; a
    reloaded module runs both per pixel, and counts them as the oracle does."""
    r = ctx(flags, STEPS)
    for k, (p, ref) in enumerate(step_zero_frames(oracle)):
        rc.check_frame(r, p, 96, 54, ref, rc.launches(flags), f"camera {k}")


HW = frm.FRM_FLAG_HW_MATH


def test_hw_math_persistent_equals_simple(ctx):
    """FRM_FLAG_HW_MATH has no oracle: the reloaded persistent kernel gives the reloaded simple
    kernel's bytes and counters (the rule of test_gpu_body_count for the built-in pair). One context
    without a kernel flag runs both: frm_render of the whole frame is a persistent launch, its four
    ranks of bands are simple ones (frm_kernel_for_pixels says so). Whether the reloaded bytes equal
    the built-in hardware-math kernels' is printed, not asserted: nothing promises it."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    w = 768
    h = -(-1536 * cus // w)
    h += -h % 32
    p = _camera_params(ec.P1, w, h)
    r = ctx(HW, STEPS)
    r.resize(w, h)
    r.update_parameters_buffer(p)
    assert r.kernel_for(w * h) == "persistent"
    simple_img, simple_counters, largest = rc.render_by_bands(r, w, h, 8, 4)
    assert r.kernel_for(largest) == "simple"
    assert 0 < simple_counters[1] < w * h
    for launch in range(2):
        st = r.render(stats=True)
        rc.assert_frame(r.read_frame(), simple_img, f"launch {launch}")
        assert counters_of(st) == simple_counters, f"launch {launch}"
    with frm.Renderer(device=0, max_steps=STEPS, flags=HW) as b:
        b.resize(w, h)
        b.update_parameters_buffer(p)
        st = b.render(stats=True)
        same = bool(np.array_equal(b.read_frame(), simple_img)) and counters_of(st) == simple_counters
    print(f"hardware math: reloaded bytes and counters {'equal' if same else 'differ from'} the built-in kernels'")


# ---- 3. source variants that only reload can reach -------------------------------------------------

FALLBACK_EDGES = ("mb_axis_odd", "mb_inside", "mb_deep_dr_inf", "mb_small_r")


def test_forced_fallbacks(ctx, oracle):
    """lane_in, div_fixup_ and xor_sign_ through their fallback branches (shipped code, whichever
    compiler needs it): edge frames, the service cameras at N = 200 and the mixed lean frame."""
    r = ctx(PERSISTENT, STEPS, variant="fallback")
    for name in FALLBACK_EDGES:
        case = ec.CASES[ec.CASE_IDS.index(name)]
        assert case.max_steps == STEPS
        rc.check_frame(r, case.params(), case.width, case.height, ec.reference(oracle, case), 2, name, trace=True)
    for k, (p, ref) in enumerate(zip(*service_frames(oracle, 200))):
        rc.check_frame(r, p, 96, 54, ref, 2, f"camera {k}", trace=True)
    w, h = mixed_single()
    rc.check_frame(r, _camera_params(ec.P1, w, h), w, h, lean_ref(oracle, ec.P1, w, h, STEPS), 3, "mixed lean")


def test_returning_to_the_built_in_kernels(ctx, oracle):
    """The step-0 cameras on the fallback context, reloaded and then after reload(None): the built-in
    path (P1's step 0 on the host again) gives the same bytes and counters. The context leaves the
    shared ones: it is no longer a reloaded one."""
    r = ctx(PERSISTENT, STEPS, variant="fallback")
    frames = step_zero_frames(oracle)
    for k, (p, ref) in enumerate(frames):
        rc.check_frame(r, p, 96, 54, ref, 2, f"reloaded camera {k}")
    rc.retire(r)
    with r:
        r.reload(None)
        for k, (p, ref) in enumerate(frames):
            rc.check_frame(r, p, 96, 54, ref, 2, f"built-in camera {k}")


def test_a_wrong_kernel_is_noticed(ctx, oracle):
    """mb_tame without its r term: 7 log2 r of mb_tiny_r's bodies lies below exp2_tame's range
    (edge_cases.py), so the frame must differ from the oracle's, while mb_p1_n64 still matches. A
    reloaded edit reaches the edge frames, and they detect it."""
    r = ctx(PERSISTENT, STEPS, **rc.RING_LOOP)
    tiny, ordinary = (ec.CASES[ec.CASE_IDS.index(n)] for n in ("mb_tiny_r", "mb_p1_n64"))
    assert rc.frame_differs(r, tiny.params(), tiny.width, tiny.height, ec.reference(oracle, tiny))
    rc.check_frame(r, ordinary.params(), ordinary.width, ordinary.height, ec.reference(oracle, ordinary), 2, "mb_p1_n64")


def test_simple_kernel_returns_to_the_built_in_path(ctx, oracle):
    """The simple-kernel context of the step-0 test, reloaded and then after reload(None). It is
    this module's last use of that context, which leaves the shared ones."""
    r = ctx(SIMPLE, STEPS)
    frames = step_zero_frames(oracle)
    for k, (p, ref) in enumerate(frames):
        rc.check_frame(r, p, 96, 54, ref, 1, f"reloaded camera {k}")
    rc.retire(r)
    with r:
        r.reload(None)
        for k, (p, ref) in enumerate(frames):
            rc.check_frame(r, p, 96, 54, ref, 1, f"built-in camera {k}")


def test_compile_cap(ctx):
    print(f"frm_reload(dir) calls so far: {rc.reload_calls()}; compile seconds {[round(s, 2) for s in rc.compile_seconds]}")
    assert rc.reload_calls() <= rc.MAX_RELOADS
