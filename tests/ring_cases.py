"""The resident frame ring (frm_ring.hip, frm_ring_kernels.h, march_persistent<..., RES>) held to
the tables the per-frame grid and the reloaded kernels are held to: the loops of
test_gpu_ring_edges.py as data, shared with the CPU census (test_ring_cases.py), and the helper
that creates ring contexts, runs a loop of posts with a lag of readback and reads, from the line
ring_destroy prints under FRM_RING_DEBUG, how many frames the ring served.

A ring frame has no stats, and a context whose frames silently took the ordinary path would pass
every byte comparison. So every GPU test closes its contexts itself and compares the line's
`frames posted` with the count that eligible() below, a restatement of frm_ring.hip ring_eligible in
Python, gives for the frames it rendered. A frame the ring never marches or never shades keeps its
slot's earlier bytes, which only shows when neighbouring frames differ: test_ring_cases.py asserts,
from the oracle alone, that in every loop here frame k differs from frame k - 1 and from frame
k - slots."""
import re

import numpy as np

import edge_cases as ec
import frm
from helpers import params_for

PERSISTENT, SIMPLE, SPHERE = frm.FRM_FLAG_PERSISTENT_KERNEL, frm.FRM_FLAG_SIMPLE_KERNEL, frm.FRM_FLAG_SCENE_SPHERE
ENV = (("FRM_RING", "1"), ("FRM_RING_DEBUG", "1"))

# frm_ring.hip / frm_internal.h, restated
TASK_PIXELS = 16384     # kRingTaskPixels: pixels of one shade or rank task
GRID_IDS = 8            # kRingGridIds: grid_stop[id % 8]
FRAME_TABLES = 64       # per-frame tables indexed seq % 64
TRIP_BUDGET = 1 << 21   # 2 marches of max_steps DEs of N + 2 trips, at most
MAX_PIXELS = 1 << 28
FIFS = (2, 3)           # frames in flight of the loops: a ring of 2 and of 4 slots


def slots_for(frames_in_flight):
    """ring_size: the ring's slots (0: such a context has no ring)."""
    return 0 if frames_in_flight < 2 else 4 if frames_in_flight >= 3 else 2


def eligible(max_steps, iters, *, pixels, frames_in_flight, flags=PERSISTENT, ring=True, mode="plain", group=False,
             reloaded=False, stats=False):
    """Whether frm_render posts this frame to the ring (ring_eligible and frm_render's own tests). The
    kernel choice without a kernel flag depends on the device and is not restated: callers pass one."""
    assert flags & (PERSISTENT | SIMPLE), "the default kernel choice depends on the device"
    if not ring or stats or group or reloaded or mode != "plain" or slots_for(frames_in_flight) == 0:
        return False
    if not flags & PERSISTENT or pixels > MAX_PIXELS:
        return False
    n = 0 if flags & SPHERE else iters
    return 2 * max_steps * (n + 2) <= TRIP_BUDGET


# ---- contexts and the posted count ------------------------------------------------------------------

def set_env(monkeypatch):
    """FRM_RING is read when a context is created, FRM_RING_DEBUG when a grid is launched and when
    the context is destroyed: set for the whole test."""
    for k, v in ENV:
        monkeypatch.setenv(k, v)


def open_ring(max_steps, frames_in_flight, flags=PERSISTENT, **kw):
    return frm.Renderer(device=0, max_steps=max_steps, flags=flags, frames_in_flight=frames_in_flight, **kw)


_TOTALS = re.compile(r"frm ring: (\d+) frames posted, (\d+) grids launched, (\d+) service waves")


def close_and_count(r, capfd, contexts=1):
    """Closes the context; (frames posted, grids launched) of the line its ring_destroy printed (a
    group of n devices destroys n contexts and prints n lines: their sums)."""
    capfd.readouterr()
    r.close()
    err = capfd.readouterr().err
    found = _TOTALS.findall(err)
    assert len(found) == contexts if contexts else found, f"{contexts or 'some'} totals line(s) expected, got {err!r}"
    return sum(int(f[0]) for f in found), sum(int(f[1]) for f in found)


# ---- oracle frames, rendered once ---------------------------------------------------------------------

_REFS = {}


def reference(oracle, p, w, h, max_steps, flags=0):
    """The oracle's RGBA8 frame of Parameters p (cached by the parameter bytes; read-only)."""
    key = (p.to_bytes(), w, h, max_steps, flags)
    if key not in _REFS:
        img = oracle.render(p, w, h, max_steps, flags=flags)["rgba"]
        img.setflags(write=False)
        _REFS[key] = img
    return _REFS[key]


def run_loop(r, frames, lag):
    """frm_render + frm_read_frame_async per frame; the pixels of frame k - lag are fetched after
    frame k was posted, the rest at the end. Returns the frames read, in order."""
    held, got = [], []
    for p in frames:
        r.update_parameters_buffer(p)
        r.render(stats=False)
        held.append(r.read_frame_async())
        if len(held) > lag:
            got.append(r.frame_pixels(held.pop(0)))
    got += [r.frame_pixels(t) for t in held]
    assert len(got) == len(frames)
    return got


def neighbours_differ(images, slots):
    """None, or (k, j): frame k equals frame j = k - 1 or k - slots byte for byte."""
    for k in range(len(images)):
        for j in (k - 1, k - slots):
            if j >= 0 and np.array_equal(images[k], images[j]):
                return k, j
    return None


# ---- section 1: the 69 edge frames -----------------------------------------------------------------------

# Cases whose scene and N give the same all-black image from every pose (test_ring_cases.py
# test_other_n_is_needed): Koch once every distance is NaN or inf (scene 17 already at N = 211, where
# nothing is hit from outside), the Mandelbulb's single body at N = 0, Sierpinski's wrapped scale at
# N = 33. No neighbour of their own generation can differ from them, so their A and B keep everything
# but N, which they take from an ordinary count: each post of such a loop starts a new ring generation.
OTHER_N = {"koch16_n217": 214, "koch16_n218": 214, "koch16_n219": 214,
           "koch17_n211": 3, "koch17_n214": 3, "koch17_n217": 3, "koch17_n218": 3, "koch17_n219": 3,
           "mb_origin_n0": 12, "mb_tiny_xz_n0": 12, "sierpinski_n33": 31}


def edge_loop(case):
    """[A, case, B, A, case]: A and B are ordinary frames of the case's generation (scene, N, size,
    max_steps, aspect; the time too, but B of a Mandelbulb case, which takes another power), A at pose
    P1 and B at P2. A case that itself stands at P1 gets its A at P0."""
    w, h = case.width, case.height
    n = OTHER_N.get(case.name, case.iters)
    at_p1 = tuple(case.camera) == (ec.P1[0], ec.P1[1], ec.P1[2])
    a = params_for(case.scene, n, case.time, w, h, pose="P0" if at_p1 else "P1")
    b_time = case.time
    if case.mandelbulb:
        b_time = ec.P4_TIME if case.time == ec.P9_TIME else ec.P9_TIME
    b = params_for(case.scene, n, b_time, w, h, pose="P2")
    c = case.params()
    return [a, c, b, a, c]


def edge_loop_eligible(case, frames_in_flight):
    """How many of edge_loop(case)'s five frames the ring serves."""
    ns = [OTHER_N.get(case.name, case.iters), case.iters]
    return sum(eligible(case.max_steps, n, pixels=case.width * case.height, frames_in_flight=frames_in_flight)
               for n in (ns[0], ns[1], ns[0], ns[0], ns[1]))


# ---- section 2: lanes of several frames in one wave -----------------------------------------------------------

MIXED_STEPS = 64
MIXED_TIMES = [(ec.P8, 12), (ec.P9_TIME, 12), (ec.P8, 0)]  # (time, N) of test_gpu_edges._mixed_refs
MIXED_IDS = ["power8", "power9", "power8_n0"]
# Two rounds of the four cameras. Cameras 1 and 3 both give an all-black frame, so no order of two bare
# rounds keeps every frame different from the one before it and from the one four posts (a ring of
# slots) before it; with one ordinary frame from pose P0 (index 4) between the rounds this order does.
MIXED_ORDER = [0, 1, 2, 3, 4, 2, 1, 0, 3]
MIXED_POWER_TIMES = [ec.P8, ec.P9_TIME, ec.P4_TIME, ec.P8 + 0.37]
MIXED_CUS = 256  # the MI355X's compute units (the census renders the size the GPU test uses there)


def mixed_separator(time, w, h, iters=12):
    """Frame 4 of MIXED_ORDER: the generation's ordinary frame from pose P0."""
    return params_for(18, iters, time, w, h, pose="P0")


def mixed_power_params(w, h):
    """The four cameras of ec.MIXED_CAMERAS, each frame with a power of its own."""
    out = []
    for (pos, yaw, pitch), time in zip(ec.MIXED_CAMERAS, MIXED_POWER_TIMES):
        p = params_for(18, 12, time, w, h)
        p.update_camera(frm.Camera(pos, yaw, pitch))
        out.append(p)
    return out


# ---- section 3: sizes at the ring's own boundaries ------------------------------------------------------------

SIZES = [(1, 1), (7, 3), (64, 1), (65, 1), (130, 9), (129, 127), (128, 128), (129, 128), (181, 181)]
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]
# one context resized through all of them: the second size grows the slot buffers, every later one
# runs in buffers larger than its frame
RESIZE_ORDER = [(130, 9), (181, 181), (129, 128), (128, 128), (129, 127), (65, 1), (64, 1), (7, 3), (1, 1)]
SIZE_STEPS = 64
SIZE_SCENES = [(18, 8), (0, 4)]  # (scene, N)
# three cameras close to the set and looking at its centre, found by a search over random ones: their
# frames differ from each other in both scenes at every size, the 1 x 1 and 64 x 1 frames included
# (from the poses P0 to P2 those are background alone)
SIZE_CAMERAS = [((0.0, 0.81, -0.75), 0.0, 0.824), ((-0.68, -1.49, 0.09), 1.702, -1.139), ((-0.88, -0.43, -0.15), 1.402, -0.449)]


def size_frames(scene, iters, w, h):
    """Three moving frames of one scene: the camera changes, and the time (the Mandelbulb's power)."""
    out = []
    for k, cam in enumerate(SIZE_CAMERAS):
        p = params_for(scene, iters, frm.POWER8_TIME + 0.37 * k, w, h)
        p.update_camera(frm.Camera(*cam))
        out.append(p)
    return out


# ---- section 4: the eligibility edge ---------------------------------------------------------------------------

EDGE_W = EDGE_H = 8
IN_N64 = ec.CASES[ec.CASE_IDS.index("mb_in_n64")]


def _n64_params(iters):
    p = params_for(18, iters, IN_N64.time, EDGE_W, EDGE_H)
    p.update_camera(frm.Camera(*IN_N64.camera))
    return p


# (id, context flags, max_steps, N, Parameters, served by the ring). The budget is
# 2 * max_steps * (N + 2) <= 2^21 (N = 0 under the sphere flag). For the Mandelbulb at N = 65534 / 65536
# the step cap at which the two fall on either side is 16: (65534 + 2) * 32 = 2^21. At a cap of 8 both
# are inside (N + 2 <= 2^17), which is kept as a pair of its own.
ELIGIBILITY_EDGE = [
    ("menger_4096_n254", PERSISTENT, 4096, 254, params_for(0, 254, 1.0, EDGE_W, EDGE_H), True),
    ("menger_4096_n255", PERSISTENT, 4096, 255, params_for(0, 255, 1.0, EDGE_W, EDGE_H), False),
    ("bulb_16_n65534", PERSISTENT, 16, 65534, _n64_params(65534), True),
    ("bulb_16_n65536", PERSISTENT, 16, 65536, _n64_params(65536), False),
    ("bulb_8_n65534", PERSISTENT, 8, 65534, _n64_params(65534), True),
    ("bulb_8_n65536", PERSISTENT, 8, 65536, _n64_params(65536), True),
    ("sphere_524288", PERSISTENT | SPHERE, 524288, 3, params_for(18, 3, frm.POWER8_TIME, EDGE_W, EDGE_H), True),
    ("sphere_524289", PERSISTENT | SPHERE, 524289, 3, params_for(18, 3, frm.POWER8_TIME, EDGE_W, EDGE_H), False),
]
EDGE_IDS = [e[0] for e in ELIGIBILITY_EDGE]


BULB_SECOND_CAMERA = ((0.0, 0.0, -1.12), 0.0, 0.0)  # a step from the surface: a few pixels hit within 16 steps
# within 8 steps nothing is hit from any camera tried, and inside the set every pixel is black: the two
# frames of these tests are both black, and only their posted counts tell anything
BLACK_PAIRS = ("bulb_8_n65534", "bulb_8_n65536")


def edge_pair(p):
    """The second frame of an eligibility test: the same parameters from pose P2 (the Mandelbulb
    frames, which 8 or 16 steps do not reach from there: from BULB_SECOND_CAMERA)."""
    q = frm.Parameters.from_bytes(p.to_bytes())
    q.update_camera(frm.Camera(*(BULB_SECOND_CAMERA if p.num_iterations >= 65534 else ec.P2)))
    return q


# ---- section 6: loops over the ring's moduli --------------------------------------------------------------------

SMALL_W, SMALL_H = 64, 36
GRID_ROUNDS = 12   # > GRID_IDS: grid_stop's index wraps
LONG_LOOP = 70     # > FRAME_TABLES
LONG_DISTINCT = 35


def moving(n, w, h, scene=18, iters=8, distinct=None):
    """n frames whose time (the Mandelbulb's power) and pose change every frame; with `distinct`, frame
    k repeats frame k - distinct."""
    d = distinct or n
    return [params_for(scene, iters, frm.POWER8_TIME + 0.37 * (k % d), w, h, pose=("P0", "P1", "P2")[(k % d) % 3])
            for k in range(n)]


def ticket_bound(slots):
    """A ring frame's zero-copy image is R.img[(k - 1) % slots][((k - 1) / slots) & 1] (ring_render):
    frame k + 2 * slots is the next to post into it, and its post expires frame k's ticket. The
    ticket of frame k therefore holds while at most 2 * slots - 1 further frames are posted.
    include/frm.h promises a ticket "until frames_in_flight further frm_render calls have been made":
    2 slots serve 2 frames in flight (4 >= 2) and 4 slots serve 3 to FRM_MAX_FRAMES_IN_FLIGHT = 8
    (8 >= 8), so the ring keeps the promise everywhere and the two agree exactly at 8."""
    return 2 * slots - 1
