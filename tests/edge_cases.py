"""One table of numerically delicate inputs, shared by the CPU census test
(test_edge_census.py) and the GPU tests (test_gpu_edges.py, test_gpu_de.py). Plain data and
helpers: every input is a legal frm_parameters (or a plain float array) that the oracle maps
to a defined answer.

A frame case names the census events (oracle/frm_oracle.py CENSUS_COUNTS) it exists for;
test_edge_census.py asserts, from the oracle alone, that each occurs at least once (and that
the events in `absent` do not occur: the near side of a threshold). A GPU case can therefore
not silently test nothing."""
from dataclasses import dataclass

import numpy as np

import frm
from helpers import params_for

P8 = frm.POWER8_TIME
P9_TIME = 7.853981634   # sin(0.2 t) = +1: Mandelbulb power 9, the upper end of animate_between(4, 9)
P4_TIME = 23.561944902  # sin(0.2 t) = -1: power 4, the lower end
P1 = frm.POSES["P1"]
P2 = frm.POSES["P2"]


@dataclass(frozen=True)
class EdgeCase:
    name: str
    scene: int
    iters: int
    time: float
    camera: tuple  # (position, yaw, pitch)
    width: int
    height: int
    max_steps: int
    events: tuple
    absent: tuple = ()

    def params(self, width=None, height=None):
        w, h = width or self.width, height or self.height
        p = params_for(self.scene, self.iters, self.time, w, h)
        pos, yaw, pitch = self.camera
        p.update_camera(frm.Camera(pos, yaw, pitch))
        return p

    @property
    def mandelbulb(self):
        return self.scene == 18


def _mb(name, pos, events, w=33, h=19, iters=12, time=P8, steps=64, yaw=0.0, pitch=0.0, absent=()):
    return EdgeCase(name, 18, iters, time, (pos, yaw, pitch), w, h, steps, tuple(events), tuple(absent))


# every pixel: |z|^2 underflows or is 0, the magnitude is 0 or subnormal, DE = NaN, closeness
# NaN / 0, t becomes NaN and the march ends after one step
_NAN_AT_ORIGIN = ("mb_dot_wide", "mb_mag_not_normal", "mb_r_small", "mb_dr_nan", "mb_de_nan",
                  "primary_t0_dnan", "primary_q_nan", "primary_end_nan")
# every body has r < 2^-13, DE < 0: hit at step 0, and the shadow march's first step too (-x / 0)
_SMALL_R = ("mb_r_small", "mb_de_neg", "primary_t0_dnonpos", "primary_q_inf", "shadow_t0_dnonpos", "shadow_q_inf")
_ORDINARY = ("mb_dr_ge_2p64", "mb_de_neg", "shadow_t0_dpos", "shadow_t0_dnonpos", "shadow_q_inf",
             "primary_end_hit", "primary_end_steps", "primary_end_far", "shadow_end_hit", "shadow_end_steps",
             "shadow_end_far")

# Points inside the power-9 bulb whose orbit neither escapes nor is attracted for 200 iterations
# (found by test_edge_census's seeded search): dr grows by about 2^0.63 per body and passes 2^125
# near N = 200 and overflows before N = 219; the distance there is a subnormal, or x / inf = 0.
DEEP_A = (0.7762567400932312, 0.15817494690418243, -0.015379374846816063)
DEEP_B = (-0.655980110168457, 0.447213351726532, -0.032787490636110306)
DEEP_C = (-0.7092583179473877, -0.38535070419311523, -0.43509793281555176)

CASES = [
    _mb("mb_origin", (0.0, 0.0, 0.0), _NAN_AT_ORIGIN + ("mb_comp_zero",)),
    _mb("mb_tiny_xz", (1e-30, 0.0, 1e-25), _NAN_AT_ORIGIN + ("mb_comp_zero",)),
    _mb("mb_subnormal", (3e-39, -2e-41, 1e-40), _NAN_AT_ORIGIN + ("mb_comp_tiny",)),
    # N = 0: the one body leaves dr = 1, so the distance is 0.5 log(0) 0 / 1 = NaN from the magnitude
    # alone (at N >= 1 above dr is NaN too, and any logarithm of the magnitude gives NaN)
    _mb("mb_origin_n0", (0.0, 0.0, 0.0), ("mb_dot_wide", "mb_mag_not_normal", "mb_de_nan", "primary_t0_dnan",
                                          "primary_end_nan"), iters=0, absent=("mb_dr_nan",)),
    _mb("mb_tiny_xz_n0", (1e-30, 0.0, 1e-25), ("mb_dot_wide", "mb_mag_not_normal", "mb_de_nan", "primary_t0_dnan",
                                               "primary_end_nan"), iters=0, absent=("mb_dr_nan",)),
    _mb("mb_small_r", (1e-5, -2e-5, 3e-5), _SMALL_R, absent=("mb_comp_zero", "mb_comp_tiny")),
    _mb("mb_small_z", (0.0, 0.0, 1e-13), _SMALL_R + ("mb_comp_zero",)),
    # r = 2^-21.4 with no tiny component: 7 log2 r = -150 lies below exp2_tame's argument range
    # (r = 2^-14.7 above is under the tame bound, but its power is still a normal number), so a
    # tame test without its r term computes another pow(r, P - 1) here
    _mb("mb_tiny_r", (1e-7, -2e-7, 3e-7), _SMALL_R, absent=("mb_comp_zero", "mb_comp_tiny")),
    # a mix in one frame: r < 2^-13 bodies, DE = 0, DE = NaN, dr = NaN
    _mb("mb_inside", (0.0, 0.0, -1.0), ("mb_r_small", "mb_comp_zero", "mb_dot_wide", "mb_mag_not_normal", "mb_dr_nan",
                                        "mb_de_nan", "mb_de_zero", "mb_de_neg", "primary_t0_dnonpos",
                                        "primary_q_nan", "shadow_t0_dnan", "shadow_q_nan", "shadow_end_nan")),
    # axis-aligned rays: the centre column and row of an odd-sized frame keep x = 0 or y = 0 at
    # every sample (test_edge_census compares the count with the even twin's)
    _mb("mb_axis_odd", P1[0], ("mb_comp_zero",) + _ORDINARY),
    _mb("mb_axis_even", P1[0], ("mb_comp_zero",) + _ORDINARY, w=32, h=18),
    # the two ends of the power, where exp2_tame's argument range is tightest
    _mb("mb_power9", P1[0], _ORDINARY, w=48, h=27, time=P9_TIME),
    _mb("mb_power4", P1[0], ("mb_de_neg", "shadow_t0_dnonpos", "shadow_q_inf", "primary_end_hit", "shadow_end_hit"),
        w=48, h=27, time=P4_TIME),
    # large iteration counts: outside, rays bail out as at N = 12; inside, every DE runs all N + 1 bodies
    _mb("mb_p1_n64", P1[0], _ORDINARY, w=48, h=27, iters=64),
    _mb("mb_p1_n200", P1[0], _ORDINARY, w=48, h=27, iters=200),
    _mb("mb_in_n64", (0.3, 0.2, -0.5), ("mb_de_neg", "primary_t0_dnonpos", "shadow_t0_dnonpos", "shadow_q_inf"),
        w=48, h=27, iters=64),
    _mb("mb_in_n200", (0.3, 0.2, -0.5), ("mb_de_neg", "primary_t0_dnonpos", "shadow_t0_dnonpos", "shadow_q_inf"),
        w=48, h=27, iters=200),
    # the camera at a deep point: step 0 and the four normal taps divide by dr >= 2^125 (subnormal
    # DE), by dr = inf (DE = 0, closeness 0 / 0), or take log(inf) * inf / NaN
    _mb("mb_deep_dr_huge", DEEP_A, ("mb_dr_ge_2p125", "mb_de_subnormal", "mb_de_neg", "primary_t0_dnonpos",
                                    "shadow_t0_dpos", "shadow_end_far"), iters=200, time=P9_TIME),
    _mb("mb_deep_dr_inf", DEEP_A, ("mb_dr_inf", "mb_de_zero", "mb_dr_nan", "mb_de_nan", "mb_mag_not_normal",
                                   "primary_q_nan", "shadow_t0_dnan"), iters=219, time=P9_TIME),
    _mb("mb_deep_zero_de", DEEP_B, ("mb_dr_inf", "mb_de_zero", "mb_dr_ge_2p64", "primary_q_nan", "shadow_q_inf"),
        iters=200, time=P9_TIME),
]

# Koch: the folded point and scale_factor = 2 * 1.5^N overflow together; rays whose fold overflows
# first give inf - inf = NaN, the others +-inf or finite / 2^125; from N = 218 (16: 217 at this
# camera) the scale is inf and every DE is NaN
for _scene in (16, 17):
    for _n in (211, 214, 217, 218, 219):
        _all_nan = _n >= 218 or (_scene == 16 and _n == 217)
        _ev = ("de_nan", "primary_t0_dnan", "primary_end_nan") if _all_nan else \
            ("de_nan", "de_inf", "primary_q_inf", "primary_q_nan", "primary_end_nan", "primary_end_far")
        CASES.append(EdgeCase(f"koch{_scene}_n{_n}", _scene, _n, 1.0, P1, 48, 27, 64, _ev))

# Menger: -cross_inside / scale with scale = factor^i gives subnormal distances from N = 80 (scale
# factor 3; N = 78 is the near side). Scene 12 at this time has factor 4.2: its scale is inf from
# i = 62 on, repeat(p * inf) is NaN and max() drops the NaN quotient, which no result shows.
def _menger_events(scene, n):
    if scene == 12:
        return (), ()
    return (("de_subnormal",), ()) if n >= 80 else ((), ("de_subnormal",))


for _scene in (0, 4, 12):
    for _n in (78, 80, 82):
        _ev, _absent = _menger_events(_scene, _n)
        CASES.append(EdgeCase(f"menger{_scene}_n{_n}", _scene, _n, 1.0, P1, 48, 27, 64, ("primary_end_hit",) + _ev,
                              _absent))

# Sierpinski: 1 << (i % 32) wraps (i = 31 is i32's sign bit; N = 33 scales by 0.5 / 2)
CASES.append(EdgeCase("sierpinski_n31", 15, 31, 0.5, P1, 40, 24, 100, ("de_zero", "primary_end_hit", "shadow_end_hit")))
CASES.append(EdgeCase("sierpinski_n33", 15, 33, 0.5, P1, 40, 24, 100, ("primary_end_far",)))

# Extreme cameras: nothing refuses a subnormal, far, infinite or NaN camera position, so these are
# legal frames. The far cameras end every ray at step 0 (distance over MAX_TOTAL_DISTANCE; Koch's
# folds overflow to inf - inf = NaN at 3e38). The subnormal, inf and NaN cameras do not: minNum /
# maxNum drop a NaN or inf coordinate in Menger's box and folds, so scene 0 still hits pixels and
# marches shadow rays; Sierpinski and Koch give NaN distances; the Mandelbulb's atan2 of two
# subnormals (max below 2^-128: RN(1 / max) = inf) is NaN, and so is every body of the inf and
# NaN cameras, which run all N + 1 bodies per pixel without a bailout.
CAMERA_POSITIONS = (
    ("sub", (1e-40, -1e-42, -2.0)), ("far_1e4", (0.0, 0.0, -1e4)), ("far_oblique", (3e3, 2e3, -1e4)),
    ("far_1e19", (0.0, 0.0, -1e19)), ("far_3e38", (1e30, 0.0, -3e38)), ("inf", (float("inf"), 0.0, -1.0)),
    ("nan", (float("nan"), 0.0, -2.0)))
CAMERA_SCENES = ((0, 3, 1.0), (15, 3, 1.0), (16, 3, 1.0), (18, 6, P8))  # (scene, N, time)
_CAM_HITS = (("primary_end_hit", "primary_end_far", "shadow_divs"), ("primary_end_nan",))
_CAM_FAR = (("primary_end_far",), ("primary_end_hit", "primary_end_nan", "primary_end_steps", "shadow_divs"))
_CAM_NAN = (("primary_end_nan", "primary_t0_dnan"), ("primary_end_hit", "primary_end_far", "primary_end_steps", "shadow_divs"))


def _camera_events(scene, tag):
    if tag.startswith("far"):
        return _CAM_NAN if (scene, tag) == (16, "far_3e38") else _CAM_FAR
    if scene == 0 or tag == "sub" and scene != 18:
        return _CAM_HITS
    return (_CAM_NAN[0] + ("mb_de_nan", "mb_dr_nan"), _CAM_NAN[1]) if scene == 18 else _CAM_NAN


CAMERA_CASES = []
for _scene, _n, _time in CAMERA_SCENES:
    for _tag, _pos in CAMERA_POSITIONS:
        _ev, _absent = _camera_events(_scene, _tag)
        CAMERA_CASES.append(EdgeCase(f"cam{_scene}_{_tag}", _scene, _n, _time, (_pos, 0.0, 0.0), 33, 19, 64, _ev, _absent))
CASES += CAMERA_CASES

CASE_IDS = [c.name for c in CASES]
MANDELBULB_CASES = [c for c in CASES if c.mandelbulb]

# the four cameras of the mixed-wave launch and of the frames-in-flight sequence: ordinary P1, the
# origin (every lane NaN after one body), ordinary P2, and r < 2^-13 at every body
MIXED_CAMERAS = [P1, ((0.0, 0.0, 0.0), 0.0, 0.0), P2, ((1e-5, -2e-5, 3e-5), 0.0, 0.0)]


_REFS = {}


def reference(oracle, case):
    """The oracle's render of a frame case with its trace and census (rendered once per
    session; callers must not write to it)."""
    if case.name not in _REFS:
        _REFS[case.name] = oracle.render(case.params(), case.width, case.height, case.max_steps, trace=True,
                                         census=True)
    return _REFS[case.name]


def camera_batch_params(scene=0):
    """The seven extreme cameras of one scene as the frames of one batch launch."""
    return [c.params() for c in CAMERA_CASES if c.scene == scene]


def mixed_params(time, width, height, iters=12):
    """The four frames of MIXED_CAMERAS (one scene, N and time, as a batch launch requires)."""
    out = []
    for pos, yaw, pitch in MIXED_CAMERAS:
        p = params_for(18, iters, time, width, height)
        p.update_camera(frm.Camera(pos, yaw, pitch))
        out.append(p)
    return out


# ---- point sets for the distance estimators --------------------------------------------------
@dataclass(frozen=True)
class PointCase:
    name: str
    scene: int
    iters: int
    time: float
    points: str  # key of point_set()
    events: tuple
    absent: tuple = ()

    def params(self):
        return params_for(self.scene, self.iters, self.time, 8, 8)


def _ulps(x, ks):
    """float32 x moved by each of ks encodings."""
    b = np.float32(x).view(np.uint32).astype(np.int64)
    return (b + np.asarray(ks, np.int64)).astype(np.uint32).view(np.float32)


def tame_boundary_points():
    """(below, above, edge): points just outside and just inside the tame Mandelbulb body's
    operand domain at its two boundaries. `below`: |p| = 2^-13 (1 + k 2^-23) with k <= -2, or one
    component 1 to 3 encodings under 2^-60; `above`: the same with k >= 2 (all components far
    above 2^-60), or one component 0 to 3 encodings over 2^-60 (the test is >=). The f32 length
    (three roundings in the dot product, one in the sqrt, one per component) is within
    1.4 * 2^-23 of |p|, so those sides are certain; `edge` holds k = -1, 0, 1, which fall on
    whichever side the rounding puts them."""
    rng = np.random.default_rng(2013)
    below, above, edge = [], [], []
    for _ in range(48):
        d = rng.uniform(0.2, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
        d /= np.linalg.norm(d)
        for k in (-6, -3, -2, -1, 0, 1, 2, 3, 6):
            p = (d * 2.0 ** -13 * (1.0 + k * 2.0 ** -23)).astype(np.float32)
            (edge if abs(k) < 2 else below if k < 0 else above).append(p)
    for axis in range(3):
        for k in (-3, -2, -1, 0, 1, 2, 3):
            for sign in (1.0, -1.0):
                p = rng.uniform(0.3, 1.1, 3).astype(np.float32) * rng.choice([-1.0, 1.0], 3).astype(np.float32)
                p[axis] = sign * _ulps(2.0 ** -60, [k])[0]
                (below if k < 0 else above).append(p)
    return np.array(below, np.float32), np.array(above, np.float32), np.array(edge, np.float32)


def far_below_points():
    """Points with |p| from 2^-16 down to 2^-58 and every component above 2^-60: r is far under
    the tame bound, (P - 1) log2 r is below exp2_tame's argument range for every power (at P = 4
    from 2^-42 on) and pow(r, P - 1) underflows, while the component test alone would pass."""
    rng = np.random.default_rng(58)
    d = rng.uniform(0.4, 1.0, (128, 3)) * rng.choice([-1.0, 1.0], (128, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (d * np.exp2(-rng.uniform(16, 58, 128))[:, None]).astype(np.float32)


def _mandelbulb_points():
    """4096 points = 64 waves of 64 lanes: waves 0, 4, 8.. ordinary points (all tame), waves
    1, 9.. all lanes just outside the tame domain and waves 5, 13.. far outside it, by r alone (all
    exact), waves 2, 6.. all lanes just inside
    it (all tame, at the boundary), waves 3, 7.. ordinary points with a few lanes from either
    side, the origin and a point whose |z|^2 underflows (mixed)."""
    rng = np.random.default_rng(64)
    pts = rng.uniform(-1.2, 1.2, (4096, 3)).astype(np.float32)
    below, above, edge = tame_boundary_points()
    far = far_below_points()
    for w in range(64):
        lanes = slice(64 * w, 64 * w + 64)
        if w % 8 == 1:
            pts[lanes] = below[(np.arange(64) + 7 * w) % len(below)]
        elif w % 8 == 5:
            pts[lanes] = far[(np.arange(64) + 7 * w) % len(far)]
        elif w % 4 == 2:
            pts[lanes] = above[(np.arange(64) + 7 * w) % len(above)]
        elif w % 4 == 3:
            pts[64 * w + 5] = below[w % len(below)]
            pts[64 * w + 40] = below[(3 * w) % len(below)]
            pts[64 * w + 41] = above[w % len(above)]
            pts[64 * w + 42] = edge[w % len(edge)]
            pts[64 * w + 63] = edge[(5 * w) % len(edge)]
            pts[64 * w + 7] = 0.0                   # |z| = 0
            pts[64 * w + 8] = [1e-30, 0.0, 1e-25]   # |z|^2 underflows to 0
    return pts


_POINT_SETS = {}


def point_set(key):
    """The 4096 points of a PointCase (built once; callers must not write to them)."""
    if key not in _POINT_SETS:
        if key == "koch":
            pts = np.random.default_rng(16).uniform(-1.5, 1.5, (4096, 3)).astype(np.float32)
        elif key == "menger":  # half of them inside the cube, where only the finest folds bound the distance
            rng = np.random.default_rng(80)
            pts = np.concatenate([rng.uniform(-1.5, 1.5, (2048, 3)), rng.uniform(-0.5, 0.5, (2048, 3))]).astype(np.float32)
        elif key == "mandelbulb_deep":  # the deep points and their neighbours within 64 encodings
            rng = np.random.default_rng(200)
            base = np.array([DEEP_A, DEEP_B, DEEP_C], np.float32)[np.arange(4096) % 3]
            off = rng.integers(-64, 65, (4096, 3))
            off[:3] = 0
            pts = (base.view(np.uint32).astype(np.int64) + off).astype(np.uint32).view(np.float32)
        else:
            pts = _mandelbulb_points()
        pts.setflags(write=False)
        _POINT_SETS[key] = pts
    return _POINT_SETS[key]


POINT_CASES = []
for _scene in (16, 17):
    POINT_CASES += [
        PointCase(f"koch{_scene}_n214", _scene, 214, 1.0, "koch", (), ("de_nan", "de_inf")),
        PointCase(f"koch{_scene}_n217", _scene, 217, 1.0, "koch", ("de_nan", "de_inf")),
        PointCase(f"koch{_scene}_n218", _scene, 218, 1.0, "koch", ("de_nan", "de_zero")),
        PointCase(f"koch{_scene}_n219", _scene, 219, 1.0, "koch", ("de_nan", "de_zero")),
    ]
for _scene in (0, 4, 12):
    POINT_CASES += [PointCase(f"menger{_scene}_n{_n}", _scene, _n, 1.0, "menger", *_menger_events(_scene, _n))
                    for _n in (78, 80, 82)]
_MB_POINT_EVENTS = ("mb_r_small", "mb_comp_tiny", "mb_de_neg", "mb_dr_ge_2p64")
POINT_CASES += [
    PointCase("mandelbulb_n0", 18, 0, P8, "mandelbulb", ("mb_r_small", "mb_comp_tiny", "mb_mag_not_normal", "mb_de_nan"),
              ("mb_dr_nan",)),
    PointCase("mandelbulb_n64", 18, 64, P8, "mandelbulb", _MB_POINT_EVENTS),
    PointCase("mandelbulb_n200", 18, 200, P8, "mandelbulb", _MB_POINT_EVENTS),
    PointCase("mandelbulb_power9", 18, 12, P9_TIME, "mandelbulb", _MB_POINT_EVENTS),
    PointCase("mandelbulb_power4", 18, 12, P4_TIME, "mandelbulb", ("mb_r_small", "mb_comp_tiny", "mb_de_neg")),
]
POINT_CASES += [
    PointCase("mandelbulb_deep_n200", 18, 200, P9_TIME, "mandelbulb_deep",
              ("mb_dr_ge_2p125", "mb_dr_inf", "mb_de_subnormal", "mb_de_zero")),
    PointCase("mandelbulb_deep_n219", 18, 219, P9_TIME, "mandelbulb_deep",
              ("mb_dr_ge_2p125", "mb_dr_inf", "mb_de_subnormal", "mb_de_zero")),
]
POINT_CASE_IDS = [c.name for c in POINT_CASES]


# ---- operands for div and sqrt over the whole type ------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
DIV_SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126, -(2.0 ** -126),
                         FLT_MAX, -FLT_MAX, 1.0, -1.0, 0.75 * 2.0 ** -126, 2.0 ** 125, 2.0 ** -125, 2.0 ** 126,
                         2.0 ** 127], np.float32)


def random_finite_encodings(rng, n, signed=True):
    """n float32 whose sign, exponent field (0..254: subnormals included, no inf / NaN) and
    mantissa are uniformly random."""
    bits = (rng.integers(0, 255, n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    if signed:
        bits |= rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
    return bits.view(np.float32)


def _quotients_near(rng, targets, n_each):
    """Pairs (a, b) whose exact quotient lies within a few ulp of each float64 target: b random
    over the exponents that keep a = target * b normal, a = RN(target * b) moved by -2..2
    encodings."""
    a_out, b_out = [], []
    for q in targets:
        lo = max(-120.0, -120.0 - np.log2(abs(q)))
        hi = min(120.0, 120.0 - np.log2(abs(q)))
        b = (np.exp2(rng.uniform(lo, hi, n_each)) * rng.choice([-1.0, 1.0], n_each)).astype(np.float32)
        a = (q * b.astype(np.float64)).astype(np.float32)
        for k in (-2, -1, 0, 1, 2):
            a_out.append((a.view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(np.float32))
            b_out.append(b)
    return np.concatenate(a_out), np.concatenate(b_out)


def div_whole_type_inputs():
    """(a, b) float32: 400 k pairs of random finite encodings; the cross product of
    DIV_SPECIALS; quotients within a few ulp of 2^-126 (the subnormal threshold), of FLT_MAX
    (the overflow threshold) and of half-way points between adjacent subnormals, the exact ties
    (odd * 2^k / 2^(k + 150)) included."""
    rng = np.random.default_rng(149)
    a0, b0 = random_finite_encodings(rng, 400000), random_finite_encodings(rng, 400000)
    sa, sb = (g.ravel() for g in np.meshgrid(DIV_SPECIALS, DIV_SPECIALS))
    halves = [(m + 0.5) * 2.0 ** -149 for m in (0, 1, 2, 3, 6, 7, 1000, 1001, 2 ** 22, 2 ** 23 - 2, 2 ** 23 - 1)]
    targets = [2.0 ** -126, -(2.0 ** -126), FLT_MAX, -FLT_MAX, 2.0 ** 128] + halves + [-h for h in halves[:4]]
    a1, b1 = _quotients_near(rng, targets, 200)
    odd = np.array([2 * m + 1 for m in (0, 1, 2, 3, 500, 2 ** 22, 2 ** 23 - 1)], np.float64)  # exact ties
    ks = np.arange(-120, -22, 7)  # a = odd * 2^k and b = 2^(k + 150) both normal: a / b = odd * 2^-150
    a2 = np.concatenate([odd * 2.0 ** k for k in ks]).astype(np.float32)
    b2 = np.concatenate([np.full(len(odd), 2.0 ** (k + 150)) for k in ks]).astype(np.float32)
    return np.concatenate([a0, sa, a1, a2, -a2]), np.concatenate([b0, sb, b1, b2, b2])


def sqrt_whole_type_inputs():
    """Non-negative float32: 400 k uniformly random finite encodings, 20 k subnormals, every
    power of two with its neighbours, and the specials."""
    rng = np.random.default_rng(23)
    a = random_finite_encodings(rng, 400000, signed=False)
    sub = rng.integers(1, 1 << 23, 20000, dtype=np.uint32).view(np.float32)
    pw = (np.arange(0, 255, dtype=np.int64)[:, None] << 23) + np.arange(-2, 3)
    pw = pw[(pw >= 0) & (pw < 0x7f800000)].astype(np.uint32).view(np.float32)
    special = np.array([0.0, -0.0, np.inf, np.nan, 2.0 ** -149, 2.0 ** -126, FLT_MAX, 1.0, 4.0], np.float32)
    return np.concatenate([a, sub, pw, special])


def div_tame_edge_inputs():
    """(a, b) at the ends of div_tame's operand range: every pair of values within 3 encodings
    of 2^-60 and of 2^40, both signs (the extreme quotients 2^40 / 2^-60 and 2^-60 / 2^40
    included)."""
    ks = np.arange(-3, 4)
    v = np.concatenate([_ulps(2.0 ** -60, ks), _ulps(2.0 ** 40, ks)])
    v = np.concatenate([v, -v])
    a, b = (g.ravel() for g in np.meshgrid(v, v))
    return a, b
