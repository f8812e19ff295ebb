"""Frames at the four hard limits of include/frm.h, shared by the CPU census test
(test_limit_census.py) and the GPU tests (test_gpu_limits.py): FRM_MAX_STEPS_LIMIT (marches of
up to 4194303 steps), FRM_MAX_DIMENSION (frames 32768 pixels long), FRM_MAX_NUM_ITERATIONS (65536
fractal loop trips) and strides of 4 GiB and more. Plain data and helpers, in the style of
edge_cases.py: every input is a legal frm_parameters that the oracle maps to a defined answer, and
test_limit_census.py proves from the oracle alone that each case reaches what it is named for.

Deep marches (DEEP_CASES, all 8 x 8 at max_steps = FRM_MAX_STEPS_LIMIT). A march step is at least
kMinDistance = 5e-7, so a deep march needs a ray that stays within a few 1e-6 of a surface, or one
that stops moving. aspect_scale = (a, a) with a far below 1 makes the 64 rays almost parallel.
Figures are the oracle's (hit pixels; primary steps of the hits; full = miss pixels whose march ran
all 4194303 steps):

  graze: the ray crawls along a flat face at height h0, sinking by p per unit length
    cube_g1   scene 0 N 0, (-0.49, 0.5 + 7e-7, -0.49) yaw pi/4 pitch 1.2e-7 a 6e-8: 16 hits, 2038489..2255462
    cube_g2   h0 6e-7 p 6e-8 a 3e-8:                                                24 hits, 1873993..2319024
    cube_g3   h0 1e-6 p 4e-7 a 2e-7:                                                40 hits, 1202550..1879368
    cube_g4   h0 4e-6 p 3e-6 a 2e-6:                                                40 hits,  433912..754642
      over the four: every bit 13..21 of the step count is set in one hit pixel and clear in another
    sier_g1   scene 15 N 0: under the tetrahedron's base (y = -sqrt(6)/6), from (-0.42, base - 4e-6, -0.26)
              yaw pi/3 pitch -3e-6 a 2e-6:                                           8 hits, 440909
    sier_g2   h0 1e-5 p 1e-5 a 5e-6:                                                16 hits, 209390..229389
    koch16_g1 scene 16 N 0: along the face through (0, 0.5, 0), (+-0.75, 0, -sqrt(3)/4), from the face point
              (-0.5, 0.15, .) + 4e-6 n, yaw pi/2 pitch 3e-6 a 2e-6:                  6 hits, 471242..584668
    koch16_g2 h0 1e-5 p 1e-5 a 5e-6:                                                11 hits, 237321..317992
    koch17_g1, koch17_g2: scene 17 (its own kernel instantiation; at N 0 the same surface and figures)
  stall: far from the scene `t += d` stops moving t once d < ulp(t) / 2; the ray neither hits nor
  leaves and ends as a miss at it == max_steps
    cube_stall   scene 0 N 0, (0, 0, -600) a 5e-4:            36 hits (1..2 steps), 28 full
    sphere_stall FRM_FLAG_SCENE_SPHERE, (0, 0, -600) a 5e-4:  28 hits (5..7 steps), 36 full
  crawl: the Mandelbulb (scene 18, power 8) at N = 0
    mb_crawl  (0, 0, -7) yaw pi/2 a 0.2:                      14 hits, 3884417..4192401; 50 full

Why the Mandelbulb case is a crawl at N = 0 and not a stall at N = 1. A stall needs t >= 16 (ulp(t) / 2
> 5e-7) at a point whose DE is between 5e-7 and ulp(t) / 2. The reference's DE bails out at |z| > 100
with dr = 1, so beyond r = 100 it is 0.5 r ln r (233 at r = 101, 1919 at r = 600: the camera at
z = -600 ends every march after one step, 64 primary steps in all), and at N >= 1 every point with
1.78 < r <= 100 bails out at the second body with the same value (0.52 at r = 1.8, 6.8 at r = 7).
That exceeds r from r = e^2 = 7.39 on, so a ray that starts further out steps past the set and
never comes back, and one that starts nearer converges with t < 8. Inside r = 1.78 the N = 1 DE
falls from 1e-4 to 1e-15 within 0.2: a straight ray crosses that in some 1e4 steps. No camera gives
an N = 1 march of 4194303 steps. At N = 0 the one body leaves dr = 8 r^7 + 1 and the DE is
0.5 r ln r / dr: 1.03e-6 at r = 7, under 5e-7 from r = 8 to 100. A camera at r = 7 looking along
the tangent crawls outwards for 3.9 units at 5e-7..1e-6 per step: the rays that bend outwards hit
the r = 8 shell after 3.9 to 4.19 million steps, the others run out of steps. These are the deepest
hits of the table (bit 21 set, 1902 steps below the limit).

Frames at FRM_MAX_DIMENSION (DIM_CASES, 64 steps, pose P1): 32768 x 1 and 1 x 32768 of the Mandelbulb
(N 8, power 8) and the Menger sponge (scene 0, N 3). With update_aspect(w, h) the long axis spans
+-32768 and every ray misses (the reference's own setting for such a window); with aspect (1, 1) it
sweeps the object: per half of the axis 14346 / 14462 (wide) and 11957 / 11957 (tall) Mandelbulb hits,
5845 / 5842 Menger hits, misses in both halves.

FRM_MAX_NUM_ITERATIONS (ITER_CASES, 8 x 8, 64 steps, N = 65536). mb_inside: all 64 rays start at
(0, 0, -1), a point of the set: step 0 hits, and each pixel's 6 DEs (primary, four normal taps, one
shadow step) run all 65537 bodies: 25166208 bodies, no bailout (one origin gives one point set, so no
frame of this camera mixes the two exits at this N). mb_p1: 3448 DEs, every one bails out (18429
bodies). The launch of both cameras holds count exits and bailouts. mb_pole and mb_edge stand on the
set's boundary, at the last float32 inside it on a line along -z: every pixel hits at step 0, and of
its normal taps and shadow steps some leave by the count and some bail out, in one lane. mb_pole:
3200 DEs, 192 count exits, 3008 bailouts (shadow marches of 45 steps). mb_edge: 496 DEs, 314 count
exits, 182 bailouts, and pixels that march on past step 0 (150 primary steps), so lanes differ.
Scenes 0, 12, 15, 16, 17 from P1: their scales overflow long before 65536 folds; 12, 15, 16, 17 hit
nothing, scene 0 hits 12 pixels.

Strides: one allocation of 4 GiB + 1 MiB, frames and ranks BIG_STRIDE = 2^32 + 64 bytes apart."""
import math
from dataclasses import dataclass

import numpy as np

import frm
from helpers import params_for

P8 = frm.POWER8_TIME
P1 = frm.POSES["P1"]
MAX_STEPS = 4194303  # FRM_MAX_STEPS_LIMIT; test_limit_census.py compares the three with include/frm.h
MAX_DIM = 32768      # FRM_MAX_DIMENSION
MAX_ITERS = 65536    # FRM_MAX_NUM_ITERATIONS


def with_camera(p, camera, aspect=None):
    pos, yaw, pitch = camera
    p.update_camera(frm.Camera(pos, yaw, pitch))
    if aspect is not None:  # the field is the caller's: any value is legitimate
        p.raw.aspect_scale[0], p.raw.aspect_scale[1] = aspect
    return p


# ---- 1. deep marches -----------------------------------------------------------------------------
@dataclass(frozen=True)
class DeepCase:
    name: str
    kind: str            # graze, stall or crawl
    scene: int
    iters: int
    time: float
    camera: tuple        # (position, yaw, pitch)
    aspect: float
    min_hit_steps: int   # the census asserts max hit steps >= this (0: none asked)
    flags: int = 0
    width: int = 8
    height: int = 8
    max_steps: int = MAX_STEPS

    def params(self, width=None, height=None, camera=None, time=None):
        p = params_for(self.scene, self.iters, self.time if time is None else time, width or self.width,
                       height or self.height)
        return with_camera(p, camera or self.camera, (self.aspect, self.aspect))


def _cube(name, h0, p, a, min_hit):
    return DeepCase(name, "graze", 0, 0, 0.0, ((-0.49, 0.5 + h0, -0.49), math.pi / 4, p), a, min_hit)


SIER_BASE_Y = -math.sqrt(6.0) / 6.0  # the N = 0 tetrahedron's base, facing down


def _sier(name, h0, p, a):
    return DeepCase(name, "graze", 15, 0, 0.0, ((-0.42, SIER_BASE_Y - h0, -0.26), math.pi / 3, -p), a, 1 << 16)


# Koch N = 0: the face through (0, 0.5, 0) and (+-0.75, 0, -sqrt(3)/4); its outward normal and the
# point of it at x = -0.5, y = 0.15, from which a ray along +x stays on it for a length of 1
_KOCH_N = (0.0, math.sqrt(3.0) / 4 / math.hypot(math.sqrt(3.0) / 4, 0.5), -0.5 / math.hypot(math.sqrt(3.0) / 4, 0.5))
_KOCH_P = (-0.5, 0.15, -math.sqrt(3.0) / 4 + 0.15 * math.sqrt(3.0) / 2)


def _koch(name, scene, h0, p, a):
    pos = tuple(q + h0 * n for q, n in zip(_KOCH_P, _KOCH_N))
    return DeepCase(name, "graze", scene, 0, 0.0, (pos, math.pi / 2, p), a, 1 << 16)


_FAR = ((0.0, 0.0, -600.0), 0.0, 0.0)

DEEP_CASES = [
    _cube("cube_g1", 7e-7, 1.2e-7, 6e-8, 1 << 21),
    _cube("cube_g2", 6e-7, 6e-8, 3e-8, 1 << 21),
    _cube("cube_g3", 1e-6, 4e-7, 2e-7, 1 << 13),
    _cube("cube_g4", 4e-6, 3e-6, 2e-6, 1 << 13),
    _sier("sier_g1", 4e-6, 3e-6, 2e-6),
    _sier("sier_g2", 1e-5, 1e-5, 5e-6),
    _koch("koch16_g1", 16, 4e-6, 3e-6, 2e-6),
    _koch("koch16_g2", 16, 1e-5, 1e-5, 5e-6),
    _koch("koch17_g1", 17, 4e-6, 3e-6, 2e-6),
    _koch("koch17_g2", 17, 1e-5, 1e-5, 5e-6),
    DeepCase("cube_stall", "stall", 0, 0, 0.0, _FAR, 5e-4, 0),
    DeepCase("sphere_stall", "stall", 0, 0, 0.0, _FAR, 5e-4, 0, flags=frm.FRM_FLAG_SCENE_SPHERE),
    DeepCase("mb_crawl", "crawl", 18, 0, P8, ((0.0, 0.0, -7.0), math.pi / 2, 0.0), 0.2, 1 << 21),
]
DEEP_IDS = [c.name for c in DEEP_CASES]
CUBE_GRAZES = [c for c in DEEP_CASES if c.name.startswith("cube_g")]
STEP_BITS = range(13, 22)  # the bits of kRecStepsMask that no frame of 5000 steps sets

# launches of several frames (frm_render_bands_batch): the case's camera and P1 under the case's
# aspect; and the Mandelbulb crawl at two times (each lane carries its frame's power): power 8, and
# power 9 (sin(0.2 t) = 1), whose DE at the camera is 1.3e-7, so that all its pixels hit at step 0
# beside the other frame's lanes four million steps deep: only the power-8 lanes are deep
BATCH_CAMERA_CASES = ("cube_g2", "mb_crawl")
MB_CRAWL_TIMES = (P8, 7.853981634)
SUPERSAMPLED_CASE = "cube_g3"  # also rendered as the 2 x 2 samples of a 4 x 4 frame


def deep_case(name):
    return DEEP_CASES[DEEP_IDS.index(name)]


_REFS = {}


def _once(key, make):
    """The oracle's render of a case (once per session; callers must not write to it)."""
    if key not in _REFS:
        ref = make()
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def deep_reference(oracle, case, camera=None, time=None, width=None, height=None):
    w, h = width or case.width, height or case.height
    key = ("deep", case.name, camera, time, w, h)
    return _once(key, lambda: oracle.render(case.params(w, h, camera, time), w, h, case.max_steps, flags=case.flags,
                                            trace=True, info=True, census=True))


def step_census(ref, max_steps=MAX_STEPS):
    """What a deep case's name promises, from the oracle's per-pixel info words: hit and miss pixels,
    the hits' least and greatest primary step count, the bits 13..21 that some hit pixel's count has
    set (`ones`) and that some hit pixel's count has clear (`zeros`), and the misses that ran exactly
    max_steps steps."""
    info = ref["info"].ravel()
    hit = (info & 1) != 0
    steps = (info >> 8).astype(np.int64)
    hs = steps[hit]
    span = sum(1 << b for b in STEP_BITS)
    return {"hits": int(hit.sum()), "misses": int((~hit).sum()),
            "min_hit_steps": int(hs.min()) if len(hs) else 0, "max_hit_steps": int(hs.max()) if len(hs) else 0,
            "ones": int(np.bitwise_or.reduce(hs)) & span if len(hs) else 0,
            "zeros": int(np.bitwise_or.reduce(~hs)) & span if len(hs) else 0,
            "full": int((~hit & (steps == max_steps)).sum())}


# ---- 2. frames at FRM_MAX_DIMENSION ----------------------------------------------------------------
DIM_STEPS = 64
DIM_SCENES = {"mandelbulb": (18, 8), "menger": (0, 3)}  # scene, num_iterations; pose P1, power 8


@dataclass(frozen=True)
class DimCase:
    name: str
    scene: int
    iters: int
    width: int
    height: int
    unit_aspect: bool  # aspect_scale (1, 1): the long axis sweeps across the object

    def params(self, width=None, height=None, pose="P1"):
        """The parameters a caller showing width x height (default: the case's size) would set."""
        w, h = width or self.width, height or self.height
        p = params_for(self.scene, self.iters, P8, w, h, pose=pose)  # update_aspect(w, h), as the reference sets it
        if self.unit_aspect:
            p.raw.aspect_scale[0], p.raw.aspect_scale[1] = 1.0, 1.0
        return p


DIM_CASES = [DimCase(f"{name}_{'wide' if w > 1 else 'tall'}_{'unit' if unit else 'ref'}", scene, iters, w, h, unit)
             for name, (scene, iters) in DIM_SCENES.items()
             for w, h in ((MAX_DIM, 1), (1, MAX_DIM))
             for unit in (False, True)]
DIM_IDS = [c.name for c in DIM_CASES]


def dim_case(name):
    return DIM_CASES[DIM_IDS.index(name)]


def dim_reference(oracle, case, out_size=None, factor=1, pose="P1", costs=False):
    """The oracle's frame of a DimCase: the parameters of an out_size = (width, height) output (default:
    the case's own size) rendered at factor x that size, as the supersampled and adaptive paths
    sample it. costs: also the per-sample scheduling cost (oracle.render_costs)."""
    ow, oh = out_size or (case.width, case.height)
    p = case.params(ow, oh, pose=pose)
    w, h = factor * ow, factor * oh

    def make():
        ref = oracle.render(p, w, h, DIM_STEPS, trace=True, info=True)
        if costs:
            ref["cost"] = oracle.render_costs(p, w, h, DIM_STEPS)
        return ref

    return _once(("dim", case.name, ow, oh, factor, pose, costs), make)


# ---- 3. FRM_MAX_NUM_ITERATIONS rendered --------------------------------------------------------------
ITER_STEPS = 64


@dataclass(frozen=True)
class IterCase:
    name: str
    scene: int
    camera: tuple
    time: float = 1.0
    iters: int = MAX_ITERS
    width: int = 8
    height: int = 8

    def params(self, camera=None):
        return with_camera(params_for(self.scene, self.iters, self.time, self.width, self.height), camera or self.camera)


# Cameras at the last float32 inside the set along -z (found by bisection on "no bailout in 65537
# bodies"): the origin's DE leaves by the count while DEs 5e-7 away bail out.
MB_POLE = ((0.0, 0.0, -1.1040894985198975), 0.0, 0.0)
MB_EDGE = ((0.45, 0.1, -0.6351578235626221), 0.0, 0.0)

ITER_CASES = [IterCase("mb_inside", 18, ((0.0, 0.0, -1.0), 0.0, 0.0), P8), IterCase("mb_p1", 18, P1, P8),
              IterCase("mb_pole", 18, MB_POLE, P8), IterCase("mb_edge", 18, MB_EDGE, P8)] + \
    [IterCase(f"scene{s}", s, P1) for s in (0, 12, 15, 16, 17)]
ITER_IDS = [c.name for c in ITER_CASES]
ITER_SECOND_CAMERA = frm.POSES["P2"]  # the other frame of the batch of two


def iter_reference(oracle, case, camera=None):
    return _once(("iter", case.name, camera),
                 lambda: oracle.render(case.params(camera), case.width, case.height, ITER_STEPS, census=True))


# ---- 4. strides of 4 GiB and more ------------------------------------------------------------------
BIG_STRIDE = (1 << 32) + 64
BIG_BUFFER_BYTES = (1 << 32) + (1 << 20)
STRIDE_W, STRIDE_H, STRIDE_STEPS = 40, 24, 64
