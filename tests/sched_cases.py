"""The frames the scheduler tests run (test_sched_reference.py on the CPU, test_gpu_sched.py on the
GPU): plain data and helpers. Every frame stays below 20 k pixels, so an oracle render takes
milliseconds. Sizes are chosen against the 4096 pixels a rank_pass / shade_pass block handles
(kShadeBlockPixels), its 256 threads and the march's 64-pixel chunk."""
from dataclasses import dataclass

import numpy as np

import frm
from helpers import params_for

import edge_cases

P8 = frm.POWER8_TIME
P1 = frm.POSES["P1"]


@dataclass(frozen=True)
class SchedCase:
    name: str
    scene: int
    iters: int
    time: float
    width: int
    height: int
    max_steps: int = 256
    flags: int = 0
    camera: tuple = P1       # (position, yaw, pitch)
    neg_zero_x: bool = None  # None: the camera as given; True / False: the origin's x forced to -0 / +0
    supersampling: int = 1

    @property
    def mandelbulb(self):
        return self.scene == 18 and not (self.flags & frm.FRM_FLAG_SCENE_SPHERE)

    @property
    def render_size(self):
        return self.width * self.supersampling, self.height * self.supersampling

    def params(self):
        p = params_for(self.scene, self.iters, self.time, self.width, self.height)
        pos, yaw, pitch = self.camera
        p.update_camera(frm.Camera(pos, yaw, pitch))
        if self.neg_zero_x is not None:
            # origin.x = fma(1, m[3], fma(0, m[2], fma(0, m[1], 0 * m[0]))) is -0 only if every term
            # is: a camera mirrored in x (m[0] = -1) with -0 in the rest of the row. Its twin differs
            # in the sign of the translation's zero alone.
            m = p.raw.camera_matrix
            assert m[1] == 0.0 and m[2] == 0.0 and m[3] == 0.0
            m[0], m[1], m[2] = -1.0, -0.0, -0.0
            m[3] = -0.0 if self.neg_zero_x else 0.0
        return p


def _mb(name, w, h, **kw):
    kw.setdefault("iters", 12)
    return SchedCase(name, 18, kw.pop("iters"), kw.pop("time", P8), w, h, **kw)


FAMILIES = [
    _mb("mandelbulb_n12", 96, 54),
    _mb("mandelbulb_n0", 96, 54, iters=0),
    SchedCase("menger0_n5", 0, 5, 0.0, 96, 54),
    SchedCase("menger12_animated", 12, 5, 3.2175055, 96, 54),
    SchedCase("sierpinski_n6", 15, 6, 1.0, 96, 54),
    SchedCase("koch_n4", 16, 4, 1.0, 96, 54),
    SchedCase("sphere", 0, 5, 0.0, 96, 54, flags=frm.FRM_FLAG_SCENE_SPHERE),
]
# 96 x 54 (5184: a full rank block and a ragged one) is FAMILIES' size
SIZES = [_mb(f"size_{w}x{h}", w, h) for w, h in
         ((1, 1), (64, 1), (65, 63), (64, 64), (4097, 1), (127, 97), (130, 9))]
KEY_RANGE = [
    # more than the bailout radius (100) from the origin, looking away: every DE bails out at entry
    _mb("all_zero", 96, 54, camera=((0.0, 0.0, 150.0), 0.0, 0.0)),
    # the camera inside the power-9 set (edge_cases.DEEP_A), N = 200, 512 steps: every pixel hits
    # at step 0 and runs 5 DEs of 201 bodies (one key for the whole frame)
    _mb("inside_p9_n200", 32, 18, iters=200, time=edge_cases.P9_TIME, max_steps=512,
        camera=(edge_cases.DEEP_A, 0.0, 0.0)),
    # grazing rays at N = 200 creep for hundreds of steps of up to 201 bodies: some costs pass
    # sched_reference.SATURATED_COST and their keys saturate at 255, next to keys from 80 up
    _mb("saturating", 32, 18, iters=200, max_steps=1024),
    # inside the set at N = 13000: 5 DEs of 13001 bodies, every key 255
    _mb("all_saturated", 16, 9, iters=13000, time=edge_cases.P9_TIME, max_steps=512,
        camera=(edge_cases.DEEP_A, 0.0, 0.0)),
]
STEP0 = [
    _mb("max_steps_1", 33, 19, max_steps=1),   # step 0 ends the march: never skipped
    _mb("max_steps_2", 33, 19, max_steps=2),   # the smallest count with the shortcut
    SchedCase("menger_max_steps_2", 0, 5, 0.0, 33, 19, max_steps=2),
    _mb("hit_at_step0", 33, 19, camera=((0.3, 0.2, -0.5), 0.0, 0.0)),  # inside geometry: nothing skipped
    _mb("origin_neg_zero", 33, 19, neg_zero_x=True),    # the kernel runs step 0 per pixel
    _mb("origin_pos_zero", 33, 19, neg_zero_x=False),   # the same frame with the shortcut
]
SUPERSAMPLED = [_mb("supersampled_2", 48, 27, supersampling=2)]

CASES = FAMILIES + SIZES + KEY_RANGE + STEP0 + SUPERSAMPLED
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}

# batch of 3 poses: the keys and the order are those of the launch's last frame
BATCH_POSES = ("P0", "P2", "P1")
# two simulated ranks' interleaved bands: 6 bands of 8 rows, the last one 5 rows
BANDS = dict(width=80, height=45, band_rows=8, ranks=2)

_REFS = {}


def reference(oracle, case):
    """The oracle's frame of a case at its render size and its per-pixel costs (computed once per
    session; callers must not write to them)."""
    if case.name not in _REFS:
        w, h = case.render_size
        p = case.params()
        ref = oracle.render(p, w, h, case.max_steps, flags=case.flags)
        cost = oracle.render_costs(p, w, h, case.max_steps, flags=case.flags)
        for a in (ref["rgba"], ref["counters"], cost):
            a.setflags(write=False)
        _REFS[case.name] = {"rgba": ref["rgba"], "counters": ref["counters"], "cost": cost}
    return _REFS[case.name]


def band_rows_of(height, band_rows, first, stride):
    """The frame rows of a rank's interleaved bands, in its local order."""
    rows = []
    for b in range(first, (height + band_rows - 1) // band_rows, stride):
        rows += list(range(b * band_rows, min((b + 1) * band_rows, height)))
    return np.array(rows, dtype=np.uint32)
