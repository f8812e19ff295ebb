"""Points over all of float32 for the scene evaluators, shared by the CPU test
(test_scene_points.py) and the GPU test (test_gpu_scene_points.py). Nothing refuses a non-finite
or extreme camera, so points of any magnitude, subnormal, infinite or NaN reach Menger's repeat
(floor of huge values), Sierpinski's mirrors and i32 shifts, Koch's folds, the Mandelbulb body and
colorize. Plain data from fixed seeds."""
import numpy as np

import frm
from helpers import params_for

N_POINTS = 32768
SCENES = list(range(19)) + ["sphere"]
SETTINGS = ((0, 0.0), (3, 3.2175055), (12, 1.0))  # (N, time)
ORDERS = ("sorted", "shuffled")


def family(scene):
    if scene == "sphere":
        return "sphere"
    return "menger" if scene <= 14 else "sierpinski" if scene == 15 else "koch" if scene <= 17 else "mandelbulb"


def _stratified(rng, n):
    """n float32 with a random sign, a random one of the 256 exponent fields (0: zeros and
    subnormals, 255: inf and NaN) and a random mantissa that is zero for a fifth of them."""
    mant = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    mant[rng.random(n) < 0.2] = 0
    bits = (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)) | (rng.integers(0, 256, n, dtype=np.uint32) << np.uint32(23)) | mant
    return bits.view(np.float32)


_POINTS = {}


def points(order):
    """[32768, 3] float32. One half has all three coordinates stratified; the other two
    coordinates uniform in [-1.5, 1.5] and one (a random axis) stratified. "sorted": by the largest
    coordinate's encoding without its sign, so the lanes of a wave are alike; "shuffled": the same
    points in a seeded random order, so the Mandelbulb's wave-level tame test sees mixed waves."""
    if not _POINTS:
        rng = np.random.default_rng(32768)
        half = N_POINTS // 2
        a = _stratified(rng, 3 * half).reshape(half, 3)
        b = rng.uniform(-1.5, 1.5, (half, 3)).astype(np.float32)
        b[np.arange(half), rng.integers(0, 3, half)] = _stratified(rng, half)
        pts = np.concatenate([a, b])
        key = (pts.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=1)
        _POINTS["sorted"] = np.ascontiguousarray(pts[np.argsort(key, kind="stable")])
        _POINTS["shuffled"] = np.ascontiguousarray(pts[rng.permutation(N_POINTS)])
        for v in _POINTS.values():
            v.setflags(write=False)
    return _POINTS[order]


def flags_of(scene):
    return frm.FRM_FLAG_SCENE_SPHERE if scene == "sphere" else 0


def params_of(scene, iters, time):
    return params_for(0 if scene == "sphere" else scene, iters, time, 8, 8)


_REFS = {}


def reference(oracle, scene, iters, time, order):
    """The oracle's (distance, colour) on points(order) (evaluated once per session; callers must
    not write to them)."""
    key = (scene, iters, time, order)
    if key not in _REFS:
        d, col, _ = oracle.scene_de(params_of(scene, iters, time), points(order), flags=flags_of(scene))
        d.setflags(write=False)
        col.setflags(write=False)
        _REFS[key] = (d, col)
    return _REFS[key]


def differing(a, b):
    """Rows of a and b whose bits differ, NaN matching NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad = ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    return bad if bad.ndim == 1 else bad.any(axis=1)
