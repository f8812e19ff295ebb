"""tests/f64_reference.py pinned by definitions that share nothing with it, then the CPU oracle
(oracle/frm_oracle.c, both math modes) held to it: distances, colours and the scene table on point
sets that reach the iterations, and whole frames through invariants that do not care which path a
march took (tests/f64_cases.py has the rules). tests/test_gpu_f64_reference.py applies the same
rules to the GPU.

The oracle, frm_scene.h and frm_host.cpp were transcribed from one shader by one hand; the
reference here is a second, independent statement of the same mathematics, so a slip shared by
those three no longer passes. Each of these one-line edits of the oracle was tried and fails here:
scene 1's cross size 1/5 -> 1/6 (test_oracle_distances[1], test_oracle_scene_table), Koch's two
mirrors swapped (test_oracle_distances[17]; at normal_z = sqrt(3) the planes meet at 60 degrees and
the two folds commute, so scene 16 cannot see it), taps 1 and 2 of the normal exchanged
(test_oracle_frames, from the sphere on: the normal), the camera matrix read transposed
(test_oracle_frames: on the ray), SHADOW_FACTOR 0.7 -> 0.75 (test_oracle_frames: the shading, from
Menger N = 3 on; both poses look at the lit side of the sphere and the box).
"""
import math
import os
import sys

import numpy as np
import pytest

import f64_cases as fc
import f64_reference as ref
import frm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64, f32 = np.float64, np.float32


def blob(scene, iterations, time=0.0, width=8, height=8, pose=None):
    return fc.make_params(scene, iterations, time, width, height, pose)[1]


# ---- 2. the reference's own pins -----------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 4])
def test_menger_is_the_ternary_digit_rule(n):
    """Scene 0: a point of the unit cube is in the sponge (d <= 0) exactly when at no level 1..N two
    of its three base-3 digits equal 1."""
    rng = np.random.default_rng(n)
    u = rng.uniform(0.0, 1.0, (20000, 3))
    solid = np.ones(len(u), bool)
    clear = np.ones(len(u), bool)
    for level in range(1, n + 1):
        x = u * 3.0 ** level
        digit = np.floor(x).astype(np.int64) % 3
        solid &= (digit == 1).sum(axis=1) < 2
        clear &= (np.abs(x - np.round(x)) > 1e-9 * 3.0 ** level).all(axis=1)
    assert clear.mean() > 0.99
    d = ref.scene_distance(blob(0, n), u - 0.5, f64)
    assert np.array_equal(d[clear] <= 0.0, solid[clear])
    assert 0.3 < solid.mean() < 0.8  # (20/27)^N


def test_box_closed_form():
    pts = np.array([[1, 0, 0], [0, 0, 0], [1, 1, 1], [0.25, 0.1, -0.3], [0, 2, 0]], f64)
    d = ref.scene_distance(blob(0, 0), pts, f64)
    assert np.allclose(d, [0.5, -0.5, math.sqrt(0.75), -0.2, 1.5], rtol=0, atol=1e-15)
    assert np.allclose(ref.scene_color(blob(0, 0), pts[1:2], f64), 0.5)
    assert np.array_equal(ref.scene_color(blob(0, 0), pts[4:5], f64), [[0.5, 1.0, 0.5]])
    assert ref.scene_distance(blob(0, 1), np.zeros((1, 3)), f64)[0] == pytest.approx(1 / 6, abs=1e-16)


def test_sphere_closed_form():
    pts = np.random.default_rng(3).uniform(-2, 2, (1000, 3))
    d = ref.scene_distance(blob("sphere", 0), pts, f64, sphere_scene=True)
    assert np.max(np.abs(d - (np.linalg.norm(pts, axis=1) - 0.5))) < 1e-15


def _tetrahedron(q, top, a, b, c):
    def pn(a, b, c):
        n = np.cross(c - a, b - a)
        return n / np.linalg.norm(n)
    planes = [(top, pn(top, a, b)), (top, pn(top, b, c)), (top, pn(top, c, a)), (a, pn(a, c, b))]
    return np.max([(q - an) @ n for an, n in planes], axis=0)


def test_sierpinski_n0_is_one_tetrahedron():
    h = 4 / math.sqrt(6)
    top = np.array([0, h * 0.5, 0])
    a = top + 0.5 * np.array([-1, -h, -1 / math.sqrt(3)])
    b = top + 0.5 * np.array([1, -h, -1 / math.sqrt(3)])
    c = top + 0.5 * np.array([0, -h, 2 / math.sqrt(3)])
    pts = np.random.default_rng(5).uniform(-1, 1, (2000, 3))
    want = _tetrahedron(pts + np.array([0, h * 0.25, 0]), top, a, b, c)
    assert np.max(np.abs(ref.scene_distance(blob(15, 0), pts, f64) - want)) < 1e-14
    assert np.allclose(ref.scene_color(blob(15, 0), pts, f64), np.minimum(1.0, 1.5 * pts + 0.5))


def test_sierpinski_shift_is_32_bit():
    assert [ref.shl32(k) for k in (0, 5, 31, 32, 33)] == [1, 32, -2 ** 31, 1, 2]


def test_koch_n0_is_half_the_plain_tetrahedron():
    off = math.sqrt(9 - 2.25) - math.sqrt(3)
    top, left = np.array([0.0, 1, 0]), np.array([-1.5, 0, -off])
    right, back = np.array([1.5, 0, -off]), np.array([0, 0, math.sqrt(3)])
    pts = np.random.default_rng(6).uniform(-1.5, 1.5, (2000, 3))
    q = 2.0 * pts
    q[:, 1] = np.abs(q[:, 1])
    want = _tetrahedron(q, top, left, right, back) / 2.0
    for scene in (16, 17):
        assert np.max(np.abs(ref.scene_distance(blob(scene, 0), pts, f64) - want)) < 1e-14


def test_mandelbulb_against_mpmath():
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(8)
    pts = rng.uniform(-1.1, 1.1, (200, 3)).astype(f32).astype(f64)
    for n, time in ((3, frm.POWER8_TIME), (8, 0.0)):
        P = blob(18, n, time)
        d, bodies, margin = ref.mandelbulb(pts, ref.scene_table(P)["power"], n)
        power = 4 + 5 * (mp.mpf("0.5") + mp.mpf("0.5") * mp.sin(mp.mpf(P["time"]) * mp.mpf(0.2)))
        checked = 0
        for p, got, ran, room in zip(pts, d, bodies, margin):
            z = [mp.mpf(float(v)) for v in p]
            dr, r, count = mp.mpf(1), mp.mpf(0), 0
            for _ in range(n + 1):
                r = mp.sqrt(z[0] ** 2 + z[1] ** 2 + z[2] ** 2)
                if r > 100:
                    break
                theta, phi = mp.acos(z[2] / r), mp.atan2(z[1], z[0])
                dr = r ** (power - 1) * power * dr + 1
                zr = r ** power
                z = [zr * mp.sin(theta * power) * mp.cos(phi * power) + mp.mpf(float(p[0])),
                     zr * mp.sin(phi * power) * mp.sin(theta * power) + mp.mpf(float(p[1])),
                     zr * mp.cos(theta * power) + mp.mpf(float(p[2]))]
                count += 1
            want = mp.mpf("0.5") * mp.log(r) * r / dr
            assert count == ran
            # float64 carries the chaos of the iteration too: where 2^-22 moves change the distance by
            # more than a thousandth of it (or the bailout nearly flips) 1e-12 cannot hold
            cond = max(abs(ref.mandelbulb((p + e)[None], ref.scene_table(P)["power"], n)[0][0] - got)
                       for e in 2.0 ** -22 * np.concatenate([np.eye(3), -np.eye(3)]))
            if room < 1e-5 or cond > 1e-3 * abs(got):
                continue
            checked += 1
            assert abs(mp.mpf(float(got)) - want) <= mp.mpf("1e-12") * abs(want), (p, got, want)
        assert checked >= 180


POSES = [fc.POSES["P2"], fc.HAND_POSE]


def _rotation(yaw, pitch):
    ry = np.array([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]])
    rx = np.array([[1, 0, 0], [0, math.cos(pitch), -math.sin(pitch)], [0, math.sin(pitch), math.cos(pitch)]])
    return ry @ rx


@pytest.mark.parametrize("pose", POSES, ids=["P2", "hand"])
@pytest.mark.parametrize("size", fc.FRAME_SIZES)
def test_camera_against_a_rebuilt_matrix(pose, size):
    """T(position) Ry(yaw) Rx(pitch) rebuilt here in float64: the blob holds it, the ray origin is its
    translation, the centre ray its rotated +z axis, and the corner rays lean to the side and the
    height of their corner (x grows to the right, y upwards, row 0 is the top)."""
    w, h = size
    pos, yaw, pitch = pose
    P = blob(18, 3, 0.0, w, h, pose)
    R = _rotation(yaw, pitch)
    M = np.array(P["matrix"]).reshape(4, 4)
    assert np.allclose(M[:3, :3], R, atol=2e-7) and np.allclose(M[:3, 3], pos, atol=2e-7)
    assert np.allclose(P["aspect_scale"], (w / min(w, h), h / min(w, h)), atol=1e-7)
    origin, dirs = ref.camera_rays(P, w, h)
    dirs = dirs.reshape(h, w, 3)
    assert np.allclose(origin, pos, atol=2e-7)
    centre = dirs[h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1].mean(axis=(0, 1))
    assert np.allclose(centre / np.linalg.norm(centre), R @ [0, 0, 1], atol=1e-6)
    right, up, forward = R @ [1, 0, 0], R @ [0, 1, 0], R @ [0, 0, 1]
    z = 1 / math.atan(math.pi / 2)
    for (y, x), (sx, sy) in {(0, 0): (-1, 1), (0, w - 1): (1, 1), (h - 1, 0): (-1, -1), (h - 1, w - 1): (1, -1)}.items():
        d = dirs[y, x]
        assert np.sign(d @ right) == sx and np.sign(d @ up) == sy and d @ forward > 0
        ex = np.array([sx * (1 - 1 / w) * w / min(w, h), sy * (1 - 1 / h) * h / min(w, h), z])
        assert np.allclose([d @ right, d @ up, d @ forward], ex / np.linalg.norm(ex), atol=1e-6)


def test_store_against_the_threshold_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_srgb_table
    t = np.array(gen_srgb_table.thresholds()[1:], f64)
    c = np.random.default_rng(1).uniform(-0.1, 1.1, 10000).astype(f32)
    c[:6] = [0, 1, 0.5, 0.0031308, -1, 2]
    want = np.searchsorted(t, c.astype(f64), side="right")
    s = ref.srgb_scaled(c)
    away = np.abs(s - np.floor(s) - 0.5) > 1e-9
    assert away.mean() > 0.999 and np.array_equal(ref.encode(c)[away], want[away])
    assert list(ref.encode(np.array([np.nan, 0.5, 0.2]))) == [0, 188, 124]


def test_reference_frame_of_the_sphere():
    """render() end to end on the analytic scene: lit exactly where the ray meets the sphere (away
    from the rim), black elsewhere, float32 and float64 within one code on nearly every channel."""
    w, h = 48, 36
    P = blob("sphere", 0, 0.0, w, h, "hand")
    a = ref.render(P, w, h, 256, f64, sphere_scene=True)
    b = ref.render(P, w, h, 256, f32, sphere_scene=True)
    origin, dirs = ref.camera_rays(P, w, h)
    F = {"origin": origin, "dirs": dirs, "sphere": True}
    lit = a[..., :3].any(axis=2).ravel()
    assert lit[fc.analytic_hits(F, -1e-4)].all() and not lit[~fc.analytic_hits(F, 1e-4)].any()
    assert 100 < lit.sum() < w * h / 2 and (a[..., 3] == 255).all()
    assert np.mean(np.abs(a.astype(int) - b.astype(int)) <= 1) > 0.95  # float32 moves the shadow edge


# ---- 3. the oracle against the reference ------------------------------------------------------------

@pytest.mark.parametrize("scene", fc.SCENES)
def test_oracle_distances(oracle, scene):
    sphere = scene == "sphere"
    for n in fc.ITERATIONS:
        for time in fc.TIMES:
            p, P, flags, pts, R = fc.distance_case(scene, n, time)
            fc.assert_coverage(R)
            for mode in (oracle.MODE_FRM, oracle.MODE_LIBM):
                label = f"scene {scene} N={n} t={time} mode={mode}"
                d, col, _ = oracle.scene_de(p, pts, flags=flags, mode=mode)
                fig = fc.check_distances(d, R, label)
                worst = fc.check_colors(col, P, sphere, pts, label)
                print(label, {k: float(f"{v:.3g}") for k, v in fig.items()}, "colour ulp", round(worst, 2))


def test_oracle_scene_table(oracle):
    keys = {"power": "mb_power", "cross_size": "menger_cross", "scale_factor": "menger_scale", "normal_z": "koch_normal_z"}
    family = {ref.MENGER: 0, ref.SIERPINSKI: 1, ref.KOCH: 2, ref.MANDELBULB: 3, ref.SPHERE: 4}
    for scene in fc.SCENES + [19, 1000, 2 ** 32 - 1]:
        for time in fc.TIMES + (1.0, 20.0):
            p, P, flags = fc.make_params(scene, 3, time)
            tab = ref.scene_table(P, f64, scene == "sphere")
            for mode in (oracle.MODE_FRM, oracle.MODE_LIBM):
                info = oracle.frame_info(p, flags=flags, mode=mode)
                assert info["family"] == family[tab["family"]], (scene, time)
                for k, name in keys.items():
                    if k in tab:
                        off = int(fc.ulps32(f32(info[name]), f32(tab[k])))
                        assert off <= 2, (scene, time, mode, k, info[name], float(tab[k]))
    assert ref.scene_table(blob(18, 3, frm.POWER8_TIME))["power"] == pytest.approx(8.0, abs=1e-6)


# ---- 4. whole frames ----------------------------------------------------------------------------------

@pytest.mark.parametrize("pose", list(fc.POSES))
@pytest.mark.parametrize("name", list(fc.FRAME_SCENES))
def test_oracle_frames(oracle, name, pose):
    for w, h in fc.FRAME_SIZES:
        F = fc.frame_reference(name, pose, w, h)
        r = oracle.render(F["params"], w, h, fc.FRAME_STEPS, flags=F["flags"], trace=True)
        fig = fc.check_frame(F, r["rgba"], r["trace"], f"{name} {pose} {w}x{h}")
        print(name, pose, f"{w}x{h}", {k: float(f"{v:.3g}") for k, v in fig.items()})
