"""Cases, point sets and checks shared by tests/test_f64_reference.py (the CPU oracle) and
tests/test_gpu_f64_reference.py (the GPU): both are held to tests/f64_reference.py by the same rules.

Every tolerance here comes from the reference alone (its float32 run against its float64 run, its
own sensitivity to the input) or from the precision of float32; none was tuned to the code under
test. Each check returns the figures it measured; the callers print them before asserting.
"""
import math

import numpy as np

import f64_reference as ref
import frm
from helpers import params_for

U = 2.0 ** -24  # half an ulp of a float32 in [1, 2): the unit of the distance tables

TIME_POWER9 = 7.853981633974483  # sin(0.2 t) = 1: every animate_between(a, b) gives b
TIMES = (0.0, frm.POWER8_TIME, TIME_POWER9)
ITERATIONS = (0, 1, 3, 8)
SCENES = list(range(19)) + ["sphere"]
POINTS = 8192

HAND_POSE = ((0.4, 0.3, -1.3), 0.7, -0.3)  # position, yaw, pitch
POSES = {"P2": frm.POSES["P2"], "hand": HAND_POSE}
FRAME_SIZES = ((96, 72), (72, 96))
FRAME_STEPS = 256
# name -> (scene, num_iterations, time, sphere)
FRAME_SCENES = {
    "sphere": (0, 0, 0.0, True),
    "box": (0, 0, 0.0, False),
    "menger3": (0, 3, 0.0, False),
    "menger12-scale": (12, 3, 2.0, False),
    "sierpinski3": (15, 3, 0.0, False),
    "koch2": (17, 2, 1.5, False),
    "mandelbulb12": (18, 12, frm.POWER8_TIME, False),
    "mandelbulb5": (18, 5, 0.0, False),
}
MARCHED = ("sphere", "box", "menger3", "koch2", "sierpinski3")  # "nothing skipped" runs the float64 march
SHADOWED = ("sphere", "box")


def make_params(scene, iterations, time, width=8, height=8, pose=None):
    """(frm.Parameters, decoded blob, flags) of a case; scene "sphere" is the extension sphere."""
    sphere = scene == "sphere"
    p = params_for(0 if sphere else scene, iterations, time, width, height)
    if pose is not None:
        pos, yaw, pitch = POSES[pose] if isinstance(pose, str) else pose
        p.update_camera(frm.Camera(pos, yaw, pitch))
    return p, ref.decode(p.to_bytes()), (frm.FRM_FLAG_SCENE_SPHERE if sphere else 0)


def ulps32(a, b):
    """Distance in float32 encodings between float32 arrays (finite values)."""
    def key(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---- point sets ----------------------------------------------------------------------------------

def body_box(P, sphere):
    """A box in which the scene's iterations act: the unit cube for Menger (and the sphere), the
    bounding box of the four base vertices for Sierpinski and Koch, [-1.1, 1.1]^3 for the Mandelbulb."""
    fam = ref.scene_table(P, np.float64, sphere)["family"]
    if fam == ref.SIERPINSKI:
        g = ref.sierpinski_geometry(0)
        v = np.stack([g["top"], g["a"], g["b"], g["c"]]) - np.array([0.0, g["shift"], 0.0])
        return v.min(axis=0), v.max(axis=0)
    if fam == ref.KOCH:
        g = ref.koch_geometry(math.sqrt(3.0))
        v = np.stack([g["top"], g["left"], g["right"], g["back"], -g["top"]]) / 2.0  # p.y = |p.y|: both signs
        return v.min(axis=0), v.max(axis=0)
    if fam == ref.MANDELBULB:
        return np.full(3, -1.1), np.full(3, 1.1)
    return np.full(3, -0.5), np.full(3, 0.5)


def fold_planes(P, sphere):
    """(anchor, normal) of the planes the scene folds space about, in position space: the two
    outermost levels of Sierpinski mirrors, Koch's first pair (through the origin, in the swapped
    coordinates). Scenes without folds get two diagonal planes."""
    tab = ref.scene_table(P, np.float64, sphere)
    n = P["num_iterations"]
    planes = []
    if tab["family"] == ref.SIERPINSKI:
        g = ref.sierpinski_geometry(n)
        shift = np.array([0.0, g["shift"], 0.0])
        for i in range(n - 1, max(n - 3, -1), -1):
            for v, nrm in zip((g["a"], g["b"], g["c"]), g["normals"]):
                planes.append((g["top"] + ref.shl32(i) * (v - g["top"]) - shift, nrm))
    if tab["family"] == ref.KOCH and n > 0:
        g = ref.koch_geometry(tab["normal_z"])
        for nrm in (g["normal_1"], g["normal_2"]):
            planes.append((np.zeros(3), nrm[[1, 0, 2]]))
    if not planes:
        planes = [(np.zeros(3), np.array([1.0, 0.0, -1.0]) / math.sqrt(2)),
                  (np.zeros(3), np.array([0.0, 1.0, -1.0]) / math.sqrt(2))]
    return planes


def menger_last_level_points(P, sphere, rng, count):
    """Up to `count` points at which the last Menger iteration acts, found with the float64 reference
    alone. With a wide cross (1/3, 1/4) or a scale other than 3 the solid left after seven levels is
    dust (for cross 1/3 and scale 3, bars 8e-5 thick along the cube's edges), and uniform or plain
    grid points meet it too rarely for 50 of them to differ between N and N - 1. The pool: uniform
    points walked down the gradient of the distance at N - 1, and points on the cell edges (two
    coordinates on cell faces) of the scene's own grids, all jittered by up to a quarter of, or one,
    last-level cross size; the points of the pool whose distance differs between N and N - 1 are taken."""
    tab = ref.scene_table(P, np.float64, sphere)
    n = P["num_iterations"]
    cross, scale = float(tab["cross_size"]), float(tab["scale_factor"])
    de = lambda q, k: ref.menger_sponge(q, cross, scale, k)
    p = rng.uniform(-0.5, 0.5, (2048, 3))
    h = 1e-9
    for _ in range(12):
        d = de(p, n - 1)
        grad = np.stack([(de(p + h * e, n - 1) - de(p - h * e, n - 1)) / (2 * h) for e in np.eye(3)], axis=-1)
        p = p - d[:, None] * grad / np.maximum((grad * grad).sum(axis=1), 0.25)[:, None]
    m = 4096
    edges = rng.uniform(-0.5, 0.5, (m, 3))
    cell = scale ** -rng.integers(0, n, m).astype(np.float64)  # the cell size of a level 0 .. N - 1
    free = rng.integers(0, 3, m)
    for k in range(3):
        on = free != k
        edges[on, k] = ((np.round(edges[:, k] / cell + 0.5) - 0.5) * cell)[on]
    pool = np.concatenate([p, edges])
    reach = rng.choice([0.25, 1.0], (len(pool), 1))  # at a cube edge the box term gives way only past 1/8
    pool = pool + rng.uniform(-1, 1, pool.shape) * reach * cross / scale ** (n - 1)
    pool = pool.astype(np.float32).astype(np.float64)
    return pool[de(pool, n) != de(pool, n - 1)][:count]


def point_set(P, sphere, seed=0):
    """8192 float32 points: half uniform in the scene's body, a quarter uniform in [-1.5, 1.5]^3, a
    quarter structured (coordinate planes and axes, x = y, the fold planes, cell faces k / 3^j, and
    for the Menger scenes points at the surface of the level before the last)."""
    rng = np.random.default_rng([seed, P["scene_index"], int(sphere)])
    lo, hi = body_box(P, sphere)
    body = rng.uniform(lo, hi, (POINTS // 2, 3))
    cube = rng.uniform(-1.5, 1.5, (POINTS // 4, 3))
    g = POINTS // 32  # 8 groups of structured points
    s = rng.uniform(np.minimum(lo, -0.6), np.maximum(hi, 0.6), (8, g, 3))
    for k in range(3):
        s[0, k::3, k] = 0.0  # coordinate planes
        s[1, k::3, (k + 1) % 3] = 0.0  # axes
        s[1, k::3, (k + 2) % 3] = 0.0
    s[2, :, 1] = s[2, :, 0]  # x = y
    planes = fold_planes(P, sphere)
    for j in range(g):  # fold planes: project in float64, the float32 rounding leaves them within half an ulp
        for grp in (3, 4, 5):
            a, nrm = planes[(j + grp) % len(planes)]
            s[grp, j] = s[grp, j] - np.dot(s[grp, j] - a, nrm) * nrm
    for grp, level in ((6, 1), (7, 3)):  # cell faces of the unit cube at 3^-1 .. 3^-level, one coordinate each
        j = rng.integers(1, level + 1, g)
        k = rng.integers(0, 3 ** j + 1)
        s[grp, np.arange(g), rng.integers(0, 3, g)] = k / 3.0 ** j - 0.5
    s = s.reshape(-1, 3)
    pts = np.concatenate([body, cube, s]).astype(np.float32)
    n = P["num_iterations"]
    if ref.scene_table(P, np.float64, sphere)["family"] == ref.MENGER and n > 0:
        moved = ref.scene_distance(P, pts, np.float64) != ref.scene_distance(P, pts, np.float64, iterations=n - 1)
        if moved.sum() < 100:  # the coverage rule asks for 50
            extra = menger_last_level_points(P, sphere, rng, g).astype(np.float32)
            at = POINTS * 3 // 4 + g // 2  # in place of half the coordinate-plane and half the axis points
            pts[at:at + len(extra)] = extra
    assert pts.shape == (POINTS, 3)
    return pts


# ---- distances -----------------------------------------------------------------------------------

def distance_reference(P, sphere, pts):
    """Everything section 3 needs from the reference alone for one case."""
    fam = ref.scene_table(P, np.float64, sphere)["family"]
    n = P["num_iterations"]
    R = {"family": fam, "n": n}
    if fam == ref.MANDELBULB:
        tab64 = ref.scene_table(P, np.float64)
        p64 = pts.astype(np.float64)
        d64, bodies, margin = ref.mandelbulb(p64, tab64["power"], n)
        d32 = ref.scene_distance(P, pts, np.float32).astype(np.float64)
        cond = np.zeros(len(pts))
        with np.errstate(all="ignore"):
            for k in range(3):
                for sign in (-1.0, 1.0):
                    q = p64.copy()
                    q[:, k] += sign * 2.0 ** -22
                    cond = np.fmax(cond, np.abs(ref.mandelbulb(q, tab64["power"], n)[0] - d64))
            tol = 4.0 * cond + 64.0 * U * np.abs(d64)
            keep = (tol <= 1e-3 * np.abs(d64)) & (margin >= 1e-5) & np.isfinite(d64)
            R.update(ref64=d64, ref32=d32, tol=tol, keep=keep, full=float(np.mean(bodies == n + 1)),
                     omitted=float(1.0 - keep.mean()),
                     ref32_median=float(np.median((np.abs(d32 - d64) / np.abs(d64))[keep])))
        return R
    d64 = ref.scene_distance(P, pts, np.float64, sphere)
    d32 = ref.scene_distance(P, pts, np.float32, sphere).astype(np.float64)
    yard = float(np.max(np.abs(d32 - d64)))
    R.update(ref64=d64, ref32=d32, yard=yard, tol=4.0 * yard + 4.0 * U * max(1.0, float(np.max(np.abs(d64)))))
    if fam != ref.SPHERE and n > 0:
        R["moved"] = int(np.sum(d64 != ref.scene_distance(P, pts, np.float64, sphere, iterations=n - 1)))
    return R


_cases = {}


def distance_case(scene, iterations, time):
    """(parameters, flags, points, distance_reference) of one section-3 case, computed once. Scenes
    that do not read the time share one entry."""
    p, P, flags = make_params(scene, iterations, time)
    sphere = scene == "sphere"
    tab = ref.scene_table(P, np.float64, sphere)
    key = (scene, iterations) + tuple(float(tab[k]) for k in sorted(tab) if k != "family")
    if key not in _cases:
        pts = point_set(P, sphere)
        pts.setflags(write=False)
        _cases[key] = (pts, distance_reference(P, sphere, pts))
    return (p, P, flags) + _cases[key]


def assert_coverage(R):
    """The point set reaches the iterations: asserted from the reference alone."""
    if R["family"] == ref.MANDELBULB:
        assert R["full"] >= 0.05, f"only {R['full']:.3f} of the points run all {R['n'] + 1} bodies"
        assert R["omitted"] <= 0.05, f"the reference omits {R['omitted']:.3f} of the points"
    elif "moved" in R:
        assert R["moved"] >= 50, f"only {R['moved']} points differ between N = {R['n']} and N - 1"


def check_distances(got, R, label):
    """Section 3's rule for one case -> the measured figures; raises AssertionError beyond it."""
    got = np.asarray(got).astype(np.float64)
    if R["family"] != ref.MANDELBULB:
        err = float(np.max(np.abs(got - R["ref64"])))
        fig = {"yard_u": R["yard"] / U, "err_u": err / U, "tol_u": R["tol"] / U}
        assert err <= R["tol"], f"{label}: {fig}"
        return fig
    k = R["keep"]
    with np.errstate(all="ignore"):
        e = np.abs(got - R["ref64"])[k]
        rel = e / np.abs(R["ref64"][k])
    beyond = float(np.mean(~(e <= R["tol"][k])))
    fig = {"omitted": R["omitted"], "beyond": beyond, "median_rel": float(np.median(rel)),
           "ref32_median_rel": R["ref32_median"], "worst_over_tol": float(np.nanmax(e / R["tol"][k]))}
    assert beyond <= 1e-3, f"{label}: {fig}"
    assert fig["median_rel"] < 4.0 * R["ref32_median"], f"{label}: {fig}"
    return fig


def check_colors(got, P, sphere, pts, label):
    """The colour against the float64 one, within 1 float32 ulp. The ulp is taken at the larger of
    the sum and its summands (0.5 and the position, times 1.5 for Sierpinski): the sum cancels near
    colour 0, where float32's own rounding of 1.5 * position (half an ulp of a number near 0.75,
    3e-8) is thousands of ulps of the result; the reference's float32 run shows the same."""
    want = ref.scene_color(P, pts, np.float64, sphere)
    k = 1.5 if ref.scene_table(P, np.float64, sphere)["family"] == ref.SIERPINSKI else 1.0
    scale = np.maximum(np.maximum(np.abs(want), np.abs(k * pts.astype(np.float64))), 0.5)
    unit = np.spacing(scale.astype(np.float32)).astype(np.float64)
    own = float(np.max(np.abs(ref.scene_color(P, pts, np.float32, sphere) - want) / unit))
    worst = float(np.max(np.abs(np.asarray(got).astype(np.float64) - want) / unit))
    assert worst <= 1.0, f"{label}: colour {worst:.2f} ulp from the float64 value (the float32 reference: {own:.2f})"
    return worst


# ---- frames --------------------------------------------------------------------------------------

_frame_refs = {}


def frame_reference(name, pose, width, height):
    """The float64 side of one frame, computed once: parameters, rays, and for MARCHED scenes the
    float64 march of every pixel plus the same march of the scene shrunk by 1e-4."""
    key = (name, pose, width, height)
    if key not in _frame_refs:
        scene, n, time, sphere = FRAME_SCENES[name]
        p, P, flags = make_params("sphere" if sphere else scene, n, time, width, height, pose)
        origin, dirs = ref.camera_rays(P, width, height)
        F = {"name": name, "pose": pose, "params": p, "P": P, "flags": flags, "sphere": sphere, "origin": origin, "dirs": dirs,
             "family": ref.scene_table(P, np.float64, sphere)["family"], "width": width, "height": height}
        if name in MARCHED:
            m = ref.march(P, origin, dirs, FRAME_STEPS, np.float64, sphere)
            inner = ref.march(P, origin, dirs, FRAME_STEPS, np.float64, sphere, erode=1e-4)
            # A ray that hits comes within 1e-4 of the threshold by definition, so its margin is taken
            # on the other side: it still hits the scene shrunk by 1e-4. A ray that misses is firm
            # when the smallest distance it met stays 1e-4 above the threshold.
            F["march"] = m
            F["firm_hit"] = inner["hit"] & m["hit"]
            F["firm_miss"] = ~m["hit"] & ~(m["min_d"] <= ref.MIN_DISTANCE + 1e-4)
        for v in F.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _frame_refs[key] = F
    return _frame_refs[key]


def analytic_hits(F, grow):
    """Whether each ray meets the sphere of radius 0.5 + grow / the cube of half side 0.5 + grow."""
    o, d = F["origin"], F["dirs"]
    r = 0.5 + grow
    if F["sphere"]:
        b = d @ o
        disc = b * b - (o @ o - r * r)
        return (disc > 0) & (-b + np.sqrt(np.maximum(disc, 0)) > 0)
    with np.errstate(all="ignore"):
        t1, t2 = (-r - o) / d, (r - o) / d
    near = np.minimum(t1, t2).max(axis=1)
    far = np.maximum(t1, t2).min(axis=1)
    return (near < far) & (far > 0)


def hit_points(F, trace):
    """(pixel indices, positions) of the hit pixels whose object colour gives the position back:
    all three components below 1; p = colour - 0.5, or (colour - 0.5) / 1.5 for Sierpinski."""
    tr = trace.reshape(-1, 10).astype(np.float64)
    hit = tr[:, 0] != 0
    usable = hit & (tr[:, 7:10] < 1.0).all(axis=1)
    idx = np.nonzero(usable)[0]
    p = tr[idx, 7:10] - 0.5
    if F["family"] == ref.SIERPINSKI:
        p = p / 1.5
    return hit, idx, p


def surface_tolerance(F, p):
    """The distance tolerance of section 3 for the frame's scene at the hit points, plus
    3 * 2^-24 * |p| for the position read back from the colour. -> (tol per point, kept mask)."""
    P, sphere = F["P"], F["sphere"]
    back = 3.0 * U * np.linalg.norm(p, axis=1)
    if F["family"] != ref.MANDELBULB:
        scene, n, time, _ = FRAME_SCENES[F["name"]]
        R = distance_case("sphere" if sphere else scene, n, time)[4]
        return R["tol"] + back, np.ones(len(p), bool)
    tab = ref.scene_table(P, np.float64)
    n = P["num_iterations"]
    d64, _, margin = ref.mandelbulb(p, tab["power"], n)
    cond = np.zeros(len(p))
    with np.errstate(all="ignore"):
        for k in range(3):
            for sign in (-1.0, 1.0):
                q = p.copy()
                q[:, k] += sign * 2.0 ** -22
                cond = np.fmax(cond, np.abs(ref.mandelbulb(q, tab["power"], n)[0] - d64))
    tol = 4.0 * cond + 64.0 * U * np.abs(d64) + back
    # The distance rule leaves a point out when tol > 1e-3 |ref64|. On the surface |ref64| <= 5e-7
    # while a move of 2^-22 changes a distance by about 2.4e-7, so that rule would leave every hit
    # out. Here the tolerance is used as an absolute one at every point (a large one makes the check
    # weak there, never wrong), only points whose bailout margin is below 1e-5 are left out, and
    # check_frame asserts that half the points are held to within four thresholds.
    keep = (margin >= 1e-5) & np.isfinite(tol)
    return tol, keep


def check_frame(F, rgba, trace, label, bytes_only=False):
    """Section 4 for one frame: rgba [H, W, 4] uint8 and the trace [H, W, 10] of the same parameters.
    bytes_only: the trace belongs to another kernel's frame of the same parameters, so only the byte
    checks apply. -> figures; raises AssertionError beyond a rule."""
    P, sphere, name = F["P"], F["sphere"], F["name"]
    W, H = F["width"], F["height"]
    rgba = np.asarray(rgba).reshape(-1, 4)
    tr = np.asarray(trace).reshape(-1, 10)
    hit, idx, p = hit_points(F, tr)
    fig = {"hits": int(hit.sum()), "usable": len(idx) / max(1, int(hit.sum()))}

    # shading: the trace shaded in float64 gives the frame's bytes
    want = np.zeros((W * H, 4), np.uint8)
    want[:, 3] = 255
    h = np.nonzero(hit)[0]
    t64 = tr[h].astype(np.float64)
    col = ref.shade(t64[:, 7:10], t64[:, 1], t64[:, 2:5], t64[:, 5] != 0, t64[:, 6], F["dirs"][h], FRAME_STEPS)
    nan = np.isnan(col).any(axis=1)
    col[nan] = np.nan
    want[h, :3] = ref.encode(col)
    s = ref.srgb_scaled(col)
    tie = np.zeros((W * H, 3), bool)
    with np.errstate(all="ignore"):
        tie[h] = np.abs(s - np.floor(s) - 0.5) <= 0.01
    diff = np.abs(rgba[:, :3].astype(int) - want[:, :3].astype(int))
    fig["nan_pixels"] = int(nan.sum())
    fig["channels_off"] = int((diff != 0).sum())
    fig["tie_share"] = float(tie[h].mean()) if len(h) else 0.0
    assert (rgba[:, 3] == 255).all(), f"{label}: alpha"
    assert (rgba[~hit][:, :3] == 0).all(), f"{label}: a miss pixel is not black"
    assert (rgba[h[nan]][:, :3] == 0).all(), f"{label}: a NaN pixel is not black"
    assert (diff <= np.where(tie, 1, 0)).all(), f"{label}: {int((diff > np.where(tie, 1, 0)).sum())} channels off, {fig}"
    assert fig["tie_share"] <= 0.05, f"{label}: {fig}"
    if bytes_only:
        return fig

    # A quarter of the hits must give their position back. How many do is the geometry of scene and
    # pose alone (a colour component saturates where a coordinate reaches 0.5, and P2 looks at the
    # +x and +y sides): for the 12-iteration Mandelbulb at P2 the float64 march of the reference
    # itself hits 954 pixels of which 231 (24.2 %) are usable, at both frame sizes; that frame asks
    # for a fifth. A frame without hits (the hand-made pose sees little of the tetrahedra in
    # portrait) still goes through the byte checks above and the hit-mask check below.
    need = 0.20 if (name, F["pose"]) == ("mandelbulb12", "P2") else 0.25
    assert fig["hits"] == 0 or fig["usable"] >= need, f"{label}: {fig}"
    if len(idx) == 0:
        assert name in MARCHED
        assert not F["firm_hit"].any(), f"{label}: no hits, but the float64 march has firm ones"
        return fig

    # on the ray
    o, d = F["origin"], F["dirs"][idx]
    t = ((p - o) * d).sum(axis=1) / (d * d).sum(axis=1)
    off = np.linalg.norm(p - (o + t[:, None] * d), axis=1) / (U * np.maximum(t, 1.0))
    fig["ray_ulp"] = float(off.max())
    assert fig["ray_ulp"] <= 8.0, f"{label}: {fig}"

    # on the surface
    tol, keep = surface_tolerance(F, p)
    d64 = ref.scene_distance(P, p, np.float64, sphere)
    fig["surface_omitted"] = float(1.0 - keep.mean())
    fig["de_min"], fig["de_max"] = float(d64[keep].min()), float(d64[keep].max())
    fig["surface_tol"] = float(np.median(tol[keep]))
    bad = keep & ~(d64 <= ref.MIN_DISTANCE + tol)
    if F["family"] == ref.MANDELBULB:
        # No lower bound: the Mandelbulb's estimate is no bound on the distance, so a march can step
        # over the surface and end inside, at a negative distance. The reference's own float32
        # distance is below -tol at the same 0.3 % to 4 % of these points as its float64 one.
        fig["inside"] = float(np.mean(d64[keep] < -tol[keep]))
        assert fig["surface_tol"] <= 4.0 * ref.MIN_DISTANCE, f"{label}: {fig}"
    else:
        bad |= keep & ~(d64 >= -tol)
    assert fig["surface_omitted"] <= 0.05, f"{label}: {fig}"
    assert not bad.any(), f"{label}: {int(bad.sum())} hit points off the surface, {fig}"

    # nothing skipped
    if name in MARCHED:
        out = ~(F["firm_hit"] | F["firm_miss"])
        fig["march_left_out"] = float(out.mean())
        assert fig["march_left_out"] <= 0.05, f"{label}: {fig}"
        wrong = ~out & (hit != F["march"]["hit"])
        assert not wrong.any(), f"{label}: {int(wrong.sum())} pixels hit where the float64 march misses or the reverse"
        if name in ("sphere", "box"):
            must, may = analytic_hits(F, -1e-4), analytic_hits(F, 1e-4)
            assert np.mean(may & ~must) <= 0.05
            assert hit[must].all() and not hit[~may].any(), f"{label}: hit mask against the analytic intersection"

    # normal
    n = tr[idx, 2:5].astype(np.float64)
    n64 = ref.normal(P, p, np.float64, sphere)
    n32 = ref.normal(P, p, np.float32, sphere).astype(np.float64)
    with np.errstate(all="ignore"):
        own = float(np.mean(~((n32 * n64).sum(axis=1) > 0.9)))
        got = float(np.mean(~((n * n64).sum(axis=1) > 0.9)))
    fig["normal_fail"], fig["normal_fail_ref32"] = got, own
    # The unit length holds where float32 can square the summed taps: deep in the Mandelbulb the
    # distance is below 1e-19, the squares fall under 2^-126 and lose their low bits (up to 23 units
    # measured on the oracle at such pixels, 1.9 elsewhere). Those points, told by the float64 taps
    # (length below 2^-60), are left out: 1.3 % and 4.6 % of the usable hits of the two poses by the
    # reference alone; there may be at most 10 % of them.
    taps = sum(np.array(k, np.float64) * ref.scene_distance(P, p + np.array(k) * ref.MIN_DISTANCE, np.float64, sphere)[:, None]
               for k in ref.TAPS)
    sound = np.isfinite(n).all(axis=1) & (np.linalg.norm(taps, axis=1) >= 2.0 ** -60)
    fig["normal_len_u"] = float(np.max(np.abs(np.linalg.norm(n[sound], axis=1) - 1.0)) / U)
    fig["normal_underflow"] = float(np.mean(np.linalg.norm(taps, axis=1) < 2.0 ** -60))
    assert fig["normal_underflow"] <= 0.10, f"{label}: {fig}"
    assert fig["normal_len_u"] <= 4.0, f"{label}: {fig}"
    assert got <= 2.0 * own + 0.01, f"{label}: {fig}"

    # shadow
    if name in SHADOWED:
        sun = ref.march(P, ref.shadow_start(p, n), np.broadcast_to(ref.to_sun(), p.shape), FRAME_STEPS, np.float64, sphere)
        lit = np.abs(n @ ref.to_sun()) >= 0.02
        got_hit = tr[idx, 5] != 0
        fig["shadow_kept"] = float(lit.mean())
        assert np.array_equal(got_hit[lit], sun["hit"][lit]), \
            f"{label}: {int((got_hit != sun['hit'])[lit].sum())} sun rays differ from the float64 shadow march"
        # the closeness enters the colour only where the sun ray missed (a hit multiplies it by 0)
        both = lit & ~got_hit & ~sun["hit"]
        c, c64 = tr[idx, 6].astype(np.float64)[both], sun["closeness"][both]
        fig["closeness_rel"] = float(np.max(np.abs(c - c64) / np.abs(c64))) if both.any() else 0.0
        assert fig["closeness_rel"] <= 1e-3, f"{label}: {fig}"
    return fig
