"""The renderer's operation restated in plain numpy, from the mathematics of the reference shader
(src/fragment.wgsl, src/vertex.wgsl, src/parameters.rs) in this file's own words.

It shares nothing with oracle/frm_oracle.c, frm_scene.h or frm_host.cpp: nothing is imported from
`oracle` or `frm`, nothing is loaded through ctypes, and its only input is the 96-byte `Parameters`
blob (decoded here) plus the frame size and the step limit. Every function takes a `dtype`:
float64 is the reference; float32 is the same code in single precision, the yardstick of how much
rounding alone moves a result. Vectorised over points [n, 3] and pixels.

tests/test_f64_reference.py pins this file with definitions that share nothing with it (ternary
digits, closed forms, mpmath, a rebuilt camera matrix), then holds the oracle to it;
tests/test_gpu_f64_reference.py holds the GPU to it.
"""
import math
import struct

import numpy as np

F64 = np.float64
F32 = np.float32

MAX_TOTAL_DISTANCE = 1.0e3
MIN_DISTANCE = 5.0e-7
INFINITY = 1.0e20
SUN_DIRECTION = (-1.0, -0.5, 1.0)
SHADOW_FACTOR = 0.7
SHADOW_SHARPNESS = 32.0
SPECULAR_FACTOR = 0.15
SPECULAR_SHARPNESS = 16.0
AMBIENT_OCCLUSION_FACTOR = 0.2
AMBIENT_OCCLUSION_SHARPNESS = 100.0
BAILOUT = 100.0
NUM_SCENES = 19

MENGER, SIERPINSKI, KOCH, MANDELBULB, SPHERE = "menger", "sierpinski", "koch", "mandelbulb", "sphere"


# ---- the uniform -------------------------------------------------------------------------------

def decode(blob):
    """The 96-byte Parameters: 16 f32 matrix entries, 2 f32 aspect scales, f32 time, u32 iteration
    count, u32 scene index, 12 bytes of padding."""
    blob = bytes(blob)
    assert len(blob) == 96
    v = struct.unpack("<16f2ffII12x", blob)
    return {"matrix": v[0:16], "aspect_scale": v[16:18], "time": v[18], "num_iterations": v[19], "scene_index": v[20]}


def _vec(values, dtype):
    return np.array(values, dtype=dtype)


def _c(x, dtype):
    return np.dtype(dtype).type(x)


# ---- scene table ---------------------------------------------------------------------------------

def animate_between(a, b, time, dtype=F64):
    t = _c
    return t(a, dtype) + (t(b, dtype) - t(a, dtype)) * (t(0.5, dtype) + t(0.5, dtype) * np.sin(t(time, dtype) * t(0.2, dtype)))


def scene_table(P, dtype=F64, sphere=False):
    """What scene() selects: the family and its arguments (cross size and scale of the Menger sponge,
    the Koch normal's z, the Mandelbulb power). Any index outside 1..18 is scene 0."""
    t = lambda x: _c(x, dtype)
    one = t(1.0)
    anim = lambda a, b: animate_between(a, b, P["time"], dtype)
    s = P["scene_index"]
    if sphere:
        return {"family": SPHERE}
    menger = {
        0: (one / t(6), t(3)), 1: (one / t(5), t(3)), 2: (one / t(4), t(3)), 3: (one / t(3), t(3)),
        5: (one / t(6), t(2)), 6: (one / t(4), t(2)), 7: (one / t(8), t(2)),
        9: (one / t(4), t(4)), 10: (one / t(5), t(5)), 11: (one / t(4), t(6)),
    }
    if s in menger:
        return {"family": MENGER, "cross_size": menger[s][0], "scale_factor": menger[s][1]}
    if s == 4:
        return {"family": MENGER, "cross_size": one / anim(2, 8), "scale_factor": t(3)}
    if s == 8:
        return {"family": MENGER, "cross_size": one / anim(3, 10), "scale_factor": t(2)}
    if s == 12:
        return {"family": MENGER, "cross_size": one / t(3), "scale_factor": anim(3, 5)}
    if s == 13:
        return {"family": MENGER, "cross_size": one / t(4), "scale_factor": anim(2, 4)}
    if s == 14:
        return {"family": MENGER, "cross_size": one / t(6), "scale_factor": anim(1.2, 3)}
    if s == 15:
        return {"family": SIERPINSKI}
    if s == 16:
        return {"family": KOCH, "normal_z": np.sqrt(t(3))}
    if s == 17:
        return {"family": KOCH, "normal_z": anim(np.sqrt(t(3)), 4)}
    if s == 18:
        return {"family": MANDELBULB, "power": anim(4, 9)}
    return {"family": MENGER, "cross_size": one / t(6), "scale_factor": t(3)}


# ---- small vector helpers ------------------------------------------------------------------------

def _dot(a, b):
    return (a * b).sum(axis=-1)


def _length(a):
    return np.sqrt(_dot(a, a))


def _normalize(a):
    return a / _length(a)[..., None]


def shl32(n):
    """`1 << n` as the shader computes it: a 32-bit signed integer, the shift count taken modulo 32."""
    v = (1 << (int(n) % 32)) & 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


# ---- distance estimators -------------------------------------------------------------------------

def box(p, size):
    q = np.abs(p) - size
    zero = q.dtype.type(0)
    return _length(np.maximum(q, zero)) + np.minimum(q.max(axis=-1), zero)


def cross_inside(p, size):
    a = np.abs(p)
    x = np.maximum(a[..., 1], a[..., 2])
    y = np.maximum(a[..., 2], a[..., 0])
    z = np.maximum(a[..., 0], a[..., 1])
    return np.minimum(np.minimum(x, y), z) - size


def repeat(p):
    half = p.dtype.type(0.5)
    s = p + half
    return (s - np.floor(s)) - half


def menger_sponge(p, cross_size, scale_factor, iterations):
    dt = p.dtype.type
    distance = box(p, dt(0.5))
    scale = dt(1.0)
    for _ in range(iterations):
        distance = np.maximum(distance, -cross_inside(repeat(p * scale), cross_size) / scale)
        scale = scale * scale_factor
    return distance


def mirror(p, anchor, normal):
    d = _dot(p - anchor, normal)
    return p + (np.abs(d) - d)[..., None] * normal


def plane_normal(a, b, c):
    return _normalize(np.cross(c - a, b - a))


def tetrahedron(p, a, b, c, d):
    h = lambda anchor, n: _dot(p - anchor, n)
    return np.maximum(np.maximum(np.maximum(h(a, plane_normal(a, b, c)), h(a, plane_normal(a, c, d))),
                                 h(a, plane_normal(a, d, b))), h(b, plane_normal(b, d, c)))


def sierpinski_geometry(iterations, dtype=F64):
    """TOP, the three base vertices, the three fold normals and the y shift of sierpinski_tetrahedron."""
    t = lambda x: _c(x, dtype)
    base = t(0.5)
    scale = base / t(shl32(iterations))
    height = t(4) / np.sqrt(t(6))
    r3 = t(1) / np.sqrt(t(3))
    top = _vec([0, height * base, 0], dtype)
    a = top + scale * _vec([-1, -height, -r3], dtype)
    b = top + scale * _vec([1, -height, -r3], dtype)
    c = top + scale * _vec([0, -height, t(2) * r3], dtype)
    return {"top": top, "a": a, "b": b, "c": c, "normals": [_normalize(top - v) for v in (a, b, c)],
            "shift": height * base * t(0.5)}


def sierpinski_tetrahedron(p, iterations):
    dtype = p.dtype
    g = sierpinski_geometry(iterations, dtype)
    top = g["top"]
    q = p.copy()
    q[..., 1] = q[..., 1] + g["shift"]
    for i in range(int(np.int32(np.uint32(iterations))) - 1, -1, -1):
        distance = dtype.type(shl32(i))
        for v, n in zip((g["a"], g["b"], g["c"]), g["normals"]):
            q = mirror(q, top + distance * (v - top), n)
    return tetrahedron(q, top, g["a"], g["b"], g["c"])


def koch_geometry(normal_z, dtype=F64):
    t = lambda x: _c(x, dtype)
    side = t(3)
    half = side / t(2)
    side_sqrt = np.sqrt(side)
    offset = np.sqrt(side * side - half * half) - side_sqrt
    n1 = _normalize(_vec([0, 1, normal_z], dtype))
    return {"top": _vec([0, 1, 0], dtype), "left": _vec([-half, 0, -offset], dtype),
            "right": _vec([half, 0, -offset], dtype), "back": _vec([0, 0, side_sqrt], dtype),
            "offset": offset, "normal_1": n1, "normal_2": n1 * _vec([1, -1, 1], dtype)}


def koch3d(p, normal_z, iterations):
    dtype = p.dtype
    t = dtype.type
    g = koch_geometry(normal_z, dtype)
    origin = np.zeros(3, dtype)
    scale = t(2)
    q = p * scale
    for _ in range(iterations):
        scale = scale * t(1.5)
        q = q * t(1.5)
        q = q[..., [1, 0, 2]]
        q = mirror(q, origin, g["normal_1"])
        q = mirror(q, origin, g["normal_2"])
        q[..., 2] = q[..., 2] - g["offset"]
    q = q.copy()
    q[..., 1] = np.abs(q[..., 1])
    return tetrahedron(q, g["top"], g["left"], g["right"], g["back"]) / scale


def mandelbulb(p, power, iterations):
    """-> (distance, bodies run, smallest |magnitude / 100 - 1| met at a bailout test)."""
    dtype = p.dtype
    t = dtype.type
    n = len(p)
    current = p.copy()
    derivative = np.ones(n, dtype)
    magnitude = np.zeros(n, dtype)
    bodies = np.zeros(n, np.int64)
    margin = np.full(n, np.inf)
    active = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for _ in range(int(iterations) + 1):
            idx = np.nonzero(active)[0]
            if len(idx) == 0:
                break
            cur = current[idx]
            mag = _length(cur)
            magnitude[idx] = mag
            margin[idx] = np.fmin(margin[idx], np.abs(mag.astype(F64) / BAILOUT - 1.0))
            go = ~(mag > t(BAILOUT))
            active[idx[~go]] = False
            idx, cur, mag = idx[go], cur[go], mag[go]
            theta = np.arccos(cur[:, 2] / mag)
            phi = np.arctan2(cur[:, 1], cur[:, 0])
            derivative[idx] = np.power(mag, power - t(1)) * power * derivative[idx] + t(1)
            r = np.power(mag, power)
            et, ep = theta * power, phi * power
            unit = np.stack([np.sin(et) * np.cos(ep), np.sin(ep) * np.sin(et), np.cos(et)], axis=-1)
            current[idx] = r[:, None] * unit + p[idx]
            bodies[idx] += 1
        distance = t(0.5) * np.log(magnitude) * magnitude / derivative
    return distance, bodies, margin


def sphere(p):
    return _length(p) - p.dtype.type(0.5)


def scene_distance(P, points, dtype=F64, sphere_scene=False, iterations=None):
    """scene(position).distance at points [n, 3]; `iterations` overrides the blob's count."""
    p = np.asarray(points).astype(dtype)
    tab = scene_table(P, dtype, sphere_scene)
    n = P["num_iterations"] if iterations is None else iterations
    fam = tab["family"]
    with np.errstate(all="ignore"):
        if fam == SPHERE:
            return sphere(p)
        if fam == MENGER:
            return menger_sponge(p, tab["cross_size"], tab["scale_factor"], n)
        if fam == SIERPINSKI:
            return sierpinski_tetrahedron(p, n)
        if fam == KOCH:
            return koch3d(p, tab["normal_z"], n)
        return mandelbulb(p, tab["power"], n)[0]


def colorize(p):
    return np.minimum(p.dtype.type(1), p + p.dtype.type(0.5))


def scene_color(P, points, dtype=F64, sphere_scene=False):
    p = np.asarray(points).astype(dtype)
    if scene_table(P, dtype, sphere_scene)["family"] == SIERPINSKI:
        return colorize(np.dtype(dtype).type(1.5) * p)
    return colorize(p)


# ---- camera --------------------------------------------------------------------------------------

def camera_rays(P, width, height, dtype=F64, xs=None, ys=None):
    """-> (origin [3], directions [n, 3]) of pixels (xs, ys); default every pixel, row-major."""
    t = lambda x: _c(x, dtype)
    if xs is None:
        ys, xs = np.divmod(np.arange(width * height), width)
    x = np.asarray(xs).astype(dtype)
    y = np.asarray(ys).astype(dtype)
    sx = (t(2) * x + t(1)) / t(width) - t(1)
    sy = t(1) - (t(2) * y + t(1)) / t(height)
    z = t(1) / np.arctan(t(90) * t(math.pi) / t(180))
    d = np.stack([sx * t(P["aspect_scale"][0]), sy * t(P["aspect_scale"][1]), np.full(len(x), z, dtype)], axis=-1)
    d = _normalize(d)
    M = _vec(P["matrix"], dtype)
    directions = np.stack([d[:, 0] * M[4 * j] + d[:, 1] * M[4 * j + 1] + d[:, 2] * M[4 * j + 2] for j in range(3)], axis=-1)
    origin = _vec([M[3], M[7], M[11]], dtype)
    return origin, directions


# ---- march, normal, shading ----------------------------------------------------------------------

def march(P, starts, directions, max_steps, dtype=F64, sphere_scene=False, erode=0.0):
    """The shader's march of rays starts[n, 3] + t * directions[n, 3]: while fewer than max_steps
    steps are done and total < 1000, evaluate the scene at the ray's point; the closeness is
    min(closeness, d / total) from 1e20; d <= 5e-7 ends the march as a hit at distance total.
    -> dict(hit, distance (-1e20 on a miss), position, steps, closeness, min_d (the smallest d met)).
    `erode` is added to every distance (the scene shrunk by that much): a robustness probe."""
    t = lambda x: _c(x, dtype)
    starts = np.broadcast_to(np.asarray(starts).astype(dtype), np.asarray(directions).shape).copy()
    directions = np.asarray(directions).astype(dtype)
    n = len(directions)
    total = np.zeros(n, dtype)
    closeness = np.full(n, t(INFINITY), dtype)
    hit = np.zeros(n, bool)
    steps = np.zeros(n, np.int64)
    min_d = np.full(n, np.inf, dtype)
    position = starts.copy()
    distance = np.full(n, t(-INFINITY), dtype)
    live = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for _ in range(int(max_steps)):
            live &= total < t(MAX_TOTAL_DISTANCE)
            idx = np.nonzero(live)[0]
            if len(idx) == 0:
                break
            pos = starts[idx] + total[idx][:, None] * directions[idx]
            d = scene_distance(P, pos, dtype, sphere_scene) + t(erode)
            closeness[idx] = np.fmin(closeness[idx], d / total[idx])
            min_d[idx] = np.fmin(min_d[idx], d)
            stop = d <= t(MIN_DISTANCE)
            h = idx[stop]
            hit[h] = True
            distance[h] = total[h]
            position[h] = pos[stop]
            live[h] = False
            go = idx[~stop]
            total[go] = total[go] + d[~stop]
            steps[go] += 1
    return {"hit": hit, "distance": distance, "position": position, "steps": steps, "closeness": closeness,
            "min_d": min_d}


TAPS = ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))  # k.xyy, k.yyx, k.yxy, k.xxx with k = (1, -1)


def normal(P, points, dtype=F64, sphere_scene=False):
    """The four-tap normal: normalize(sum of tap * scene(p + tap * 5e-7))."""
    p = np.asarray(points).astype(dtype)
    acc = np.zeros_like(p)
    for tap in TAPS:
        k = _vec(tap, dtype)
        acc = acc + k * scene_distance(P, p + k * _c(MIN_DISTANCE, dtype), dtype, sphere_scene)[:, None]
    with np.errstate(all="ignore"):
        return _normalize(acc)


def to_sun(dtype=F64):
    return _normalize(-_vec(SUN_DIRECTION, dtype))


def shadow_start(points, normals, dtype=F64):
    return np.asarray(points).astype(dtype) + np.asarray(normals).astype(dtype) * _c(2, dtype) * _c(MIN_DISTANCE, dtype)


def _mix(a, b, w):
    return a * (w.dtype.type(1) - w) + b * w


def shade(color, steps, normals, sun_hit, sun_closeness, ray_directions, max_steps, dtype=F64):
    """The colour of hit pixels from the object colour, the primary step count, the normal, whether
    the sun ray hit something and its closeness, and the camera ray."""
    t = lambda x: _c(x, dtype)
    color = np.asarray(color).astype(dtype)
    n = np.asarray(normals).astype(dtype)
    with np.errstate(all="ignore"):
        halfway = _normalize(-np.asarray(ray_directions).astype(dtype) + to_sun(dtype))
        specular = np.power(np.maximum(_dot(halfway, n), t(0)), t(SPECULAR_SHARPNESS))
        occlusion = np.power(t(1) - np.asarray(steps).astype(dtype) / t(max_steps), t(AMBIENT_OCCLUSION_SHARPNESS))
        color = color * _mix(t(AMBIENT_OCCLUSION_FACTOR), t(1), occlusion)[:, None]
        missed = np.where(np.asarray(sun_hit).astype(bool), t(0), t(1))
        shadow = missed * t(SHADOW_SHARPNESS) * np.asarray(sun_closeness).astype(dtype)
        color = color * _mix(t(SHADOW_FACTOR), t(1), np.clip(shadow, t(0), t(1)))[:, None]
        return color + (t(SPECULAR_FACTOR) * shadow * specular)[:, None]


# ---- store ---------------------------------------------------------------------------------------

def srgb_scaled(c):
    """255 * srgb(clamp(c, 0, 1)) in float64; NaN stays NaN."""
    c = np.asarray(c).astype(F64)
    with np.errstate(all="ignore"):
        x = np.clip(c, 0.0, 1.0)
        return 255.0 * np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)


def encode(c):
    """The 8-bit sRGB code of linear c: round(255 * srgb(clamp(c))), NaN -> 0."""
    s = srgb_scaled(c)
    return np.where(np.isnan(s), 0.0, np.floor(s + 0.5)).astype(np.uint8)


def render(P, width, height, max_steps, dtype=F64, sphere_scene=False):
    """A whole frame -> uint8 [height, width, 4]."""
    origin, dirs = camera_rays(P, width, height, dtype)
    m = march(P, origin, dirs, max_steps, dtype, sphere_scene)
    out = np.zeros((width * height, 4), np.uint8)
    out[:, 3] = 255
    h = np.nonzero(m["hit"])[0]
    if len(h):
        pos = m["position"][h]
        nrm = normal(P, pos, dtype, sphere_scene)
        sun = march(P, shadow_start(pos, nrm, dtype), np.broadcast_to(to_sun(dtype), pos.shape), max_steps, dtype, sphere_scene)
        col = shade(scene_color(P, pos, dtype, sphere_scene), m["steps"][h], nrm, sun["hit"], sun["closeness"],
                    dirs[h], max_steps, dtype)
        col = np.where(np.isnan(col).any(axis=1)[:, None], np.nan, col)
        out[h, :3] = encode(col)
    return out.reshape(height, width, 4)
