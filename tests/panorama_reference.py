"""Expected values of the panorama (include/frm.h frm_set_panorama, frm_project_equirect): the numpy
float32 restatement of the pinned semantics, and a float64 variant that shows the pin matters.

N is the face size, M = N + 2 (one guard texel all round), q = f32(M) / f32(N) and
a = kCameraDirectionZ * q (one f32 multiply).

Face frames. Face f of a parameter set p is the M x M frame of p_f: p with aspect_scale = (a, a) and the
camera C_f = C * [r_f u_f w_f] (C the 4x4 camera matrix, the face vectors in the camera's basis: x right,
y up, z forward; column 3 unchanged):

    f  face       r (right)   u (up)      w (forward)
    0  +z front   ( 1,0, 0)   (0,1, 0)    ( 0, 0, 1)
    1  -z back    (-1,0, 0)   (0,1, 0)    ( 0, 0,-1)
    2  +x right   ( 0,0,-1)   (0,1, 0)    ( 1, 0, 0)
    3  -x left    ( 0,0, 1)   (0,1, 0)    (-1, 0, 0)
    4  +y up      ( 1,0, 0)   (0,0,-1)    ( 0, 1, 0)
    5  -y down    ( 1,0, 0)   (0,0, 1)    ( 0,-1, 0)

so camera_matrix[4j+i] of p_f is + or - camera_matrix[4j+k] of p, for all four j.

Direction tables. Output pixel (X, Y) of a W x H panorama has longitude lon = ((2X+1)/W - 1) * pi and
latitude lat = (1 - (2Y+1)/H) * pi/2; sin_lon[X], cos_lon[X], sin_lat[Y], cos_lat[Y] are computed in
float64 and rounded once to f32.

Per pixel, all f32, every operation rounded on its own:

    dx = cos_lat*sin_lon;  dy = sin_lat;  dz = cos_lat*cos_lon
    face: |dz| >= |dx| && |dz| >= |dy| ? (dz > 0 ? 0 : 1)
        : |dx| >= |dy|                 ? (dx > 0 ? 2 : 3)
        :                                (dy > 0 ? 4 : 5)
    A = d.r_f;  B = d.u_f;  m = d.w_f          (each a signed component of d)
    u = A / m;  v = B / m
    fx = u*(0.5f*N) + (0.5f*M - 0.5f);   fy = (0.5f*M - 0.5f) - v*(0.5f*N)
    x0 = floor(fx); tx = fx - x0;  y0 = floor(fy); ty = fy - y0
    x0, x0+1, y0, y0+1 clamped to [0, M-1]

then the blit's linear filter over the texels t00 (x0, y0), t10 (x0+1, y0), t01 (x0, y0+1), t11 of face
f: per channel top = mix(D[t00], D[t10], tx), bot = mix(D[t01], D[t11], tx), c = mix(top, bot, ty) with
mix(a, b, t) = a*(1.0f - t) + b*t and D = oracle.srgb_decode(); stored by oracle.encode_srgb, alpha 255.
"""
import struct

import numpy as np

CAMERA_DIRECTION_Z = np.float32(float.fromhex("0x1.fe04c8p-1"))  # f32(1/atan(pi/2)), the z of every camera ray

# r, u, w of face f in the camera's basis
FACES = (
    ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
    ((-1, 0, 0), (0, 1, 0), (0, 0, -1)),
    ((0, 0, -1), (0, 1, 0), (1, 0, 0)),
    ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),
    ((1, 0, 0), (0, 0, -1), (0, 1, 0)),
    ((1, 0, 0), (0, 0, 1), (0, -1, 0)),
)
# The GPU tests' kernel shapes (N, W, H): for these no tap of a pixel leaves its face
# (tests/test_panorama_reference.py asserts it), so the clamp never acts.
SHAPES = ((1, 4, 2), (2, 9, 5), (5, 33, 17), (4, 130, 3), (3, 1, 1), (16, 64, 32))


def face_parameters(p, N):
    """The six 96-byte parameter blocks p_f of `p` (anything with to_bytes(), or 96 bytes)."""
    raw = p.to_bytes() if hasattr(p, "to_bytes") else bytes(p)
    assert len(raw) == 96 and N >= 1
    c = np.frombuffer(raw, dtype=np.float32, count=16).reshape(4, 4)  # c[j][i] = camera_matrix[4j+i]
    a = CAMERA_DIRECTION_Z * (np.float32(N + 2) / np.float32(N))
    assert a.dtype == np.float32
    out = []
    for basis in FACES:
        cf = c.copy()
        for i, vec in enumerate(basis):
            k = [abs(e) for e in vec].index(1)
            cf[:, i] = c[:, k] if vec[k] > 0 else -c[:, k]
        out.append(cf.tobytes() + struct.pack("<2f", a, a) + raw[72:])
    return out


def tables(W, H):
    """(sin_lon[W], cos_lon[W], sin_lat[H], cos_lat[H]) in float64."""
    lon = ((2.0 * np.arange(W, dtype=np.float64) + 1.0) / W - 1.0) * np.pi
    lat = (1.0 - (2.0 * np.arange(H, dtype=np.float64) + 1.0) / H) * (np.pi / 2.0)
    return np.sin(lon), np.cos(lon), np.sin(lat), np.cos(lat)


def select_face(dx, dy, dz):
    ax, ay, az = np.abs(dx), np.abs(dy), np.abs(dz)
    return np.where((az >= ax) & (az >= ay), np.where(dz > 0, 0, 1),
                    np.where(ax >= ay, np.where(dx > 0, 2, 3), np.where(dy > 0, 4, 5)))


def taps(N, W, H, tabs, dtype=np.float32):
    """Per pixel [H, W]: face, the unclamped x0, y0 (integers) and the weights tx, ty, in `dtype`."""
    t = dtype
    sl, cl, sp, cp = (np.asarray(x).astype(t) for x in tabs)
    assert sl.shape == cl.shape == (W,) and sp.shape == cp.shape == (H,)
    dx = cp[:, None] * sl[None, :]
    dy = np.broadcast_to(sp[:, None], (H, W))
    dz = cp[:, None] * cl[None, :]
    face = select_face(dx, dy, dz)
    d = np.stack([dx, dy, dz])
    A, B, m = (np.zeros((H, W), t) for _ in range(3))
    for f, basis in enumerate(FACES):
        for dest, vec in zip((A, B, m), basis):
            k = [abs(e) for e in vec].index(1)
            np.copyto(dest, d[k] if vec[k] > 0 else -d[k], where=face == f)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = A / m, B / m
    M = N + 2
    half_n, centre = t(0.5) * t(N), t(0.5) * t(M) - t(0.5)
    fx, fy = u * half_n + centre, centre - v * half_n
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = fx - x0, fy - y0
    for arr in (dx, dz, u, v, fx, fy, tx, ty):
        assert arr.dtype == t
    return face, x0, y0, tx, ty


def clamped(N, x0, y0):
    """Where a tap of the pixel would leave the face's M x M texels."""
    M = N + 2
    return (x0 < 0) | (x0 + 1 > M - 1) | (y0 < 0) | (y0 + 1 > M - 1)


def project(faces, N, W, H, tabs, oracle, dtype=np.float32):
    """faces: [6, M, M, 4] uint8 sRGB texels -> the W x H panorama [H, W, 4] uint8. dtype=np.float64 is
    the variant (everything up to the store in float64, rounded to f32 once before it)."""
    t = dtype
    faces = np.asarray(faces, dtype=np.uint8)
    M = N + 2
    assert faces.shape == (6, M, M, 4)
    face, x0, y0, tx, ty = taps(N, W, H, tabs, t)
    with np.errstate(invalid="ignore"):
        cl = lambda a: np.nan_to_num(np.minimum(np.maximum(a, 0), M - 1), nan=0.0).astype(np.int64)  # noqa: E731
        xa, xb, ya, yb = cl(x0), cl(x0 + 1), cl(y0), cl(y0 + 1)
    D = oracle.srgb_decode().astype(t)
    one = t(1.0)
    mix = lambda a, b, w: a * (one - w) + b * w  # noqa: E731
    t00, t10 = D[faces[face, ya, xa, :3]], D[faces[face, ya, xb, :3]]
    t01, t11 = D[faces[face, yb, xa, :3]], D[faces[face, yb, xb, :3]]
    top, bot = mix(t00, t10, tx[..., None]), mix(t01, t11, tx[..., None])
    c = mix(top, bot, ty[..., None])
    assert c.dtype == t
    out = np.empty((H, W, 4), np.uint8)
    out[..., :3] = oracle.encode_srgb(np.ascontiguousarray(c.astype(np.float32)))
    out[..., 3] = 255
    return out


def project_f64(faces, N, W, H, tabs, oracle):
    return project(faces, N, W, H, tabs, oracle, dtype=np.float64)


def constant_faces(N, colours):
    """Six faces, face f all colours[f] (RGB), alpha 255."""
    M = N + 2
    faces = np.empty((6, M, M, 4), np.uint8)
    faces[..., :3] = np.asarray(colours, np.uint8)[:, None, None, :]
    faces[..., 3] = 255
    return faces


SIX_COLOURS = ((255, 0, 0), (0, 255, 255), (0, 255, 0), (255, 0, 255), (0, 0, 255), (255, 255, 0))
