"""The panorama's reference (tests/panorama_reference.py, no GPU needed): its face bases, where the
axes land, the face selection with its ties, the no-clamp condition of the GPU tests' shapes, that
the f32 pin differs from a float64 evaluation, and that a panorama is none of its faces resized."""
import math

import numpy as np
import pytest

import frm
import panorama_reference as ref
from helpers import params_for


def test_face_bases_are_right_handed_and_orthonormal():
    seen = set()
    for r, u, w in ref.FACES:
        r, u, w = (np.array(v, np.int64) for v in (r, u, w))
        for v in (r, u, w):
            assert np.abs(v).sum() == 1  # +- a unit vector
        assert r @ u == 0 and r @ w == 0 and u @ w == 0
        assert np.array_equal(np.cross(r, u), w)
        seen.add(tuple(w))
    assert seen == {(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)}


def centre_case(N, W, H, tabs, X, Y, f, oracle):
    M = N + 2
    face, x0, y0, tx, ty = ref.taps(N, W, H, tabs)
    c = (M - 1) // 2
    assert face[Y, X] == f, (f, face[Y, X])
    assert (x0[Y, X], y0[Y, X], tx[Y, X], ty[Y, X]) == (c, c, 0.0, 0.0), f
    faces = np.random.default_rng(f).integers(0, 256, size=(6, M, M, 4), dtype=np.uint8)
    got = ref.project(faces, N, W, H, tabs, oracle)
    assert np.array_equal(got[Y, X, :3], faces[f, c, c, :3]) and got[Y, X, 3] == 255


@pytest.mark.parametrize("N", [1, 3, 5])
def test_axis_pixels_land_on_face_centres(oracle, N):
    # pixel centres of real tables reach +z (W, H odd) and +-x (W = 2 mod 4): lon = 0, +-pi/2, lat = 0
    centre_case(N, 5, 3, ref.tables(5, 3), 2, 1, 0, oracle)
    centre_case(N, 6, 3, ref.tables(6, 3), 4, 1, 2, oracle)
    centre_case(N, 6, 3, ref.tables(6, 3), 1, 1, 3, oracle)
    # no pixel centre has lon = +-pi or lat = +-pi/2: the other axes through hand-made table entries
    sl, cl = np.array([0.0, 0.0, 1.0, -1.0]), np.array([1.0, -1.0, 0.0, 0.0])
    sp, cp = np.array([0.0, 1.0, -1.0]), np.array([1.0, 0.0, 0.0])
    tabs = (sl, cl, sp, cp)
    for X, Y, f in ((0, 0, 0), (1, 0, 1), (2, 0, 2), (3, 0, 3), (0, 1, 4), (2, 1, 4), (1, 2, 5), (3, 2, 5)):
        centre_case(N, 4, 3, tabs, X, Y, f, oracle)


def scalar_face(dx, dy, dz):
    """The selection rule, one pixel at a time, in the issue's words."""
    if abs(dz) >= abs(dx) and abs(dz) >= abs(dy):
        return 0 if dz > 0 else 1
    if abs(dx) >= abs(dy):
        return 2 if dx > 0 else 3
    return 4 if dy > 0 else 5


def face_map(W, H, tabs):
    sl, cl, sp, cp = (np.asarray(t).astype(np.float32) for t in tabs)
    return np.array([[scalar_face(cp[y] * sl[x], sp[y], cp[y] * cl[x]) for x in range(W)] for y in range(H)])


@pytest.mark.parametrize("N,W,H", ref.SHAPES + ((7, 48, 24),))
def test_six_colours_follow_the_selection_rule(oracle, N, W, H):
    tabs = ref.tables(W, H)
    want = face_map(W, H, tabs)
    got = ref.project(ref.constant_faces(N, ref.SIX_COLOURS), N, W, H, tabs, oracle)
    assert np.array_equal(got[..., :3], np.array(ref.SIX_COLOURS, np.uint8)[want])
    assert np.all(got[..., 3] == 255)
    if W >= 8 and H >= 4:
        assert set(want.reshape(-1)) == set(range(6))  # every face is seen


def test_selection_ties_go_to_the_earlier_face(oracle):
    h = np.float32(0.5)
    # columns: (sin_lon, cos_lon); rows: (sin_lat, cos_lat): hand-made entries with exact ties
    sl = np.array([h, -h, h, -h, 1.0, -1.0, 0.0], np.float32)
    cl = np.array([h, h, -h, -h, h, h, 1.0], np.float32)
    sp = np.array([0.0, h, -h, 1.0], np.float32)
    cp = np.array([1.0, 1.0, 1.0, h], np.float32)
    tabs = (sl, cl, sp, cp)
    want = np.array([
        # |dz| = |dx| (> |dy|): +-z wins over +-x; col 4, 5: |dx| > |dz|; col 6: the axis
        [0, 0, 1, 1, 2, 3, 0],
        # dy = +h: |dz| = |dx| = |dy|: +-z; cols 4, 5: dx = +-1 over dy = h
        [0, 0, 1, 1, 2, 3, 0],
        [0, 0, 1, 1, 2, 3, 0],
        # dy = 1, cos_lat = h: cols 0..3 |dx| = |dz| = h/2 < 1: +y; cols 4, 5: |dx| = h < 1: +y
        [4, 4, 4, 4, 4, 4, 4],
    ])
    assert np.array_equal(face_map(7, 4, tabs), want)
    # |dx| = |dy| > |dz|: +-x wins over +-y
    sl2, cl2 = np.array([1.0, -1.0], np.float32), np.array([h, h], np.float32)
    sp2, cp2 = np.array([h, -h], np.float32), np.array([h, h], np.float32)
    tabs2 = (sl2, cl2, sp2, cp2)
    want2 = np.array([[2, 3], [2, 3]])
    assert np.array_equal(face_map(2, 2, tabs2), want2)
    colours = np.array(ref.SIX_COLOURS, np.uint8)
    for N in (1, 4):
        faces = ref.constant_faces(N, ref.SIX_COLOURS)
        assert np.array_equal(ref.project(faces, N, 7, 4, tabs, oracle)[..., :3], colours[want])
        assert np.array_equal(ref.project(faces, N, 2, 2, tabs2, oracle)[..., :3], colours[want2])
        assert np.array_equal(ref.taps(N, 7, 4, tabs)[0], want)


@pytest.mark.parametrize("N,W,H", ref.SHAPES + ((14, 48, 24), (6, 32, 16)))
def test_no_tap_is_clamped_for_the_gpu_shapes(N, W, H):
    """The guard band's purpose: every tap of every pixel lies inside its face."""
    _, x0, y0, tx, ty = ref.taps(N, W, H, ref.tables(W, H))
    assert not ref.clamped(N, x0, y0).any()
    assert tx.min() >= 0 and tx.max() < 1 and ty.min() >= 0 and ty.max() < 1


def test_the_float64_variant_gives_other_codes(oracle):
    """The f32 sequence is a pin, not a detail: evaluated in float64 a few codes differ."""
    N, W, H = 64, 512, 256  # about one code in ten thousand differs: a large frame shows some
    faces = np.random.default_rng(2).integers(0, 256, size=(6, N + 2, N + 2, 4), dtype=np.uint8)
    tabs = ref.tables(W, H)
    a, b = ref.project(faces, N, W, H, tabs, oracle), ref.project_f64(faces, N, W, H, tabs, oracle)
    differ = int((a != b).sum())
    assert 0 < differ < a.size // 1000, differ  # some, and only a few: the two agree elsewhere
    assert np.abs(a.astype(int) - b.astype(int)).max() <= 1


def test_a_panorama_is_none_of_its_faces(oracle):
    N, W, H, steps = 16, 48, 24, 48
    p = params_for(18, 4, frm.POWER8_TIME, W, H)
    faces = np.stack([oracle.render(q, N + 2, N + 2, steps)["rgba"] for q in ref.face_parameters(p, N)])
    pano = ref.project(faces, N, W, H, ref.tables(W, H), oracle)
    assert len(np.unique(pano.reshape(-1, 4), axis=0)) > 16  # a picture, not a flat colour
    for f in range(6):
        assert np.any(oracle.blit(faces[f], W, H) != pano), f
    # the front face sees the set; from this pose the ones looking away see the background
    assert len({faces[f].tobytes() for f in range(6)}) >= 2


def test_the_centre_of_the_panorama_is_the_plain_view(oracle):
    """Face 0 keeps the camera and takes the face's aspect; the panorama's centre pixel is its centre texel."""
    N, steps = 15, 48
    M = N + 2
    p = params_for(18, 4, frm.POWER8_TIME, M, M)
    f0 = frm.Parameters.from_bytes(ref.face_parameters(p, N)[0])
    assert f0.camera_matrix == p.camera_matrix
    a = float(ref.CAMERA_DIRECTION_Z * (np.float32(M) / np.float32(N)))
    assert f0.aspect_scale == (a, a) and math.isclose(a, 0.99613023 * M / N, rel_tol=1e-6)
    face = oracle.render(f0, M, M, steps)["rgba"]
    pano = ref.project(np.stack([face] * 6), N, 5, 3, ref.tables(5, 3), oracle)
    assert np.array_equal(pano[1, 2, :3], face[M // 2, M // 2, :3])
