"""tests/dof_reference.py itself (no GPU, no libfrm): the properties the pinned depth-of-field sequence
must have, and the circle of confusion against values worked out by hand in float64."""
import numpy as np
import pytest

import dof_reference as ref


def frame_and_depths(seed, W=23, H=17):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8), ref.test_depths(rng, W, H)


def with_alpha_255(src):
    out = src.copy()
    out[..., 3] = 255
    return out


@pytest.mark.parametrize("aperture,radius", [(0.0, 16), (0.0, 1), (8.0, 0), (1e30, 0)])
def test_no_aperture_or_no_radius_returns_the_source(oracle, aperture, radius):
    src, z = frame_and_depths(1)
    assert np.isinf(z).any() and np.isnan(z).any() and (z == 0).any() and (z < 0).any()
    assert np.array_equal(ref.gather(src, z, aperture, 2.0, radius, oracle), with_alpha_255(src))


def test_outputs_stay_finite_for_special_depths(oracle):
    src, z = frame_and_depths(2, 40, 24)
    sw, s = ref.gather(src, z, 8.0, 2.0, 16, oracle, return_sums=True)
    assert np.isfinite(sw).all() and np.isfinite(s).all() and (sw > 0).all()


@pytest.mark.parametrize("colour", [(0, 0, 0), (255, 255, 255), (17, 128, 254), (1, 2, 3)])
def test_a_uniform_frame_keeps_its_colour(oracle, colour):
    """sr / sw = (sum of w * D) / (sum of w) is D again only up to rounding: the codes must not move."""
    _, z = frame_and_depths(3)
    src = np.empty(z.shape + (4,), np.uint8)
    src[..., :3] = colour
    src[..., 3] = 9
    for aperture, focus, radius in ((8.0, 2.0, 16), (3.0, 0.7, 4), (40.0, 5.0, 7)):
        assert np.array_equal(ref.gather(src, z, aperture, focus, radius, oracle), with_alpha_255(src))


def test_a_sharp_foreground_keeps_its_bytes_before_a_blurred_background(oracle):
    """The use_p rule: the in-focus pixels (c = 0) take nothing from the far, blurred pixels behind."""
    H, W, F = 21, 25, 2.0
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    z = np.full((H, W), np.inf, np.float32)
    fg = np.zeros((H, W), bool)
    fg[6:15, 8:17] = True
    fg[10, 3] = True  # and a lone pixel
    z[fg] = F
    out = ref.gather(src, z, 6.0, F, 16, oracle)
    assert np.array_equal(out[fg][:, :3], src[fg][:, :3])
    # while the background is blurred, also by the foreground's colours next to it
    assert np.mean(np.any(out[~fg][:, :3] != src[~fg][:, :3], axis=-1)) > 0.9
    # without the rule (the depths swapped: the sharp pixels behind) the blurred ones bleed over them
    z2 = np.where(fg, np.float32(F), np.float32(F / 4))
    out2 = ref.gather(src, z2, 2.0, F, 16, oracle)  # c = 2 * |1 - 4| = 6 in front
    assert np.any(out2[fg][:, :3] != src[fg][:, :3])


@pytest.mark.parametrize("aperture", [0.5, 1.0, 2.5, 5.0, 16.0, 40.0])
def test_a_bright_texel_at_infinity_spreads_over_its_disc(oracle, aperture):
    R, n = 16, 41
    src = np.zeros((n, n, 4), np.uint8)
    src[n // 2, n // 2, :3] = 255
    z = np.full((n, n), np.inf, np.float32)
    sw, s = ref.gather(src, z, aperture, 2.0, R, oracle, return_sums=True)
    c = np.float32(min(aperture, R))  # Z = +inf: c = A, clamped to R
    dy, dx = np.mgrid[:n, :n] - n // 2
    disc = (dx * dx + dy * dy).astype(np.float32) <= c * c
    assert np.array_equal(s[..., 0] > 0, disc) and np.array_equal(s[..., 1] > 0, disc)
    assert disc.sum() > 1 or aperture < 1
    out = ref.gather(src, z, aperture, 2.0, R, oracle)
    assert np.array_equal(out[..., 0] > 0, disc)


def test_circle_of_confusion_by_hand():
    A, F, R = 3.0, 2.0, 16
    z = np.array([np.inf, 0.0, np.nan, F, 2 * F, F / 2, -0.0, -1.0], np.float32)
    # A * |1 - F / Z| in float64 (these are exact in f32 too): inf -> A; 0 -> inf -> R; NaN -> NaN,
    # in focus: 0; F -> 0; 2F -> A / 2; F / 2 -> A; -0 -> inf -> R; -1 -> A * 3
    want = np.array([3.0, 16.0, 0.0, 0.0, 1.5, 3.0, 16.0, 9.0])
    got = ref.coc(A, F, R, z)
    assert got.dtype == np.float32
    assert np.array_equal(got, want.astype(np.float32))
    # A = 0: 0 * inf = NaN at Z = 0 is in focus as well, and everything else is 0
    assert np.array_equal(ref.coc(0.0, F, R, z), np.zeros(len(z), np.float32))
    # values that round: float64 first, rounded once
    A, F = 7.3, 1.7
    z = np.array([np.inf, F, 2 * F, F / 2, 3.1, 0.9], np.float32)
    A32, F32 = np.float32(A), np.float32(F)
    q = (np.float64(F32) / z.astype(np.float64)).astype(np.float32)  # each f32 operation rounded once
    d = (1.0 - q.astype(np.float64)).astype(np.float32)
    c = (np.float64(A32) * np.abs(d).astype(np.float64)).astype(np.float32)
    assert np.array_equal(ref.coc(A, F, 16, z), np.minimum(c, np.float32(16)))
    assert np.array_equal(ref.coc(A, F, 4, z), np.minimum(c, np.float32(4)))
    a, w = ref.area_weight(np.array([0.0, 1.0, 16.0], np.float32))
    assert a.tolist() == [0.0, 1.0, 256.0] and w[0] == 1.0
    assert w[1] == np.float32(1.0) / (np.float32(np.pi) + np.float32(1.0))
    assert abs(float(w[2]) - 1.0 / (np.pi * 256.0 + 1.0)) < 1e-9


def test_shapes_cover_the_kernel_paths():
    tile = 16
    assert any(w < 2 * r + 1 and h < 2 * r + 1 for w, h, r in ref.SHAPES)  # smaller than the window
    assert {r for w, h, r in ref.SHAPES if (w, h) == (37, 19)} == {1, 3, 16}  # partial tiles
    assert any(w > 2 * tile and h > 2 * tile and w % tile and h % tile and r == 16 for w, h, r in ref.SHAPES)
    assert (1, 1, 16) in ref.SHAPES
