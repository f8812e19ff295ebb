"""The numpy reference of adaptive supersampling (tests/adaptive_reference.py) against hand cases,
and on oracle frames: the edge mask is a non-empty strict subset there and the plain, the fully
supersampled and the adaptive frame are three different images, so the GPU tests that compare
against the composed frame can tell them apart. No GPU needed."""
import numpy as np
import pytest

import adaptive_reference as ada
import frm
import ssaa_reference as ssaa
from helpers import params_for


def flat(h, w, value=(100, 100, 100, 7)):
    img = np.empty((h, w, 4), np.uint8)
    img[...] = value
    return img


def test_single_pixel_frame_is_flagged_at_threshold_zero_only():
    img = flat(1, 1)
    assert ada.edge_mask(img, 0).tolist() == [[True]]
    for t in (1, 16, 255, 256):
        assert ada.edge_mask(img, t).tolist() == [[False]]


def test_threshold_zero_flags_all_and_256_none():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(9, 11, 4), dtype=np.uint8)
    assert ada.edge_mask(img, 0).all()
    assert not ada.edge_mask(img, 256).any()
    img[0, 0, :3], img[0, 1, :3] = 0, 255  # the largest contrast there is
    m = ada.edge_mask(img, 255)
    assert m[0, 0] and m[0, 1] and m[1, 1] and not ada.edge_mask(img, 256).any()


@pytest.mark.parametrize("y,x", [(3, 4), (0, 0), (0, 4), (6, 8), (6, 0), (3, 8)])
def test_one_odd_pixel_flags_its_clipped_neighbourhood(y, x):
    img = flat(7, 9)
    img[y, x, 1] = 140
    want = np.zeros((7, 9), bool)
    want[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    assert np.array_equal(ada.edge_mask(img, 40), want)
    assert want.sum() == (3 if 0 < y < 6 else 2) * (3 if 0 < x < 8 else 2)


def test_the_comparison_is_greater_or_equal():
    img = flat(5, 5)
    img[2, 2, 0] = 100 + 16
    assert ada.edge_mask(img, 16).sum() == 9
    assert ada.edge_mask(img, 17).sum() == 0
    img[2, 2, 0] = 100 - 16  # the range, not a signed difference
    assert ada.edge_mask(img, 16).sum() == 9
    assert ada.edge_mask(img, 17).sum() == 0


@pytest.mark.parametrize("channel", [0, 1, 2])
def test_each_colour_channel_alone_triggers(channel):
    img = flat(5, 5)
    img[2, 2, channel] = 130
    assert ada.edge_mask(img, 30).sum() == 9
    assert ada.edge_mask(img, 31).sum() == 0  # the maximum over the channels, not their sum
    img[2, 2, (channel + 1) % 3] = 80
    assert ada.edge_mask(img, 30).sum() == 9
    assert ada.edge_mask(img, 31).sum() == 0


def test_alpha_never_triggers():
    img = flat(5, 5)
    img[..., 3] = np.random.default_rng(5).integers(0, 256, size=(5, 5), dtype=np.uint8)
    assert not ada.edge_mask(img, 1).any()


def test_one_row_and_one_column_frames():
    row = flat(1, 8)
    row[0, 5, 2] = 0
    assert ada.edge_mask(row, 100).tolist() == [[False, False, False, False, True, True, True, False]]
    col = flat(8, 1)
    col[0, 0, 0] = 255
    assert ada.edge_mask(col, 100)[:, 0].tolist() == [True, True] + [False] * 6


def test_compose_takes_refined_pixels_and_forces_alpha():
    plain, fine = flat(2, 3, (1, 2, 3, 4)), flat(2, 3, (9, 8, 7, 6))
    mask = np.array([[True, False, False], [False, False, True]])
    out = ada.compose(plain, fine, mask)
    assert out[0, 0].tolist() == [9, 8, 7, 255] and out[1, 2].tolist() == [9, 8, 7, 255]
    assert out[0, 1].tolist() == [1, 2, 3, 255] and out[1, 0].tolist() == [1, 2, 3, 255]
    assert plain[0, 0, 3] == 4  # the inputs are not written


# scene, iterations, size, steps -> (flagged, flagged pixels that differ F1/FS, unflagged that differ):
# counted on the oracle at S = 2, threshold 16, pose P1
ORACLE_CASES = {
    "mandelbulb": ((18, 6, 33, 17, 128), (228, 130, 15)),
    "menger-small": ((3, 3, 33, 17, 128), (80, 68, 0)),
    "menger": ((3, 3, 48, 27, 256), (186, None, 4)),
}


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_mask_on_oracle_frames(oracle, name):
    (scene, iters, w, h, steps), (flagged, diff_in, diff_out) = ORACLE_CASES[name]
    S, T = 2, frm.FRM_ADAPTIVE_DEFAULT_THRESHOLD
    assert T == 16
    p = params_for(scene, iters, frm.POWER8_TIME, w, h)
    f1 = oracle.render(p, w, h, steps)["rgba"]
    fs = ssaa.box_resolve(oracle.render(p, S * w, S * h, steps)["rgba"], S, oracle)
    mask = ada.edge_mask(f1, T)
    assert 0 < mask.sum() < w * h
    assert mask.sum() == flagged
    differ = np.any(f1 != fs, axis=2)
    if diff_in is not None:
        assert (differ & mask).sum() == diff_in
    assert (differ & ~mask).sum() == diff_out
    a = ada.compose(f1, fs, mask)
    assert not np.array_equal(a, f1)  # some refined pixel changed
    if diff_out:  # and some unrefined pixel would have: the three images differ pairwise
        assert not np.array_equal(a, fs)
    else:  # here only the work counters separate the adaptive from the supersampled frame
        assert np.array_equal(a, fs)
    assert np.array_equal(a[mask], fs[mask]) and np.array_equal(a[~mask], f1[~mask])
