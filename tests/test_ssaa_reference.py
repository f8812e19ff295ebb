"""The supersampling resolve's expected values (tests/ssaa_reference.py) and its summation-order
fixture (tests/golden/ssaa_order_cases.npz, written by tests/golden/make_ssaa_cases.py), checked on
the CPU against the oracle's sRGB tables: the fixture's cases are re-derived, really separate the
pinned order from each alternative, and there are enough of them per (factor, alternative) pair for
the GPU test that tiles them into an image (tests/test_gpu_supersample.py) to pin the kernel's order."""
import os

import numpy as np
import pytest

import ssaa_reference as ref
from helpers import params_for

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssaa_order_cases.npz")


@pytest.fixture(scope="module")
def cases():
    return np.load(FIXTURE)


def test_encode_inverts_decode(oracle):
    assert np.array_equal(oracle.encode_srgb(oracle.srgb_decode()), np.arange(256, dtype=np.uint8))


def test_factor_one_is_identity(oracle):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(7, 11, 4), dtype=np.uint8)
    out = ref.box_resolve(img, 1, oracle)
    assert np.array_equal(out[..., :3], img[..., :3])
    assert np.all(out[..., 3] == 255)


@pytest.mark.parametrize("S", ref.FACTORS)
def test_constant_image_keeps_its_code(oracle, S):
    # one output pixel per code: an S x S block of code k in all channels resolves to k
    codes = np.arange(256, dtype=np.uint8)
    hi = np.repeat(np.repeat(codes.reshape(16, 16), S, axis=0), S, axis=1)
    hi = np.repeat(hi[..., None], 4, axis=2)
    out = ref.box_resolve(hi, S, oracle)
    assert np.array_equal(out[..., 0], codes.reshape(16, 16))
    assert np.array_equal(out[..., 1], out[..., 0]) and np.array_equal(out[..., 2], out[..., 0])
    assert np.all(out[..., 3] == 255)


@pytest.mark.parametrize("S", ref.FACTORS)
def test_box_resolve_agrees_with_block_codes(oracle, S):
    """The image form (box_resolve) and the block form (pinned_codes) are the same sum."""
    rng = np.random.default_rng(S)
    blocks = rng.integers(0, 256, size=(40, S, S), dtype=np.uint8)
    hi = np.zeros((S * 5, S * 8, 4), np.uint8)
    for k, b in enumerate(blocks):
        y, x = divmod(k, 8)
        hi[S * y:S * y + S, S * x:S * x + S, :3] = b[..., None]
    out = ref.box_resolve(hi, S, oracle)
    assert np.array_equal(out[..., 0].reshape(-1), ref.pinned_codes(blocks, S, oracle))


@pytest.mark.parametrize("S", ref.FACTORS)
def test_order_fixture_separates_every_alternative(oracle, cases, S):
    blocks, pinned = cases[f"blocks_{S}"], cases[f"pinned_{S}"]
    alt, altcode = cases[f"alt_{S}"], cases[f"altcode_{S}"]
    names = ref.alternatives_for(S)
    assert blocks.shape[1:] == (S, S) and blocks.dtype == np.uint8
    assert len(blocks) == len(pinned) == len(alt) == len(altcode)
    assert np.array_equal(ref.pinned_codes(blocks, S, oracle), pinned)
    for a, name in enumerate(names):
        sel = alt == a
        assert int(sel.sum()) >= ref.MIN_CASES, (S, name, int(sel.sum()))
        got = ref.ALTERNATIVES[name](blocks[sel], S, oracle)
        assert np.array_equal(got, altcode[sel]), (S, name)
        assert np.all(got != pinned[sel]), (S, name)
    assert set(np.unique(alt)) == set(range(len(names)))


def test_exact_reciprocal_factors(oracle):
    """S = 2 and 4: the multiply by the exact reciprocal and the pre-scaled terms give the division's
    bits (why the fixture searches them for S = 3 only)."""
    rng = np.random.default_rng(7)
    for S in (2, 4):
        blocks = rng.integers(0, 256, size=(200000, S, S), dtype=np.uint8)
        pin = ref.pinned_codes(blocks, S, oracle)
        assert np.array_equal(ref.alt_reciprocal(blocks, S, oracle), pin)
        assert np.array_equal(ref.alt_prescale(blocks, S, oracle), pin)


@pytest.mark.parametrize("w,h", [(16, 9), (33, 17)])
def test_resolved_frames_differ_from_one_sample(oracle, w, h):
    """The frame tests have power: the resolved Mandelbulb frames differ from the one-sample frame
    in a good part of their pixels, and some output pixels mix hits and background."""
    p = params_for(18, 6, 3.2175055, w, h)
    one = oracle.render(p, w, h, 128)["rgba"]
    for S in ref.FACTORS:
        r = oracle.render(p, S * w, S * h, 128, info=True)
        res = ref.box_resolve(r["rgba"], S, oracle)
        assert res.shape == one.shape
        differ = int(np.any(res != one, axis=-1).sum())
        assert differ >= w * h // 8, (S, differ)
        hit = (r["info"] & oracle.INFO_HIT).astype(bool).reshape(h, S, w, S)
        per = hit.sum(axis=(1, 3))
        mixed = int(((per > 0) & (per < S * S)).sum())
        assert mixed >= 10, (S, mixed)
