"""The motion blur's expected values (tests/shutter_reference.py) and its summation-order fixture
(tests/golden/shutter_order_cases.npz, written by tests/golden/make_shutter_cases.py), checked on
the CPU against the oracle's sRGB tables: identical samples give their code back, one sub-frame is
the supersampling resolve, the fixture's cases are re-derived, really separate the pinned order from
each alternative, and there are enough of them per (shape, alternative) pair for the GPU test that
tiles them into sub-frames (tests/test_gpu_shutter.py) to pin the kernel's order."""
import os

import numpy as np
import pytest

import shutter_reference as ref
import ssaa_reference

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shutter_order_cases.npz")


@pytest.fixture(scope="module")
def cases():
    return np.load(FIXTURE)


@pytest.mark.parametrize("n", list(range(1, 33)) + [512])
def test_identical_samples_keep_their_code(oracle, n):
    """n equal texels of any code average to that code: identical sub-frames reproduce the frame."""
    codes = np.arange(256, dtype=np.uint8)
    blocks = np.repeat(codes[:, None], n, axis=1).reshape(256, n, 1, 1)
    assert np.array_equal(ref.pinned_codes(blocks, oracle), codes)


def test_identical_sub_frames_in_image_form(oracle):
    rng = np.random.default_rng(3)
    one = rng.integers(0, 256, size=(6, 10, 4), dtype=np.uint8)
    for S, T in ((1, 5), (2, 3)):
        out = ref.accumulate(np.stack([one] * T), S, oracle)
        assert np.array_equal(out, ssaa_reference.box_resolve(one, S, oracle)), (S, T)


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_one_sub_frame_is_the_box_resolve(oracle, S):
    rng = np.random.default_rng(S)
    hi = rng.integers(0, 256, size=(S * 9, S * 13, 4), dtype=np.uint8)
    out = ref.accumulate(hi[None], S, oracle)
    assert np.array_equal(out, ssaa_reference.box_resolve(hi, S, oracle))
    if S == 1:
        assert np.array_equal(out[..., :3], hi[..., :3]) and np.all(out[..., 3] == 255)


@pytest.mark.parametrize("S,T", ref.SHAPES)
def test_accumulate_agrees_with_block_codes(oracle, S, T):
    """The image form (accumulate) and the block form (pinned_codes) are the same sum; so is a sum
    carried on from a first part of the sub-frames."""
    rng = np.random.default_rng(10 * S + T)
    blocks = rng.integers(0, 256, size=(40, T, S, S), dtype=np.uint8)
    frames = np.zeros((T, S * 5, S * 8, 4), np.uint8)
    for k, b in enumerate(blocks):
        y, x = divmod(k, 8)
        frames[:, S * y:S * y + S, S * x:S * x + S, :3] = b[..., None]
    out = ref.accumulate(frames, S, oracle)
    assert np.array_equal(out[..., 0].reshape(-1), ref.pinned_codes(blocks, oracle))
    part = ref.accumulate_sum(frames[:T // 2], S, oracle)
    whole = ref.accumulate_sum(frames[T // 2:], S, oracle, start=part)
    assert np.array_equal(ref.encode_mean(whole, T * S * S, oracle), out)


@pytest.mark.parametrize("S,T", ref.SHAPES)
def test_order_fixture_separates_every_alternative(oracle, cases, S, T):
    key = f"{S}_{T}"
    blocks, pinned = cases[f"blocks_{key}"], cases[f"pinned_{key}"]
    alt, altcode = cases[f"alt_{key}"], cases[f"altcode_{key}"]
    names = ref.alternatives_for(S)
    assert blocks.shape[1:] == (T, S, S) and blocks.dtype == np.uint8
    assert len(blocks) == len(pinned) == len(alt) == len(altcode)
    assert np.array_equal(ref.pinned_codes(blocks, oracle), pinned)
    for a, name in enumerate(names):
        sel = alt == a
        assert int(sel.sum()) >= ref.MIN_CASES, (S, T, name, int(sel.sum()))
        got = ref.ALTERNATIVES[name](blocks[sel], oracle)
        assert np.array_equal(got, altcode[sel]), (S, T, name)
        assert np.all(got != pinned[sel]), (S, T, name)
    assert set(np.unique(alt)) == set(range(len(names)))
    # float64 is the exact mean rounded once: the pinned code is never more than one code from it
    f64 = ref.alt_float64(blocks, oracle).astype(np.int32)
    assert np.abs(f64 - pinned.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("S,T", ref.SHAPES)
def test_float64_is_within_one_code_on_random_blocks(oracle, S, T):
    rng = np.random.default_rng(100 * S + T)
    blocks = rng.integers(0, 256, size=(100000, T, S, S), dtype=np.uint8)
    near = (rng.integers(6, 250, size=(100000, 1, 1, 1)) + rng.integers(-6, 7, size=blocks.shape)).astype(np.uint8)
    for b in (blocks, near):
        d = ref.alt_float64(b, oracle).astype(np.int32) - ref.pinned_codes(b, oracle).astype(np.int32)
        assert np.abs(d).max() <= 1
