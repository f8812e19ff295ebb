"""The presentation blit on the CPU. First tests/blit_reference.py is pinned by properties that do not
use its formulas (constant images, a monotone two-texel ramp with clamped ends, block centres of an
odd integer upscale, the middle texel of a 3:1 minification, the decode against mpmath); then the
case table's own conditions (caps, ties, spans) are checked on the reference alone; then the f32
oracle (om_blit) is held to the rules of tests/blit_cases.py on every case x source x flags."""
import mpmath as mp
import numpy as np
import pytest

import blit_cases as bc
import blit_reference as ref

SWAP = [2, 1, 0, 3]


def texels(codes_rgb):
    """[h, w, 3] codes -> an RGBA8 source with a varying alpha."""
    codes_rgb = np.asarray(codes_rgb, np.uint8)
    h, w = codes_rgb.shape[:2]
    alpha = (np.arange(h * w, dtype=np.uint32) * 37 % 256).astype(np.uint8).reshape(h, w, 1)
    return np.concatenate([codes_rgb, alpha], axis=-1)


# ---- 1. the reference, by properties that are not its formulas -------------------------------------

def test_decode_is_the_inverse_transfer_function():
    mp.mp.dps = 40
    got = ref.decode_table()
    for k in range(256):
        s = mp.mpf(k) / 255
        want = s / mp.mpf("12.92") if s <= mp.mpf("0.04045") else ((s + mp.mpf("0.055")) / mp.mpf("1.055")) ** mp.mpf("2.4")
        # float64: four roundings reach the base (k / 255, + 0.055, / 1.055 and that constant), the
        # power 2.4 multiplies them, pow adds one: (4 * 2.4 + 1) * 2^-53 < 2^-49
        assert abs(mp.mpf(float(got[k])) - want) <= want * mp.mpf(2) ** -49, k
    assert got[0] == 0.0 and got[255] == 1.0 and np.all(np.diff(got) > 0)


@pytest.mark.parametrize("dw,dh", [(21, 13), (8, 6), (3, 2), (5, 11), (16, 3)])  # linear, same, nearest, mixed x 2
def test_constant_image_stays_constant(dw, dh):
    mp.mp.dps = 40
    code = (188, 3, 77)
    src = texels(np.broadcast_to(np.array(code, np.uint8), (6, 8, 3)))
    srgb = ref.blit(src, dw, dh, ref.SRGB)
    assert srgb.shape == (dh, dw, 4)
    assert (srgb == np.array(code + (255,), np.uint8)).all()
    assert (ref.blit(src, dw, dh, ref.SRGB | ref.BGRA) == srgb[..., SWAP]).all()
    lin = [int(mp.floor(255 * (((mp.mpf(k) / 255 + mp.mpf("0.055")) / mp.mpf("1.055")) ** mp.mpf("2.4")
                               if k > 10 else mp.mpf(k) / 255 / mp.mpf("12.92")) + mp.mpf("0.5"))) for k in code]
    assert (ref.blit(src, dw, dh, 0) == np.array(lin + [255], np.uint8)).all()


@pytest.mark.parametrize("flags", bc.FLAGS)
@pytest.mark.parametrize("n", [8, 33, 200])
def test_two_texels_magnified_are_a_monotone_ramp_with_clamped_ends(n, flags):
    src = texels([[[10, 250, 128], [240, 5, 128]]])
    row = ref.blit(src, n, 1, flags)[0].astype(int)
    if flags & ref.BGRA:
        row = row[:, SWAP]
    assert np.all(np.diff(row[:, 0]) >= 0) and np.all(np.diff(row[:, 1]) <= 0) and np.all(row[:, 2] == row[0, 2])
    assert row[0, 0] < row[-1, 0] and row[0, 1] > row[-1, 1]
    # pixel centres (x + 1/2) / n left of 1/4 or right of 3/4 lie outside both texel centres
    x = np.arange(n) + 0.5
    left, right = x <= n / 4, x >= 3 * n / 4
    assert left.sum() >= n // 4 and right.sum() >= n // 4
    assert (row[left] == row[0]).all() and (row[right] == row[-1]).all()
    if flags & ref.SRGB:
        assert row[0].tolist() == [10, 250, 128, 255] and row[-1].tolist() == [240, 5, 128, 255]


@pytest.mark.parametrize("f", [3, 5, 7])
def test_odd_integer_upscale_reproduces_each_texel_at_its_block_centre(f):
    src = bc.source("random", 7, 5)
    out = ref.blit(src, 7 * f, 5 * f, ref.SRGB)
    centres = out[f // 2::f, f // 2::f]
    assert np.array_equal(centres[..., :3], src[..., :3]) and (out[..., 3] == 255).all()
    # between two block centres of a row every channel stays between the two texels
    y = f // 2
    for i in range(6):
        lo = np.minimum(src[0, i, :3], src[0, i + 1, :3])
        hi = np.maximum(src[0, i, :3], src[0, i + 1, :3])
        seg = out[y, i * f + f // 2:(i + 1) * f + f // 2 + 1, :3]
        assert np.all(seg >= lo) and np.all(seg <= hi), i


@pytest.mark.parametrize("flags", [ref.SRGB, ref.SRGB | ref.BGRA])
def test_three_to_one_minification_picks_the_middle_texel(flags):
    src = bc.source("random", 63, 45)
    want = src[1::3, 1::3].copy()
    want[..., 3] = 255
    assert np.array_equal(ref.blit(src, 21, 15, flags), want[..., SWAP] if flags & ref.BGRA else want)
    # minified along x alone, or along y alone: still nearest on both axes (the texel under the centre)
    assert np.array_equal(ref.blit(src, 21, 45, ref.SRGB)[..., :3], src[:, 1::3, :3])
    assert np.array_equal(ref.blit(src, 63, 15, ref.SRGB)[..., :3], src[1::3, :, :3])
    assert np.array_equal(ref.blit(src, 21, 135, ref.SRGB)[..., :3], src[:, 1::3, :3].repeat(3, axis=0))
    assert np.array_equal(ref.blit(src, 189, 15, ref.SRGB)[..., :3], src[1::3, :, :3].repeat(3, axis=1))


def test_rows_and_columns_are_not_exchanged():
    """A source that varies along x only gives an output that varies along x only, and likewise y;
    row 0 of the output is the top of the source."""
    ramp = np.linspace(0, 255, 12).astype(np.uint8)
    along_x = texels(np.broadcast_to(ramp[None, :, None], (7, 12, 3)))
    along_y = texels(np.broadcast_to(ramp[:7, None, None], (7, 12, 3)))
    for dw, dh in ((30, 20), (5, 3), (30, 3), (5, 20)):
        ox, oy = ref.blit(along_x, dw, dh, 1).astype(int), ref.blit(along_y, dw, dh, 1).astype(int)
        assert (ox == ox[:1]).all() and np.all(np.diff(ox[0, :, 0]) >= 0) and ox[0, 0, 0] < ox[0, -1, 0]
        assert (oy == oy[:, :1]).all() and np.all(np.diff(oy[:, 0, 0]) >= 0) and oy[0, 0, 0] < oy[-1, 0, 0]


# ---- 2. the case table's conditions, from the reference alone -------------------------------------

def test_the_table_holds_what_it_must():
    assert bc.K <= 16
    zero = [k for k, c in bc.CASES.items() if c.cap == 0.0 and c.cap_srgb == 0.0]
    assert len(zero) >= 8, zero
    for k, c in bc.CASES.items():
        linear = ref.is_linear(c.sw, c.sh, c.dw, c.dh)
        assert k.startswith(("mag-", "same-")) == linear, k
        if c.tie:  # an even integer minification ratio on an axis
            assert not linear and any(s % d == 0 and (s // d) % 2 == 0 for s, d in ((c.sw, c.dw), (c.sh, c.dh))), k
        else:
            assert c.cap <= (bc.MAGNIFY_CAP if linear else 0.34) and c.cap_srgb <= c.cap, k
    for k in bc.MIXED:
        c = bc.CASES[k]
        assert (c.sw < c.dw) != (c.sh < c.dh) and not ref.is_linear(c.sw, c.sh, c.dw, c.dh), k
    sizes_w = {c.dw for c in bc.CASES.values()}
    sizes_h = {c.dh for c in bc.CASES.values()}
    assert {15, 16, 17} <= sizes_w and {63, 64, 65} <= sizes_h  # both sides of a block edge
    assert any(1 in (c.sw, c.sh) for c in bc.CASES.values())


@pytest.mark.parametrize("case_id", list(bc.CASES))
def test_open_share_is_under_the_cap(case_id):
    c = bc.CASES[case_id]
    for name in bc.SOURCES:
        for flags in bc.FLAGS:
            e = bc.expectation(case_id, name, flags)
            print(f"{case_id} {name} flags {flags}: open {100 * e.share:.2f} %, span {e.span}")
            assert e.span <= 1, (name, flags)  # never more than two codes in an interval
            assert not len(bc.violations(e.image, e)), (name, flags)  # the reference keeps its own rules
            if c.tie:
                assert e.open.all(), (name, flags)
            else:
                assert e.share <= bc.cap(case_id, flags), (name, flags, e.share)


# ---- 3. the f32 oracle held to the rules ------------------------------------------------------------

@pytest.mark.parametrize("flags", bc.FLAGS)
@pytest.mark.parametrize("case_id", list(bc.CASES))
def test_oracle_blit_keeps_the_rules(oracle, case_id, flags):
    c = bc.CASES[case_id]
    for name in bc.SOURCES:
        src = bc.source(name, c.sw, c.sh)
        got = oracle.blit(src, c.dw, c.dh, flags)
        e = bc.expectation(case_id, name, flags)
        bad = bc.violations(got, e)
        assert not len(bad), (name, bc.describe(got, e, bad))
        decided = ~e.open
        assert np.array_equal(got[decided], e.image[decided]), name  # follows from the rules; states them plainly


def test_oracle_same_size_srgb_is_the_source(oracle):
    for name in bc.SOURCES:
        src = bc.source(name, 64, 48)
        want = src.copy()
        want[..., 3] = 255
        assert np.array_equal(oracle.blit(src, 64, 48, 1), want), name
        assert np.array_equal(oracle.blit(src, 64, 48, 3), want[..., SWAP]), name
