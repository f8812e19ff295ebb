"""The row arithmetic of the band entry points against tests/band_reference.py (plain Python
integers): frm_band_rows_for on a grid and at the edges of its 32-bit arguments, where a band
count computed as (height + band_rows - 1) / band_rows wraps; frm_group_band_rows against a
restatement of its rule; and frm/tiling.py, the product's own Python geometry, held to the same
model instead of serving as a reference. No GPU."""
import ctypes

import numpy as np
import pytest

import band_reference as model
from frm import _lib, tiling

U32 = 0xFFFFFFFF
UNTOUCHED = 0xDEADBEEF

GRID_HEIGHTS = range(1, 41)
GRID_BAND_ROWS = range(1, 46)
GRID_STRIDES = range(1, 6)
GRID_FIRSTS = range(0, 7)


def lib_rows(lib, h, band_rows, first, stride):
    """(status, *out_rows) of frm_band_rows_for; *out_rows starts as UNTOUCHED."""
    out = ctypes.c_uint32(UNTOUCHED)
    rc = lib.frm_band_rows_for(h, band_rows, first, stride, ctypes.byref(out))
    return rc, out.value


def expected_rows(h, band_rows, first, stride):
    """What frm_band_rows_for owes the model: its row count, or a refusal that leaves *out_rows
    alone where the count does not fit the uint32_t output."""
    rows = model.rank_rows(h, band_rows, first, stride)
    return (_lib.FRM_OK, rows) if rows <= U32 else (_lib.FRM_ERR_INVALID_ARGUMENT, UNTOUCHED)


def test_model_by_hand():
    """The model itself, against layouts written out by hand."""
    # 5 rows in bands of 2 over 2 ranks: bands 0 1 2 -> rank 0 holds 0 and 2 (row 4 and a pad), rank 1 holds 1
    assert model.num_bands(5, 2) == 3
    assert list(model.rank_bands(5, 2, 0, 2)) == [0, 2] and list(model.rank_bands(5, 2, 1, 2)) == [1]
    assert model.rank_rows(5, 2, 0, 2) == 4 and model.valid_rows(5, 2, 0, 2) == 3
    assert model.rank_rows(5, 2, 1, 2) == 2 and model.valid_rows(5, 2, 1, 2) == 2
    assert [model.global_row(i, 5, 2, 0, 2) for i in range(4)] == [0, 1, 4, -1]
    assert [model.global_row(i, 5, 2, 1, 2) for i in range(2)] == [2, 3]
    with pytest.raises(IndexError):
        model.global_row(2, 5, 2, 1, 2)
    # one band taller than the frame: 6 rows in a slot of 9, the second rank empty
    assert model.rank_rows(6, 9, 0, 2) == 9 and model.valid_rows(6, 9, 0, 2) == 6
    assert model.rank_rows(6, 9, 1, 2) == 0 and model.valid_rows(6, 9, 1, 2) == 0
    # 8 x 5 texels, bands of 2, 2 ranks 4 rows (128 bytes) apart: rank 1's one band ends at 128 + 64
    assert model.read_extent(128, 8, 5, 2, 2) == 192
    # 5 ranks for 2 bands: ranks 2..4 are never read, whatever the stride
    assert model.read_extent(100, 8, 4, 2, 5) == 100 + 64
    assert model.read_extent(64, 12, 5, 2, 1) == 6 * 48  # one rank: its three slots, the pad row included
    src = np.arange(2 * 128, dtype=np.uint8)
    got = model.unshuffle(src, 128, 8, 5, 2, 2)
    rows = [src[0:32], src[32:64], src[128:160], src[160:192], src[64:96]]
    assert np.array_equal(got.reshape(5, 32), np.stack(rows))


def test_model_is_consistent_on_the_grid():
    """valid_rows counts the local rows global_row places; the ranks' bands partition the frame's."""
    for h in GRID_HEIGHTS:
        for br in GRID_BAND_ROWS:
            for ranks in GRID_STRIDES:
                held = []
                for rank in range(ranks):
                    rows = [model.global_row(i, h, br, rank, ranks) for i in range(model.rank_rows(h, br, rank, ranks))]
                    placed = [y for y in rows if y >= 0]
                    assert len(placed) == model.valid_rows(h, br, rank, ranks)
                    assert rows[len(placed):] == [-1] * (len(rows) - len(placed))  # padding comes last
                    held += placed
                assert sorted(held) == list(range(h))


def test_band_rows_for_equals_the_model_on_the_grid(frm_lib):
    wrong = []
    for h in GRID_HEIGHTS:
        for br in GRID_BAND_ROWS:
            for stride in GRID_STRIDES:
                for first in GRID_FIRSTS:
                    got, want = lib_rows(frm_lib, h, br, first, stride), expected_rows(h, br, first, stride)
                    if got != want:
                        wrong.append(((h, br, first, stride), got, want))
    assert not wrong, wrong[:10]


EDGES = [
    # first_band at and beyond the band count (10 rows in bands of 3: 4 bands)
    (10, 3, 3, 1), (10, 3, 4, 1), (10, 3, 5, 1), (10, 3, 3, 2), (10, 3, 4, 2), (10, 3, 1000, 7),
    # band_rows above the height
    (5, 9, 0, 1), (5, 9, 0, 2), (5, 9, 1, 2), (1, 45, 0, 1),
    # the largest frame, split into the most bands, into two and into one
    (32768, 1, 0, 1), (32768, 1, 1, 2), (32768, 1, 32767, 1), (32768, 1, 32768, 1),
    (32768, 32767, 0, 1), (32768, 32767, 1, 1), (32768, 32767, 0, 2), (32768, 32767, 1, 2), (32768, 32767, 2, 1),
    (32768, 32768, 0, 1), (32768, 32768, 0, 2), (32768, 32768, 1, 1), (32768, 32768, 1, 2),
    # stride and first at the top of their type
    (10, 3, 0, U32), (10, 3, 3, U32), (10, 3, U32, 1), (10, 3, U32, U32), (10, 3, U32 - 1, 2), (32768, 1, 0, U32),
    # the top of the other two, where nothing wraps
    (U32, 1, 0, 1), (U32, 1, U32 - 1, 1), (U32, 1, U32, 1), (U32 - 1, 1, 0, 2), (32768, 0xFFFF8000, 0, 1),
    (32768, 0xFFFF8000, 1, 1),
]
# height + band_rows - 1 does not fit 32 bits: the first three hold one band, the last one's 2^31
# bands of 2 rows are one row more than *out_rows can say
WRAPS = [(2, U32, 0, 1), (16, 0xFFFFFFF8, 0, 1), (32768, 0xFFFF8001, 0, 1), (U32, 2, 0, 1)]


@pytest.mark.parametrize("h,band_rows,first,stride", EDGES + WRAPS)
def test_band_rows_for_equals_the_model_at_the_edges(frm_lib, h, band_rows, first, stride):
    assert lib_rows(frm_lib, h, band_rows, first, stride) == expected_rows(h, band_rows, first, stride)


def test_the_wrap_rows_are_what_the_model_says():
    """The expectations of WRAPS, spelled out: they come from the model, not from the library."""
    assert [model.rank_rows(*c) for c in WRAPS] == [U32, 0xFFFFFFF8, 0xFFFF8001, 1 << 32]
    assert [expected_rows(*c)[0] for c in WRAPS] == [_lib.FRM_OK] * 3 + [_lib.FRM_ERR_INVALID_ARGUMENT]


def group_band_rows(h, n):
    """frm_group_band_rows' rule (the smallest band height >= 16 that splits the frame into a
    multiple of n bands, else 16), restated from the other end: the frame is n * k bands of
    h / (n * k) rows, and the largest k that leaves 16 rows gives the smallest height."""
    for k in range(h // (16 * n), 0, -1):
        if h % (n * k) == 0:
            return h // (n * k)
    return 16


def test_group_band_rows_equals_its_rule_and_covers_every_band_once(frm_lib):
    for h in range(1, 301):
        for n in range(1, 17):
            out = ctypes.c_uint32(UNTOUCHED)
            assert frm_lib.frm_group_band_rows(h, n, ctypes.byref(out)) == _lib.FRM_OK
            br = out.value
            assert br == group_band_rows(h, n), (h, n)
            held = sorted(b for r in range(n) for b in model.rank_bands(h, br, r, n))
            assert held == list(range(model.num_bands(h, br))), (h, n)
            rows = [lib_rows(frm_lib, h, br, r, n) for r in range(n)]
            assert rows == [(_lib.FRM_OK, model.rank_rows(h, br, r, n)) for r in range(n)], (h, n)
            assert sum(v for _, v in rows) == model.num_bands(h, br) * br
            if h % (16 * n) == 0:
                assert len(set(rows)) == 1  # the split it is made for: every device the same rows


def test_tiling_geometry_equals_the_model_on_the_grid():
    for h in GRID_HEIGHTS:
        for br in GRID_BAND_ROWS:
            assert tiling.num_bands(h, br) == model.num_bands(h, br)
            for ranks in GRID_STRIDES:
                assert tiling.rank_buffer_rows(h, br, ranks) == max(model.rank_rows(h, br, r, ranks) for r in range(ranks))
                for rank in GRID_FIRSTS:
                    key = (h, br, rank, ranks)
                    rows = model.rank_rows(*key)
                    assert tiling.rank_rows(*key) == rows, key
                    assert tiling.bands_of_rank(*key) == list(model.rank_bands(*key)), key
                    assert tiling.global_rows(*key) == [model.global_row(i, *key) for i in range(rows)], key


def test_tiling_unshuffle_equals_the_model_on_the_grid():
    rng = np.random.default_rng(20)
    width = 3
    for h in GRID_HEIGHTS:
        for br in GRID_BAND_ROWS:
            for ranks in GRID_STRIDES:
                buffer_rows = model.rank_rows(h, br, 0, ranks)
                gathered = rng.integers(0, 256, (ranks, buffer_rows, width, 4), dtype=np.uint8)
                want = model.unshuffle(gathered.reshape(-1), buffer_rows * width * 4, width, h, br, ranks)
                assert np.array_equal(tiling.unshuffle(gathered, h, br, ranks), want), (h, br, ranks)


def test_tiling_choose_band_rows_equals_the_rule():
    for h in range(1, 301):
        for n in range(1, 17):
            assert tiling.choose_band_rows(h, n) == group_band_rows(h, n), (h, n)
