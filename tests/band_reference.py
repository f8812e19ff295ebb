"""An independent model of the row-band layout behind frm_band_rows_for, frm_render_bands,
frm_render_bands_batch and frm_unshuffle_bands (include/frm.h): plain Python integers, which
never wrap, and numpy bytes. It imports neither frm.tiling nor the library: both are held to it
(test_band_reference.py, test_gpu_band_buffers.py).

The layout: band b covers frame rows [b * band_rows, (b + 1) * band_rows); a launch (a rank)
holds bands first, first + stride, ... below the band count, back to back. The frame's last band
may be short, but it keeps a whole slot of band_rows rows: the rows it lacks are padding."""
import numpy as np


def num_bands(h, band_rows):
    """Bands of a frame of h rows: ceil(h / band_rows)."""
    return -(-h // band_rows)


def rank_bands(h, band_rows, first, stride):
    """The bands a rank holds, in the order of its buffer (a range: huge counts stay cheap)."""
    return range(first, num_bands(h, band_rows), stride)


def rank_rows(h, band_rows, first, stride):
    """Rows of the rank's buffer: whole bands, the short last band included as a whole slot."""
    return len(rank_bands(h, band_rows, first, stride)) * band_rows


def valid_rows(h, band_rows, first, stride):
    """The rank's rows that hold frame rows: all but the rows the frame's last band lacks (only
    the rank that holds it has any, and they are its buffer's last rows)."""
    bands = rank_bands(h, band_rows, first, stride)
    if len(bands) == 0:
        return 0
    lacking = max(0, (bands[-1] + 1) * band_rows - h)
    return len(bands) * band_rows - lacking


def global_row(local_row, h, band_rows, first, stride):
    """The frame row that local row `local_row` of the rank's buffer holds, or -1 for padding."""
    if not 0 <= local_row < rank_rows(h, band_rows, first, stride):
        raise IndexError(f"local row {local_row} outside the rank's {rank_rows(h, band_rows, first, stride)} rows")
    slot, r = divmod(local_row, band_rows)
    y = (first + slot * stride) * band_rows + r
    return y if y < h else -1


def unshuffle(src_bytes, rank_stride_bytes, width, height, band_rows, ranks):
    """frm_unshuffle_bands: src_bytes is a flat uint8 array in which rank r's rows start at byte
    r * rank_stride_bytes (any stride, pads included). Every local row of every rank is scattered
    to the frame row it holds; returns the height x width x 4 frame. Padding is never read."""
    src = np.asarray(src_bytes, dtype=np.uint8).reshape(-1)
    pitch = width * 4
    frame = np.zeros((height, width, 4), np.uint8)
    seen = np.zeros(height, bool)
    for rank in range(ranks):
        for local in range(rank_rows(height, band_rows, rank, ranks)):
            y = global_row(local, height, band_rows, rank, ranks)
            if y < 0:
                continue
            at = rank * rank_stride_bytes + local * pitch
            assert not seen[y] and at + pitch <= src.size
            frame[y] = src[at:at + pitch].reshape(width, 4)
            seen[y] = True
    assert seen.all()
    return frame


def read_extent(rank_stride_bytes, width, height, band_rows, ranks):
    """The span [0, read_extent) of src bytes a reassembly may read: up to the end of the rows
    (whole bands) of the last rank that holds a band. Ranks beyond it are never touched."""
    last = min(ranks, num_bands(height, band_rows)) - 1
    return last * rank_stride_bytes + rank_rows(height, band_rows, last, ranks) * width * 4
