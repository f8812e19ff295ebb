"""Expected values of the motion blur's accumulation (include/frm.h frm_render_shutter,
frm_accumulate): the numpy float32 restatement of the pinned semantics, and the alternatives the
summation-order fixture (tests/golden/shutter_order_cases.npz) separates it from.

With T sub-frames of S*H rows of S*W RGBA8 sRGB texels and D = oracle.srgb_decode(), output pixel
(X, Y) is, for each of R, G, B:

    sum = 0.0f
    for k in 0..T-1:              # sub-frames, in the order given
      for j in 0..S-1:            # source rows, top to bottom
        for i in 0..S-1:          # texels, left to right
          sum = sum + D[frame[k][S*Y+j][S*X+i].c]     # f32 adds, exactly this order
    mean = sum / (float)(T*S*S)   # correctly rounded f32 division
    code = encode_srgb(mean)      # the sRGB store's threshold table

Alpha is 255. T = 1 is ssaa_reference.box_resolve.
"""
import numpy as np


def accumulate_sum(frames, S, oracle, start=None):
    """frames: [T, S*H, S*W, 4] uint8 -> the [H, W, 3] float32 sums, continuing from `start`."""
    frames = np.asarray(frames, dtype=np.uint8)
    assert frames.ndim == 4 and frames.shape[3] == 4 and frames.shape[1] % S == 0 and frames.shape[2] % S == 0
    D = oracle.srgb_decode()
    H, W = frames.shape[1] // S, frames.shape[2] // S
    acc = np.zeros((H, W, 3), dtype=np.float32) if start is None else np.array(start, dtype=np.float32)
    for k in range(len(frames)):
        for j in range(S):
            for i in range(S):
                acc = acc + D[frames[k, j::S, i::S, :3]]
    assert acc.dtype == np.float32
    return acc


def encode_mean(acc, divisor, oracle):
    """The frame [H, W, 4] uint8 of the sums acc / divisor."""
    mean = acc / np.float32(divisor)
    assert mean.dtype == np.float32
    out = np.empty(acc.shape[:2] + (4,), dtype=np.uint8)
    out[..., :3] = oracle.encode_srgb(np.ascontiguousarray(mean))
    out[..., 3] = 255
    return out


def accumulate(frames, S, oracle):
    """frames: [T, S*H, S*W, 4] uint8 sRGB texels -> [H, W, 4] uint8, the pinned mean."""
    frames = np.asarray(frames, dtype=np.uint8)
    return encode_mean(accumulate_sum(frames, S, oracle), len(frames) * S * S, oracle)


# ---- the order fixture: codes of n blocks [n, T, S, S] (sub-frame k, row j, texel i) ----------------

def _encode(oracle, mean):
    assert mean.dtype == np.float32
    return oracle.encode_srgb(np.ascontiguousarray(mean))


def pinned_codes(blocks, oracle):
    n, T, S, _ = blocks.shape
    v = oracle.srgb_decode()[blocks]
    acc = np.zeros(n, dtype=np.float32)
    for k in range(T):
        for j in range(S):
            for i in range(S):
                acc = acc + v[:, k, j, i]
    return _encode(oracle, acc / np.float32(T * S * S))


def _pairwise(terms):
    terms = list(terms)
    while len(terms) > 1:
        nxt = [terms[k] + terms[k + 1] for k in range(0, len(terms) - 1, 2)]
        if len(terms) % 2:
            nxt.append(terms[-1])
        terms = nxt
    return terms[0]


def alt_pairwise(blocks, oracle):
    """A tree sum over the samples in the pinned order: (t0 + t1) + (t2 + t3), ...; an odd one carried up."""
    n, T, S, _ = blocks.shape
    v = oracle.srgb_decode()[blocks].reshape(n, T * S * S)
    acc = _pairwise([v[:, k] for k in range(T * S * S)])
    return _encode(oracle, acc / np.float32(T * S * S))


def alt_float64(blocks, oracle):
    """Accumulate and divide in float64, round the mean to f32 once."""
    n, T, S, _ = blocks.shape
    v = oracle.srgb_decode()[blocks].astype(np.float64).reshape(n, T * S * S)
    return _encode(oracle, (v.sum(axis=1) / float(T * S * S)).astype(np.float32))


def alt_texel_major(blocks, oracle):
    """Sequential f32 adds with the sub-frames innermost: texel (j, i) of every sub-frame, then the next texel."""
    n, T, S, _ = blocks.shape
    v = oracle.srgb_decode()[blocks]
    acc = np.zeros(n, dtype=np.float32)
    for j in range(S):
        for i in range(S):
            for k in range(T):
                acc = acc + v[:, k, j, i]
    return _encode(oracle, acc / np.float32(T * S * S))


ALTERNATIVES = {"pairwise": alt_pairwise, "float64": alt_float64, "texel_major": alt_texel_major}
SHAPES = ((1, 8), (1, 32), (2, 4), (3, 2))  # (S, T) of the fixture
MIN_CASES = 8  # per (shape, alternative) pair in the fixture


def alternatives_for(S):
    """The alternatives that can differ at factor S: with one texel per sub-frame the texel-major
    order is the pinned one."""
    return ["pairwise", "float64"] + (["texel_major"] if S > 1 else [])
