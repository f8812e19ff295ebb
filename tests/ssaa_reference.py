"""Expected values of the supersampling resolve (include/frm.h frm_set_supersampling, frm_resolve):
the numpy float32 restatement of the pinned semantics, and the alternatives the summation-order
fixture (tests/golden/ssaa_order_cases.npz) separates it from.

For output pixel (X, Y) and each of R, G, B, with D = oracle.srgb_decode():

    sum = 0.0f
    for j in 0..S-1:            # source rows, top to bottom
      for i in 0..S-1:          # texels of the row, left to right
        sum = sum + D[hi[S*Y+j][S*X+i].c]        # f32 adds, in this order
    mean = sum / (float)(S*S)                     # correctly rounded f32 division
    code = encode_srgb(mean)                      # the sRGB store's threshold table

Alpha is 255; S = 1 is the identity on R, G, B.
"""
import numpy as np


def box_resolve(hi, S, oracle):
    """hi: [S*H, S*W, 4] uint8 sRGB texels -> [H, W, 4] uint8, the pinned resolve."""
    hi = np.asarray(hi, dtype=np.uint8)
    assert hi.ndim == 3 and hi.shape[2] == 4 and hi.shape[0] % S == 0 and hi.shape[1] % S == 0
    D = oracle.srgb_decode()
    H, W = hi.shape[0] // S, hi.shape[1] // S
    acc = np.zeros((H, W, 3), dtype=np.float32)
    for j in range(S):
        for i in range(S):
            acc = acc + D[hi[j::S, i::S, :3]]
    mean = acc / np.float32(S * S)
    assert acc.dtype == np.float32 and mean.dtype == np.float32
    out = np.empty((H, W, 4), dtype=np.uint8)
    out[..., :3] = oracle.encode_srgb(mean)
    out[..., 3] = 255
    return out


# ---- the order fixture: codes of n blocks [n, S, S] (row j, texel i) under each summation ------------

def _encode(oracle, mean):
    assert mean.dtype == np.float32
    return oracle.encode_srgb(np.ascontiguousarray(mean))


def pinned_codes(blocks, S, oracle):
    v = oracle.srgb_decode()[blocks]
    acc = np.zeros(len(blocks), dtype=np.float32)
    for j in range(S):
        for i in range(S):
            acc = acc + v[:, j, i]
    return _encode(oracle, acc / np.float32(S * S))


def _pairwise(terms):
    terms = list(terms)
    while len(terms) > 1:
        nxt = [terms[k] + terms[k + 1] for k in range(0, len(terms) - 1, 2)]
        if len(terms) % 2:
            nxt.append(terms[-1])
        terms = nxt
    return terms[0]


def alt_pairwise(blocks, S, oracle):
    """A tree sum over the row-major texel list: (t0 + t1) + (t2 + t3), ...; an odd one carried up."""
    v = oracle.srgb_decode()[blocks].reshape(len(blocks), S * S)
    acc = _pairwise([v[:, k] for k in range(S * S)])
    return _encode(oracle, acc / np.float32(S * S))


def alt_column_major(blocks, S, oracle):
    v = oracle.srgb_decode()[blocks]
    acc = np.zeros(len(blocks), dtype=np.float32)
    for i in range(S):
        for j in range(S):
            acc = acc + v[:, j, i]
    return _encode(oracle, acc / np.float32(S * S))


def alt_float64(blocks, S, oracle):
    """Accumulate and divide in float64, round the mean to f32 once."""
    v = oracle.srgb_decode()[blocks].astype(np.float64).reshape(len(blocks), S * S)
    return _encode(oracle, (v.sum(axis=1) / float(S * S)).astype(np.float32))


def alt_reciprocal(blocks, S, oracle):
    """sum * (1.0f / (S*S)) instead of the division."""
    v = oracle.srgb_decode()[blocks]
    acc = np.zeros(len(blocks), dtype=np.float32)
    for j in range(S):
        for i in range(S):
            acc = acc + v[:, j, i]
    return _encode(oracle, acc * (np.float32(1.0) / np.float32(S * S)))


def alt_prescale(blocks, S, oracle):
    """Each term multiplied by 1.0f / (S*S) before the sequential sum."""
    v = oracle.srgb_decode()[blocks] * (np.float32(1.0) / np.float32(S * S))
    acc = np.zeros(len(blocks), dtype=np.float32)
    for j in range(S):
        for i in range(S):
            acc = acc + v[:, j, i]
    return _encode(oracle, acc)


ALTERNATIVES = {"pairwise": alt_pairwise, "column_major": alt_column_major, "float64": alt_float64,
                "reciprocal": alt_reciprocal, "prescale": alt_prescale}
FACTORS = (2, 3, 4)
MIN_CASES = 8  # per (S, alternative) pair in the fixture


def alternatives_for(S):
    """The alternatives that can differ at factor S: with S*S a power of two the reciprocal and the
    pre-scaling are exact, so they are searched for S = 3 only."""
    names = ["pairwise", "column_major", "float64"]
    if S == 3:
        names += ["reciprocal", "prescale"]
    return names
