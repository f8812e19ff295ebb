"""Summation-order fixture of the motion blur's accumulation (run from the repo root:
`python tests/golden/make_shutter_cases.py`; well under a minute).

The accumulation's result is pinned bit for bit (tests/shutter_reference.py): the decoded texels of
the T sub-frames added in f32, sub-frame by sub-frame, each row by row, left to right, then one
correctly rounded division. Another order changes the final sRGB code only in rare blocks, and most
often where the samples are close to each other, as the sub-frames of a shutter interval are. This
script searches seeded random blocks of T x S x S codes drawn within +-SPREAD of a common base for
the ones where the pinned result differs from an alternative (pairwise sum, float64 accumulation,
for S > 1 the texel-major order) and keeps KEEP of them per (shape, alternative) pair, at least
shutter_reference.MIN_CASES (it searches further chunks until every pair has KEEP).

Output: tests/golden/shutter_order_cases.npz, for (S, T) in shutter_reference.SHAPES:
  blocks_S_T  [n, T, S, S] uint8  the texel codes (sub-frame k, row j, texel i)
  pinned_S_T  [n] uint8           the pinned code
  alt_S_T     [n] uint8           index into shutter_reference.alternatives_for(S): the alternative the
                                  block separates (it may separate others as well)
  altcode_S_T [n] uint8           that alternative's code
tests/test_shutter_reference.py re-derives every case from the oracle's tables."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import shutter_reference as ref  # noqa: E402
from oracle import frm_oracle as fo  # noqa: E402

OUT = os.path.join(HERE, "shutter_order_cases.npz")
SEED = 20240917
CHUNK = 1 << 18
KEEP = 10
SPREAD = 6
MAX_CHUNKS = 64


def search(S, T, rng):
    names = ref.alternatives_for(S)
    found = {n: [] for n in names}
    for chunk in range(MAX_CHUNKS):
        base = rng.integers(SPREAD, 256 - SPREAD, size=(CHUNK, 1, 1, 1))
        blocks = (base + rng.integers(-SPREAD, SPREAD + 1, size=(CHUNK, T, S, S))).astype(np.uint8)
        pin = ref.pinned_codes(blocks, fo)
        for n in names:
            if len(found[n]) >= KEEP:
                continue
            alt = ref.ALTERNATIVES[n](blocks, fo)
            for k in np.nonzero(alt != pin)[0][:KEEP - len(found[n])]:
                found[n].append((blocks[k].copy(), int(pin[k]), int(alt[k])))
        print(f"S={S} T={T} after {(chunk + 1) * CHUNK} blocks:", {n: len(v) for n, v in found.items()}, flush=True)
        if all(len(v) >= KEEP for v in found.values()):
            break
    short = {n: len(v) for n, v in found.items() if len(v) < ref.MIN_CASES}
    if short:
        raise SystemExit(f"S={S} T={T}: fewer than {ref.MIN_CASES} cases for {short}")
    blocks, pinned, alt_idx, alt_code = [], [], [], []
    for a, n in enumerate(names):
        for b, pc, ac in found[n]:
            blocks.append(b)
            pinned.append(pc)
            alt_idx.append(a)
            alt_code.append(ac)
    return (np.stack(blocks), np.array(pinned, np.uint8), np.array(alt_idx, np.uint8), np.array(alt_code, np.uint8))


def main():
    rng = np.random.default_rng(SEED)
    out = {}
    for S, T in ref.SHAPES:
        b, p, a, c = search(S, T, rng)
        key = f"{S}_{T}"
        out[f"blocks_{key}"], out[f"pinned_{key}"], out[f"alt_{key}"], out[f"altcode_{key}"] = b, p, a, c
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
