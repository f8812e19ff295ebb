"""Summation-order fixture of the supersampling resolve (run from the repo root:
`python tests/golden/make_ssaa_cases.py`; a minute or two).

The resolve's result is pinned bit for bit (tests/ssaa_reference.py): decoded texels added in f32
row by row, left to right, one correctly rounded division. Another order changes the final sRGB
code in a few blocks per million only, so random images barely tell the orders apart. This script
searches seeded random S x S code blocks for the ones where the pinned result differs from an
alternative (pairwise sum, column-major sum, float64 accumulation; for S = 3 also the multiply by
1.0f/9 and the pre-scaled terms) and keeps up to KEEP of them per (S, alternative) pair, at least
ssaa_reference.MIN_CASES (it searches further chunks until every pair has that many).

Output: tests/golden/ssaa_order_cases.npz, for S in 2, 3, 4:
  blocks_S  [n, S, S] uint8   the texel codes (row j, texel i)
  pinned_S  [n] uint8         the pinned code
  alt_S     [n] uint8         index into ssaa_reference.alternatives_for(S): the alternative the
                              block separates (it may separate others as well)
  altcode_S [n] uint8         that alternative's code
tests/test_ssaa_reference.py re-derives every case from the oracle's tables."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ssaa_reference as ref  # noqa: E402
from oracle import frm_oracle as fo  # noqa: E402

OUT = os.path.join(HERE, "ssaa_order_cases.npz")
SEED = 20240611
CHUNK = 1 << 20
KEEP = 12
MAX_CHUNKS = 64


def search(S, rng):
    names = ref.alternatives_for(S)
    found = {n: [] for n in names}
    for chunk in range(MAX_CHUNKS):
        blocks = rng.integers(0, 256, size=(CHUNK, S, S), dtype=np.uint8)
        pin = ref.pinned_codes(blocks, S, fo)
        for n in names:
            if len(found[n]) >= KEEP:
                continue
            alt = ref.ALTERNATIVES[n](blocks, S, fo)
            for k in np.nonzero(alt != pin)[0][:KEEP - len(found[n])]:
                found[n].append((blocks[k].copy(), int(pin[k]), int(alt[k])))
        print(f"S={S} after {(chunk + 1) * CHUNK} blocks:", {n: len(v) for n, v in found.items()}, flush=True)
        if all(len(v) >= KEEP for v in found.values()):
            break
    short = {n: len(v) for n, v in found.items() if len(v) < ref.MIN_CASES}
    if short:
        raise SystemExit(f"S={S}: fewer than {ref.MIN_CASES} cases for {short}")
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
    for S in ref.FACTORS:
        b, p, a, c = search(S, rng)
        out[f"blocks_{S}"], out[f"pinned_{S}"], out[f"alt_{S}"], out[f"altcode_{S}"] = b, p, a, c
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
