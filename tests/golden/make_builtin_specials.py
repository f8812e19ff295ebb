"""Record tests/golden/builtin_specials.json from the CPU oracle (run from the repo root:
`python tests/golden/make_builtin_specials.py [output.json]`; `--table` prints the rows of
DESIGN.md section 2's "Builtins outside the hot path's ranges" from the recorded file instead).

The file pins what frm semantics v3 gives the special inputs of tests/builtin_cases.py
(`specials(name)`): zeros, subnormals, the branch and clamp ends, huge and non-finite operands.
No accuracy bound exists out there; the bits are recorded, and tests/test_builtin_census.py asserts
that the oracle still reproduces them. Contents: {"builtins": {name: {"a": [...], "b": [...] (atan2:
a is y, b is x; pow: a is x, b is y), "out": [...]}}}, every float32 as 8 hex digits, every NaN
result as 7fc00000."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import builtin_cases as bc  # noqa: E402

PATH = os.path.join(HERE, "builtin_specials.json")


def record():
    from oracle import frm_oracle
    frm_oracle.load()
    hexes = lambda v: [f"{int(u):08x}" for u in v]  # noqa: E731
    out = {}
    for name in bc.NAMES:
        a, b = bc.specials(name)
        rec = {"a": hexes(bc.bits_of(a))}
        if b is not None:
            rec["b"] = hexes(bc.bits_of(b))
        rec["out"] = hexes(bc.canonical_bits(frm_oracle.math_fn(name, a, b)))
        out[name] = rec
    return {"semantics": "frm v3", "builtins": out}


def main():
    args = [a for a in sys.argv[1:] if a != "--table"]
    path = args[0] if args else PATH
    if "--table" in sys.argv[1:]:
        with open(path) as f:
            print("\n".join(bc.design_table(json.load(f))))
        return
    data = record()
    with open(path, "w") as f:
        json.dump(data, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{sum(len(v['a']) for v in data['builtins'].values())} specials written to {path}")


if __name__ == "__main__":
    main()
