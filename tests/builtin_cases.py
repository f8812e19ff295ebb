"""Input sets for the eight frm builtins over all of float32, shared by the CPU census test
(test_builtin_census.py) and the GPU test (test_gpu_builtins_whole_type.py). Every set is built
from encodings with fixed seeds: plain data, no code under test.

`whole_type()` holds every sign and exponent field with 1,036 mantissas each. `sets(name)` gives a
builtin's named sets, `(label, a, b)` with b None for the unary ones: the whole type and dense
neighbourhoods (4,096 consecutive encodings either side of a value unless stated otherwise) of the
inputs at which frm_math.h takes another branch or leans on frexp, ldexp, rint, minNum / maxNum,
the float to int conversion or subnormal arithmetic. `strata(name)` names, from numpy alone, what
the union of a builtin's sets must reach; test_builtin_census.py fails when one is missed.
`specials(name)` is the fixed list whose oracle bits tests/golden/builtin_specials.json records."""
import numpy as np

NAMES = ("sin", "cos", "acos", "atan2", "log", "log2", "exp2", "pow")
BINARY = ("atan2", "pow")
MAX_SET = 1_500_000
HOOD = 4096

SQRT2_MANT = 0x3504F3  # the mantissa field of f32(sqrt 2) and of f32(sqrt 1/2): log_split_'s cut
FIXED_MANTISSAS = (0, 1, 2, 3, 0x7FFFFE, 0x7FFFFF, 0x3FFFFF, 0x400000, 0x400001,
                   SQRT2_MANT - 1, SQRT2_MANT, SQRT2_MANT + 1)
RANDOM_MANTISSAS = 1024

INV_PI_HI = float(np.float32(float.fromhex("0x1.45f306p-2")))  # frm_math.h kInvPiHi
FLT_MAX = float(np.finfo(np.float32).max)
SQRT_HALF = float(np.float32(0.70710677))
PI = float(np.float32(np.pi))
HALF_PI = float(np.float32(np.pi / 2))
# the float32 whose product with kInvPiHi is nearest 2^24: sincos_'s parity rule changes there
PARITY_X = float(np.float32(2.0 ** 24 / INV_PI_HI))

SNAN = np.array([0x7F800001], np.uint32).view(np.float32)[0]  # a signalling NaN (the quiet bit clear)

EXP2_TARGETS = (-151.0, -149.0, -126.0, 128.0, 129.0)  # of y * log2(x) in pow's pairs
ATAN2_THRESHOLDS = (2.0 ** -128, 2.0 ** -126, 2.0 ** 126)
POW_Y_SPECIALS = (0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.0, 3.0, 16.0, 100.0, np.inf, -np.inf, np.nan)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        v = make()
        for arr in (v if isinstance(v, tuple) else (v,)):
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def f32(bits):
    """float32 of uint32 encodings."""
    return np.ascontiguousarray(np.asarray(bits).astype(np.uint32)).view(np.float32)


def bits_of(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def mag_bits(x):
    """The encodings without their sign bit, as int64 (ordered like the magnitudes, NaN last)."""
    return (bits_of(x) & np.uint32(0x7FFFFFFF)).astype(np.int64)


def around(x, k=HOOD, signs=(1,)):
    """The float32 within k encodings of x on either side (never across zero or past inf), for
    each of `signs` times x."""
    out = []
    for s in signs:
        b = int(np.float32(s * x).view(np.uint32))
        sign, mag = b & 0x80000000, b & 0x7FFFFFFF
        m = np.arange(max(mag - k, 0), min(mag + k, 0x7F800000) + 1, dtype=np.int64)
        out.append(f32(m | sign))
    return np.concatenate(out)


def both(x, k=HOOD):
    return around(x, k, signs=(1, -1))


def whole_type():
    """530,432 float32: each sign x each of the 256 exponent fields (0: zeros and subnormals,
    255: inf and NaN) x (FIXED_MANTISSAS + 1,024 seeded random mantissas)."""
    def make():
        rng = np.random.default_rng(2301)
        mant = np.concatenate([np.broadcast_to(np.array(FIXED_MANTISSAS, np.uint32), (2, 256, len(FIXED_MANTISSAS))),
                               rng.integers(0, 1 << 23, (2, 256, RANDOM_MANTISSAS), dtype=np.uint32)], axis=-1)
        sign = (np.arange(2, dtype=np.uint32) << np.uint32(31))[:, None, None]
        exp = (np.arange(256, dtype=np.uint32) << np.uint32(23))[None, :, None]
        return f32((sign | exp | mant).ravel())
    return _cached("whole_type", make)


def thinned():
    """444 float32: both signs x (every 8th exponent field and fields 0, 1, 2, 253, 254, 255) x
    (mantissas 0, 1, 0x7FFFFF and 3 seeded random ones): the operands of the pair sets."""
    def make():
        rng = np.random.default_rng(444)
        fields = np.array(sorted(set(range(0, 256, 8)) | {0, 1, 2, 253, 254, 255}), np.uint32)
        mant = np.concatenate([np.broadcast_to(np.array([0, 1, 0x7FFFFF], np.uint32), (2, len(fields), 3)),
                               rng.integers(2, 0x7FFFFF, (2, len(fields), 3), dtype=np.uint32)], axis=-1)
        sign = (np.arange(2, dtype=np.uint32) << np.uint32(31))[:, None, None]
        return f32((sign | (fields << np.uint32(23))[None, :, None] | mant).ravel())
    return _cached("thinned", make)


def _smallest(k=HOOD):
    """+-0 and the k smallest subnormals of either sign."""
    m = np.arange(0, k + 1, dtype=np.int64)
    return f32(np.concatenate([m, m | 0x80000000]))


# ---- the sets ------------------------------------------------------------------------------------
def tie_centres():
    """+-(j + 1/2) pi for j = 0..64 as float32: where the half-turn reduction's rint ties."""
    c = np.array([(j + 0.5) * np.pi for j in range(65)]).astype(np.float32)
    return np.concatenate([c, -c])


def _sincos_sets():
    hoods = np.concatenate([both(2.0 ** 20), both(PARITY_X), both(PI), both(HALF_PI), _smallest()])
    ties = np.concatenate([around(float(c)) for c in tie_centres()])
    return [("whole_type", whole_type(), None), ("branch_parity_zero", hoods, None), ("rint_ties", ties, None)]


def _acos_sets():
    hoods = np.concatenate([both(1.0), _smallest(), both(0.5)])
    return [("whole_type", whole_type(), None), ("ends_zero_half", hoods, None)]


def powers_of_two():
    return np.exp2(np.arange(-149, 128, dtype=np.float64)).astype(np.float32)


def sqrt_half_cuts():
    """f32(sqrt 1/2) 2^e for e in {-126, -1, 0, 1, 127}: frexp's mantissa sits on the cut there
    (e = -126 is a subnormal)."""
    return np.array([SQRT_HALF * 2.0 ** e for e in (-126, -1, 0, 1, 127)]).astype(np.float32)


def _log_sets():
    rng = np.random.default_rng(126)
    hoods = [around(1.0), around(2.0 ** -126), around(FLT_MAX)]
    hoods += [around(float(c)) for c in sqrt_half_cuts()]
    hoods += [np.concatenate([around(float(p), 2) for p in powers_of_two()])]
    hoods += [f32(rng.integers(1, 1 << 23, 20000, dtype=np.uint32))]
    return [("whole_type", whole_type(), None), ("cuts_powers_subnormals", np.concatenate(hoods), None)]


def exp2_halves():
    """Every integer and half-integer of [-152, 130]."""
    return (np.arange(-304, 261) * 0.5).astype(np.float32)


def _exp2_sets():
    rng = np.random.default_rng(149)
    hoods = [np.concatenate([around(float(h), 2) for h in exp2_halves()])]
    hoods += [around(v) for v in (-149.0, -126.0, 127.0, 128.0)]
    hoods += [rng.uniform(-152.0, -125.0, 100000).astype(np.float32)]
    return [("whole_type", whole_type(), None), ("ties_clamps_subnormal_results", np.concatenate(hoods), None)]


def _signs(rng, n):
    return rng.choice(np.array([-1.0, 1.0], np.float32), n)


def _atan2_sets():
    t = thinned()
    y, x = (g.ravel() for g in np.meshgrid(t, t, indexing="ij"))
    rng = np.random.default_rng(128)
    # |y| = |x| and |y| up to 2 encodings either side of |x|, in every quadrant
    base = np.concatenate([mag_bits(t[np.isfinite(t)]), rng.integers(3, 0x7F7FFFFD, 4000)])
    base = base[(base >= 2) & (base <= 0x7F7FFFFD)]
    fy, fx = [], []
    for k in (-2, -1, 0, 1, 2):
        fy.append(f32(base + k) * _signs(rng, len(base)))
        fx.append(f32(base) * _signs(rng, len(base)))
    # max(|x|, |y|) within 256 encodings of 2^-128, 2^-126 and 2^126, the other operand anywhere
    # below it: six smaller operands per maximum, either one being x
    ty, tx = [], []
    for thr in ATAN2_THRESHOLDS:
        mx = np.tile(mag_bits(around(thr, 256)), 6)
        mn = (mx * rng.random(len(mx)) ** 2).astype(np.int64)
        a, b = f32(mx) * _signs(rng, len(mx)), f32(mn) * _signs(rng, len(mx))
        swap = rng.random(len(mx)) < 0.5
        ty.append(np.where(swap, a, b))
        tx.append(np.where(swap, b, a))
    return [("thinned_cross", y, x),
            ("octant_flip_and_thresholds", np.concatenate(fy + ty), np.concatenate(fx + tx))]


def pow_y_values():
    rng = np.random.default_rng(150)
    return np.concatenate([np.array(POW_Y_SPECIALS), rng.uniform(-150.0, 150.0, 64)]).astype(np.float32)


def _pow_sets():
    x, y = (g.ravel() for g in np.meshgrid(thinned(), pow_y_values(), indexing="ij"))
    # y * log2(x) within 2 of each exp2 target (float64): x any positive finite encoding whose
    # log2 is at least 2^-6 in magnitude, y the float32 nearest (target + offset) / log2(x)
    rng = np.random.default_rng(151)
    px, py = [], []
    for target in EXP2_TARGETS:
        xs = f32(rng.integers(1, 0x7F800000, 24000))
        l2 = np.log2(xs.astype(np.float64))
        xs, l2 = xs[np.abs(l2) >= 2.0 ** -6][:20000], l2[np.abs(l2) >= 2.0 ** -6][:20000]
        px.append(xs)
        py.append(((target + rng.uniform(-1.9, 1.9, len(xs))) / l2).astype(np.float32))
    return [("thinned_cross", x, y), ("exp2_ends", np.concatenate(px), np.concatenate(py))]


_MAKERS = {"sin": _sincos_sets, "cos": _sincos_sets, "acos": _acos_sets, "atan2": _atan2_sets, "log": _log_sets,
           "log2": _log_sets, "exp2": _exp2_sets, "pow": _pow_sets}


def sets(name):
    """[(label, a, b)] for a builtin (b is None for the unary ones); float32, read-only, built once."""
    def make():
        out = []
        for label, a, b in _MAKERS[name]():
            a = np.ascontiguousarray(a, np.float32)
            b = None if b is None else np.ascontiguousarray(b, np.float32)
            for arr in (a, b):
                if arr is not None:
                    arr.setflags(write=False)
            out.append((label, a, b))
        return tuple(out)
    return _cached(("sets", _MAKERS[name]), make)


def set_ids():
    """[(builtin, label)] over every set: the GPU test's parametrisation."""
    return [(name, label) for name in NAMES for label, _, _ in sets(name)]


def get_set(name, label):
    for lab, a, b in sets(name):
        if lab == label:
            return a, b
    raise KeyError((name, label))


def union(name):
    """(a, b) of all of a builtin's sets together."""
    ss = sets(name)
    a = np.concatenate([s[1] for s in ss])
    b = None if ss[0][2] is None else np.concatenate([s[2] for s in ss])
    return a, b


# ---- the census: what the sets must reach, from numpy alone ------------------------------------
def _near(x, centre, lo, hi):
    """x has the sign of `centre` and its encoding lies lo..hi encodings from centre's."""
    c = int(np.float32(centre).view(np.uint32))
    d = mag_bits(x) - (c & 0x7FFFFFFF)
    return (np.signbit(x) == bool(c >> 31)) & (d >= lo) & (d <= hi)


def _distinct(x, mask):
    return len(np.unique(bits_of(x)[mask]))


def _common(x):
    """Strata every unary set shares: (label, count, least)."""
    sub = (mag_bits(x) > 0) & (mag_bits(x) < 0x00800000)
    return [("+0", int(np.sum(bits_of(x) == 0)), 1), ("-0", int(np.sum(bits_of(x) == 0x80000000)), 1),
            ("+inf", int(np.sum(x == np.inf)), 1), ("-inf", int(np.sum(x == -np.inf)), 1),
            ("NaN", int(np.isnan(x).sum()), 100),
            ("positive subnormals", int(np.sum(sub & ~np.signbit(x))), 100),
            ("negative subnormals", int(np.sum(sub & np.signbit(x))), 100),
            ("every sign and exponent field", len(np.unique(bits_of(x) >> np.uint32(23))), 512)]


def _hood_strata(x, label, centre, k=HOOD, signs=(1, -1)):
    """Both sides of a neighbourhood: k distinct encodings below and k above, per sign."""
    out = []
    for s in signs:
        c = s * centre
        out.append((f"{label}: {k} below {c!r}", _distinct(x, _near(x, c, -k, -1)), k))
        out.append((f"{label}: at {c!r}", int(_near(x, c, 0, 0).sum()), 1))
        out.append((f"{label}: {k} above {c!r}", _distinct(x, _near(x, c, 1, k)), k))
    return out


def strata(name):
    """[(label, count, least)]: the set reaches the stratum when count >= least. Classified with
    numpy in float64 and on the encodings, never with the code under test."""
    with np.errstate(all="ignore"):
        return _cached(("strata", _MAKERS[name]), lambda: tuple(_strata(name)))


def _strata(name):
    a, b = union(name)
    x64 = a.astype(np.float64)
    if name in ("sin", "cos"):
        out = _common(a)
        out += _hood_strata(a, "the |x| <= 2^20 branch", 2.0 ** 20)
        with np.errstate(all="ignore"):
            prod = np.abs(x64) * INV_PI_HI
        out += [("|x / pi| >= 2^24, finite", int(np.sum((prod >= 2.0 ** 24) & np.isfinite(x64))), 100),
                ("2^20 < |x|, |x / pi| < 2^24", int(np.sum((np.abs(x64) > 2.0 ** 20) & (prod < 2.0 ** 24))), 100)]
        for s in (1, -1):
            side = (np.signbit(a) == (s < 0))
            out.append((f"parity rule: product within 5000 under 2^24, sign {s}",
                        int(np.sum(side & (prod < 2.0 ** 24) & (prod > 2.0 ** 24 - 5000))), 3000))
            out.append((f"parity rule: product within 5000 over 2^24, sign {s}",
                        int(np.sum(side & (prod >= 2.0 ** 24) & (prod < 2.0 ** 24 + 5000))), 3000))
        out += _hood_strata(a, "pi", PI) + _hood_strata(a, "pi / 2", HALF_PI)
        for c in tie_centres():
            out += _hood_strata(a, "rint tie", float(c), signs=(1,))
        out.append(("the 4,096 smallest subnormals of either sign",
                    _distinct(a, (mag_bits(a) >= 1) & (mag_bits(a) <= HOOD)), 2 * HOOD))
        return out
    if name == "acos":
        out = _common(a)
        out += _hood_strata(a, "the end of the domain", 1.0) + _hood_strata(a, "a half", 0.5)
        out += [("the 4,096 smallest subnormals of either sign",
                 _distinct(a, (mag_bits(a) >= 1) & (mag_bits(a) <= HOOD)), 2 * HOOD),
                ("1 < |t| < inf", int(np.sum((np.abs(x64) > 1) & np.isfinite(x64))), 100),
                ("inside [-1, 1]", int(np.sum(np.abs(x64) <= 1)), 100000)]
        return out
    if name in ("log", "log2"):
        out = _common(a)
        out += _hood_strata(a, "log's zero", 1.0, signs=(1,))
        out += _hood_strata(a, "the first normal", 2.0 ** -126, signs=(1,))
        out += [(f"{HOOD} down from FLT_MAX", _distinct(a, _near(a, FLT_MAX, -HOOD, 0)), HOOD + 1),
                ("positive subnormals, distinct", _distinct(a, (mag_bits(a) > 0) & (mag_bits(a) < 0x00800000) & ~np.signbit(a)),
                 20000),
                ("negative finite", int(np.sum((x64 < 0) & np.isfinite(x64))), 100)]
        for c in sqrt_half_cuts():
            out += _hood_strata(a, "mantissa cut", float(c), signs=(1,))
        ub = np.unique(bits_of(a))
        pw = bits_of(powers_of_two()).astype(np.int64)
        for k in (-2, -1, 0, 1, 2):
            want = pw + k
            want = want[want > 0]
            out.append((f"every power of two moved by {k} encodings", int(np.isin(want.astype(np.uint32), ub).sum()), len(want)))
        return out
    if name == "exp2":
        out = _common(a)
        ub = np.unique(bits_of(a))
        hb = bits_of(exp2_halves()).astype(np.int64)
        for k in (-2, -1, 0, 1, 2):
            out.append((f"every integer and half-integer of [-152, 130] moved by {k} encodings",
                        int(np.isin((hb + k).astype(np.uint32), ub).sum()), len(hb)))
        for c in (-149.0, -126.0, 127.0, 128.0):
            out += _hood_strata(a, "dense", c, signs=(1,))
        with np.errstate(all="ignore"):
            ref = np.exp2(x64)
        frac = x64 - np.floor(x64)
        fin = np.isfinite(x64)
        out += [("float64 result subnormal in float32", int(np.sum((ref > 0) & (ref < 2.0 ** -126))), 100000),
                ("below the clamp, x < -151, finite", int(np.sum((x64 < -151) & fin)), 100),
                ("above the clamp, x > 129, finite", int(np.sum((x64 > 129) & fin)), 100),
                ("the clamp ends -151 and 129", int(np.sum(x64 == -151) > 0) + int(np.sum(x64 == 129) > 0), 2),
                ("rint ties to an even integer", int(np.sum(fin & (frac == 0.5) & (np.floor(x64) % 2 == 0) & (np.abs(x64) < 200))), 100),
                ("rint ties to an odd integer", int(np.sum(fin & (frac == 0.5) & (np.floor(x64) % 2 == 1) & (np.abs(x64) < 200))), 100)]
        return out
    y64 = b.astype(np.float64)
    if name == "atan2":  # a is y, b is x
        ay, ax = mag_bits(a), mag_bits(b)
        fin = (ay < 0x7F800000) & (ax < 0x7F800000)
        nz = fin & (ay > 0) & (ax > 0)
        out = []
        for qy in (False, True):
            for qx in (False, True):
                quad = nz & (np.signbit(a) == qy) & (np.signbit(b) == qx)
                tag = f"y {'<' if qy else '>'} 0, x {'<' if qx else '>'} 0"
                out += [(f"{tag}, |y| < |x|", int(np.sum(quad & (ay < ax))), 100),
                        (f"{tag}, |y| > |x|", int(np.sum(quad & (ay > ax))), 100)]
                for k in (-2, -1, 0, 1, 2):
                    out.append((f"{tag}, |y| {k:+d} encodings from |x|", int(np.sum(quad & (ay - ax == k))), 100))
        mx = np.maximum(ay, ax)
        t128, t126, t126p = (int(np.float32(t).view(np.uint32)) for t in ATAN2_THRESHOLDS)
        out += [("0 < max < 2^-128", int(np.sum(fin & (mx > 0) & (mx < t128))), 100),
                ("2^-128 <= max < 2^-126", int(np.sum(fin & (mx >= t128) & (mx < t126))), 100),
                ("2^126 < max < inf", int(np.sum(fin & (mx > t126p))), 100)]
        for t, tag in ((t128, "2^-128"), (t126, "2^-126"), (t126p, "2^126")):
            out += [(f"max within 256 encodings under {tag}", int(np.sum(fin & (mx < t) & (mx >= t - 256))), 256),
                    (f"max within 256 encodings of {tag} from above", int(np.sum(fin & (mx >= t) & (mx <= t + 256))), 256)]
        ny, nx = np.isnan(a), np.isnan(b)
        out += [("NaN in y only", int(np.sum(ny & ~nx)), 100), ("NaN in x only", int(np.sum(~ny & nx)), 100),
                ("NaN in both", int(np.sum(ny & nx)), 100)]
        # minNum / maxNum drop a quiet NaN and answer a signalling one with NaN
        sy, sx = ny & (bits_of(a) & 0x00400000 == 0), nx & (bits_of(b) & 0x00400000 == 0)
        out += [("a signalling NaN in y, x not NaN", int(np.sum(sy & ~nx)), 100), ("a signalling NaN in x, y not NaN", int(np.sum(sx & ~ny)), 100),
                ("a quiet NaN in y, x not NaN", int(np.sum(ny & ~sy & ~nx)), 100), ("a quiet NaN in x, y not NaN", int(np.sum(nx & ~sx & ~ny)), 100)]
        kinds = (("+0", 0), ("-0", 0x80000000), ("+inf", 0x7F800000), ("-inf", 0xFF800000))
        for ty, vy in kinds:
            for tx, vx in kinds:
                out.append((f"y = {ty}, x = {tx}", int(np.sum((bits_of(a) == vy) & (bits_of(b) == vx))), 1))
            out += [(f"y = {ty}, x finite and non-zero", int(np.sum((bits_of(a) == vy) & (ax > 0) & (ax < 0x7F800000))), 100),
                    (f"x = {ty}, y finite and non-zero", int(np.sum((bits_of(b) == vy) & (ay > 0) & (ay < 0x7F800000))), 100)]
        out.append(("pairs", len(a), 150000))
        return out
    # pow: a is x, b is y
    out = [("x < 0, finite", int(np.sum((x64 < 0) & np.isfinite(x64))), 100),
           ("x = +0", int(np.sum(bits_of(a) == 0)), 10), ("x = -0", int(np.sum(bits_of(a) == 0x80000000)), 10),
           ("x = +inf", int(np.sum(x64 == np.inf)), 10), ("x = -inf", int(np.sum(x64 == -np.inf)), 10),
           ("x NaN", int(np.isnan(x64).sum()), 100),
           ("x a positive subnormal", int(np.sum((mag_bits(a) > 0) & (mag_bits(a) < 0x00800000) & ~np.signbit(a))), 100),
           ("y random in [-150, 150]", len(np.unique(bits_of(b)[np.isfinite(y64) & (np.abs(y64) <= 150)])), 64)]
    for v in POW_Y_SPECIALS:
        same = np.isnan(b) if np.isnan(v) else (bits_of(b) == np.float32(v).view(np.uint32))
        out.append((f"y = {v!r}", int(same.sum()), 100))
    with np.errstate(all="ignore"):
        z = y64 * np.log2(np.where((x64 > 0) & np.isfinite(x64), x64, np.nan))
    for t in EXP2_TARGETS:
        out += [(f"y log2 x within 2 under {t}", int(np.sum((z < t) & (z > t - 2))), 5000),
                (f"y log2 x within 2 over {t}", int(np.sum((z >= t) & (z < t + 2))), 5000)]
    return out


# ---- the specials whose oracle bits are recorded ---------------------------------------------------
def _up(x, k=1):
    return float(f32(np.array([int(np.float32(x).view(np.uint32)) + k]))[0])


def specials(name):
    """(a, b): the fixed special inputs of a builtin (b None for the unary ones), float32."""
    nan, inf = np.nan, np.inf
    if name in ("sin", "cos"):
        v = [0.0, 2.0 ** -149, 2.0 ** -126, 1e-20, HALF_PI, PI, 2.5 * np.pi, 30.0, _up(2.0 ** 20, -1), 2.0 ** 20, _up(2.0 ** 20), 1e6,
             2.0 ** 23, _up(PARITY_X, -1), PARITY_X, _up(PARITY_X), 1e8, 1e10, 1e15, 1e20, 1e30, 2.0 ** 127, FLT_MAX, inf]
        return np.array(v + [-t for t in v] + [nan], np.float32), None
    if name == "acos":
        v = [0.0, 2.0 ** -149, 2.0 ** -126, 0.5, _up(1.0, -1), 1.0, _up(1.0), 1.0000001, 1.5, 2.0, 4.0, 1e10, 2.0 ** 127, FLT_MAX, inf]
        return np.array(v + [-t for t in v] + [nan], np.float32), None
    if name in ("log", "log2"):
        v = [0.0, -0.0, 2.0 ** -149, 2.0 ** -140, _up(2.0 ** -126, -1), 2.0 ** -126, _up(2.0 ** -126), SQRT_HALF * 2.0 ** -126,
             0.5, _up(SQRT_HALF, -1), SQRT_HALF, _up(SQRT_HALF), _up(1.0, -1), 1.0, _up(1.0), 2.0 * SQRT_HALF, 2.0, 10.0,
             2.0 ** 127, FLT_MAX, inf, -(2.0 ** -149), -(2.0 ** -126), -1.0, -FLT_MAX, -inf, nan]
        return np.array(v, np.float32), None
    if name == "exp2":
        v = [0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 0.5, -0.5, 1.5, 2.5, -1.5, -2.5, -125.5, -126.0, -126.5, -127.0, -148.5, -149.0,
             -149.5, -150.0, -150.5, -151.0, _up(-151.0), _up(-151.0, -1), -151.5, -152.0, -200.0, -1e10, -FLT_MAX, -inf,
             126.5, 127.0, 127.5, _up(128.0, -1), 128.0, 128.5, 129.0, _up(129.0), 129.5, 130.0, 200.0, 1e10, FLT_MAX, inf, nan]
        return np.array(v, np.float32), None
    if name == "atan2":
        v = [0.0, 2.0 ** -149, 2.0 ** -129, 2.0 ** -128, 2.0 ** -126, 1.0, 2.0 ** 126, 2.0 ** 127, inf]
        v = np.concatenate([np.array(v + [-t for t in v] + [nan], np.float32), [SNAN, -SNAN]])
        y, x = (g.ravel() for g in np.meshgrid(v, v, indexing="ij"))
        return y, x
    xs = np.array([0.0, -0.0, 2.0 ** -149, 0.5, 1.0, 2.0, FLT_MAX, inf, -(2.0 ** -149), -0.5, -1.0, -2.0, -inf, nan], np.float32)
    ys = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.0, 3.0, 100.0, inf, -inf, nan], np.float32)
    x, y = (g.ravel() for g in np.meshgrid(xs, ys, indexing="ij"))
    return x, y


def canonical_bits(out):
    """The encodings of results with every NaN as 0x7FC00000 (a NaN's sign and payload are not
    part of the semantics: NaN matches NaN)."""
    b = bits_of(out).copy()
    b[np.isnan(out)] = 0x7FC00000
    return b


def mismatches(got, ref):
    """Elements whose bits differ (the sign of zero counts), NaN matching NaN."""
    return ~((bits_of(got) == bits_of(ref)) | (np.isnan(got) & np.isnan(ref)))


def report(name, label, a, b, got, ref, who="gpu"):
    """The failure text for a set: the count and the first operands with both results."""
    bad = mismatches(got, ref)
    hexes = lambda v: [f"{float(t)!r} (0x{int(u):08x})" for t, u in zip(v[bad][:4], bits_of(v)[bad][:4])]  # noqa: E731
    return (f"{name} on {label}: {int(bad.sum())} of {len(a)} differ, e.g. a={hexes(a)}"
            f"{'' if b is None else ' b=' + str(hexes(b))} {who}={hexes(got)} oracle={hexes(ref)}")


# ---- the recorded specials as DESIGN.md shows them --------------------------------------------------
# (builtin, a, b): the rows of DESIGN.md section 2's "Builtins outside the hot path's ranges"
DESIGN_ROWS = (
    ("atan2", 2.0 ** -129, 2.0 ** -129), ("atan2", 2.0 ** -149, 0.0), ("atan2", 0.0, -(2.0 ** -129)),
    ("atan2", 2.0 ** -128, 2.0 ** -149), ("atan2", 2.0 ** 127, 1.0), ("atan2", 2.0 ** 127, 2.0 ** 127),
    ("atan2", 1.0, np.nan), ("atan2", np.nan, 1.0), ("atan2", np.nan, -1.0), ("atan2", np.nan, np.nan),
    ("atan2", 1.0, SNAN), ("atan2", SNAN, 1.0), ("atan2", 0.0, -SNAN),
    ("atan2", np.inf, np.inf), ("atan2", 1.0, np.inf), ("atan2", np.inf, 1.0), ("atan2", 1.0, -np.inf),
    ("sin", 2.0 ** 20, None), ("sin", 1e8, None), ("sin", 1e10, None), ("cos", 1e10, None), ("sin", 1e30, None),
    ("cos", 1e30, None), ("sin", FLT_MAX, None), ("sin", np.inf, None), ("cos", np.nan, None),
    ("acos", 1.0000001, None), ("acos", -1.0000001, None), ("acos", 2.0, None), ("acos", -2.0, None), ("acos", np.inf, None),
    ("pow", -2.0, 2.0), ("pow", -1.0, 3.0), ("pow", 0.0, 0.0), ("pow", 0.0, -1.0), ("pow", -0.0, 2.0), ("pow", 1.0, np.inf),
    ("pow", 2.0, np.inf), ("pow", 0.5, np.inf), ("pow", np.inf, 0.0), ("pow", np.inf, -1.0), ("pow", np.inf, 2.0),
    ("pow", -np.inf, 2.0), ("pow", 2.0, np.nan), ("pow", np.nan, 0.0),
    ("log", 2.0 ** -149, None), ("log2", 2.0 ** -149, None), ("log", -0.0, None), ("log2", -(2.0 ** -149), None),
    ("exp2", -149.0, None), ("exp2", -149.5, None), ("exp2", -150.0, None), ("exp2", -150.5, None), ("exp2", 128.0, None),
)


def _show(v):
    v = np.float32(v)
    if np.isnan(v):
        return "NaN" if int(v.view(np.uint32)) & 0x00400000 else "sNaN"
    if np.isinf(v):
        return "−inf" if v < 0 else "inf"
    m, e = np.frexp(np.float64(v))
    if m in (0.5, -0.5) and abs(e) > 20:
        return f"{'−' if m < 0 else ''}2^{e - 1}"
    if v == np.float32(FLT_MAX):
        return "FLT_MAX"
    return str(v).replace("-", "−")


def design_table(golden):
    """The markdown rows of DESIGN.md's table, from the recorded bits (the loaded
    tests/golden/builtin_specials.json)."""
    lines = ["| call | frm v3 result | encoding |", "|---|---|---|"]
    for name, a, b in DESIGN_ROWS:
        rec = golden["builtins"][name]
        ka = f"{int(np.float32(a).view(np.uint32)):08x}"
        kb = None if b is None else f"{int(np.float32(b).view(np.uint32)):08x}"
        hit = [i for i, h in enumerate(rec["a"]) if h == ka and (b is None or rec["b"][i] == kb)]
        out = f32(np.array([int(rec["out"][hit[0]], 16)]))[0]
        call = f"`{name}({_show(a)})`" if b is None else f"`{name}({_show(a)}, {_show(b)})`"
        lines.append(f"| {call} | {_show(out)} | `0x{rec['out'][hit[0]]}` |")
    return lines
