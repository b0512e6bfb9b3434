"""GRIB2 CCSDS packing on the device (include/aec_gpu_grib.h): the NumPy restatement of the contract and the case list
shared by tests/test_grib_emul.py, tests/test_grib_layout.py, tests/test_gpu_grib.py and tests/golden/make_golden_grib.py.

The model: every step is one NumPy float64 operation (correctly rounded, never fused) --
    s(y)   y * 10^D for D > 0, y / 10^-D for D < 0, y for D = 0; 10^|D| from a table, exact for |D| <= 22
    R      np.float32 of s(min), one nextafter down where that lies above it
    E      frexp of range = s(max) - R and one correction; [-127, 127]; a constant field: E = 0, X = 0
    X      trunc((s(y) - R) * 2^-E + 0.5), ties up
    Y      (X * 2^E + R) / 10^D, one rounding to the element type

Behind the model: the same contract in exact rationals (exact_R, exact_E, exact_x, exact_y), which the model is tested
against, and two generated lists outside the fixture -- edge_batches(), the pack side at its thresholds, and
dequantise_cases(), Y under parameters no pack produced.
"""
import math
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "grib_vectors.npz")

SIGNED, THREE_BYTE, MSB, PP, RESTRICTED, PAD_RSI, NOT_ENFORCE = 1, 2, 4, 8, 16, 32, 64
BAD, CONSTANT, CLAMPED = 1, 2, 4
F32, F64 = 4, 8
MAX_D = 22
POW10 = [float(10 ** k) for k in range(MAX_D + 1)]
FLT_MAX = float(np.finfo(np.float32).max)
RECORD_DTYPE = np.dtype([("R", "<f4"), ("E", "<i4"), ("D", "<i4"), ("status", "<u4")])
SPAN, WAVE_ROOM = 4096, 1024          # bytes of values a wavefront of the min/max reduces; bytes of room a wavefront owns


def container(nbits):
    return 1 if nbits <= 8 else 2 if nbits <= 16 else 4


def coder_flags(options, for_encode=True):
    return (options & (PP | RESTRICTED | PAD_RSI)) | (NOT_ENFORCE if for_encode else 0)


def room(n, bs, nbits):
    return (n + bs - 1) // bs * bs * container(nbits)


def up16(v):
    return (v + 15) // 16 * 16


# ---- the model ---------------------------------------------------------------------------------------------------------
def scale(y, D):
    y = np.asarray(y).astype(np.float64)
    return y * POW10[D] if D > 0 else y / POW10[-D] if D < 0 else y


def float_below(v):
    with np.errstate(over="ignore"):
        f = np.float32(v)
    if float(f) > v:
        f = np.nextafter(f, np.float32(-np.inf))
    return f


def params(y, D, nbits):
    """(R as np.float32, E, status) of a field"""
    y = np.asarray(y)
    if np.isnan(y).any():
        return np.float32(0), 0, BAD
    lo, hi = float(scale(y.min(), D)), float(scale(y.max(), D))
    if not (abs(lo) <= FLT_MAX and abs(hi) <= FLT_MAX):
        return np.float32(0), 0, BAD
    lo, hi = lo + 0.0, hi + 0.0                   # -0.0 -> +0.0
    R = float_below(lo)
    if lo == hi:
        return R, 0, CONSTANT
    rng = hi - float(R)
    M = float(2 ** nbits - 1)
    m, e = math.frexp(rng)
    E = e - nbits + (1 if math.ldexp(m, nbits) > M else 0)
    return R, max(-127, min(127, E)), 0


def quantise(y, D, nbits, R, E, zero=False):
    """(X as uint32, clamped) -- zero: a constant field packed without given parameters"""
    y = np.asarray(y)
    if zero:
        return np.zeros(y.size, np.uint32), False
    M = float(2 ** nbits - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (scale(y, D) - float(R)) * math.ldexp(1.0, -E) + 0.5
        x = np.trunc(u)
        clamped = bool(((x < 0) | (x > M) | np.isnan(x)).any())
        x = np.where(np.isnan(x), 0.0, np.clip(x, 0.0, M))
    return x.astype(np.uint32), clamped


def dequantise(x, R, E, D, dtype):
    with np.errstate(over="ignore"):
        v = np.asarray(x).astype(np.float64) * math.ldexp(1.0, E) + float(R)
        return (v / POW10[D] if D > 0 else v * POW10[-D] if D < 0 else v).astype(dtype)


def pack_model(y, D, nbits, given=None):
    """the record and X of a field: (R, E, status, X); given = (R, E) of have_params"""
    R, E, status = params(y, D, nbits)
    if given is not None:
        if status & BAD:
            return np.float32(given[0]), given[1], status, None
        x, clamped = quantise(y, D, nbits, np.float32(given[0]), given[1])
        return np.float32(given[0]), given[1], status | (CLAMPED if clamped else 0), x
    if status & BAD:
        return R, E, status, None
    x, clamped = quantise(y, D, nbits, R, E, zero=bool(status & CONSTANT))
    assert not clamped or E == 127, "the contract: 0 <= X <= M without clamping unless E is held at 127"
    return R, E, status | (CLAMPED if clamped else 0), x


def x_bytes(x, nbits, n_room):
    """X in the room of its field: little-endian containers, the last block padded with the last X"""
    full = np.concatenate([x, np.full(n_room - x.size, x[-1], np.uint32)])
    return full.astype({1: "<u1", 2: "<u2", 4: "<u4"}[container(nbits)]).view(np.uint8)


# ---- contraction witnesses --------------------------------------------------------------------------------------------------
def one_rounding_x(y, D, R, E):
    """X of one value when s(y) - R is rounded ONCE (what a fused multiply-add computes for D > 0), by exact rationals"""
    assert D > 0
    d = float(Fraction(float(y)) * 10 ** D - Fraction(float(R)))
    return int(math.trunc(d * math.ldexp(1.0, -E) + 0.5))


def witnesses(rng, count, R, D, lo, hi):
    """float64 values in [lo, hi] (units of Y) whose X under E = 0 differs between the two-rounding contract and one rounding"""
    out = []
    while len(out) < count:
        k = int(rng.integers(int(lo * 10 ** D - R) + 1, int(hi * 10 ** D - R) - 1))
        y = (R + k + 0.5) / 10 ** D
        for _ in range(8):
            x2, _ = quantise(np.array([y]), D, 32, np.float32(R), 0)
            if int(x2[0]) != one_rounding_x(y, D, np.float32(R), 0):
                out.append(y)
                break
            y = np.nextafter(y, -np.inf if len(out) % 2 else np.inf)
    return out


# ---- the case list ---------------------------------------------------------------------------------------------------------
def _smooth(rng, n, dtype, base=280.0, amp=25.0):
    t = np.arange(n)
    y = base + amp * np.sin(t / 37.0) + rng.normal(0, 0.4, n)
    return np.round(y * 64) / 64 if dtype == np.float32 else y        # (float32 fields: values that a deflated fixture keeps small)


def _field(kind, rng, n, dtype, nbits):
    if kind == "smooth":
        y = _smooth(rng, n, dtype)
    elif kind == "ends":                      # the maximum first, the minimum last
        y = _smooth(rng, n, dtype)
        y[0], y[-1] = y.max() + 3.0, y.min() - 5.0
    elif kind == "negative":
        y = -_smooth(rng, n, dtype)
    elif kind == "zeros":                     # both zeros, nothing below them
        y = np.abs(_smooth(rng, n, dtype, 0.0, 4.0))
        y[::3] = 0.0
        y[1::5] = -0.0
        y[-1] = -0.0
    elif kind == "constant":
        y = np.full(n, 273.15 if dtype == np.float64 else 273.25)
    elif kind == "constant_inexact":          # a constant float32 cannot hold
        y = np.full(n, 0.1)
    elif kind == "r_down":                    # a minimum float32 cannot hold: R rounds down, the smallest X is not 0
        y = 1e7 + 0.7 + np.abs(_smooth(rng, n, dtype, 0.0, 300.0))
        y[n // 2] = 1e7 + 0.7
    elif kind == "ties":                      # t exactly k + 0.5, k even and odd: min 0, max M * 2^-2, so R = 0 and E = -2
        M = 2 ** nbits - 1
        k = rng.integers(0, M - 1, n).astype(np.float64)
        k[:4] = [0, 1, 2, 3]
        y = (k + 0.5) * 0.25
        y[-2], y[-1] = 0.0, M * 0.25
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(y.astype(dtype))


def _batch(name, nbits, options, bs, rsi, dtype, fields, D, given=None):
    return dict(name=name, tmpl=(nbits, options, bs, rsi), elem=np.dtype(dtype).itemsize, dtype=np.dtype(dtype), fields=fields,
                D=list(D), given=given)


SIZES_F4 = [1, 31, 32, 33, 4095, 4096, 4097, 9001]       # 9001 float32: 9 wavefronts of the min/max, three workgroups and more
SIZES_F8 = [1, 31, 32, 33, 4095, 4096, 4097, 4700]       # 4700 float64: 10 wavefronts
SMALL = [1, 33, 100, 257]
D_CYCLE = [0, 3, -2]


def batches():
    """every batch of the case list, generated: dicts of name, tmpl = (nbits, options, block size, rsi), elem, dtype, fields
    (arrays), D and, for have_params, given = [(R, E)]"""
    out = []

    def rng_of(name):
        return np.random.default_rng(sum(name.encode()) * 7919 + len(name))

    def mixed(name, nbits, options, bs, rsi, dtype, sizes):
        rng = rng_of(name)
        fields = [_field("smooth" if i % 3 else "ends", rng, n, dtype, nbits) for i, n in enumerate(sizes)]
        out.append(_batch(name, nbits, options, bs, rsi, dtype, fields, [D_CYCLE[i % 3] for i in range(len(sizes))]))

    mixed("mix12_f4", 12, PP, 32, 128, np.float32, SIZES_F4)
    mixed("mix16_f8", 16, PP, 16, 128, np.float64, SIZES_F8)
    mixed("n1_f4", 1, 0, 8, 1, np.float32, SMALL)
    mixed("n8_f8", 8, PP, 8, 128, np.float64, SMALL)
    mixed("n9_f4", 9, PP | MSB, 16, 1, np.float32, SMALL)
    mixed("n17_f8", 17, 0, 32, 128, np.float64, SMALL)
    mixed("n24_f4", 24, PP | THREE_BYTE, 32, 128, np.float32, SMALL)
    mixed("n25_f8", 25, PP, 16, 128, np.float64, SMALL)
    mixed("n32_f4", 32, PP, 32, 128, np.float32, SMALL)
    mixed("n32_f8", 32, PP, 32, 1, np.float64, SMALL)
    for dtype, tag in ((np.float32, "f4"), (np.float64, "f8")):
        name = "shapes_" + tag
        rng = rng_of(name)
        kinds = ["ends", "negative", "zeros", "constant", "constant_inexact", "r_down", "ties", "ends"]
        sizes = [301, 64, 77, 40, 9, 130, 200, 5]
        fields = [_field(k, rng, n, dtype, 16) for k, n in zip(kinds, sizes)]
        out.append(_batch(name, 16, PP, 32, 128, dtype, fields, [0, 3, 0, -2, 3, 3, 0, 3]))
    # contraction witnesses: D = 3, R = 250000 (250.0 is the minimum), E = 0 (the maximum is 310.0: range 60000 <= 65535)
    rng = rng_of("witness_f8")
    y = _smooth(rng, 150, np.float64, 280.0, 20.0)
    y[0], y[1] = 250.0, 310.0
    y[10:16] = witnesses(rng, 6, 250000.0, 3, 251.0, 309.0)
    out.append(_batch("witness_f8", 16, PP, 32, 128, np.float64, [np.ascontiguousarray(y), _smooth(rng, 40, np.float64)], [3, 3]))
    # have_params: the second field's E is two too small (X beyond M are held), the third's R lies above its minimum
    rng = rng_of("given_f4")
    fields = [_field("smooth", rng, n, np.float32, 12) for n in (100, 257, 33)]
    given = []
    for i, f in enumerate(fields):
        R, E, _ = params(f, 0, 12)
        given.append([(float(R), E), (float(R), E - 2), (float(R) + 2.0, E)][i])
    out.append(_batch("given_f4", 12, PP, 16, 128, np.float32, fields, [0, 0, 0], given))
    # a NaN in one field and an Inf in another: status bit 0 there, the neighbours exact
    for dtype, tag in ((np.float32, "f4"), (np.float64, "f8")):
        name = "nonfinite_" + tag
        rng = rng_of(name)
        fields = [_field("smooth", rng, n, dtype, 12) for n in (70, 1500, 33, 300, 64, 90)]
        fields[1][1234] = np.nan
        fields[3][0] = np.inf
        fields[5][89] = -np.nan
        out.append(_batch(name, 12, PP, 32, 128, dtype, fields, [0, 3, 0, 0, -2, 3]))
    return out


def extra_batches():
    """batches outside the fixture (no streams are compared: records and X against the model only) --
    given_nonfinite_f4  have_params with a NaN in one field: that field is bad and nothing else, its neighbours are exact
    wide_f8             1 bit and extremes near +-FLT_MAX: E is held at 127, X is held to M and the field says so"""
    rng = np.random.default_rng(4242)
    fields = [_field("smooth", rng, n, np.float32, 12) for n in (100, 257, 33)]
    given = [(float(params(f, 0, 12)[0]), params(f, 0, 12)[1]) for f in fields]
    fields[1][200] = np.nan
    out = [_batch("given_nonfinite_f4", 12, PP, 16, 128, np.float32, fields, [0, 0, 0], given)]
    wide = np.linspace(-3.0e38, 3.0e38, 70)
    out.append(_batch("wide_f8", 1, 0, 8, 128, np.float64, [np.ascontiguousarray(wide), _smooth(rng, 20, np.float64)], [0, 0]))
    return out


def placement(b, seed=0):
    """where the fields of a batch lie: shuffled order, gaps of 0 .. 3 elements, so that bases are and are not 16-byte
    aligned; (byte offsets, extent in bytes)"""
    n = len(b["fields"])
    order = np.random.default_rng(seed + n).permutation(n)
    offs, at = [0] * n, 0
    for k, i in enumerate(order):
        if k % 3 == 2:
            at = up16(at)                                   # (an aligned base that is not the first)
        offs[i] = at
        at += (b["fields"][i].size + (k * 5 + 1) % 4) * b["elem"]
    return offs, at


def model_of(b):
    """per field: (R, E, status, X or None)"""
    return [pack_model(f, D, b["tmpl"][0], None if b["given"] is None else b["given"][i])
            for i, (f, D) in enumerate(zip(b["fields"], b["D"]))]


def golden_batches():
    """the batches as the fixture holds them: the generated batch with fields, X and streams taken from the file; X and
    stream are None for a field whose status says bad"""
    z = np.load(GOLDEN)
    names = [str(s) for s in z["names"]]
    out = []
    fi = 0
    vals4, vals8, xs, streams = z["values_f4"], z["values_f8"], z["x"], z["streams"]
    at = {"f4": 0, "f8": 0, "x": 0, "s": 0}
    for b in batches():
        bi = names.index(b["name"])
        assert tuple(int(v) for v in z["tmpl"][bi]) == b["tmpl"] and int(z["elem"][bi]) == b["elem"], b["name"]
        key, vals = ("f4", vals4) if b["elem"] == 4 else ("f8", vals8)
        fields, X, S = [], [], []
        for f in b["fields"]:
            n = int(z["n_values"][fi])
            assert n == f.size, b["name"]
            fields.append(np.ascontiguousarray(vals[at[key]:at[key] + n]))
            at[key] += n
            if int(z["status"][fi]) & BAD:
                X.append(None)
                S.append(None)
            else:
                X.append(xs[at["x"]:at["x"] + n].copy())
                at["x"] += n
                ln = int(z["stream_bytes"][fi])
                S.append(streams[at["s"]:at["s"] + ln].tobytes())
                at["s"] += ln
            fi += 1
        out.append(dict(b, fields=fields, X=X, streams=S))
    assert names == [b["name"] for b in out]
    return out


# ---- the contract in exact rationals ------------------------------------------------------------------------------------------
# include/aec_gpu_grib.h restated with fractions.Fraction, independently of params() / quantise() / dequantise() above
# and of aec_grib.h: no frexp, no nextafter, no cast decides anything.  A rounding to double is float() of a Fraction,
# which is correctly rounded; a rounding to float32 is found among the float32 by comparing Fractions.
def _f32_key(bits):
    """the float32 in their numeric order, -0.0 just below +0.0"""
    return ~bits & 0xFFFFFFFF if bits >> 31 else bits | 0x80000000


def _f32_bits(key):
    return key & 0x7FFFFFFF if key >> 31 else ~key & 0xFFFFFFFF


def _f32_value(bits):
    sign, ex, man = bits >> 31, bits >> 23 & 0xFF, bits & 0x7FFFFF
    assert ex != 0xFF
    v = Fraction(man, 1 << 149) if ex == 0 else ((1 << 23) | man) * Fraction(2) ** (ex - 150)
    return -v if sign else v


def f32_of_bits(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def bits_of_f32(f):
    return int(np.array([f], np.float32).view(np.uint32)[0])


_KEY_LOWEST, _KEY_HIGHEST = _f32_key(0xFF7FFFFF), _f32_key(0x7F7FFFFF)


def _f32_key_below(v, lo_key):
    """the largest key in [lo_key, the key of FLT_MAX] whose float32 is <= the rational v"""
    a, b = lo_key, _KEY_HIGHEST
    assert _f32_value(_f32_bits(a)) <= v
    while a < b:
        mid = (a + b + 1) // 2
        if _f32_value(_f32_bits(mid)) <= v:
            a = mid
        else:
            b = mid - 1
    return a


def _rn(v):
    """the double nearest a rational, ties to even; an infinity beyond the doubles"""
    try:
        return float(v)
    except OverflowError:
        return math.inf if v > 0 else -math.inf


def _rn_f32(w):
    """one rounding of a double to float32: nearest, ties to even, Inf from FLT_MAX + half an ulp on, the sign of a zero kept"""
    if math.isinf(w) or w == 0.0:
        return np.float32(w)
    a = abs(Fraction(w))
    e = a.numerator.bit_length() - a.denominator.bit_length()
    e -= Fraction(2) ** e > a                               # 2^e <= a < 2^(e+1)
    if e > 127:
        return np.float32(math.copysign(math.inf, w))
    e = max(e, -126)                                        # (the subnormals share the quantum of the smallest normals)
    n = a / Fraction(2) ** (e - 23)                         # a in units of the float32 quantum at a
    k = n.numerator // n.denominator
    k += n - k > Fraction(1, 2) or (n - k == Fraction(1, 2) and k & 1 == 1)
    # k < 2^23: a subnormal, its bits are k.  Else the mantissa behind the exponent; k = 2^24 carries into the exponent,
    # and from the largest exponent that is the bit pattern of Inf
    bits = k if k < 1 << 23 else ((e + 127) << 23) + (k - (1 << 23))
    return f32_of_bits(bits | (0x80000000 if w < 0 else 0))


def exact_scale(y, D):
    """s(y), one rounding"""
    y = Fraction(float(y))
    return float(y) if D == 0 else _rn(y * 10 ** D) if D > 0 else _rn(y / 10 ** -D)


def exact_R(lo):
    """the largest float32 <= lo, |lo| <= FLT_MAX; +0.0 for a zero"""
    return f32_of_bits(_f32_bits(_f32_key_below(Fraction(lo), _KEY_LOWEST)))


def exact_E(rng, nbits):
    """the smallest integer E with rng * 2^-E <= 2^nbits - 1, held to [-127, 127]; rng > 0"""
    rng, M = Fraction(rng), 2 ** nbits - 1
    assert rng > 0
    if rng / Fraction(2) ** 127 > M:
        return 127
    a, b = -127, 127                                        # (the condition holds at b)
    while a < b:
        mid = (a + b) // 2
        if rng / Fraction(2) ** mid <= M:
            b = mid
        else:
            a = mid + 1
    return a


def exact_params(y, D, nbits):
    """(R, E, status) of a field by the contract's steps 1 - 4"""
    y = np.asarray(y)
    if not np.isfinite(y).all():
        return np.float32(0), 0, BAD
    lo, hi = exact_scale(y.min(), D), exact_scale(y.max(), D)
    if math.isinf(lo) or math.isinf(hi) or max(abs(Fraction(lo)), abs(Fraction(hi))) > Fraction(FLT_MAX):
        return np.float32(0), 0, BAD
    R = exact_R(lo)
    if Fraction(lo) == Fraction(hi):
        return R, 0, CONSTANT
    return R, exact_E(_rn(Fraction(hi) - Fraction(float(R))), nbits), 0


def exact_x(y, D, R, E):
    """trunc((s(y) - R) * 2^-E + 0.5), every step one correct rounding; NOT held to [0, M]"""
    d = _rn(Fraction(exact_scale(y, D)) - Fraction(float(R)))
    t = _rn(Fraction(d) / Fraction(2) ** E)
    u = _rn(Fraction(t) + Fraction(1, 2))
    return math.trunc(Fraction(u))


def exact_y(x, R, E, D, dtype):
    """(X * 2^E + R) / 10^D: the sum rounded once, the scaling rounded once, then one rounding to the element type"""
    v = _rn(int(x) * Fraction(2) ** E + Fraction(float(R)))       # (an exact zero is +0.0: X * 2^E is never -0.0)
    if math.isinf(v) or v == 0.0 or D == 0:
        w = v
    else:
        w = _rn(Fraction(v) / 10 ** D) if D > 0 else _rn(Fraction(v) * 10 ** -D)
        if w == 0.0:
            w = math.copysign(0.0, v)
    return np.float64(w) if np.dtype(dtype) == np.float64 else _rn_f32(w)


# ---- cases at the thresholds ---------------------------------------------------------------------------------------------------
# Outside the fixture: records, X and Y against the model (which tests/test_grib_emul.py checks against the exact
# rationals above), streams against aec_buffer_encode of the model's X.  Every field carries `expect`: where the case is
# meant to sit (E, status, bits of R, X), asserted by test_the_edge_batches_hold_what_they_are_for.
NBITS_EDGE = [1, 8, 9, 16, 17, 24, 25, 32]
TAGS = ((np.float64, "f8"), (np.float32, "f4"))
# (family, element type, why) -- what a family does not hold for an element type
NOT_BUILT = [
    ("e_at_m", "f4", "M * 2^e with its double neighbours and (M + 0.5) * 2^e: float32 fields hold 2^(nbits+e) and its float32 predecessor"),
    ("e_clamp", "f4", "the subnormal range 5e-320 is below every float32"),
    ("r", "f4", "minima inside (-denorm_min, denorm_min), one double ulp off a float32, beyond FLT_MAX (its successor, 1e39)"),
    ("subnormal_f4", "f8", "the family is about float32 values that are subnormal"),
    ("x_limits", "f4", "M + 0.5 at 32 bits is no float32; the D = 3 batch is float64"),
    ("ties_below", "f4", "the predecessors of (k + 0.5) / 4 near k = 2^32 are no float32"),
]


def _up(v, dtype=np.float64):
    return float(np.nextafter(dtype(v), dtype(np.inf)))


def _down(v, dtype=np.float64):
    return float(np.nextafter(dtype(v), dtype(-np.inf)))


def _edge(family, name, nbits, options, bs, rsi, dtype, cases, given=None, bases=None):
    """cases: (values as float64, D, expect) per field; the values must be exact in dtype"""
    fields = []
    for v, D, e in cases:
        v = np.asarray(v, np.float64)
        with np.errstate(over="ignore"):
            f = np.ascontiguousarray(v.astype(dtype))
        assert np.array_equal(f.astype(np.float64), v), (name, "a value is not exact in the element type")
        assert e, (name, "a case that says nothing about where it sits")
        fields.append(f)
    b = _batch(name, nbits, options, bs, rsi, dtype, fields, [D for v, D, e in cases], given)
    return dict(b, family=family, expect=[e for v, D, e in cases], bases=bases)


def _between(rng, lo, hi, n, ends, dtype):
    """n values in [lo, hi] with the two ends at random places"""
    y = rng.uniform(lo, hi, n).astype(dtype).astype(np.float64).clip(lo, hi)
    a, b = rng.permutation(n)[:2]
    y[a], y[b] = ends
    return y


def _e_at_m(out):
    """R = 0 and a maximum on, one step beside and half a step beyond M * 2^e: the decision m * 2^nbits > M of grib_params"""
    for nbits in NBITS_EDGE:
        M = 2 ** nbits - 1
        rng = np.random.default_rng(1000 + nbits)
        cases = []
        for e in (-3, 0, 5):
            top = math.ldexp(M, e)
            for hi, E, xmax in ((top, e, M), (_up(top), e + 1, None), (_down(top), e, None), (math.ldexp(M + 0.5, e), e + 1, None)):
                exp = dict(E=E, rbits=0, status=0)
                if xmax is not None:
                    exp["xmax"] = xmax
                cases.append((_between(rng, 0.0, hi, 3 + int(rng.integers(0, 40)), (0.0, hi), np.float64), 0, exp))
        out.append(_edge("e_at_m", f"e_at_m{nbits}_f8", nbits, PP, 16, 128, np.float64, cases))
        cases = []
        for e in (-3, 0, 5):
            top = math.ldexp(1.0, nbits + e)
            pred = _down(top, np.float32)
            cases.append((_between(rng, 0.0, top, 3 + int(rng.integers(0, 40)), (0.0, top), np.float32), 0,
                          dict(E=e + 1, rbits=0, status=0, xmax=2 ** (nbits - 1))))
            exp = dict(E=e + 1 if nbits <= 17 else e, rbits=0, status=0)
            if nbits >= 24:
                exp["xmax"] = {24: M, 25: M - 1, 32: 2 ** 32 - 256}[nbits]
            cases.append((_between(rng, 0.0, pred, 3 + int(rng.integers(0, 40)), (0.0, pred), np.float32), 0, exp))
        out.append(_edge("e_at_m", f"e_at_m{nbits}_f4", nbits, PP, 32, 128, np.float32, cases))


def _e_clamp(out):
    """E at -127 and at 127, reached exactly and held"""
    for dtype, tag in TAGS:
        r = lambda v: float(dtype(v))
        cases = [([0.0, 2.0 ** -113, 2.0 ** -112], 0, dict(E=-127, status=0, rbits=0, xmax=32768)),
                 ([2.0 ** -114, 0.0, 2.0 ** -113], 0, dict(E=-127, status=0, rbits=0, xmax=16384))]
        if dtype == np.float64:
            cases.append(([0.0, 5e-320, 2e-320], 0, dict(E=-127, status=0, rbits=0, x=[0, 0, 0])))
        out.append(_edge("e_clamp", "e_clamp16_" + tag, 16, PP, 16, 128, dtype, cases))
        cases = [([0.0, 2.0 ** 127], 0, dict(E=127, status=0, x=[0, 1])),
                 ([0.0, _up(2.0 ** 127, dtype)], 0, dict(E=127, status=0, x=[0, 1]))]          # held at 127, nothing held
        out.append(_edge("e_clamp", "e_clamp1_" + tag, 1, 0, 8, 128, dtype, cases))
        cases = [([r(-3.4e38), 0.0, r(3.4e38)], 0, dict(E=127, status=CLAMPED, x=[0, 2, 3]))]
        out.append(_edge("e_clamp", "e_clamp2_" + tag, 2, PP, 8, 128, dtype, cases))


def _r_family(out):
    """grib_float_below at zero, at the subnormals, at +-FLT_MAX and across it by D"""
    tiny = 2.0 ** -150                                    # half of float32's denorm_min
    f = float(np.float32(0.1))
    for dtype, tag in TAGS:
        r = lambda v: float(dtype(v))
        f8 = dtype == np.float64
        cases = [([1.0, -0.0, 2.0], 0, dict(rbits=0, status=0, xmin=0)),
                 ([-0.0] * 5, 0, dict(rbits=0, status=CONSTANT, E=0)),
                 ([-3.0, -1.5, -0.0], 0, dict(rbits=0xC0400000, status=0, E=-14, xmax=49152)),
                 ([-FLT_MAX, 0.0, r(-1e38)], 0, dict(rbits=0xFF7FFFFF, status=0, E=113)),
                 ([1.0, r(1e38)], 1, dict(status=BAD)),
                 ([1.0, -np.inf, 2.0], 0, dict(status=BAD)),
                 ([f, r(0.2), r(0.15)], 0, dict(rbits=0x3DCCCCCD, status=0, xmin=0))]
        if f8:
            cases += [([tiny, 1.0, 0.5], 0, dict(rbits=0, status=0, xmin=0)),
                      ([-tiny, 1.0, 0.5], 0, dict(rbits=0x80000001, status=0, xmin=0)),
                      ([0.0, _up(FLT_MAX)], 0, dict(status=BAD)),
                      ([0.0, 1e39], -2, dict(rbits=0, status=0, E=107)),
                      ([0.0, 1e39], 0, dict(status=BAD)),
                      ([_up(f), 0.2, 0.15], 0, dict(rbits=0x3DCCCCCD, status=0, xmin=0, r_below_min=True)),
                      ([_down(-1.0), -1.0 + 2.0 ** -10, -1.0 + 2.0 ** -11], 0,
                       dict(rbits=0xBF800001, status=0, E=-25, xmin=4, r_below_min=True))]
        out.append(_edge("r", "r_" + tag, 16, PP, 32, 128, dtype, cases))


def _d22(out):
    for dtype, tag in TAGS:
        rng = np.random.default_rng(2200 + np.dtype(dtype).itemsize)
        r = lambda v: float(dtype(v))
        cases = [(_between(rng, r(1e-10), r(2.5e-10), 60, (r(1e-10), r(2.5e-10)), dtype), 22, dict(E=17, status=0)),
                 (_between(rng, r(1e30), r(2.5e30), 45, (r(1e30), r(2.5e30)), dtype), -22, dict(E=4, status=0))]
        out.append(_edge("d22", "d22_" + tag, 24, PP, 32, 128, dtype, cases))


def _subnormal_f4(out):
    """float32 values that are subnormal: under D = 22 they spread over X, under D = 0 every X is 0.  A conversion that
    flushes them changes R or X of the first"""
    rng = np.random.default_rng(40)
    r = lambda v: float(np.float32(v))
    y = _between(rng, r(1e-40), r(9.5e-40), 200, (r(1e-40), r(9.5e-40)), np.float32)
    assert (np.abs(y) < 2.0 ** -126).all()
    cases = [(y, 22, dict(E=-72, status=0, xmin=0, xmax=40140)), (y, 0, dict(E=-127, status=0, xmax=0, rbits=bits_of_f32(np.float32(1e-40))))]
    out.append(_edge("subnormal_f4", "subnormal_f4", 16, PP, 16, 128, np.float32, cases))


def _y_with_s(target, D):
    """a double y with s(y) == target exactly (by the rationals), or None"""
    y = target / 10.0 ** D if D > 0 else target * 10.0 ** -D
    for k in range(13):                      # (y * 10^D steps by one or two ulps of the product: the neighbours of y are tried)
        for toward in (np.inf, -np.inf):
            c = y
            for _ in range(k):
                c = float(np.nextafter(c, toward))
            if exact_scale(c, D) == target:
                return c
    return None


def _x_limits(out):
    """t = (s(y) - R) * 2^-E on and one step beside the limits of grib_quantise, under given parameters: beside a second
    value whose X is 7, so that a status bit is the first value's"""
    def rows(top):      # (t, the neighbour taken: 0 none, 1 its successor, -1 its predecessor, X, held)
        return [(top + 0.5, 0, top, True), (top + 0.5, -1, top, False), (-0.5, 0, 0, False), (-0.5, -1, 0, False),
                (-1.5, 0, 0, True), (-1.5, 1, 0, False), (100.5, 0, 101, False), (100.5, -1, 100, False)]

    def beside(v, step, dtype):
        return v if step == 0 else _up(v, dtype) if step > 0 else _down(v, dtype)

    for nbits, dtype, tag in ((8, np.float64, "f8"), (8, np.float32, "f4"), (32, np.float64, "f8")):
        cases, given = [], []
        for t, step, x, held in rows(2 ** nbits - 1):
            cases.append(([beside(t, step, dtype), 7.0], 0, dict(x=[x, 7], status=CLAMPED if held else 0)))
            given.append((0.0, 0))
        if nbits == 8:              # constant fields under given parameters follow the formula: X is not 0
            cases += [([7.0] * 9, 0, dict(x=[5] * 9, status=CONSTANT)), ([float(dtype(0.1))] * 9, 3, dict(x=[50] * 9, status=CONSTANT))]
            given += [(2.0, 0), (50.0, 0)]
        out.append(_edge("x_limits", f"x_limits{nbits}_{tag}", nbits, PP, 8, 128, dtype, cases, given))
    # D = 3: s(y) = fl(y * 1000) has to land on the limit, so every field brings an S it can reach with both neighbours
    cases, given = [], []
    for t, step, x, held in rows(255):
        for S in np.arange(300.0, 400.0, 0.5):
            y, y2 = _y_with_s(beside(float(S), step, np.float64), 3), _y_with_s(float(S) - t + 7.0, 3)
            if y is not None and y2 is not None:
                break
        else:
            raise AssertionError("no double reaches the limit under D = 3")
        cases.append(([y, y2], 3, dict(x=[x, 7], status=CLAMPED if held else 0)))
        given.append((float(S) - t, 0))
    out.append(_edge("x_limits", "x_limits8_d3_f8", 8, PP, 8, 128, np.float64, cases, given))


def _ties_below(out):
    """the "ties" construction (R = 0, E = -2) with the predecessor of every (k + 0.5) / 4 beside it: X = k against k + 1"""
    for nbits in (16, 32):
        M = 2 ** nbits - 1
        y, x = [], []
        for k in (0, 1, 2, 3, M - 4, M - 3, M - 2, M - 1):
            tie = (k + 0.5) * 0.25
            y += [tie, _down(tie)]
            x += [k + 1, k if k else 1]       # (k = 0: t + 0.5 = 1 - 2^-54 is itself a tie and rounds to 1.0, so X = 1)
        y += [0.0, M * 0.25]
        x += [0, M]
        out.append(_edge("ties_below", f"ties_below{nbits}_f8", nbits, PP, 32, 128, np.float64,
                         [(y, 0, dict(E=-2, rbits=0, status=0, x=x, ties=list(range(0, 16, 2))))]))


def position_list(elem):
    """where k_grib_minmax could lose a value: first and last element of a 16-byte group, of a step (64 groups), of a
    wavefront's span, and the tail behind two whole spans"""
    per, span = 16 // elem, SPAN // elem
    step, n = 64 * per, 2 * span + 5
    return [0, per - 1, per, step - 1, step, span - 1, span, 2 * span - 1, 2 * span, n - 1], n


def _positions(out):
    for dtype, tag in TAGS:
        elem = np.dtype(dtype).itemsize
        P, n = position_list(elem)
        back = 5.0 + np.sin(np.arange(n) / 37.0)
        back = back.astype(dtype).astype(np.float64)
        cases, bases = [], []
        for i, p in enumerate(P):
            q = P[(i + 3) % len(P)]
            y = back.copy()
            y[p], y[q] = 1.0, 9.0
            for how in ("aligned", "elem"):
                cases.append((y, 0, dict(E=-12, rbits=0x3F800000, status=0, xmin=0, xmax=32768, argmin=p, argmax=q)))
                bases.append(how)
        out.append(_edge("positions", "positions_" + tag, 16, PP, 32, 128, dtype, cases, bases=bases))


def _flags(out):
    """the coder flags grib_flags passes through besides preprocessing: RSI padding and the restricted code set"""
    for k, (nbits, options, bs, rsi, (dtype, tag)) in enumerate(((12, PP | PAD_RSI, 16, 4, TAGS[1]), (2, PP | RESTRICTED, 8, 128, TAGS[0]),
                                                                 (4, PP | RESTRICTED, 8, 128, TAGS[1]), (4, RESTRICTED | PAD_RSI, 8, 2, TAGS[0]))):
        rng = np.random.default_rng(7000 + k)
        fields = [_field("smooth" if i % 3 else "ends", rng, n, dtype, nbits).astype(np.float64) for i, n in enumerate(SMALL + [4097])]
        cases = [(f, D_CYCLE[i % 3], dict(status=0 if f.size > 1 else CONSTANT, xmin=0, xmax_over=((2 ** nbits - 1) // 2 if f.size > 1 else -1)))
                 for i, f in enumerate(fields)]
        out.append(_edge("flags", f"flags{nbits}_o{options}_{tag}", nbits, options, bs, rsi, dtype, cases))


_EDGE = []


def edge_batches():
    """the batches at the thresholds of the pack side: as batches() gives them, with family, expect (per field) and bases
    (per field "aligned" / "elem" for edge_placement, or None)"""
    if not _EDGE:
        for family in (_e_at_m, _e_clamp, _r_family, _d22, _subnormal_f4, _x_limits, _ties_below, _positions, _flags):
            family(_EDGE)
        names = [b["name"] for b in _EDGE]
        assert len(set(names)) == len(names)
    return _EDGE


def edge_placement(b, seed=0):
    """placement(), except for a batch that says where its fields lie: "aligned" on a multiple of 16 bytes, "elem" one
    element behind one"""
    if b.get("bases") is None:
        return placement(b, seed)
    offs, at = [], 0
    for f, how in zip(b["fields"], b["bases"]):
        at = up16(at) + (0 if how == "aligned" else b["elem"])
        offs.append(at)
        at += f.nbytes
    return offs, at


# ---- Y under parameters no pack produced ----------------------------------------------------------------------------------------
def run_lengths(nbits):
    per = 16 // container(nbits)          # the values a lane of k_grib_dequantise handles
    return [1, per - 1, per, per + 1, 64 * per + 1]


def _deq(family, name, nbits, dtype, sets, options=PP, bs=16, rsi=128, rng=None):
    """sets: (R, E, D, the X to cycle through or None for random ones, spots) -- a field per run length of each; spots:
    {X: the bits Y must have}"""
    params, X, expect = [], [], []
    for R, E, D, xs, spots in sets:
        for n in run_lengths(nbits):
            x = rng.integers(0, 2 ** nbits, n, dtype=np.uint64) if xs is None else np.resize(np.array(xs, np.uint64), n)
            assert int(x.max()) < 2 ** nbits
            params.append((np.float32(R), E, D))
            X.append(x.astype(np.uint32))
            expect.append(spots)
    return dict(name=name, family=family, tmpl=(nbits, options, bs, rsi), elem=np.dtype(dtype).itemsize, dtype=np.dtype(dtype), params=params,
                X=X, expect=expect)


_DEQ = []


def dequantise_cases():
    """parameters of a foreign message: dicts of name, family, tmpl, elem, dtype, params [(R, E, D)] and X [uint32 arrays] per
    field, expect [{X: bits of Y}] per field"""
    if _DEQ:
        return _DEQ
    out = _DEQ
    inf4, dmin = 0x7F800000, 1
    out.append(_deq("f4_ties", "deq_ties_f4", 8, np.float32,
                    [(1.0, -24, 0, [0, 1, 2, 3, 5, 7], {0: 0x3F800000, 1: 0x3F800000, 2: 0x3F800001, 3: 0x3F800002, 5: 0x3F800002, 7: 0x3F800004})]))
    out.append(_deq("f4_overflow", "deq_overflow_f4", 12, np.float32,
                    [(0.0, 127, 0, [0, 1, 2, 3], {0: 0, 1: 0x7F000000, 2: inf4, 3: inf4}),
                     (FLT_MAX, 103, 0, [0, 1], {0: 0x7F7FFFFF, 1: inf4}),               # half an ulp above FLT_MAX
                     (FLT_MAX, 102, 0, [0, 1], {0: 0x7F7FFFFF, 1: 0x7F7FFFFF})]))
    out.append(_deq("f4_subnormal", "deq_subnormal_f4", 24, np.float32,
                    [(0.0, -140, 0, [0, 1, 2, 3, 1000, 2 ** 14 - 1, 2 ** 14], {1: 512, 3: 3 * 512, 2 ** 14 - 1: (2 ** 14 - 1) * 512, 2 ** 14: 0x00800000}),
                     (0.0, -149, 0, [0, 1], {0: 0, 1: dmin}),
                     (0.0, -150, 0, [0, 1, 3], {0: 0, 1: 0, 3: 2 * dmin}),
                     (0.0, -70, 22, [0, 1, 3, 100, 99999], {0: 0, 1: 60, 3: 181})], options=PP, bs=32))
    out.append(_deq("f8", "deq_limits_f8", 3, np.float64,
                    [(-0.0, -1022, 0, [0, 1, 3], {0: 0, 1: 0x0010000000000000, 3: 0x0028000000000000}),
                     (0.0, 1022, 0, list(range(8)), {1: 0x7FD0000000000000, 3: 0x7FE8000000000000, 4: 0x7FF0000000000000, 7: 0x7FF0000000000000})],
                    options=0, bs=8))
    for dtype, tag in TAGS:         # R = -k * 2^E: X = k gives +0.0 exactly, whatever D
        out.append(_deq("cancellation", "deq_cancel_" + tag, 16, dtype,
                        [(-125.0, -3, D, [0, 999, 1000, 1001, 65535], {1000: 0}) for D in (0, 3, -2)]))
    for dtype, tag in TAGS:
        for nbits in (9, 17, 32):
            rng = np.random.default_rng(2222 + nbits)
            out.append(_deq("d22", f"deq_d22_n{nbits}_{tag}", nbits, dtype,
                            [(3.25e21, 72 - nbits, 22, None, {}), (-1.5, 2 - nbits, -22, None, {})], bs=32, rng=rng))
    return out


def deq_as_batch(c):
    """a case of dequantise_cases() in the shape the unpack side of the tests takes a batch in: fields of the right sizes
    (their values are not looked at), D, and model = [(R, E, 0, X)]"""
    fields = [np.zeros(x.size, c["dtype"]) for x in c["X"]]
    return dict(name=c["name"], tmpl=c["tmpl"], elem=c["elem"], dtype=c["dtype"], fields=fields, D=[D for R, E, D in c["params"]], given=None,
                model=[(R, E, 0, x) for (R, E, D), x in zip(c["params"], c["X"])])
