"""GRIB2 CCSDS packing on the device (include/aec_gpu_grib.h): the NumPy restatement of the contract and the case list
shared by tests/test_grib_emul.py, tests/test_grib_layout.py, tests/test_gpu_grib.py and tests/golden/make_golden_grib.py.

The model: every step is one NumPy float64 operation (correctly rounded, never fused) --
    s(y)   y * 10^D for D > 0, y / 10^-D for D < 0, y for D = 0; 10^|D| from a table, exact for |D| <= 22
    R      np.float32 of s(min), one nextafter down where that lies above it
    E      frexp of range = s(max) - R and one correction; [-127, 127]; a constant field: E = 0, X = 0
    X      trunc((s(y) - R) * 2^-E + 0.5), ties up
    Y      (X * 2^E + R) / 10^D, one rounding to the element type
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
    v = np.asarray(x).astype(np.float64) * math.ldexp(1.0, E) + float(R)
    with np.errstate(over="ignore"):
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
