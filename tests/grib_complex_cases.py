"""GRIB2 complex packing on the device (include/aec_gpu_grib.h, COMPLEX PACKING): the definition of a template 7.2 / 7.3
stream restated twice, a writer, and the case list shared by tests/test_grib_complex_emul.py,
tests/test_grib_complex_layout.py and tests/test_gpu_grib_complex.py.

The definition.  Bit b of a stream is bit 7 - b % 8 of byte b / 8; an integer of w bits is big-endian.  A stream is
    1. for order >= 1: ival1, ival2 (order 2 only), minsd, each extra_octets octets, sign and magnitude
    2. NG references of ref_bits bits, padded to a byte
    3. NG widths of width_bits bits, padded to a byte:  width_g = width_ref + stored
    4. NG lengths of length_bits bits, padded to a byte: len_g = length_ref + stored * length_inc, len_(NG-1) = last_length
    5. the packed values, group after group, len_g integers of width_g bits
and decodes by  s_j = ref_g + packed_j;  order 0: X_j = s_j;  order 1: X_0 = ival1, X_j = X_(j-1) + s_j + minsd;  order 2:
X_0 = ival1, X_1 = ival2, X_j = 2 X_(j-1) - X_(j-2) + s_j + minsd -- all of it modulo 2^64.
    decode_loop    a sequential loop in Python integers, group by group, the recurrence value by value
    decode_numpy   unpackbits, cumsum over the group lengths, repeat, one or two cumsum in uint64
Neither knows of the other or of the code under test; tests/test_grib_complex_emul.py pins one to the other on every case.
The writer (write) takes X and ANY grouping -- every grouping is a valid stream -- and fills what a reader must ignore with
garbage: the first `order` packed values and the stored length of the last group.
Rooms are grib_cases.x_bytes of X modulo 2^nbits: little-endian containers, the last block padded with the last X.
"""
import numpy as np

import grib_cases as gc

PP = gc.PP
RANGE, MALFORMED = 1, 2
GROUP_TILE = 64
FILL = 0xA5
DESC_KEYS = ["ref_bits", "n_groups", "width_ref", "width_bits", "length_ref", "length_inc", "last_length", "length_bits", "order",
             "extra_octets", "missing"]
M64 = (1 << 64) - 1

# The fixture derived by hand from the regulation.  n = 8, order 2, extra_octets 1, ref_bits 4, NG 3, width_ref 0, width_bits 2,
# length_ref 1, length_inc 1, length_bits 3, last_length 1:
#   0A 0C 87      ival1 = 10, ival2 = 12, minsd: sign 1, magnitude 7 = -7
#   08 00         references 0000 1000 0000 + 4 pad bits = 0, 8, 0
#   20            widths 00 10 00 + 2 pad bits = 0, 2, 0
#   30 00         lengths 001 100 000 + 7 pad bits: stored 1, 4, (0 ignored) -> 1 + 1 = 2, 1 + 4 = 5, last_length = 1
#   12 00         group 0 (width 0): nothing; group 1 (width 2, 5 values): 00 01 00 10 00 = 0, 1, 0, 2, 0; group 2: nothing
# s = 0, 0 | 8, 9, 8, 10, 8 | 0; the first two are ignored.  With h_j = s_j + minsd = 1, 2, 1, 3, 1, -7 for j = 2 .. 7:
#   X_2 = 2 * 12 - 10 + 1 = 15, X_3 = 30 - 12 + 2 = 20, X_4 = 40 - 15 + 1 = 26, X_5 = 52 - 20 + 3 = 35,
#   X_6 = 70 - 26 + 1 = 45, X_7 = 90 - 35 - 7 = 48
HAND = dict(n=8, desc=dict(ref_bits=4, n_groups=3, width_ref=0, width_bits=2, length_ref=1, length_inc=1, last_length=1, length_bits=3,
                           order=2, extra_octets=1, missing=0),
            stream=bytes.fromhex("0A0C87080020300012" "00"), X=[10, 12, 15, 20, 26, 35, 45, 48])


def container(nbits):
    return gc.container(nbits)


def tile(nbits):
    """the values of a value tile: a wavefront's 1 KiB of room"""
    return gc.WAVE_ROOM // container(nbits)


def per(nbits):
    """the values of a lane: 16 bytes of room"""
    return 16 // container(nbits)


def table_bytes(ng, bits):
    return (ng * bits + 7) // 8


def head_bytes(d):
    return ((d["order"] + 1) * d["extra_octets"] if d["order"] else 0) + sum(table_bytes(d["n_groups"], d[k])
                                                                                for k in ("ref_bits", "width_bits", "length_bits"))


# ---- decoder A: a loop in Python integers ----------------------------------------------------------------------------------
def _take(stream, pos, w):
    if w == 0:
        return 0
    b0, b1 = pos // 8, (pos + w + 7) // 8
    assert b1 <= len(stream), "the stream ends inside an integer"
    return (int.from_bytes(stream[b0:b1], "big") >> (8 * b1 - pos - w)) & ((1 << w) - 1)


def _sign_magnitude(stream, at, octets):
    if octets == 0:
        return 0
    v = int.from_bytes(stream[at:at + octets], "big")
    mag = v & ((1 << (8 * octets - 1)) - 1)
    return -mag if v >> (8 * octets - 1) else mag


def decode_loop(stream, d, n):
    """X modulo 2^64 as a list of Python integers"""
    order, ex, ng = d["order"], d["extra_octets"], d["n_groups"]
    ival1 = ival2 = minsd = 0
    at = 0
    if order:
        ival1 = _sign_magnitude(stream, 0, ex)
        if order == 2:
            ival2 = _sign_magnitude(stream, ex, ex)
        minsd = _sign_magnitude(stream, order * ex, ex)
        at = (order + 1) * ex
    pos = 8 * at
    refs = [_take(stream, pos + g * d["ref_bits"], d["ref_bits"]) for g in range(ng)]
    pos += 8 * table_bytes(ng, d["ref_bits"])
    widths = [d["width_ref"] + _take(stream, pos + g * d["width_bits"], d["width_bits"]) for g in range(ng)]
    pos += 8 * table_bytes(ng, d["width_bits"])
    lengths = [d["length_ref"] + d["length_inc"] * _take(stream, pos + g * d["length_bits"], d["length_bits"]) for g in range(ng)]
    lengths[-1] = d["last_length"]
    pos += 8 * table_bytes(ng, d["length_bits"])
    assert sum(lengths) == n and max(widths) <= 32
    X, j = [], 0
    for g in range(ng):
        for _ in range(lengths[g]):
            s = refs[g] + _take(stream, pos, widths[g])
            pos += widths[g]
            if order == 0:
                x = s
            elif j == 0:
                x = ival1
            elif order == 2 and j == 1:
                x = ival2
            elif order == 1:
                x = X[j - 1] + s + minsd
            else:
                x = 2 * X[j - 1] - X[j - 2] + s + minsd
            X.append(x & M64)
            j += 1
    assert pos <= 8 * len(stream)
    return X


# ---- decoder B: NumPy --------------------------------------------------------------------------------------------------------
def _table(bits, pos, ng, w):
    if w == 0:
        return np.zeros(ng, np.uint64)
    rows = bits[pos:pos + ng * w].reshape(ng, w).astype(np.uint64)
    return (rows << np.arange(w - 1, -1, -1, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def _sm_numpy(raw):
    if raw.size == 0:
        return np.uint64(0)
    mag = np.uint64(0)
    for k, b in enumerate(raw):
        mag = (mag << np.uint64(8)) | np.uint64(int(b) & (0x7F if k == 0 else 0xFF))
    return (np.uint64(0) - mag) if raw[0] & 0x80 else mag


def decode_numpy(stream, d, n):
    """X modulo 2^64 as a uint64 array"""
    raw = np.frombuffer(stream, np.uint8)
    bits = np.concatenate([np.unpackbits(raw), np.zeros(1, np.uint8)])      # (a bit behind the stream: widths of 0 index it, masked)
    order, ex, ng = d["order"], d["extra_octets"], d["n_groups"]
    at = (order + 1) * ex if order else 0
    pos = 8 * at
    refs = _table(bits, pos, ng, d["ref_bits"])
    pos += 8 * table_bytes(ng, d["ref_bits"])
    widths = _table(bits, pos, ng, d["width_bits"]) + np.uint64(d["width_ref"])
    pos += 8 * table_bytes(ng, d["width_bits"])
    lengths = _table(bits, pos, ng, d["length_bits"]) * np.uint64(d["length_inc"]) + np.uint64(d["length_ref"])
    lengths[-1] = d["last_length"]
    pos += 8 * table_bytes(ng, d["length_bits"])
    assert int(lengths.sum()) == n
    w = np.repeat(widths, lengths.astype(np.int64)).astype(np.int64)
    ref = np.repeat(refs, lengths.astype(np.int64))
    first = pos + np.concatenate([[0], np.cumsum(w)[:-1]])
    k = np.arange(32)
    idx = np.minimum(first[:, None] + k, bits.size - 1)
    take = k < w[:, None]
    shift = np.where(take, w[:, None] - 1 - k, 0).astype(np.uint64)
    packed = ((bits[idx].astype(np.uint64) * take) << shift).sum(axis=1, dtype=np.uint64)
    s = ref + packed
    if order == 0:
        return s
    with np.errstate(over="ignore"):
        ival1 = _sm_numpy(raw[:ex])
        ival2 = _sm_numpy(raw[ex:2 * ex]) if order == 2 else np.uint64(0)
        dd = s + _sm_numpy(raw[order * ex:(order + 1) * ex])
        dd[0] = ival1                                     # X_(-1) = X_(-2) = 0: the recurrence itself gives X_0 and X_1
        if order == 1:
            return np.cumsum(dd, dtype=np.uint64)
        if n > 1:
            dd[1] = ival2 - np.uint64(2) * ival1
        return np.cumsum(np.cumsum(dd, dtype=np.uint64), dtype=np.uint64)


# ---- the writer ----------------------------------------------------------------------------------------------------------------
def _bits(values, w):
    if w == 0 or len(values) == 0:
        return np.zeros(0, np.uint8)
    v = np.array([int(x) for x in values], np.uint64)
    return ((v[:, None] >> np.arange(w - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).reshape(-1)


def _padded(b):
    return np.concatenate([b, np.zeros(-b.size % 8, np.uint8)])


def _sm_bytes(v, octets, minus_zero=False):
    if octets == 0:
        assert v == 0
        return b""
    assert abs(v) < 1 << (8 * octets - 1)
    sign = 1 if (v < 0 or (minus_zero and v == 0)) else 0
    return ((sign << (8 * octets - 1)) | abs(v)).to_bytes(octets, "big")


def write(X, lengths, order=0, extra=0, minsd=None, minus_zero=False, ref_bits=None, widths=None, width_ref=None, width_bits=None,
          length_ref=None, length_inc=1, length_bits=None, raw_lengths=None, seed=0):
    """(stream, descriptor) of the integers X (Python integers, the true ones: they may be negative or large) under the
    grouping `lengths`.  widths: per group, None or a width at least as large as the group needs.  minsd: None = the smallest
    raw difference.  raw_lengths = (length_bits, stored): every stored length is that value (a damaged stream)."""
    rng = np.random.default_rng(seed + len(X))
    X = [int(x) for x in X]
    n, ng = len(X), len(lengths)
    assert sum(lengths) == n and ng >= 1 and all(ln >= 0 for ln in lengths)
    if order == 0:
        raw = list(X)
        minsd = 0
    elif order == 1:
        raw = [None] + [X[j] - X[j - 1] for j in range(1, n)]
    else:
        raw = [None, None][:n] + [X[j] - 2 * X[j - 1] + X[j - 2] for j in range(2, n)]
    if minsd is None:
        minsd = min([r for r in raw if r is not None], default=0)
        if extra == 0:
            minsd = 0
    s = [None if r is None else r - minsd for r in raw]
    assert all(v is None or 0 <= v < 1 << 33 for v in s), "s_j = ref + packed cannot hold a residual"
    refs, wid, packed, at = [], [], [], 0
    for g, ln in enumerate(lengths):
        vals = [v for v in s[at:at + ln] if v is not None]
        ref = min(vals, default=0)
        if ref_bits is not None:
            ref = min(ref, (1 << ref_bits) - 1)
        need = max([(v - ref).bit_length() for v in vals], default=0)
        w = need if widths is None or widths[g % len(widths)] is None else widths[g % len(widths)]
        assert need <= w <= 32, (g, need, w)
        refs.append(ref)
        wid.append(w)
        packed.append([int(rng.integers(0, 1 << w)) if v is None else v - ref for v in s[at:at + ln]])       # (garbage where ignored)
        at += ln
    ref_bits = max(r.bit_length() for r in refs) if ref_bits is None else ref_bits
    width_ref = min(wid) if width_ref is None else width_ref
    width_bits = max(w - width_ref for w in wid).bit_length() if width_bits is None else width_bits
    body = lengths[:-1]
    length_ref = min(body, default=0) if length_ref is None else length_ref
    stored = [(ln - length_ref) // length_inc for ln in body]
    assert all(length_ref + k * length_inc == ln for k, ln in zip(stored, body))
    length_bits = max(stored, default=0).bit_length() if length_bits is None else length_bits
    stored.append(int(rng.integers(0, 1 << length_bits)))                                                     # (garbage: ignored)
    if raw_lengths is not None:
        length_bits, stored = raw_lengths[0], [raw_lengths[1]] * ng
    head = b""
    if order:
        ival = [X[0], X[1] if n > 1 else int(rng.integers(0, 100))][:order]
        head = b"".join(_sm_bytes(v, extra) for v in ival) + _sm_bytes(minsd, extra, minus_zero)
    data = np.concatenate([np.zeros(0, np.uint8)] + [_bits(p, w) for p, w in zip(packed, wid)])
    bits = np.concatenate([_padded(_bits(refs, ref_bits)), _padded(_bits([w - width_ref for w in wid], width_bits)),
                           _padded(_bits(stored, length_bits)), _padded(data)])
    desc = dict(ref_bits=ref_bits, n_groups=ng, width_ref=width_ref, width_bits=width_bits, length_ref=length_ref, length_inc=length_inc,
                last_length=lengths[-1], length_bits=length_bits, order=order, extra_octets=extra if order else 0, missing=0)
    return head + np.packbits(bits).tobytes(), desc


# ---- the case list ----------------------------------------------------------------------------------------------------------
SMALL = [1, 2, 7, 8, 9, 63, 64, 65]
WIDTHS = [0, 1, 7, 8, 9, 25, 31, 32]


def sizes(nbits):
    T = tile(nbits)
    return SMALL + [T - 1, T, T + 1, 2 * T + 5]


def grouping(rng, n, lo=1, hi=40):
    out = []
    while sum(out) < n:
        out.append(min(int(rng.integers(lo, hi + 1)), n - sum(out)))
    return out


def _walk(rng, n, nbits, step=9):
    top = (1 << nbits) - 1
    x = top // 2 + np.cumsum(rng.integers(-step, step + 1, n))
    return [int(v) for v in np.clip(x, 0, top)]


def _ramp(rng, n, order):
    """raw differences of at least 5: a positive minsd fits"""
    x = np.cumsum(rng.integers(5, 9, n))
    if order == 2:
        x = np.cumsum(x)
    return [int(v) for v in x - x[0]]         # (X_0 = 0: what a stream without extra octets can say)


def _by_widths(rng, lengths, nbits):
    """order 0: group g needs exactly the width WIDTHS[g % 8] held to nbits"""
    X, wid = [], []
    for g, ln in enumerate(lengths):
        w = min(WIDTHS[g % len(WIDTHS)], nbits)
        ref = int(rng.integers(0, 1 << (nbits - 1))) if w < nbits else 0
        vals = [int(v) for v in rng.integers(0, 1 << min(w, nbits - 1 if ref else nbits), ln, dtype=np.uint64)] if w else [0] * ln
        if w and ln:
            vals[0] = (1 << min(w, nbits - 1 if ref else nbits)) - 1
        X += [ref + v for v in vals]
        wid.append(WIDTHS[g % len(WIDTHS)])
    return X, wid


def _field(X, lengths, **kw):
    stream, desc = write(X, lengths, **kw)
    return dict(X=np.array([x & M64 for x in X], np.uint64), n=len(X), desc=desc, stream=stream, each=len(stream), damaged=None, lengths=lengths)


def _case(name, nbits, bs, fields, first=0, rev=False):
    return dict(name=name, tmpl=(nbits, PP, bs, 128), fields=fields, first=first, rev=rev)


def _family(name, nbits, bs, order, extra, kind, seed, xbits=None, **kw):
    """a field of every size of sizes(nbits)"""
    rng = np.random.default_rng(seed)
    fields = []
    for n in sizes(nbits):
        lengths = grouping(rng, n)
        if kind == "widths":
            X, wid = _by_widths(rng, lengths, nbits)
            fields.append(_field(X, lengths, order=0, widths=wid, seed=seed, **kw))
        elif kind == "ramp":
            fields.append(_field(_ramp(rng, n, order), lengths, order=order, extra=extra, minsd=3 if extra else 0, widths=WIDTHS[4:], seed=seed,
                                 **kw))
        else:
            fields.append(_field(_walk(rng, n, xbits or nbits), lengths, order=order, extra=extra, seed=seed, **kw))
    return _case(name, nbits, bs, fields)


def _damage(f, kind):
    """a clean field with one thing wrong"""
    f = dict(f, desc=dict(f["desc"]), damaged=kind)
    d = f["desc"]
    if kind == "cut":
        f["each"] = head_bytes(d) + (len(f["stream"]) - head_bytes(d)) // 2
    elif kind == "sum_low":
        d["last_length"] -= 1
    elif kind == "sum_high":
        d["last_length"] += 1
    elif kind == "width33":
        d["width_ref"] = 33
    else:
        raise ValueError(kind)
    return f


_CASES = []


def cases():
    """dicts of name, tmpl = (nbits, options, block size, rsi), fields (dicts of X as uint64 modulo 2^64, n, desc, stream, each =
    complex_bytes_each, damaged: None or what is wrong, lengths), first (the offset of the first stream) and rev"""
    if _CASES:
        return _CASES
    C = _CASES
    # orders, extra descriptors and the sign of minsd; every container; a field of every size
    C.append(_family("o0_n8", 8, 8, 0, 0, "widths", 1))
    C.append(_family("o0_n32", 32, 32, 0, 0, "widths", 2))
    C.append(_family("o1_n16_e1", 16, 16, 1, 1, "walk", 3, xbits=7))                        # minsd negative
    C.append(_family("o2_n31_e2", 31, 32, 2, 2, "walk", 4, xbits=15))
    C.append(_family("o2_n32_e4_pos", 32, 8, 2, 4, "ramp", 5))                     # minsd = +3
    C.append(_family("o1_n32_e8_pos", 32, 32, 1, 8, "ramp", 6))
    C.append(_family("o1_n16_e0", 16, 32, 1, 0, "ramp", 7))                        # no extra octets: ival1 = minsd = 0
    rng = np.random.default_rng(8)
    zero = [_field(_ramp(rng, n, 1), grouping(rng, n), order=1, extra=2, minsd=0, minus_zero=mz, seed=8) for n in (9, 70) for mz in (False, True)]
    C.append(_case("o1_n16_minsd_zero", 16, 16, zero))
    # bit counts of 0: references (every group starts at 0), widths (one width), lengths (one length)
    rng = np.random.default_rng(9)
    C.append(_case("zero_bits_n8", 8, 8, [
        _field([int(v) for v in rng.integers(0, 200, 100)], grouping(rng, 100), ref_bits=0, seed=9),
        _field([int(v) for v in rng.integers(0, 256, 96)], [12] * 8, widths=[8], seed=9),
        _field([5] * 64, [16] * 4, ref_bits=3, seed=9)]))
    # references of 32 bits
    C.append(_case("ref32_n32", 32, 32, [_field([0xFFFFFFFF, 0xFFFFFFFF, 7, 0x80000000, 0x80000001], [2, 1, 2], ref_bits=32, seed=10)]))
    # 65 value tiles and 3 values: the wavefront that scans a field's tiles loops; groups of 8 to 64 values
    rng = np.random.default_rng(11)
    n = 65 * tile(32) + 3
    C.append(_case("o2_n32_65_tiles", 32, 32, [_field(_walk(rng, n, 32, 1000), grouping(rng, n, 8, 64), order=2, extra=5, seed=11),
                                              _field(_walk(rng, 40, 32), grouping(rng, 40), order=2, extra=5, seed=11)]))
    # 64 group tiles and a group
    rng = np.random.default_rng(12)
    ng = 64 * GROUP_TILE + 1
    lengths = [int(v) for v in rng.integers(1, 4, ng)]
    C.append(_case("o1_n16_64_group_tiles", 16, 16, [_field(_walk(rng, sum(lengths), 16), lengths, order=1, extra=3, seed=12)]))
    # groupings: 16-bit containers, 8 values a lane, 512 a tile
    rng = np.random.default_rng(13)
    T, P = tile(16), per(16)
    edges = [P, P + 3, 2 * P - 3, T - 3 * P - 6, 12, 3, 2 * T + 80, 30]          # ends on a lane | crosses one | ... | crosses a tile | spans three
    n = sum(edges)
    groupings = [_field(_walk(rng, n, 16), edges, order=2, extra=3, seed=13),
                 _field(_walk(rng, 300, 16), [300], order=1, extra=3, seed=13),                             # NG = 1
                 _field(_walk(rng, 70, 16), [1] * 70, order=2, extra=3, seed=13),                           # NG = n
                 _field([7] * 20 + [9] * 30 + [4] * 3 + _walk(rng, 40, 16) + [1] * 100, [20, 30, 3, 40, 50, 50], seed=13),   # runs of width 0
                 _field(_walk(rng, 50, 16), [1, 9, 40], order=2, extra=3, seed=13),                         # a first group shorter than order
                 _field(_walk(rng, 50, 16), [1, 1, 48], order=2, extra=3, seed=13),
                 _field(_walk(rng, 60, 16), [0, 10, 0, 0, 50, 0], order=1, extra=3, seed=13)]              # groups without a value
    C.append(_case("groupings_n16", 16, 16, groupings))
    # placement: the first stream at every address modulo 4 (the neighbours touch); reversed with gaps
    rng = np.random.default_rng(14)
    small = [_field(_walk(rng, n, 16), grouping(rng, n, 1, 9), order=2, extra=3, seed=14) for n in (1, 2, 9, 65, 130)]
    for first in range(4):
        C.append(_case(f"at{first}_n16", 16, 16, small, first=first))
    C.append(_case("rev_n16", 16, 16, small, first=2, rev=True))
    # modular arithmetic.  Every X fits 32 bits while the decoder's unsigned running sums pass 2^64 at every swing (a second
    # difference of -2^31 + 2 is 2^64 - 2^31 + 2 as the sums hold it, minsd likewise, and the tile aggregates weigh them by up to
    # a tile's length): a sum that saturates, or is taken in fewer than 64 bits, fails
    A = (1 << 30) - 1
    swing = [0, A, 0, A, 5, A - 16, 3] * 40
    C.append(_case("o2_n32_wraps", 32, 32, [_field(swing, grouping(np.random.default_rng(15), len(swing)), order=2, extra=5, seed=15)]))
    # ... and a second-order field whose sums truly leave 64 bits (minsd = 2^63 - 1): RANGE, x_min / x_max exact modulo 2^64
    rng = np.random.default_rng(16)
    big = [3, 4]
    for j in range(2, 300):
        big.append(2 * big[-1] - big[-2] + int(rng.integers(0, 50)) + (1 << 63) - 1)
    big = [v & M64 for v in big]
    over = _field_from_residuals(big, [100, 200], 2, 8, (1 << 63) - 1, 16)
    C.append(_case("o2_n32_leaves_64", 32, 32, [small[3], over, small[2]]))
    # out of range: X above 2^nbits - 1, and negative X
    rng = np.random.default_rng(17)
    above = _field([int(v) for v in rng.integers(0, 300, 90)] + [300], grouping(rng, 91), seed=17)
    below = _field([-5] + [int(v) for v in np.cumsum(rng.integers(-2, 4, 80))], grouping(rng, 81), order=1, extra=2, seed=17)
    fine = _field(_walk(rng, 77, 8), grouping(rng, 77), order=1, extra=2, seed=17)
    C.append(_case("range_n8", 8, 8, [above, fine, below]))
    # damaged streams, each between two clean fields
    rng = np.random.default_rng(18)
    clean = [_field(_walk(rng, n, 16), grouping(rng, n), order=2, extra=3, seed=18) for n in (600, 90, 1100, 64, 520, 33)]
    C.append(_case("damaged_n16", 16, 16, [clean[0], _damage(clean[0], "cut"), clean[1], _damage(clean[2], "sum_low"), clean[3],
                                          _damage(clean[2], "sum_high"), clean[4], _damage(clean[0], "width33"), clean[5],
                                          _huge_lengths(19), clean[1]]))
    assert len({c["name"] for c in C}) == len(C)
    return C


def _field_from_residuals(X, lengths, order, extra, minsd, seed):
    """a field whose true X (taken modulo 2^64 already) only the modular recurrence reproduces: the writer's residuals are
    computed modulo 2^64 here and handed over as an order-0 string with the extra descriptors put in front"""
    n = len(X)
    s = [0, 0] + [(X[j] - 2 * X[j - 1] + X[j - 2] - minsd) & M64 for j in range(2, n)]
    assert order == 2 and all(v < 1 << 32 for v in s)
    stream, d = write(s, lengths, seed=seed)
    head = _sm_bytes(X[0], extra) + _sm_bytes(X[1], extra) + _sm_bytes(minsd, extra)
    d = dict(d, order=2, extra_octets=extra)
    return dict(X=np.array(X, np.uint64), n=n, desc=d, stream=head + stream, each=len(head) + len(stream), damaged=None, lengths=lengths)


def _huge_lengths(seed):
    """every stored length 2^32 - 1 under an increment of 255"""
    rng = np.random.default_rng(seed)
    lengths = grouping(rng, 700)
    stream, d = write(_walk(rng, 700, 16), lengths, order=1, extra=3, raw_lengths=(32, 0xFFFFFFFF), seed=seed)
    d = dict(d, length_inc=255)
    return dict(X=None, n=700, desc=d, stream=stream, each=len(stream), damaged="huge_lengths", lengths=lengths)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def n_values(c):
    return [f["n"] for f in c["fields"]]


def descs(c):
    return [f["desc"] for f in c["fields"]]


def rooms(c):
    nbits, _, bs, _ = c["tmpl"]
    return [gc.room(f["n"], bs, nbits) for f in c["fields"]]


def work_offsets(c):
    return np.concatenate([[0], np.cumsum([gc.up16(r) for r in rooms(c)])]).astype(np.uint64)


def placement(c):
    """(byte offsets of the streams, their complex_bytes_each, bytes of the buffer): back to back from c["first"]; rev: the
    last field first, and 1 .. 3 bytes between neighbours.  A cut stream keeps its whole place: what follows complex_bytes_each
    is there, and must not be loaded."""
    size = [len(f["stream"]) for f in c["fields"]]
    offs, at = [0] * len(size), c["first"]
    order = range(len(size) - 1, -1, -1) if c["rev"] else range(len(size))
    for k, i in enumerate(order):
        offs[i] = at
        at += size[i] + (k % 3 + 1 if c["rev"] else 0)
    return np.array(offs, np.uint64), np.array([f["each"] for f in c["fields"]], np.uint64), at


def buffer_of(c):
    offs, each, size = placement(c)
    buf = np.full(size, FILL, np.uint8)
    for o, f in zip(offs, c["fields"]):
        buf[int(o):int(o) + len(f["stream"])] = np.frombuffer(f["stream"], np.uint8)
    return buf, offs, each


def stored_x(f, nbits):
    """X as the room holds it: modulo 2^nbits"""
    return (f["X"] & np.uint64((1 << nbits) - 1)).astype(np.uint32)


def room_regions(c):
    """(offset, bytes) of the rooms of the clean fields; [(offset, length)] of the damaged ones"""
    nbits = c["tmpl"][0]
    exact, loose = [], []
    for f, o, r in zip(c["fields"], work_offsets(c), rooms(c)):
        if f["damaged"]:
            loose.append((int(o), r))
        else:
            exact.append((int(o), gc.x_bytes(stored_x(f, nbits), nbits, r // container(nbits))))
    return exact, loose


CX_DTYPE = np.dtype([("x_min", "<i8"), ("x_max", "<i8"), ("status", "<u4"), ("pad", "<u4")])


def records(c):
    """d_cx of the clean fields (None for a damaged one)"""
    nbits = c["tmpl"][0]
    out = []
    for f in c["fields"]:
        if f["damaged"]:
            out.append(None)
            continue
        signed = f["X"].view(np.int64)
        lo, hi = int(signed.min()), int(signed.max())
        out.append((lo, hi, RANGE if lo < 0 or hi > (1 << nbits) - 1 else 0))
    return out
