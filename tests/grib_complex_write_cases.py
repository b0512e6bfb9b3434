"""Writing GRIB2 complex packing on the device (include/aec_gpu_grib.h, COMPLEX PACKING, the writer's rule): the rule restated
twice, a fixture derived from it by hand, and the case list shared by tests/test_grib_complex_write_emul.py,
tests/test_grib_complex_write_layout.py and tests/test_gpu_grib_complex_write.py.

The rule.  Under an order o and a group length G, with X_0 .. X_(n-1) below 2^nbits:
    d_j = X_j | X_j - X_(j-1) | X_j - 2 X_(j-1) + X_(j-2) for j >= o;  minsd = min d_j (0 for o = 0 or n <= o);  s_j = d_j - minsd
    group g = [g G, min(n, (g + 1) G));  ref_g = min s_j and width_g = bit length of (max s_j - ref_g) over its j >= o, both 0
    where it has none;  packed_j = s_j - ref_g, 0 for j < o
    ref_bits = bit length of max ref_g;  width_ref = min width_g;  width_bits = bit length of (max width_g - width_ref);
    length_ref = G, length_inc = 1, length_bits = 0, last_length = n - (NG - 1) G;  extra_octets = ceil((nbits + o) / 8) for
    o >= 1 else 0;  ival1 = X_0, ival2 = X_1 (0 for n = 1), minsd in sign and magnitude with plus zero
    model_loop     Python integers, value by value, the stream through a string of '0' and '1'
    model_numpy    padded (NG, G) arrays, masked minima and maxima, packbits
Neither knows the other or the code under test.  A stream is (bytes, descriptor); the descriptor has the members of
aec_gpu_grib_complex_field, so grib_complex_cases.decode_loop / decode_numpy read it back.
Rooms are grib_cases.x_bytes of X; tests poison the samples that pad the last block, which the writer never uses.
"""
import numpy as np

import grib_cases as gc
import grib_complex_cases as cc

PP = gc.PP
GROUP_LENGTHS = [16, 32, 64, 128, 256]
TABLE_TILE, OUT_TILE = 256, 1024          # groups a wavefront of the table kernel owns; bytes of packed string one of the value kernel
POISON = 0xEE
CXW_DTYPE = np.dtype([(k, "<u4") for k in cc.DESC_KEYS] + [("pad", "<u4"), ("bytes", "<u8")])

# The fixture derived by hand from the rule: nbits 8, order 1, G = 16, n = 20.
#   X = 10 12 11 15 15 14 18 20 19 19 21 25 24 24 26 27 | 32 38 43 50
#   d (j >= 1) = 2 -1 4 0 -1 4 2 -1 0 2 4 -1 0 2 1 | 5 6 5 7;  minsd = -1;  s = d + 1 = 3 0 5 1 0 5 3 0 1 3 5 0 1 3 2 | 6 7 6 8
#   group 0: ref 0, largest 5 -> width 3, packed 0 (ignored) 3 0 5 1 0 5 3 0 1 3 5 0 1 3 2;  group 1: ref 6, width 2, packed 0 1 0 2
#   ref_bits = 3 (6), width_ref = 2, width_bits = 1 (3 - 2), extra_octets = ceil(9 / 8) = 2, last_length = 4
#   00 0A         ival1 = 10
#   80 01         minsd: sign 1, magnitude 1
#   18            references 000 110 + 2 pad bits
#   80            widths 1 0 + 6 pad bits;  no lengths
#   0C 52 2B 05 D0 5A    000 011 000 101 001 000 101 011 000 001 011 101 000 001 011 010
#   12            00 01 00 10
HAND = dict(nbits=8, order=1, G=16, X=[10, 12, 11, 15, 15, 14, 18, 20, 19, 19, 21, 25, 24, 24, 26, 27, 32, 38, 43, 50],
            desc=dict(ref_bits=3, n_groups=2, width_ref=2, width_bits=1, length_ref=16, length_inc=1, last_length=4, length_bits=0, order=1,
                      extra_octets=2, missing=0),
            stream=bytes.fromhex("000A" "8001" "18" "80" "0C522B05D05A" "12"))


def extra_octets(nbits, order):
    return (nbits + order + 7) // 8 if order else 0


def bound(n, nbits, order, G):
    """B_i: host arithmetic, no stream is longer"""
    ng, wb = (n + G - 1) // G, nbits + order
    head = (order + 1) * extra_octets(nbits, order) if order else 0
    return head + (ng * wb + 7) // 8 + (6 * ng + 7) // 8 + (n * wb + 7) // 8


# ---- the rule, A: Python integers ----------------------------------------------------------------------------------------------
def _sm(v, octets):
    return ((1 << (8 * octets - 1) if v < 0 else 0) | abs(v)).to_bytes(octets, "big") if octets else b""


def _string(pairs):
    """(value, width) pairs as a big-endian bit string padded to a byte"""
    s = "".join(format(v, "0%db" % w) for v, w in pairs if w)
    s += "0" * (-len(s) % 8)
    return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


def model_loop(X, nbits, order, G):
    X = [int(x) for x in X]
    n, o = len(X), order
    assert all(0 <= x < 1 << nbits for x in X) and nbits + o <= 32
    d = [None] * n
    for j in range(o, n):
        d[j] = X[j] if o == 0 else X[j] - X[j - 1] if o == 1 else X[j] - 2 * X[j - 1] + X[j - 2]
    minsd = min(d[o:]) if o and n > o else 0
    ng = (n + G - 1) // G
    refs, wid, packed = [], [], []
    for g in range(ng):
        js = range(g * G, min(n, (g + 1) * G))
        s = [d[j] - minsd for j in js if j >= o]
        ref = min(s) if s else 0
        w = (max(s) - ref).bit_length() if s else 0
        refs.append(ref)
        wid.append(w)
        packed += [(0 if j < o else d[j] - minsd - ref, w) for j in js]
    ex = extra_octets(nbits, o)
    ref_bits, width_ref = max(refs).bit_length(), min(wid)
    width_bits = (max(wid) - width_ref).bit_length()
    head = b""
    if o:
        head = _sm(X[0], ex) + (_sm(X[1] if n > 1 else 0, ex) if o == 2 else b"") + _sm(minsd, ex)
    stream = head + _string((r, ref_bits) for r in refs) + _string((w - width_ref, width_bits) for w in wid) + _string(packed)
    desc = dict(ref_bits=ref_bits, n_groups=ng, width_ref=width_ref, width_bits=width_bits, length_ref=G, length_inc=1,
                last_length=n - (ng - 1) * G, length_bits=0, order=o, extra_octets=ex, missing=0)
    return stream, desc


# ---- the rule, B: NumPy -----------------------------------------------------------------------------------------------------------
def _bitlen(v):
    v = np.asarray(v, np.int64)
    out = np.zeros(v.shape, np.int64)
    for k in range(33):
        out += (v >> k) > 0
    return out


def _packed_bits(values, widths):
    """the bits of values[i] in widths[i] bits, big-endian, one after the other, padded to a byte"""
    values, widths = np.asarray(values, np.uint64), np.asarray(widths, np.int64)
    k = np.arange(32, dtype=np.int64)
    take = k[None, :] < widths[:, None]
    shift = np.where(take, widths[:, None] - 1 - k[None, :], 0).astype(np.uint64)
    bits = ((values[:, None] >> shift) & np.uint64(1)).astype(np.uint8)[take]
    return np.packbits(bits).tobytes()


def model_numpy(X, nbits, order, G):
    x = np.asarray(X, np.int64)
    n, o = x.size, order
    d = np.zeros(n, np.int64)
    if o == 0:
        d[:] = x
    elif o == 1:
        d[1:] = x[1:] - x[:-1]
    else:
        d[2:] = x[2:] - 2 * x[1:-1] + x[:-2]
    counted = np.arange(n) >= o
    minsd = int(d[counted].min()) if o and counted.any() else 0
    ng = (n + G - 1) // G
    s = np.full(ng * G, -1, np.int64)
    s[:n] = np.where(counted, d - minsd, -1)
    rows = s.reshape(ng, G)
    have = (rows >= 0).any(axis=1)
    refs = np.where(have, np.where(rows >= 0, rows, np.int64(1) << 40).min(axis=1), 0)
    wid = np.where(have, _bitlen(rows.max(axis=1) - refs), 0)
    packed = np.where(rows >= 0, rows - refs[:, None], 0).reshape(-1)[:n]
    ex = extra_octets(nbits, o)
    ref_bits, width_ref = int(_bitlen(refs.max())), int(wid.min())
    width_bits = int(_bitlen(wid.max() - width_ref))
    head = b""
    if o:
        ival = [int(x[0])] + ([int(x[1]) if n > 1 else 0] if o == 2 else [])
        head = b"".join(_sm(v, ex) for v in ival + [minsd])
    stream = (head + _packed_bits(refs, np.full(ng, ref_bits)) + _packed_bits(wid - width_ref, np.full(ng, width_bits)) +
              _packed_bits(packed, np.repeat(wid, G)[:n]))
    desc = dict(ref_bits=ref_bits, n_groups=ng, width_ref=width_ref, width_bits=width_bits, length_ref=G, length_inc=1,
                last_length=n - (ng - 1) * G, length_bits=0, order=o, extra_octets=ex, missing=0)
    return stream, desc


def record_of(stream, desc):
    """the aec_gpu_grib_cxw of a model stream"""
    r = np.zeros(1, CXW_DTYPE)[0]
    for k in cc.DESC_KEYS:
        r[k] = desc[k]
    r["bytes"] = len(stream)
    return r


def string_bits(stream, desc):
    """bits of the packed string of a model stream, from its tables"""
    at = 8 * cc.head_bytes(desc) - 8 * cc.table_bytes(desc["n_groups"], desc["width_bits"])
    wid = [desc["width_ref"] + cc._take(stream, at + g * desc["width_bits"], desc["width_bits"]) for g in range(desc["n_groups"])]
    lens = [desc["length_ref"]] * (desc["n_groups"] - 1) + [desc["last_length"]]
    return sum(w * ln for w, ln in zip(wid, lens)), wid


# ---- the case list ----------------------------------------------------------------------------------------------------------------
def tile(nbits):
    return cc.tile(nbits)


def sizes(nbits, G):
    T = tile(nbits)
    return sorted({1, 2, 3, 15, 16, 17, G - 1, G, G + 1, T - 1, T, T + 1, 2 * T + 5})


def _walk(rng, n, nbits, step=9):
    top = (1 << nbits) - 1
    x = top // 2 + np.cumsum(rng.integers(-step, step + 1, n))
    return np.clip(x, 0, top).astype(np.uint32)


def _noise(rng, n, nbits):
    return rng.integers(0, 1 << nbits, n, dtype=np.uint64).astype(np.uint32)


def _ramp(rng, n, nbits, lo=5, hi=9):
    """first differences of at least lo: a positive minsd at order 1"""
    return (np.cumsum(rng.integers(lo, hi, n)) % (1 << 62)).clip(0, (1 << nbits) - 1).astype(np.uint32)


def by_widths(rng, lens, widths, nbits, zero_refs=False):
    """order 0: group g of lens[g] values needs exactly the width widths[g] (0 where it has one value)"""
    out = []
    for ln, w in zip(lens, widths):
        w = min(w, nbits) if ln > 1 else 0
        ref = 0 if zero_refs or w == nbits else int(rng.integers(0, (1 << nbits) - (1 << w) + 1))
        v = rng.integers(0, 1 << w, ln, dtype=np.uint64) if w else np.zeros(ln, np.uint64)
        if w:
            v[0], v[-1] = 0, (1 << w) - 1
        out.append(ref + v)
    return np.concatenate(out).astype(np.uint32)


def _lens(n, G):
    return [G] * (n // G) + ([n % G] if n % G else [])


def _case(name, nbits, bs, order, G, fields, first=0, rev=False):
    return dict(name=name, tmpl=(nbits, PP, bs, 128), order=order, G=G, fields=[np.asarray(f, np.uint32) for f in fields], first=first,
                rev=rev)


_CASES = []


def cases():
    """dicts of name, tmpl = (nbits, options, block size, rsi), order, G, fields (X as uint32 arrays), first (the offset of the
    first stream) and rev"""
    if _CASES:
        return _CASES
    C = _CASES
    # sizes, orders and containers: every order with nbits 8, 16 and 30, every G (256 with 4-byte containers: a tile is one group)
    plan = [(8, 0, 16), (8, 1, 32), (8, 2, 64), (16, 0, 128), (16, 1, 256), (16, 2, 16), (30, 0, 32), (30, 1, 64), (30, 2, 256), (30, 2, 128)]
    for k, (nbits, o, G) in enumerate(plan):
        rng = np.random.default_rng(100 + k)
        C.append(_case(f"o{o}_n{nbits}_g{G}", nbits, (8, 16, 32)[k % 3], o, G, [_walk(rng, n, nbits, 9 << (k % 4)) for n in sizes(nbits, G)]))
    rng = np.random.default_rng(120)
    C.append(_case("o1_n31_g32", 31, 32, 1, 32, [_noise(rng, n, 31) for n in (1, 2, 33, 300)]))
    C.append(_case("o0_n32_g64", 32, 16, 0, 64, [_noise(rng, n, 32) for n in (1, 65, 300)] + [np.array([0, 0xFFFFFFFF] * 40)]))
    M = (1 << 30) - 1
    C.append(_case("o2_n30_swing_g256", 30, 32, 2, 256, [np.array([0, M] * 300), np.array([0, M] * 8 + [0]), np.array([M, 0, M])]))
    C.append(_case("o2_n30_swing_g16", 30, 8, 2, 16, [np.array([0, M] * 300)]))
    # widths: groups that need exactly 0, 1, 7, 8, 9, 25, 31, 32 in turn
    rng = np.random.default_rng(121)
    for nbits, G in ((32, 16), (8, 32)):
        n = 37 * G + 5
        lens = _lens(n, G)
        C.append(_case(f"widths_n{nbits}_g{G}", nbits, 16, 0, G, [by_widths(rng, lens, [cc.WIDTHS[g % 8] for g in range(len(lens))], nbits)]))
    # all widths equal (width_bits 0); all references 0 (ref_bits 0); a wholly constant field at each order (order 0: S = 0)
    lens = _lens(40 * 16, 16)
    C.append(_case("one_width_n16_g16", 16, 16, 0, 16, [by_widths(rng, lens, [5] * len(lens), 16)]))
    C.append(_case("zero_refs_n16_g16", 16, 16, 0, 16, [by_widths(rng, lens, [(3, 9, 1)[g % 3] for g in range(len(lens))], 16, zero_refs=True)]))
    for o in range(3):
        C.append(_case(f"constant_o{o}_n16_g32", 16, 32, o, 32, [np.full(n, 77) for n in (1, 2, 3, 40, 700)] + [np.zeros(n) for n in (1, 40, 700)]))
    # the bound: one group of the full width whose reference fills its byte reaches B - 1 (with one group width_bits is 0)
    C.append(_case("bound_n8_g16", 8, 8, 0, 16, [np.array([127, 255]), np.array([127, 255] * 8)]))
    # runs of groups of width 0 between noisy ones: at the start, in the middle, at the end, one longer than a tile
    rng = np.random.default_rng(122)
    T = tile(16)
    runs = np.concatenate([np.full(5 * 16, 9), _noise(rng, 50, 12), np.full(48, 300), _noise(rng, 30, 9), np.full(2 * T + 40, 5), _noise(rng, 70, 16),
                           np.full(100, 1)])
    for o in (0, 1):
        C.append(_case(f"zero_runs_o{o}_n16_g16", 16, 16, o, 16, [runs, runs[80:], np.full(3 * T, 4)]))
    # output ownership: widths of 1 and 2 throughout (a lane walks 128 and 64 values and crosses groups and tiles)
    for w in (1, 2):
        n = 3 * tile(8) + 7
        lens = _lens(n, 16)
        C.append(_case(f"width{w}_n8_g16", 8, 8, 0, 16, [by_widths(rng, lens, [w] * len(lens), 8)]))
    # ... a packed string that ends exactly on a lane's 16 bytes, one bit behind, one bit before; 64 lanes and a byte
    own = [by_widths(rng, [16] * 8, [1] * 8, 8), by_widths(rng, [16] * 5 + [7], [1] * 5 + [7], 8), by_widths(rng, [16] * 7 + [5], [1] * 7 + [3], 8),
           by_widths(rng, [16] * 512 + [8], [1] * 513, 8)]
    C.append(_case("string_ends_n8_g16", 8, 8, 0, 16, own))
    # scans: 65 value tiles and 3 values (more than 64 * 64 groups at G = 16: the field scan loops)
    rng = np.random.default_rng(123)
    C.append(_case("o2_n8_65_tiles_g16", 8, 32, 2, 16, [_walk(rng, 65 * tile(8) + 3, 8, 3), _walk(rng, 40, 8)]))
    C.append(_case("o1_n31_65_tiles_g256", 31, 32, 1, 256, [_walk(rng, 65 * tile(31) + 3, 31, 1000)]))
    # minsd negative (walks above), zero, positive; ival at 0 and at M
    rng = np.random.default_rng(124)
    M16 = (1 << 16) - 1
    flat = np.cumsum(rng.integers(0, 3, 200)).astype(np.uint32)
    flat[50:60] = flat[50]
    C.append(_case("minsd_o1_n16_g32", 16, 16, 1, 32, [_ramp(rng, 200, 16), flat, np.concatenate([[0, M16], _walk(rng, 60, 16)]),
                                                      np.concatenate([[M16, 0], _walk(rng, 60, 16)])]))
    C.append(_case("ival_o2_n16_g32", 16, 16, 2, 32, [np.concatenate([[0, M16], _walk(rng, 60, 16)]), np.concatenate([[M16, 0], _walk(rng, 60, 16)]),
                                                     np.array([M16]), np.array([M16, M16])]))
    # placement: the first stream at every address modulo 4 with neighbours touching at B_i; reversed with gaps of 1 to 3 bytes
    small = [_walk(rng, n, 16) for n in (1, 2, 17, 65, 130)]
    for first in range(4):
        C.append(_case(f"at{first}_n16_g16", 16, 16, 2, 16, small, first=first))
    C.append(_case("rev_n16_g16", 16, 16, 2, 16, small, first=2, rev=True))
    assert len({c["name"] for c in C}) == len(C)
    return C


def case(name):
    return next(c for c in cases() if c["name"] == name)


def n_values(c):
    return [int(f.size) for f in c["fields"]]


def bounds(c):
    return [bound(f.size, c["tmpl"][0], c["order"], c["G"]) for f in c["fields"]]


def rooms(c):
    nbits, _, bs, _ = c["tmpl"]
    return [gc.room(f.size, bs, nbits) for f in c["fields"]]


def work_offsets(c):
    return np.concatenate([[0], np.cumsum([gc.up16(r) for r in rooms(c)])]).astype(np.uint64)


def work_of(c, fill=0x5A):
    """the work buffer of a case: every room with its X, the samples that pad the last block poisoned"""
    nbits = c["tmpl"][0]
    wo = work_offsets(c)
    work = np.full(int(wo[-1]), fill, np.uint8)
    for f, o, r in zip(c["fields"], wo, rooms(c)):
        room = gc.x_bytes(f, nbits, r // gc.container(nbits))
        room[f.size * gc.container(nbits):] = POISON
        work[int(o):int(o) + r] = room
    return work


def placement(c):
    """(byte offsets of the streams, bytes of the buffer): ranges of B_i back to back from c["first"]; rev: the last field first,
    and 1 .. 3 bytes between neighbours"""
    B = bounds(c)
    offs, at = [0] * len(B), c["first"]
    order = range(len(B) - 1, -1, -1) if c["rev"] else range(len(B))
    for k, i in enumerate(order):
        offs[i] = at
        at += B[i] + (k % 3 + 1 if c["rev"] else 0)
    return np.array(offs, np.uint64), at


_MODEL = {}


def model(c):
    """[(stream, descriptor)] of a case, computed once"""
    if c["name"] not in _MODEL:
        _MODEL[c["name"]] = [model_numpy(f, c["tmpl"][0], c["order"], c["G"]) for f in c["fields"]]
    return _MODEL[c["name"]]
