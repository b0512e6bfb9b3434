"""GRIB2 simple packing on the device (include/aec_gpu_grib.h, SIMPLE PACKING): the WMO definition of a template 7.0 bit
string restated twice, and the case list shared by tests/test_grib_simple_emul.py, tests/test_grib_simple_layout.py and
tests/test_gpu_grib_simple.py.

The definition: value j of a field occupies the bits [j * nbits, (j + 1) * nbits) of its stream, bit b of the stream is bit
7 - b % 8 of byte b / 8, the unused low bits of the last byte are 0.
    stream_numpy    numpy.packbits over the nbits bit planes of the values
    stream_bigint   the big-endian integer sum X_j * 2^(nbits * (n - 1 - j)), shifted left to a whole byte
Neither knows of the other or of the code under test; tests/test_grib_simple_emul.py pins one to the other on every case.
Rooms are grib_cases.x_bytes: little-endian containers, the last block padded with the last X.
"""
import numpy as np

import grib_cases as gc

PP = gc.PP
NBITS = [1, 3, 7, 8, 9, 12, 16, 17, 24, 25, 31, 32]
SMALL = [1, 7, 8, 9, 63, 64, 65]
KINDS = ["zeros", "max", "alternating", "walking", "random"]
FILL = 0xA5


def span(nbits):
    """the values of a wavefront: kGribWaveRoom = 1 KiB of containers"""
    return gc.WAVE_ROOM // gc.container(nbits)


def stream_bytes(n, nbits):
    return (n * nbits + 7) // 8


# ---- the two models -------------------------------------------------------------------------------------------------------
def stream_numpy(x, nbits):
    x = np.asarray(x, np.uint64)
    planes = ((x[:, None] >> np.arange(nbits - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(planes.reshape(-1))


def _sum(x, nbits):
    """sum X_j * 2^(nbits * (len - 1 - j)): the left half times 2^(nbits * the right half's length), plus the right half"""
    if len(x) == 1:
        return int(x[0])
    mid = len(x) // 2
    return (_sum(x[:mid], nbits) << (nbits * (len(x) - mid))) + _sum(x[mid:], nbits)


def stream_bigint(x, nbits):
    total = len(x) * nbits
    pad = -total % 8
    return np.frombuffer((_sum([int(v) for v in x], nbits) << pad).to_bytes((total + pad) // 8, "big"), np.uint8)


# ---- the case list ----------------------------------------------------------------------------------------------------------
def pattern(kind, n, nbits, rng):
    M = 2 ** nbits - 1
    j = np.arange(n, dtype=np.uint64)
    if kind == "zeros":
        x = np.zeros(n, np.uint64)
    elif kind == "max":
        x = np.full(n, M, np.uint64)
    elif kind == "alternating":
        x = (j % np.uint64(2)) * np.uint64(M)
    elif kind == "walking":
        x = np.uint64(1) << (j % np.uint64(nbits))
    elif kind == "random":
        x = rng.integers(0, M + 1, n, dtype=np.uint64)
    else:
        raise ValueError(kind)
    return x.astype(np.uint32)


def _case(name, nbits, bs, sizes, first=0, rev=False, shift=0):
    rng = np.random.default_rng(nbits * 1009 + bs * 31 + len(sizes))
    kinds = [KINDS[(i + shift) % len(KINDS)] for i in range(len(sizes))]
    X = [pattern(k, n, nbits, rng) for k, n in zip(kinds, sizes)]
    return dict(name=name, tmpl=(nbits, PP, bs, 128), X=X, kinds=kinds, first=first, rev=rev)


# the block size of the cases whose last value closes a wavefront's span while its block goes on: even, and no divisor of
# 256, 512 or 1024.  aec_gpu_grib_plan takes 12 (tests/test_grib_simple_layout.py asserts that it does).
ODD_BS = 12
_CASES = []


def cases():
    """dicts of name, tmpl = (nbits, options, block size, rsi), X (uint32 arrays, a field each), kinds, first (the offset of
    the first stream) and rev (streams in reversed order with gaps)"""
    if _CASES:
        return _CASES
    for k, nbits in enumerate(NBITS):
        s = span(nbits)
        sizes = SMALL + [s - 1, s, s + 1, 2 * s + 5]
        if nbits in (8, 16, 31):                                # a container each: 65 wavefronts and a tail
            sizes = sizes[:4] + [65 * s + 3] + sizes[4:]
        # (streams of 32-bit values are whole words: theirs start at byte 1, or none would start inside a word)
        _CASES.append(_case(f"n{nbits}", nbits, (8, 32)[k % 2], sizes, first=1 if nbits == 32 else 0, shift=k))
    for first in (1, 2, 3):                                    # (n17 itself starts at 0)
        _CASES.append(_case(f"n17_at{first}", 17, 8, SMALL + [255, 256, 257], first=first, shift=first))
    for nbits in (3, 12, 25):
        s = span(nbits)
        _CASES.append(_case(f"n{nbits}_rev", nbits, 32, SMALL + [s + 1, 2 * s + 5], first=2, rev=True, shift=2))
    for nbits in (7, 12, 25):
        s = span(nbits)
        _CASES.append(_case(f"n{nbits}_bs{ODD_BS}", nbits, ODD_BS, [s, 2 * s, 5, 2 * s, s], shift=4))
    assert len({c["name"] for c in _CASES}) == len(_CASES)
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


def n_values(c):
    return [x.size for x in c["X"]]


def rooms(c):
    nbits, _, bs, _ = c["tmpl"]
    return [gc.room(x.size, bs, nbits) for x in c["X"]]


def work_offsets(c):
    return np.concatenate([[0], np.cumsum([gc.up16(r) for r in rooms(c)])]).astype(np.uint64)


def placement(c):
    """(byte offsets of the streams, bytes of the buffer): back to back from c["first"]; rev: the last field first, and
    1 .. 3 bytes between neighbours"""
    nbits = c["tmpl"][0]
    sizes = [stream_bytes(x.size, nbits) for x in c["X"]]
    offs, at = [0] * len(sizes), c["first"]
    order = range(len(sizes) - 1, -1, -1) if c["rev"] else range(len(sizes))
    for k, i in enumerate(order):
        offs[i] = at
        at += sizes[i] + (k % 3 + 1 if c["rev"] else 0)
    return np.array(offs, np.uint64), at


def streams(c, model=stream_numpy):
    return [model(x, c["tmpl"][0]) for x in c["X"]]


def buffer_of(c, extra=0, fill=FILL):
    """the buffer a pack leaves: the streams at their places, `fill` everywhere else; extra bytes behind"""
    offs, size = placement(c)
    buf = np.full(size + extra, fill, np.uint8)
    for o, s in zip(offs, streams(c)):
        buf[int(o):int(o) + s.size] = s
    return buf, offs


def work_of(c, fill=0x5A, garbage=None):
    """the work buffer: every field's room (the last block padded with the last X), `fill` between the rooms.  garbage: a
    seed -- random bits above bit nbits of every container"""
    nbits = c["tmpl"][0]
    cont = gc.container(nbits)
    offs = work_offsets(c)
    work = np.full(int(offs[-1]), fill, np.uint8)
    rng = np.random.default_rng(garbage)
    for x, o, r in zip(c["X"], offs, rooms(c)):
        full = np.concatenate([x, np.full(r // cont - x.size, x[-1], np.uint32)]).astype(np.uint64)
        if garbage is not None and nbits < 8 * cont:
            full |= rng.integers(0, 2 ** (8 * cont - nbits), full.size, dtype=np.uint64) << np.uint64(nbits)
        work[int(o):int(o) + r] = full.astype({1: "<u1", 2: "<u2", 4: "<u4"}[cont]).view(np.uint8)
    return work


# the cases bits-pack also runs on containers with garbage above bit nbits (nbits below the container's width)
GARBAGE = ["n3", "n12", "n25", "n31", "n17_at3", "n7_bs12"]
