#!/usr/bin/env python3
"""Inputs that sit exactly on the thresholds of the predictor shortcuts, and a model that proves they do.

Every hot kernel replaces the CCSDS 121.0-B-2 unit-delay predictor by a shortcut behind one wave-uniform test ("nothing
can clip here"): the zigzag of the differences per stretch in the encoder (aec_enc.hip: pp_words_pk, fast_finish), the
running sum per block in the decoder (aec_dec.hip: store_block, k_decode_wave), the interval of predecessors per segment
in the bare-stream decode (seg_accumulate, k_seg_scan).  All of that is device text that no CPU test compiles, so an
off-by-one in one of the comparisons shows only on data that sits on the edge.  This module holds

  * fwd / inv / walk: the predictor in Python integers, written from the standard's section 4 (theta = the smaller
    distance to an end of the range; two-sided inside theta, one-sided beyond);
  * the vector families (FAMILIES), each a function of (bps, bs, rsi, flags) that returns sample values;
  * measure(): a numpy restatement of the CONDITIONS the shortcuts test -- not of the kernels -- that counts how often a
    vector sits on each of them, and required(): which counts a family must reach (tests/test_predictor_edges.py);
  * gpu_check(): every encoder and decoder path of the library on one vector, against the oracle's bytes and the
    reference's hash (tests/golden/predictor_edges.json); main() runs it over every case with the library AEC_AMD_LIB
    names (tests/test_gpu_encode_local.py runs it on the tuning build with AEC_ENC_LOCAL=1):

    AEC_AMD_LIB=libaec_amd/lib/tuning/libaec.so.0 AEC_ENC_LOCAL=1 python tests/predictor_edges.py
"""
import hashlib
import json
import os
import sys
from math import gcd

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helpers as H  # noqa: E402

PP, MSB, SGN, B3, NE = H.AEC_DATA_PREPROCESS, H.AEC_DATA_MSB, H.AEC_DATA_SIGNED, H.AEC_DATA_3BYTE, H.AEC_NOT_ENFORCE
GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predictor_edges.json")
MAX_SAMPLES = 150000


def limits(bps, flags):
    if flags & SGN:
        return -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    return 0, (1 << bps) - 1


# ---- the predictor, CCSDS 121.0-B-2 section 4.3 ------------------------------------------------------------------------------
def fwd(prev, cur, xmin, xmax):
    """mapped prediction error of `cur` behind `prev`"""
    theta = min(prev - xmin, xmax - prev)
    delta = cur - prev
    if 0 <= delta <= theta:
        return 2 * delta
    if -theta <= delta < 0:
        return 2 * -delta - 1
    return theta + abs(delta)


def inv(prev, d, xmin, xmax):
    """the sample whose mapped prediction error behind `prev` is d"""
    theta = min(prev - xmin, xmax - prev)
    if d <= 2 * theta:
        return prev + d // 2 if d % 2 == 0 else prev - (d + 1) // 2
    # beyond theta only one side is left: the far one
    return prev + (d - theta) if prev - xmin == theta else prev - (d - theta)


def walk(residuals, start, xmin, xmax):
    """the samples that follow `start` when the mapped residuals are `residuals`; all must stay inside the range"""
    out, x = [], start
    for d in residuals:
        x = inv(x, d, xmin, xmax)
        assert xmin <= x <= xmax, (start, d, x)
        out.append(x)
    return out


def segments(rsi):
    """(first block, blocks, starts an RSI) of the segments -- 64 blocks, or what is left of the RSI -- without end"""
    r = 0
    while True:
        for s in range(0, rsi, 64):
            yield r * rsi + s, min(64, rsi - s), s == 0
        r += 1


def _samples_per_chunk(bps, flags):
    nb = H.bytes_per_sample(bps, flags)
    return 16 // nb if nb in (1, 2, 4) else 0


def _tight_t(bs, R):
    """a distance from an end of the range at which a pulse to twice the distance is tight there and has room at the other"""
    return max(1, min(bs + 3, R // 3 - 1))


# ---- the vector families -----------------------------------------------------------------------------------------------------
def tight_pairs(bps, bs, rsi, flags):
    """(xmin+t -> xmin+2t): the step equals the room, two-sided; (xmin+t -> xmin+2t+1): one beyond, one-sided; their
    mirrors at the top; in otherwise constant data.  The pair slides over every sample slot of a block, then sits on the
    first sample behind a reference sample and across segment and RSI borders.  The input ends inside a block."""
    xmin, xmax = limits(bps, flags)
    R = xmax - xmin
    ts = sorted({t for t in (0, 1, 2, 3, bs - 1, bs, R // 3 - 1, R // 3) if t >= 0 and 2 * t + 1 <= R})
    combos = []
    for t in ts:
        combos += [(xmin + t, xmin + 2 * t), (xmin + t, xmin + 2 * t + 1), (xmax - t, xmax - 2 * t), (xmax - t, xmax - 2 * t - 1)]
    period = bs + 1 if bs <= 32 else bs // 2 + 1
    assert gcd(period, bs) == 1
    parts = []
    for a, b in combos:
        one = np.concatenate([np.full(period // 2, a, np.int64), np.full(period - period // 2, b, np.int64)])
        parts.append(np.tile(one, bs))
    x = np.concatenate(parts)
    # the borders: the pair across a segment start (q - 1, q) or, at every other RSI start, just behind the reference (q, q + 1)
    spr = (rsi + 63) // 64
    want = min(40, max(12, 3 * spr + 2))
    cursor, tail, k, behind_ref = x.size, [], 0, False
    for first, _, starts in segments(rsi):
        q = first * bs
        if q < cursor + 2:
            continue
        if k == want or q + 3 + bs > MAX_SAMPLES:
            break
        a, b = combos[(5 * k) % len(combos)]
        at = q - 1
        if starts:
            behind_ref = not behind_ref
            at = q if behind_ref else q - 1
        tail.append(np.full(at + 1 - cursor, a, np.int64))
        tail.append(np.full(2, b, np.int64))
        cursor = at + 3
        k += 1
    x = np.concatenate([x] + tail)
    pad = (-x.size) % bs + 3                                # ragged: three samples into a last block
    return np.concatenate([x, np.full(pad, x[-1], np.int64)])


def _segment_cases(bps, bs, rsi, flags):
    """(side, base, tight pulse, missing pulse) for wave_layout and inactive_lanes"""
    xmin, xmax = limits(bps, flags)
    R = xmax - xmin
    t = _tight_t(bs, R)
    sides = [("lo", xmin + t, xmin + 2 * t, xmin + 2 * t + 1), ("hi", xmax - t, xmax - 2 * t, xmax - 2 * t - 1)]
    if R % 3 == 0 and R // 3 > t:
        b = R // 3                                           # tight against both ends at once
        sides.append(("both", xmin + b, xmin + 2 * b, xmin + 2 * b + 1))
    return sides


def wave_layout(bps, bs, rsi, flags):
    """Whole segments for the encoder: constant but for one pulse, so that every stretch fits and one is tight -- and the
    same segment with the pulse one further, so that exactly one stretch misses by exactly one: in lane 0, in lane 63, in
    a later chunk round, in the last stretch; in segments that start an RSI and in segments that do not."""
    spc = _samples_per_chunk(bps, flags) or 4
    nv = min(64, rsi)
    nchunk = nv * bs // spc
    offs = {0, min(63, nchunk - 1) * spc, (nv - 1) * bs, (nchunk - 1) * spc}
    if nchunk > 64:
        offs.add(64 * spc)
    if nchunk >= 128:
        offs.add(127 * spc)
    offs = sorted(offs)
    out, base = [], None
    seg = segments(rsi)
    sides = _segment_cases(bps, bs, rsi, flags)
    for i, (_, cbase, tight, miss) in enumerate(sides):
        # (large RSIs: the positions shared out between the two ends; the stretch tight against both takes every other one)
        mine = offs if rsi * bs <= 2048 else offs[i::2] if i < 2 else offs[::3 if bs >= 64 else 2]
        queues = {True: [(o, p) for o in mine for p in (tight, miss)],
                  False: [(o, p) for o in mine for p in (tight, miss)] if rsi >= 128 else []}
        if base is not None:                                 # the way to the next base value lies inside a segment of its own
            _, n, _ = next(seg)
            f = np.full(n * bs, cbase, np.int64)
            f[:max(1, n * bs // 2)] = base
            out.append(f)
        base = cbase
        while queues[True] or queues[False]:
            _, n, starts = next(seg)
            s = np.full(n * bs, base, np.int64)
            if n == nv and queues[starts]:
                o, p = queues[starts].pop(0)
                s[o + 1] = p
            out.append(s)
    _, n, _ = next(seg)
    out.append(np.full(n * bs, base, np.int64))
    x = np.concatenate(out)
    assert x.size <= MAX_SAMPLES, x.size
    return x


def inactive_lanes(bps, bs, rsi, flags):
    """rsi = 65 or 130: the last segment of an RSI holds 1 or 2 blocks, all of whose stretches fit (one is tight), while
    what the lanes beyond it read does not: the start of the next RSI, and the input's last whole block and last 16 bytes."""
    assert rsi % 64 in (1, 2)
    cases = _segment_cases(bps, bs, rsi, flags)
    x = np.empty((2 * rsi + 1) * bs, np.int64)
    R = rsi * bs
    for r in range(3):
        _, base, tight, miss = cases[min(r, 1)]
        lo = r * R
        if r == 1:                                           # (the change of the base value: inside the first block)
            x[lo] = cases[0][1]
            lo += 1
        x[lo:(r + 1) * R] = base
        x[r * R + 2] = miss
        x[r * R + bs - 2] = miss
        if r < 2:
            x[(r * rsi + rsi // 64 * 64) * bs + 1] = tight
    return x


def _ladder_len(bs, R):
    return max(1, min(bs, (R - 2) // 4))


def block_ladders(bps, bs, rsi, flags):
    """Block A constant, block B unit steps whose residuals sum to exactly the room in front of B (nothing clips), or to
    one more (the last step clips at the bottom: the smallest sum at which one can); the same at the top.  At every block
    position of two RSIs, then shifted by a block; then alone among blocks that fit."""
    xmin, xmax = limits(bps, flags)
    L = _ladder_len(bs, xmax - xmin)
    kinds = [(xmin + L, 1), (xmin + L - 1, 1), (xmax - 2 * L, 2), (xmax - 2 * L + 1, 2), (xmax - (L - 1), 2)]
    pair = []
    for c, d in kinds:
        b = walk([d] * L, c, xmin, xmax)
        pair.append(np.array([c] * bs + b + [b[-1]] * (bs - L), np.int64))
    out, nblk = [], 0
    for phase in range(2):
        for i in range(max(rsi, 40)):
            out.append(pair[(i + phase) % len(pair)])
            nblk += 2
        out.append(np.full(bs, out[-1][-1], np.int64))
        nblk += 1
    # The test is wave-uniform: the block with sum = room + 1 can be taken for a fit only where the blocks of all other
    # lanes fit.  Whole RSIs, constant up to block k, the ladder in block k, constant behind it: a round of the wave
    # kernel (64 consecutive blocks) holds that one block beside blocks whose sum is 0; on the lane kernel 192 RSIs alike.
    n_now = sum(o.size for o in out)
    out.append(np.full((-n_now) % (rsi * bs), int(out[-1][-1]), np.int64))
    for c in (xmin + L, xmin + L - 1):
        b = walk([1] * L, c, xmin, xmax)
        ks = [1] * 192 if rsi < 16 else sorted({1, min(63, rsi - 1)} | ({69} if rsi > 70 else set()))
        for k in ks:
            r = np.full((rsi, bs), c, np.int64)
            r[k, :L] = b
            r[k, L:] = b[-1]
            r[k + 1:] = b[-1]
            out.append(r.reshape(-1))
    x = np.concatenate(out)
    assert x.size <= MAX_SAMPLES, x.size
    return x


def segment_edges(bps, bs, rsi, flags):
    """For the bare decode by segments (eight segments per RSI and more): RSIs in which every segment holds -- its
    predecessor lies inside the interval for which the running sum is the predictor -- and one segment sits exactly on
    the interval's lower or upper end; and RSIs in which that one segment is one beyond it (its last step clips).  The
    index pass leaves segment starts only for streams it takes over the trunk tables (more than 4.5 coded bits per sample
    and 80 per block), so the rest is noise in the middle of the range, whose steps never come near an end, and
    whole RSIs of it in between."""
    xmin, xmax = limits(bps, flags)
    R = xmax - xmin
    spr = (rsi + 63) // 64
    assert spr >= 8 and rsi % 64 == 0
    rng = np.random.default_rng(1000 * bps + bs)
    mid, amp = xmin + (R + 1) // 2, (R + 1) // 8
    Ls = max(1, min(_ladder_len(bs, R), bs - 1))
    seglen, per = 64 * bs, rsi * bs

    def noise():
        return mid + rng.integers(-amp, amp + 1, per)

    out = [noise()]
    for i, (c, d) in enumerate([(xmin + Ls, 1), (xmin + Ls - 1, 1), (xmax - Ls, 2), (xmax - Ls + 1, 2)]):
        r = noise()
        at = (spr - 1 - i) * seglen                          # the segment with the steps: the last, the one before ...
        v, k = int(r[at - 41]), at - 40
        while v != c:                                        # down (up) to c in halves: every step two-sided
            v = c + (v - c) // 2 if v > c else c - (c - v) // 2
            r[k] = v
            k += 1
        assert k < at
        r[k:at + 1] = c
        b = walk([d] * Ls, c, xmin, xmax)
        r[at + 1:at + 1 + Ls] = b
        r[at + 1 + Ls:] = b[-1]
        out += [r, noise()]
    return np.concatenate(out)


def extremes(bps, bs, rsi, flags):
    """xmin <-> xmax (the residual 2^bps - 1) for whole RSIs and single blocks.  For 32-bit samples: blocks whose residuals
    sum to 0 or 1 modulo 2^32 while a step clips, and blocks with one residual of exactly 2^26 - 1 or exactly 2^26 in data
    that otherwise fits."""
    xmin, xmax = limits(bps, flags)
    mid = xmin + (1 << (bps - 1))
    out = [np.tile(np.array([xmin, xmax], np.int64), (2 * rsi + 1) * bs // 2), np.full(2 * bs, mid, np.int64)]
    for _ in range(3):
        out += [np.tile(np.array([xmax, xmin], np.int64), bs // 2), np.full(bs, mid, np.int64)]
    if bps == 32:
        def block(first):
            return np.array(first + [first[-1]] * (bs - len(first)), np.int64)
        for rep in range(3):
            out += [np.full(bs, mid, np.int64), block([xmin, xmin + 1]),                 # 0, 2^32 - 1, 1, 0 ...
                    np.full(bs, mid, np.int64), block([xmin, xmin + 1, xmin]),           # ... 1, 1: the sum is 1
                    np.full(bs, mid - 1, np.int64), block([xmax, xmax - 1]),
                    np.full(bs, mid - 1, np.int64), block([xmax, xmax - 1, xmax]),
                    np.full(bs * (1 + rep % 2), mid, np.int64)]
            for k in (0, 1, bs // 2, bs - 1):
                up = np.full(bs, mid, np.int64)
                up[k:] = mid + (1 << 25)                     # residual 2^26
                down = np.full(bs, mid + (1 << 25), np.int64)
                down[k:] = mid                               # residual 2^26 - 1
                out += [up, down]
        # The tests are wave-uniform: a wrapped sum can only be taken for a fit where the blocks of all 64 lanes pass.
        # Whole RSIs, first block constant, every other block [end of the range, back]: residuals 2^32 - 1 and 2^31,
        # their sum 2^31 - 1 modulo 2^32 -- exactly the room on the tighter side.
        n_now = sum(o.size for o in out)
        out.append(np.full((-n_now) % (rsi * bs), mid, np.int64))
        n_rsi = 192 if rsi < 16 else max(2, -(-130 // rsi))
        for front, end in ((mid, xmin), (mid - 1, xmax)):
            r = np.full((n_rsi, rsi, bs), front, np.int64)
            r[:, 1:, 0] = end
            out.append(r.reshape(-1))
    return np.concatenate(out)


def every_pair(bps, bs, rsi, flags):
    """a, b for every ordered pair of sample values (bps <= 8)"""
    assert bps <= 8
    xmin, xmax = limits(bps, flags)
    v = np.arange(xmin, xmax + 1, dtype=np.int64)
    x = np.stack([np.repeat(v, v.size), np.tile(v, v.size)], axis=1).reshape(-1)
    return np.concatenate([x, np.full((-x.size) % bs, x[-1], np.int64)])


def every_block_clips(bps, bs, rsi, flags):
    """at least 260 consecutive blocks with a step one beyond the room each: the running sum never predicts the sample in
    front of the next block, so the decoder's wave kernel corrects lane after lane, a whole round and then another"""
    xmin, xmax = limits(bps, flags)
    t = _tight_t(bs, xmax - xmin)
    n = max(3 * rsi, 260)
    x = np.full((n, bs), xmin + t, np.int64)
    x[2 * n // 3:] = xmax - t
    slot = 1 + np.arange(n) % (bs - 2)
    x[np.arange(n), slot] = np.where(np.arange(n) < 2 * n // 3, xmin + 2 * t + 1, xmax - 2 * t - 1)
    return x.reshape(-1)


FAMILIES = {"tight_pairs": tight_pairs, "wave_layout": wave_layout, "inactive_lanes": inactive_lanes,
            "block_ladders": block_ladders, "segment_edges": segment_edges, "extremes": extremes, "every_pair": every_pair,
            "every_block_clips": every_block_clips}

# (bps, bs, rsi, flags) and what each is there for.  Encoder: direct_finish takes (bs, bytes) = (8,1) (16,1) (32,1) (8,2) (16,2),
# the packed rows of fast_finish (64,1) (32,2) (64,2), its branch for more than 16 bits the 4-byte containers, the generic
# loader 3-byte containers, bs 24, RSIs that are no multiple of 16 bytes and ragged ends.  Decoder: rsi < 16 stays on the lane
# kernel, the others take the wave kernel, rsi 512 of 8- or 16-sample blocks is decoded bare by segments; bs 24 and 3-byte
# containers take the generic kernel, as does every output 4 bytes behind a 16-byte boundary.
_GENERAL = [(8, 8, 512, PP), (16, 16, 512, PP | MSB | SGN), (12, 32, 128, PP | SGN), (7, 64, 4, PP | SGN),
            (32, 8, 4, PP | MSB), (17, 64, 130, PP | SGN), (32, 64, 64, PP | SGN), (24, 16, 20, PP | B3 | MSB | SGN),
            (16, 24, 4, PP | NE), (8, 8, 3, PP | SGN), (16, 8, 192, PP), (16, 64, 128, PP | MSB)]
CONFIGS = {
    "tight_pairs": _GENERAL + [(5, 16, 65, PP | MSB), (8, 32, 130, PP | SGN)],
    "wave_layout": [(8, 8, 512, PP), (16, 16, 512, PP | MSB | SGN), (12, 32, 128, PP | SGN), (7, 64, 128, PP | SGN),
                    (32, 8, 128, PP | MSB), (17, 64, 130, PP | SGN), (32, 64, 64, PP | SGN), (5, 16, 65, PP | MSB),
                    (8, 32, 130, PP | SGN), (16, 8, 192, PP), (16, 64, 128, PP | MSB), (24, 16, 128, PP | B3),
                    (16, 16, 4, PP), (16, 24, 70, PP | NE | SGN)],
    "inactive_lanes": [(5, 16, 65, PP | MSB), (8, 32, 130, PP | SGN), (17, 64, 130, PP | SGN), (16, 8, 65, PP),
                       (8, 64, 65, PP), (16, 32, 130, PP | MSB | SGN), (32, 8, 130, PP | MSB), (12, 16, 65, PP | SGN),
                       (24, 16, 65, PP | B3), (16, 24, 65, PP | NE)],
    "block_ladders": _GENERAL,
    "segment_edges": [(16, 16, 512, PP), (16, 8, 512, PP | MSB | SGN)],
    "extremes": _GENERAL + [(32, 16, 512, PP), (32, 32, 20, PP | SGN | MSB)],
    "every_pair": [(8, 8, 512, PP), (8, 8, 3, PP | SGN), (8, 64, 128, PP | SGN), (7, 64, 4, PP | SGN), (7, 16, 128, PP),
                   (5, 16, 65, PP | MSB), (5, 32, 16, PP | SGN), (3, 8, 16, PP), (3, 24, 4, PP | SGN | NE)],
    "every_block_clips": _GENERAL,
}


BY_SEGMENTS = ("segment_edges",)     # gpu_check insists that the index pass found their segment starts


def case_id(family, cfg):
    return "%s-n%d-j%d-r%d-f%d" % ((family,) + tuple(cfg))


def cases():
    return [(f, c) for f in FAMILIES for c in CONFIGS[f]]


_vectors = {}


def vector(family, cfg):
    """(sample values, packed bytes) of a case, built once"""
    key = (family, tuple(cfg))
    if key not in _vectors:
        x = FAMILIES[family](*cfg)
        xmin, xmax = limits(cfg[0], cfg[3])
        assert x.dtype == np.int64 and xmin <= x.min() and x.max() <= xmax and x.size <= MAX_SAMPLES, key
        data = H.pack_samples(x, cfg[0], cfg[3])
        x.setflags(write=False)
        data.setflags(write=False)
        _vectors[key] = (x, data)
    return _vectors[key]


def expected_decode(x, cfg):
    """what a decoder returns for the coded vector: whole blocks (the last sample repeated), and sign-extended containers"""
    bps, bs, _, flags = cfg
    nb = H.bytes_per_sample(bps, flags)
    full = np.concatenate([x, np.full((-x.size) % bs, x[-1], np.int64)])
    v = full & ((1 << (8 * nb)) - 1) if flags & SGN else full
    out = np.empty((v.size, nb), np.uint8)
    for i in range(nb):
        out[:, i] = (v >> (8 * (nb - 1 - i) if flags & MSB else 8 * i)) & 0xFF
    return out.reshape(-1).tobytes()


# ---- the model of the predicates ---------------------------------------------------------------------------------------------
def residuals(x, bps, bs, rsi, flags):
    """(mapped residuals, step clips) of the samples x, vectorised (0 and False at the reference samples)"""
    xmin, xmax = limits(bps, flags)
    R = xmax - xmin
    u = np.asarray(x, np.int64) - xmin
    prev = np.concatenate([u[:1], u[:-1]])
    theta = np.minimum(prev, R - prev)
    delta = u - prev
    two = np.abs(delta) <= theta
    d = np.where(two, np.where(delta >= 0, 2 * delta, -2 * delta - 1), theta + np.abs(delta))
    clip = ~two
    d[::rsi * bs] = 0
    clip[::rsi * bs] = False
    return d, clip


def _stretches(u, n, R):
    """per stretch of n samples with the sample in front of it: (its range, the room its smallest and largest leave)"""
    m = u.size // n
    if m == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    X = u[:m * n].reshape(m, n)
    front = np.concatenate([u[:1], X[:-1, -1]])
    lo = np.minimum(X.min(axis=1), front)
    hi = np.maximum(X.max(axis=1), front)
    return hi - lo, np.minimum(lo, R - hi)


def measure(x, bps, bs, rsi, flags):
    """how often the vector sits on each of the conditions the shortcuts test"""
    xmin, xmax = limits(bps, flags)
    R = xmax - xmin
    x = np.asarray(x, np.int64)
    u = x - xmin
    n = x.size
    nblk_whole = n // bs
    c = {}
    d, clip = residuals(x, bps, bs, rsi, flags)
    prev = np.concatenate([u[:1], u[:-1]])
    theta = np.minimum(prev, R - prev)
    step = np.abs(u - prev)
    notref = np.ones(n, bool)
    notref[::rsi * bs] = False
    c["fit_pairs"] = int((notref & (step == theta)).sum())
    c["clip_pairs"] = int((notref & (step == theta + 1)).sum())
    # where the pairs sit (by sample values: a pair across an RSI start counts though its second sample is a reference)
    at = np.flatnonzero((step > 0) & ((step == theta) | (step == theta + 1)))
    per_rsi = rsi * bs
    c["pair_behind_ref"] = int((at % per_rsi == 1).sum())
    c["pair_across_rsi"] = int((at % per_rsi == 0).sum())
    c["pair_across_block"] = int((at % bs == 0).sum())
    c["pair_across_segment"] = int((((at % per_rsi) % (64 * bs) == 0) & (at % per_rsi != 0)).sum())
    c["pair_slots"] = int(np.unique(at % bs).size)
    c["full_residual"] = int((d == (1 << bps) - 1).sum())
    c["ordered_pairs"] = int(np.unique(prev[1:] * (R + 1) + u[1:]).size) if bps <= 8 else 0

    # the segment of every whole block
    blk = np.arange(nblk_whole)
    seg_id = (blk // rsi) * ((rsi + 63) // 64) + (blk % rsi) // 64
    seg_first = np.flatnonzero(np.diff(seg_id, prepend=-1))
    seg_nblk = np.diff(np.append(seg_first, nblk_whole))
    short = seg_nblk < min(64, rsi)

    # encoder: stretches
    spc = _samples_per_chunk(bps, flags)
    for name, per in (("chunk", spc), ("blk", bs)):
        if not per:
            continue
        rng_, room = _stretches(u, per, R)
        miss = rng_ > room
        c[name + "_tight"] = int((rng_ == room).sum())
        c[name + "_miss1"] = int((rng_ == room + 1).sum())
        # per segment (whole stretches of whole blocks only)
        per_blk = bs // per if bs % per == 0 else 0
        if per_blk and nblk_whole:
            m = nblk_whole * per_blk
            s_first = seg_first * per_blk
            nmiss = np.add.reduceat(miss[:m].astype(np.int64), s_first)
            nmiss1 = np.add.reduceat((rng_[:m] == room[:m] + 1).astype(np.int64), s_first)
            ntight = np.add.reduceat((rng_[:m] == room[:m]).astype(np.int64), s_first)
            c["seg_allfit_tight_" + name] = int(((nmiss == 0) & (ntight > 0) & ~short).sum())
            c["seg_onemiss_" + name] = int(((nmiss == 1) & (nmiss1 == 1) & ~short).sum())
            c["short_allfit_tight_" + name] = int(((nmiss == 0) & (ntight > 0) & short).sum())
            # which lane (stretch of a round of 64) and which round of its segment a tight / a missing stretch is in
            n_in = seg_nblk * per_blk
            pos = np.arange(m) - np.repeat(s_first, n_in)
            last = np.repeat(np.minimum(63, n_in - 1), n_in)
            whole = np.repeat(~short, n_in)
            for what, mask in (("tight", (rng_[:m] == room[:m]) & (rng_[:m] > 0)), ("miss1", rng_[:m] == room[:m] + 1)):
                mask = mask & whole
                c["%s_%s_lane0" % (name, what)] = int((mask & (pos % 64 == 0)).sum())
                c["%s_%s_lane_last" % (name, what)] = int((mask & (pos % 64 == last)).sum())
                c["%s_%s_later_round" % (name, what)] = int((mask & (pos >= 64)).sum())
        c["last_%s_miss" % name] = int(miss[-1]) if miss.size else 0

    # decoder: blocks
    if nblk_whole:
        D = d[:nblk_whole * bs].reshape(nblk_whole, bs)
        ssum = D.sum(axis=1)
        isref = (blk % rsi) == 0
        front = np.where(isref, u[::bs][:nblk_whole], np.concatenate([u[:1], u[bs - 1::bs][:nblk_whole - 1]]))
        room = np.minimum(front, R - front)
        any_clip = clip[:nblk_whole * bs].reshape(nblk_whole, bs).any(axis=1)
        c["sum_eq_room"] = int((ssum == room).sum())
        c["sum_eq_room1"] = int((ssum == room + 1).sum())
        c["sum_eq_room1_clip"] = int(((ssum == room + 1) & any_clip).sum())
        c["wrapped"] = int((ssum >= 1 << 32).sum())
        c["wrapped_pass"] = int(((ssum >= 1 << 32) & ((ssum & 0xFFFFFFFF) <= room) & any_clip).sum())
        # the block with sum = room + 1 and a clip, every other block of its round fitting (rounds as below)
        fit_b = ssum <= room
        r1c = (ssum == room + 1) & any_clip
        c["seg_room1_clip_alone"] = int((np.logical_and.reduceat(fit_b | r1c, seg_first) &
                                         np.logical_or.reduceat(r1c, seg_first)).sum())
        g = nblk_whole // (64 * rsi)
        if rsi < 16 and g:
            c["lanes_room1_clip_alone"] = int(((fit_b | r1c)[:g * 64 * rsi].reshape(g, 64, rsi).all(axis=1) &
                                               r1c[:g * 64 * rsi].reshape(g, 64, rsi).any(axis=1)).sum())
        pass32 = (ssum & 0xFFFFFFFF) <= room
        wrapped_pass = (ssum >= 1 << 32) & pass32 & any_clip
        # ... with every other block of the round passing too: a round of the wave kernel is a segment; on the lane
        # kernel (rsi < 16) the lanes of a wavefront are 64 RSIs, all at the same block of theirs
        c["seg_wrapped_pass"] = int((np.logical_and.reduceat(pass32, seg_first) &
                                     np.logical_or.reduceat(wrapped_pass, seg_first)).sum())
        groups = nblk_whole // (64 * rsi)
        if rsi < 16 and groups:
            m = groups * 64 * rsi
            c["lanes_wrapped_pass"] = int((pass32[:m].reshape(groups, 64, rsi).all(axis=1) &
                                           wrapped_pass[:m].reshape(groups, 64, rsi).any(axis=1)).sum())
        dmax = D.max(axis=1)
        c["any26_below"] = int(((dmax == (1 << 26) - 1) & (ssum <= room)).sum())
        c["any26_at"] = int(((dmax == 1 << 26) & (ssum <= room)).sum())
        # the longest run of consecutive blocks with a clip each
        edges = np.flatnonzero(np.diff(np.concatenate([[0], any_clip.astype(np.int8), [0]])))
        c["clip_run"] = int((edges[1::2] - edges[::2]).max()) if edges.size else 0

        # bare streams: per segment the interval [lo, hi] of (predecessor - xmin) for which every step is two-sided
        half = (D >> 1) + (D & 1)
        sgn_step = np.where(D & 1, -half, half).reshape(-1)
        halfv = half.reshape(-1)
        csum = np.cumsum(sgn_step)
        s0 = seg_first * bs
        seg_len = seg_nblk * bs
        base = np.repeat(np.concatenate([[0], csum])[s0], seg_len)
        P = csum - sgn_step - base                                      # steps taken before each sample, per segment
        lo = np.maximum.reduceat(halfv - P, s0)
        hi = np.minimum.reduceat(R - halfv - P, s0)
        seg_ref = (blk[seg_first] % rsi) == 0
        pred = np.where(seg_ref, u[s0], u[np.maximum(s0 - 1, 0)])
        ok = lo <= hi
        c["seg_pred_lo"] = int((ok & (pred == lo)).sum())
        c["seg_pred_hi"] = int((ok & (pred == hi)).sum())
        c["seg_pred_lo_m1"] = int((ok & (pred == lo - 1)).sum())
        c["seg_pred_hi_p1"] = int((ok & (pred == hi + 1)).sum())
        # k_seg_scan judges an RSI as a whole: RSIs whose every segment holds, one of them on an end of its interval;
        # RSIs in which exactly one segment does not hold, and that one by exactly one
        holds = ok & (lo <= pred) & (pred <= hi)
        edge = holds & ((pred == lo) | (pred == hi)) & ((lo > 0) | (hi < R))
        beyond = ~holds & ok & ((pred == lo - 1) | (pred == hi + 1))
        r_first = np.flatnonzero(np.diff(blk[seg_first] // rsi, prepend=-1))
        n_out = np.add.reduceat((~holds).astype(np.int64), r_first)
        c["rsi_all_hold"] = int((n_out == 0).sum())
        c["rsi_holds_on_edge"] = int(((n_out == 0) & (np.add.reduceat(edge.astype(np.int64), r_first) > 0)).sum())
        c["rsi_one_beyond"] = int(((n_out == 1) & (np.add.reduceat(beyond.astype(np.int64), r_first) == 1)).sum())
    return c


def required(family, cfg):
    """{category: least count} a vector of this family must reach with this configuration"""
    bps, bs, rsi, flags = cfg
    chunk = bool(_samples_per_chunk(bps, flags)) and _samples_per_chunk(bps, flags) <= bs
    kinds = ["blk"] + (["chunk"] if chunk else [])
    if family == "tight_pairs":
        need = {"fit_pairs": 1, "clip_pairs": 1, "pair_behind_ref": 1, "pair_across_rsi": 1, "pair_across_block": 1,
                "pair_slots": bs}
        if rsi > 64:
            need["pair_across_segment"] = 1
        for k in kinds:
            need[k + "_tight"] = need[k + "_miss1"] = 1
        return need
    if family == "wave_layout":
        n = 2 if rsi >= 128 else 1                           # in segments that start an RSI, and in segments that do not
        # (a stretch that is tight against both ends misses one of them by two when a sample moves by one: not counted)
        need = {"seg_allfit_tight_" + k: 3 * n for k in kinds}
        need.update({"seg_onemiss_" + k: 2 * n for k in kinds})
        per = {"blk": bs, "chunk": _samples_per_chunk(bps, flags)}
        for k in kinds:
            for what in ("tight", "miss1"):
                need["%s_%s_lane0" % (k, what)] = need["%s_%s_lane_last" % (k, what)] = 1
                if min(64, rsi) * bs // per[k] > 64:
                    need["%s_%s_later_round" % (k, what)] = 1
        return need
    if family == "inactive_lanes":
        need = {}
        for k in kinds:
            need["short_allfit_tight_" + k] = 2
            need["last_%s_miss" % k] = 1
        return need
    if family == "block_ladders":
        need = {"sum_eq_room": 8, "sum_eq_room1": 8, "sum_eq_room1_clip": 4}
        need["lanes_room1_clip_alone" if rsi < 16 else "seg_room1_clip_alone"] = 2
        return need
    if family == "segment_edges":
        return {"seg_pred_lo": 1, "seg_pred_hi": 1, "seg_pred_lo_m1": 1, "seg_pred_hi_p1": 1, "rsi_holds_on_edge": 2,
                "rsi_one_beyond": 2, "rsi_all_hold": 7}
    if family == "extremes":
        need = {"full_residual": 2 * rsi * bs}
        if bps == 32:
            # (12 crafted blocks of each kind; one whose first sample is a reference sample loses its first step)
            need.update({"wrapped": 6, "wrapped_pass": 6, "any26_below": 6, "any26_at": 6})
            need["lanes_wrapped_pass" if rsi < 16 else "seg_wrapped_pass"] = 2
        return need
    if family == "every_pair":
        return {"ordered_pairs": 4 ** bps}
    if family == "every_block_clips":
        return {"clip_run": 130}
    raise KeyError(family)


# ---- the reference's hashes ----------------------------------------------------------------------------------------------
def digest(stream):
    return {"len": len(stream), "sha256": hashlib.sha256(stream).hexdigest()}


_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(GOLDEN_JSON) as f:
            _golden = json.load(f)
    return _golden


# ---- the GPU checks ----------------------------------------------------------------------------------------------------------
def _cut_points(x, cfg, trace):
    """byte lengths at which to cut the stream: inside the coded block that holds the first and the last clipping step, and
    inside the block behind each"""
    bps, bs, rsi, flags = cfg
    _, clip = residuals(x, *cfg)
    at = np.flatnonzero(clip)
    if at.size == 0:
        return []
    bits = trace["bits"].astype(np.int64)
    ends = np.cumsum(bits)
    cuts = set()
    for s in (int(at[0]), int(at[-1])):
        for b in (s // bs, s // bs + 1):
            if b < len(bits) and bits[b] > 0:
                mid = int(ends[b]) - int(bits[b]) // 2
                cuts.add(max(1, mid // 8))
    return sorted(cuts)


def gpu_check(family, cfg):
    """one vector through every path: device encode (stream, RSI table, segment table), table decode aligned (lane or wave
    kernel by rsi) and 4 bytes behind a 16-byte boundary (generic kernel), segment decode, bare decode (rsi 512: by
    segments where the index pass left segment starts, which it must for the families in BY_SEGMENTS; a lane per RSI
    otherwise -- the returned list says which), the libaec ABI whole and cut inside the clipping blocks.  Expected bytes
    are the oracle's and the golden hash."""
    import torch
    from libaec_amd import api, gpu
    bps, bs, rsi, flags = cfg
    tag = case_id(family, cfg)
    x, data = vector(family, cfg)
    nb = H.bytes_per_sample(bps, flags)
    nblk = (x.size + bs - 1) // bs
    out_bytes = nblk * bs * nb
    rc, want, trace, offs, bits = H.oracle_encode(data, bps, bs, rsi, flags, want_trace=True)
    assert rc == H.AEC_OK, tag
    assert digest(want) == golden()[tag], (tag, "the oracle's stream is not the reference's")
    rc, full, _ = H.oracle_decode(want, bps, bs, rsi, flags, out_bytes)
    assert rc == H.AEC_OK and len(full) == out_bytes, tag
    if bps == 8 * nb:
        assert full[:data.size] == data.tobytes(), (tag, "input identity")
    ran = []

    def rec(d_res):
        return d_res.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0]

    def same(got, what):
        if got != full:
            g, w = np.frombuffer(got, np.uint8), np.frombuffer(full, np.uint8)
            m = min(g.size, w.size)
            first = int(np.argmax(g[:m] != w[:m])) if (g[:m] != w[:m]).any() else m
            raise AssertionError((tag, what, "first wrong byte", first, "sample", first // nb, "block", first // nb // bs))
        ran.append(what)

    codec = gpu.Codec(bps, bs, rsi, flags)
    # encoder, with the segment table
    nseg = codec.segment_count(data.size)
    d_tab = torch.zeros(max(1, nseg) * 16, dtype=torch.uint8, device="cuda")
    codec.set_segment_table(d_tab)
    d_enc, nbytes, tb, _, d_off = codec.encode(torch.from_numpy(data.copy()).cuda())
    codec.set_segment_table(None)
    got = d_enc[:nbytes].cpu().numpy().tobytes()
    if got != want:
        m = min(len(got), len(want))
        g, w = np.frombuffer(got[:m], np.uint8), np.frombuffer(want[:m], np.uint8)
        first = int(np.argmax(g != w)) if (g != w).any() else m
        blk_of = int(np.searchsorted(np.cumsum(trace["bits"].astype(np.int64)), first * 8, side="right"))
        raise AssertionError((tag, "device encode", len(got), len(want), "first wrong byte", first, "block", blk_of,
                              "segment", blk_of % rsi // 64, "of RSI", blk_of // rsi))
    assert tb == bits and digest(got) == golden()[tag], tag
    assert np.array_equal(d_off.cpu().numpy()[:-1].astype(np.uint64), offs), (tag, "RSI table")
    ran.append("encode")

    d_in = torch.zeros(len(want) + 16, dtype=torch.uint8, device="cuda")
    d_in[:len(want)] = torch.frombuffer(bytearray(want), dtype=torch.uint8).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    # table decode: aligned, and 4 bytes behind a 16-byte boundary
    for off in (0, 4):
        d_out = torch.zeros(out_bytes + 32, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
        codec.decode_async(d_in, len(want), d_offs, offs.size, nblk, d_out[off:], d_res)
        assert rec(d_res)["status"] == 0, (tag, "table decode", off)
        same(d_out[off:off + out_bytes].cpu().numpy().tobytes(), "table decode, output offset %d" % off)
    # from the encoder's segment table
    d_out = torch.zeros(out_bytes + 16, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    codec.decode_segments_async(d_in, len(want), d_tab, nseg, nblk, d_out, d_res)
    assert rec(d_res)["status"] == 0, (tag, "segment decode")
    same(d_out[:out_bytes].cpu().numpy().tobytes(), "segment decode")
    # the bare stream by segments, with the index record and without
    if rsi == 512:
        n_rsi, spr = offs.size, codec.segments_per_rsi()
        for with_record in (True, False):
            d_idx = torch.zeros(n_rsi + 2, dtype=torch.int64, device="cuda")
            d_sb = torch.zeros((n_rsi + 2) * spr, dtype=torch.int64, device="cuda")
            d_ires = torch.zeros(40, dtype=torch.uint8, device="cuda")
            d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
            d_out = torch.zeros((n_rsi + 2) * rsi * bs * nb + 64 * bs * nb, dtype=torch.uint8, device="cuda")
            codec.index_segments_async(d_in, len(want), 0, d_idx, d_sb, n_rsi + 1, d_ires)
            ires = rec(d_ires)
            # (a run of zero blocks that closes a short last RSI may be counted to the end of its segment)
            assert nblk <= int(ires["n_rsi"]) * rsi + int(ires["tail_blocks"]) <= nblk + 63, (tag, ires)
            assert np.array_equal(d_idx[:n_rsi].cpu().numpy().astype(np.uint64), offs), (tag, "bare: RSI starts")
            by_segments = bool((d_sb[:(nblk // rsi) * spr] != -1).all().item())
            assert by_segments or family not in BY_SEGMENTS, (tag, "the index pass left no segment starts")
            if with_record:
                codec.decode_bare_async(d_in, len(want), d_idx, d_sb, n_rsi + 1, nblk, d_ires, d_out, d_res)
            else:
                codec.decode_bare_async(d_in, len(want), d_idx, d_sb, n_rsi, nblk, None, d_out, d_res)
            assert rec(d_res)["status"] == 0, (tag, "bare decode", with_record)
            same(d_out[:out_bytes].cpu().numpy().tobytes(), ("bare decode by segments" if by_segments else
                                                             "bare decode, a lane per RSI") + (", index record" if with_record else ""))
    codec.close()

    # the libaec ABI
    rc, got = api.aec_buffer_encode(data, bps, bs, rsi, flags)
    assert rc == H.AEC_OK and got == want, (tag, "aec_buffer_encode", rc, len(got), len(want))
    rc, dec = api.aec_buffer_decode(want, bps, bs, rsi, flags, out_bytes)
    assert rc == H.AEC_OK, (tag, "aec_buffer_decode", rc)
    same(dec, "abi")
    for cut in _cut_points(x, cfg, trace):
        rc_o, dec_o, _ = H.oracle_decode(want[:cut], bps, bs, rsi, flags, out_bytes)
        rc, dec = api.aec_buffer_decode(want[:cut], bps, bs, rsi, flags, out_bytes)
        assert rc == rc_o and dec == dec_o, (tag, "abi, stream cut at byte", cut, rc, rc_o, len(dec), len(dec_o))
        ran.append("abi cut")
    return ran


def main():
    n, paths = 0, {}
    for family, cfg in cases():
        for p in gpu_check(family, cfg):
            paths[p] = paths.get(p, 0) + 1
        n += 1
    print("paths:", paths)
    print("predictor edges ok:", n, "cases; AEC_AMD_LIB=%s" % os.environ.get("AEC_AMD_LIB"))


if __name__ == "__main__":
    main()
