#!/usr/bin/env python3
"""Streams of a foreign producer whose predictor state leaves the sample range, and a model that proves they do.

tests/predictor_edges.py pins the predictor shortcuts on valid samples only.  A stream need not stay valid: a split-option
residual above xmax takes the reference's `last_out` outside [xmin, xmax] (decode.c:91-135: the one-sided branch is an
exclusive or or a subtraction, nothing cuts it to the sample width), the reference goes on computing in 32 bits and writes
the low container bytes.  The decoder kernels carry the same 32-bit state from block to block but test once per block
whether "nothing can clip here" (aec_dec.hip: store_block) -- a test written for a state inside the range.  This module
holds

  * write_stream(): a CCSDS 121.0-B-2 stream from explicit coded data sets (split k, uncompressed, second extension,
    zero-block runs, reference samples), with the bit offset of every RSI and of every 64-block segment;
  * step() / walk(): the reference's inverse predictor in Python integers with explicit 32-bit wrap, unsigned and signed,
    `last_out` as the reference types it: the state in front of every block and the bytes the reference writes;
  * the vector families (FAMILIES), each a function of (bps, bs, rsi, flags) that returns coded data sets;
  * measure(): a numpy restatement of the CONDITION store_block tests -- not of the kernels -- and required(): the counts
    a family must reach (tests/test_foreign_predictor.py checks them on the CPU);
  * wave_rounds(): the lane-by-lane correction of k_decode_wave restated, with the per-block test as it was (the sums
    alone) and as it is (the state in front inside the range as well): whether every round ends.

Every decode entry of the library on these vectors: tests/test_gpu_foreign_predictor.py.

What a stream can and cannot do (the layout of the families follows from it).  With the state inside the range a step
either stays inside (two-sided: its half fits the room) or is one-sided, x = mask ^ d or xmax - d or d - xmax - 1, which
leaves the range only for a residual d > xmax.  The per-block test of store_block, sum <= x0 - xmin && sum <= xmax - x0,
fails for such a block (its sum is above xmax, the room on the tighter side at most xmax / 2), so the block that LEAVES the
range always takes the exact steps -- and with it its whole wavefront, the test is wave-uniform.  What is at risk is the
block BEHIND it: its state in front is outside, one of the two subtractions wraps, the test passes for any small sum, and
a step that comes back across the end of the range and then meets the end (one-sided in the reference) is taken for a
running sum.  A block that starts outside, comes back and ends outside again needs a residual above xmax once more, so
its sum cannot be small: "hover" -- many consecutive blocks outside that each cross the end -- does not exist.  What does
exist, and what the family of that name holds, is a state that stays 1 to 40 outside for hundreds of consecutive blocks of
small sums (every one passes the test with a wrapped subtraction; none of them may be changed by a fix) and then comes
back across the end in a block of small sum that the running sum gets wrong.

The wave-uniform test also says where a wrong block can show: on the wave kernel (a wavefront per RSI, rounds of 64
consecutive blocks) only in a round without a leaving block -- so the block that leaves sits at the end of a round and
the block that returns at the start of the next; on the lane kernel (a lane per RSI) only where every RSI of the
wavefront leaves at the same block index -- so all RSIs of a vector share one layout.  measure() counts the wrong blocks
that sit so ("differs_uniform": by the kernel aec_gpu_decode_async takes for a table of the vector's own size;
"differs_uniform_lane": on the lane kernel whatever the RSI's length).  An RSI of 16 to 64 blocks is a single round of the
wave kernel and can show nothing there: the 300 blocks of "hover" and the crossings of the other families at
(5, 16, 16) are seen by the lane kernel only, behind a table bound above WAVE_MAX_ITEMS.
"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helpers as H  # noqa: E402

PP, MSB, SGN, B3, NE = H.AEC_DATA_PREPROCESS, H.AEC_DATA_MSB, H.AEC_DATA_SIGNED, H.AEC_DATA_3BYTE, H.AEC_NOT_ENFORCE
GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "foreign_predictor.json")
MAX_SAMPLES = 600000
M32 = 0xFFFFFFFF


def limits(bps, flags):
    if flags & SGN:
        return -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    return 0, (1 << bps) - 1


def as_int(x, flags):
    """the 32-bit state as the number the range is about: int32 for signed samples, uint32 else"""
    return x - (1 << 32) if (flags & SGN) and (x & 0x80000000) else x


def max_k(bps, flags):
    """the largest k a split option's identifier can name"""
    return (1 << H.id_len_of(bps, flags)) - 3


# ---- the stream writer -------------------------------------------------------------------------------------------------------
def _b(v, n):
    return format(v & ((1 << n) - 1), "0%db" % n) if n else ""


def write_stream(cfg, cds):
    """The stream of the coded data sets `cds`, in order:

        ("split", k, vals)   ("uncomp", vals)   ("se", vals)   ("zero", n)   ("zero", n, ref)   ("zero", "ros"[, ref])

    vals: one mapped residual per sample of the block; in the first block of an RSI (with the preprocessor) vals[0] is the
    raw reference sample.  A zero run of n blocks stays inside its 64-block segment; "ros" closes the segment.
    Returns {"stream", "bits", "rsi_bits", "seg_bits", "blk_bits", "d", "nblk"}: the bytes and their bits before padding,
    the bit offset of every RSI start, of every segment start (segments_per_rsi entries per RSI, ~0 where the RSI has no
    such segment) and of the coded data set that holds each block, the residuals as the decoder will read them (uint32,
    one row per block) and the number of blocks."""
    bps, bs, rsi, flags = cfg
    idl = H.id_len_of(bps, flags)
    pp = bool(flags & PP)
    parts, nbits, blk = [], 0, 0
    rows, rsi_bits, seg_bits, blk_bits = [], [], {}, []
    for c in cds:
        b = blk % rsi
        ref = pp and b == 0
        if b == 0:
            rsi_bits.append(nbits)
        if b % 64 == 0:
            seg_bits[(blk // rsi, b // 64)] = nbits
        kind = c[0]
        if kind == "zero":
            n = c[1]
            refv = c[2] if len(c) > 2 else 0
            room = min(rsi - b, 64 - b % 64)
            if n == "ros":
                n, fs = room, 4
            else:
                assert 1 <= n <= room and n != 5 or n > 5, c
                fs = n - 1 if n < 5 else n
            s = _b(0, idl + 1) + (_b(refv, bps) if ref else "") + "0" * fs + "1"
            for j in range(n):
                row = [0] * bs
                if ref and j == 0:
                    row[0] = refv
                rows.append(row)
            blk_bits += [nbits] * n
            blk += n
        else:
            vals = [int(v) for v in c[-1]]
            assert len(vals) == bs, (len(vals), bs)
            first = 1 if ref else 0
            if kind == "split":
                k = c[1]
                assert 0 <= k <= max_k(bps, flags), k
                s = _b(k + 1, idl) + (_b(vals[0], bps) if ref else "")
                s += "".join("0" * (v >> k) + "1" for v in vals[first:])
                if k:
                    s += "".join(_b(v, k) for v in vals[first:])
            elif kind == "uncomp":
                assert all(0 <= v < (1 << bps) for v in vals)
                s = _b((1 << idl) - 1, idl) + "".join(_b(v, bps) for v in vals)
            elif kind == "se":
                assert bs % 2 == 0
                s = _b(1, idl + 1) + (_b(vals[0], bps) if ref else "")
                for i in range(0, bs, 2):
                    a, b2 = (0 if (ref and i == 0) else vals[i]), vals[i + 1]
                    m = (a + b2) * (a + b2 + 1) // 2 + b2
                    assert m <= 90, (a, b2)
                    s += "0" * m + "1"
            else:
                raise ValueError(kind)
            rows.append([v & M32 for v in vals])
            blk_bits.append(nbits)
            blk += 1
        parts.append(s)
        nbits += len(s)
    text = "".join(parts)
    text += "0" * (-len(text) % 8)
    stream = np.packbits(np.frombuffer(text.encode("ascii"), np.uint8) - 48).tobytes()
    spr = (rsi + 63) // 64
    n_rsi = len(rsi_bits)
    sb = np.full(n_rsi * spr, 0xFFFFFFFFFFFFFFFF, np.uint64)
    for (r, j), v in seg_bits.items():
        sb[r * spr + j] = v
    return {"stream": stream, "rsi_bits": np.array(rsi_bits, np.uint64), "seg_bits": sb, "blk_bits": np.array(blk_bits, np.uint64),
            "bits": nbits, "d": np.array(rows, np.uint32).reshape(-1, bs), "nblk": blk}


# ---- the reference's inverse predictor, decode.c:91-135 ------------------------------------------------------------------------
def step(x, d, bps, flags):
    """the state behind the mapped residual d when the state in front is x; both 32 bits wide, as the reference holds them"""
    xmax = limits(bps, flags)[1]
    half = (d >> 1) + (d & 1)
    delta = (d >> 1) ^ (M32 if d & 1 else 0)                 # + d / 2, or - (d + 1) / 2, modulo 2^32
    if not flags & SGN:
        med = xmax // 2 + 1
        mask = xmax if x & med else 0
        if half <= (mask ^ x):
            return (x + delta) & M32
        return mask ^ d
    if x & 0x80000000:                                       # data < 0
        if half <= ((xmax + x + 1) & M32):
            return (x + delta) & M32
        return (d - xmax - 1) & M32
    if half <= ((xmax - x) & M32):
        return (x + delta) & M32
    return (xmax - d) & M32


def ref_state(raw, bps, flags):
    """the state behind a reference sample: the raw bits, sign-extended for signed samples (decode.c:78-84)"""
    if flags & SGN:
        m = 1 << (bps - 1)
        return ((raw ^ m) - m) & M32
    return raw


def store_bytes(v, bps, flags):
    """uint32 values -> the container bytes the reference writes (decode.c:144-189: the low bytes, by the byte order)"""
    nb = H.bytes_per_sample(bps, flags)
    v = np.asarray(v, np.uint32).reshape(-1)
    out = np.empty((v.size, nb), np.uint8)
    for i in range(nb):
        out[:, i] = (v >> np.uint32(8 * (nb - 1 - i) if flags & MSB else 8 * i)) & np.uint32(0xFF)
    return out.reshape(-1)


def walk(cfg, d):
    """(state in front of every block, values the reference writes, their bytes) for the residuals d (one row per block);
    the state in front of the first block of an RSI is what the previous RSI left: the reference sample overwrites it"""
    bps, bs, rsi, flags = cfg
    nblk = d.shape[0]
    front = np.zeros(nblk, np.uint32)
    vals = np.empty((nblk, bs), np.uint32)
    if not flags & PP:
        return front, d.copy(), store_bytes(d, bps, flags).tobytes()
    x = 0
    rows = d.tolist()
    for b in range(nblk):
        front[b] = x
        row, out = rows[b], [0] * bs
        for i in range(bs):
            if i == 0 and b % rsi == 0:
                x = ref_state(row[0], bps, flags)
            else:
                x = step(x, row[i], bps, flags)
            out[i] = x
        vals[b] = out
    return front, vals, store_bytes(vals, bps, flags).tobytes()


# ---- the model of the per-block test ---------------------------------------------------------------------------------------
def measure(cfg, d):
    """how often the blocks of a vector meet the conditions around store_block's test (the docstring of the module)"""
    bps, bs, rsi, flags = cfg
    nb = H.bytes_per_sample(bps, flags)
    xmin, xmax = limits(bps, flags)
    nblk = d.shape[0]
    c = {"blocks": nblk, "above_container": int((d.astype(np.uint64) >> np.uint64(bps)).astype(bool).sum()) if bps < 32 else 0}
    if not flags & PP:
        return c
    front, vals, _ = walk(cfg, d)
    blk = np.arange(nblk)
    isref = blk % rsi == 0
    d0 = d.astype(np.uint64)
    d0[isref, 0] = 0
    x0 = np.where(isref, np.array([ref_state(int(v), bps, flags) for v in d[:, 0]], np.uint64), front.astype(np.uint64))
    true_sum = d0.sum(axis=1)
    s32 = true_sum & np.uint64(M32)
    below = (x0 + np.uint64(xmax + 1 if flags & SGN else 0)) & np.uint64(M32)
    above = (np.uint64(xmax & M32) - x0) & np.uint64(M32)
    passes = (s32 <= below) & (s32 <= above)
    if nb == 4:
        passes &= (np.bitwise_or.reduce(d0, axis=1) >> np.uint64(26)) == 0
    xi = x0.astype(np.int64)
    if flags & SGN:
        xi = np.where(xi >= 1 << 31, xi - (1 << 32), xi)
    inside = (xi >= xmin) & (xi <= xmax)
    dist = np.where(xi > xmax, xi - xmax, np.where(xi < xmin, xmin - xi, 0))
    # the running sum from the exact state in front of the block, and whether the container bytes are the reference's
    half = (d0 >> np.uint64(1))
    delta = np.where(d0 & np.uint64(1), half ^ np.uint64(M32), half)
    run = (x0[:, None] + np.cumsum(delta, axis=1)) & np.uint64(M32)
    cmask = np.uint64((1 << (8 * nb)) - 1)
    differs = ((run & cmask) != (vals.astype(np.uint64) & cmask)).any(axis=1)
    # a round of the wave kernel: 64 consecutive blocks of an RSI; of the lane kernel: the same block of every RSI
    if rsi >= 16:
        rid = (blk // rsi) * ((rsi + 63) // 64) + (blk % rsi) // 64
    else:
        rid = (blk // rsi // 64) * rsi + blk % rsi
    order = np.argsort(rid, kind="stable")
    firsts = np.flatnonzero(np.diff(rid[order], prepend=-1))
    all_pass = np.zeros(int(rid.max()) + 1, bool)
    all_pass[rid[order][firsts]] = np.logical_and.reduceat(passes[order], firsts)
    # the lane kernel whatever the RSI's length (an RSI of 16 blocks and more goes to it behind a table of more than
    # WAVE_MAX_ITEMS entries): the same block of 64 consecutive RSIs
    lid = (blk // rsi // 64) * rsi + blk % rsi
    lorder = np.argsort(lid, kind="stable")
    lfirsts = np.flatnonzero(np.diff(lid[lorder], prepend=-1))
    lane_pass = np.zeros(int(lid.max()) + 1, bool)
    lane_pass[lid[lorder][lfirsts]] = np.logical_and.reduceat(passes[lorder], lfirsts)
    out = ~inside & ~isref
    c.update({
        "state_out": int(out.sum()),
        "state_out_near": int((out & (dist <= 40) & (true_sum < 64)).sum()),
        "passes_wrapped": int((passes & ~inside).sum()),
        "passes_in_range": int((passes & inside).sum()),
        "differs": int(differs.sum()),
        "differs_passing": int((differs & passes).sum()),
        "differs_uniform": int((differs & passes & all_pass[rid]).sum()),
        "differs_uniform_lane": int((differs & passes & lane_pass[lid]).sum()),
        "differs_in_range": int((differs & passes & inside).sum()),
        "edge_exact": int((inside & passes & ((xi == xmax) | (xi == xmin) | (true_sum == xi - xmin) | (true_sum == xmax - xi))
                           & ((true_sum > 0) | (xi == xmax) | (xi == xmin))).sum()),
        "sum_wrapped": int((true_sum > M32).sum()),
        "sum_wrapped_passes": int(((true_sum > M32) & passes).sum()),
        "x0_xmax_p1": int((out & (xi == xmax + 1)).sum()),
        "x0_xmin_m1": int((out & (xi == xmin - 1)).sum()),
        "x0_container_max": int((out & (x0 == (1 << (8 * nb)) - 1)).sum()),
        "x0_two_pow_bps": int((out & (xi == 1 << bps)).sum()) if bps < 32 else 0,
        "longest_out_run": 0,
    })
    edges = np.flatnonzero(np.diff(np.concatenate([[0], (out | (isref & (blk > 0) & np.roll(out, 1))).astype(np.int8), [0]])))
    if edges.size:
        c["longest_out_run"] = int((edges[1::2] - edges[::2]).max())
    return c


def required(family, cfg):
    """{count: least value} -- or (count, "==", value) -- a vector of this family must reach.

    RSIs of 16 to 64 blocks are one round of the wave kernel: the block that leaves the range always shares it with the
    block that returns, the wave-uniform test fails, and the wave kernel takes the exact steps whatever the test is.  Such a
    config ((5, 16, 16), the big table) can show NO wrong block on the wave kernel; its wrong blocks show on the lane
    kernel, which such RSIs reach behind a table of more than WAVE_MAX_ITEMS entries (LANE_TABLE_BOUND), and there every
    RSI of a wavefront shares one layout: "differs_uniform_lane"."""
    bps, bs, rsi, flags = cfg
    if family == "big_table":
        return dict(required("leave_and_return", cfg), differs_uniform_lane=4096)
    if family in ("leave_and_return", "below", "edge_out"):
        need = {"differs": 8, "passes_wrapped": 8, "differs_passing": 8}
        if rsi < 16 or rsi > 64:
            need["differs_uniform"] = 8
        elif family != "edge_out":
            # (edge_out: a return from the largest value of the container has a sum beyond any room, fails the test and
            # takes its wavefront along: at rsi 16 .. 64 that family exercises the shape only, on either kernel)
            need["differs_uniform_lane"] = 8
        if family == "below":
            need["x0_xmin_m1"] = 1
        if family == "edge_out":
            need["x0_xmax_p1"] = 1
            if 8 * H.bytes_per_sample(bps, flags) > bps:
                need["x0_two_pow_bps"] = 1
                if H.bytes_per_sample(bps, flags) < 4 or (bps == 31 and not flags & SGN):
                    need["x0_container_max"] = 1
        return need
    if family == "hover":
        need = {"differs": 8, "passes_wrapped": 8, "state_out": 300, "state_out_near": 300}
        if rsi >= 512:
            need["longest_out_run"] = 300
        need["differs_uniform" if rsi < 16 or rsi > 64 else "differs_uniform_lane"] = 8
        return need
    if family == "edge_in":
        return {"differs": ("==", 0), "passes_in_range": 8, "edge_exact": 8, "state_out": ("==", 0)}
    if family == "no_pp":
        return {"above_container": 8}
    if family == "sum_wraps":
        need = {"sum_wrapped": 1}
        if H.bytes_per_sample(bps, flags) == 3:              # (a short coded data set: it reaches the test, and passes it)
            need["sum_wrapped_passes"] = 1
        return need
    raise KeyError(family)


def reaches(have, need):
    """the entries of `need` that `have` misses"""
    short = {}
    for k, n in need.items():
        if isinstance(n, tuple):
            if have.get(k, 0) != n[1]:
                short[k] = (have.get(k, 0), n)
        elif have.get(k, 0) < n:
            short[k] = (have.get(k, 0), n)
    return short


# ---- the lane-by-lane correction of the wave kernel ---------------------------------------------------------------------------
def wave_rounds(cfg, d, in_range_too):
    """(rounds, rounds that never end) of the correction loop of k_decode_wave, restated: the 64 blocks of a round start
    from the running sums of the blocks in front, all take the running sum if every block passes the per-block test and
    the exact steps else, and the first block whose state in front is not what the block in front of it left is put
    right, with all behind it, until none is left.  That ends when a block's samples do not depend on which of the two
    ways the wavefront went -- which the test must guarantee.  in_range_too: the test with its precondition (the state
    in front inside the range; a sum that did not wrap, for every container a split option can overflow), else the sum
    test alone."""
    bps, bs, rsi, flags = cfg
    nb = H.bytes_per_sample(bps, flags)
    xmin, xmax = limits(bps, flags)
    rows = d.tolist()
    span = (xmax - xmin) & M32

    def parts(b):
        ref = b % rsi == 0
        body = rows[b][1:] if ref else rows[b]
        return ref, body

    def passes(x0, b):
        ref, body = parts(b)
        if ref:
            x0 = ref_state(rows[b][0], bps, flags)
        s = sum(body) & M32
        lo = (x0 + (xmax + 1 if flags & SGN else 0)) & M32
        hi = (xmax - x0) & M32
        if in_range_too:
            hi = span - lo if lo <= span else 0
        return s <= lo and s <= hi and not ((nb == 4 or (nb == 3 and in_range_too)) and any(v >> 26 for v in body))

    def behind(x0, b, running):
        ref, body = parts(b)
        x = ref_state(rows[b][0], bps, flags) if ref else x0
        for v in body:
            x = (x + ((v >> 1) ^ (M32 if v & 1 else 0))) & M32 if running else step(x, v, bps, flags)
        return x

    n_rounds = endless = 0
    for r0 in range(0, len(rows), rsi):
        n, carry = min(rsi, len(rows) - r0), 0
        for g in range(0, n, 64):
            lanes = list(range(r0 + g, r0 + min(n, g + 64)))
            n_rounds += 1
            xin, acc = [], carry
            for b in lanes:
                xin.append(acc)
                acc = behind(acc, b, True)
            for _ in range(70):                              # (a loop that ends puts at least one more lane right each time)
                running = all(passes(x, b) for x, b in zip(xin, lanes))
                xout = [behind(x, b, running) for x, b in zip(xin, lanes)]
                wrong = [i for i in range(1, len(lanes)) if xout[i - 1] != xin[i]]
                if not wrong:
                    break
                delta = (xout[wrong[0] - 1] - xin[wrong[0]]) & M32
                for i in range(wrong[0], len(lanes)):
                    xin[i] = (xin[i] + delta) & M32
            else:
                endless += 1
            carry = xout[-1]
    return n_rounds, endless


# ---- building blocks of the families ---------------------------------------------------------------------------------------
class Build:
    """coded data sets appended block by block, with the reference's state behind them"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.bps, self.bs, self.rsi, self.flags = cfg
        self.xmin, self.xmax = limits(self.bps, self.flags)
        self.cds, self.blk, self.x, self.n = [], 0, 0, 0

    def at(self):
        return self.blk % self.rsi

    def value(self):
        return as_int(self.x, self.flags)

    def to(self, target):
        """the residual that takes the state to `target` (a number, inside the range or not), or None"""
        t = target & M32
        delta = target - self.value()
        cands = [2 * delta if delta >= 0 else -2 * delta - 1]
        if self.flags & SGN:
            cands += [(target + self.xmax + 1) & M32, (self.xmax - target) & M32]
        else:
            cands += [t, t ^ self.xmax]
        # (none beyond six times the container's range: the fundamental sequences stay short)
        top = min(M32, 6 << max(self.bps, 8 * min(3, H.bytes_per_sample(self.bps, self.flags))))
        for d in cands:
            if 0 <= d <= top and step(self.x, d, self.bps, self.flags) == t:
                return d
        return None

    def k_for(self, vals):
        top = max(vals) if vals else 0
        return min(max_k(self.bps, self.flags), max(0, top.bit_length() - 3))

    def block(self, vals, kind=None, ref=None):
        """one block of residuals; `ref`: the raw reference sample where the block starts an RSI"""
        vals = list(vals) + [0] * (self.bs - len(vals))
        first = self.flags & PP and self.at() == 0
        if first:
            assert ref is not None and vals[0] == 0
            vals[0] = ref
        body = vals[1:] if first else vals
        if kind is None:
            kind = ("se", "split", "uncomp", "split")[self.n % 4]
        if kind == "se" and not all(body[i] + body[i + 1] <= 12 for i in range(-len(body) % 2 and 1, len(body) - 1, 2)):
            kind = "split"
        if kind == "se" and first and body[0] > 12:
            kind = "split"
        if kind == "uncomp" and max(body) >= 1 << self.bps:
            kind = "split"
        if kind == "split":
            self.cds.append(("split", self.k_for(body), vals))
        else:
            self.cds.append((kind, vals))
        for i, v in enumerate(vals):
            self.x = ref_state(v, self.bps, self.flags) if (first and i == 0) else \
                (step(self.x, v, self.bps, self.flags) if self.flags & PP else 0)
        self.blk += 1
        self.n += 1

    def zeros(self, n=1, ref=None):
        first = self.flags & PP and self.at() == 0
        if first:
            assert ref is not None
            self.x = ref_state(ref, self.bps, self.flags)
        room = min(self.rsi - self.at(), 64 - self.at() % 64)
        assert n <= room
        if n == room and n > 4:
            self.cds.append(("zero", "ros", ref or 0))
        elif n == 5:
            self.cds += [("zero", 4, ref or 0), ("zero", 1)]
        else:
            self.cds.append(("zero", n, ref or 0))
        self.blk += n
        self.n += 1

    def room(self):
        v = self.value()
        return min(v - self.xmin, self.xmax - v)

    def calm(self, home, ref=None):
        """a block inside the range whose residual sum fits the room: towards `home`, or a step up and back"""
        first = self.flags & PP and self.at() == 0
        if first:
            self.x = ref_state(ref, self.bps, self.flags)
        v, room = self.value(), self.room()
        assert room >= 0, (v, "calm block with the state outside")
        avail = self.bs - (1 if first else 0)
        budget = min(room, 40)
        if v == home:
            vals = [2, 1] * min(avail // 2, budget // 3, 1 + self.n % 3)
        else:
            size = 1 + self.n % 2
            r = (2 * size - 1) if v > home else 2 * size
            cnt = min(avail, budget // r, abs(v - home) // size, 1 + self.n % 5)
            vals = [r] * cnt
        lead = self.n % max(1, avail - len(vals)) if vals else 0
        vals = [0] * lead + vals
        if not any(vals) and self.n % 2 == 0:
            return self.zeros(1, ref)
        self.block(([0] if first else []) + vals, ref=ref)

    def leave(self, target, home, ref=None):
        """a block whose one residual above xmax takes the state to `target`, outside the range"""
        first = self.flags & PP and self.at() == 0
        if first:
            self.x = ref_state(ref, self.bps, self.flags)
        vals = []
        d = self.to(target)
        if d is None:                                        # (signed: above only from below zero, below only from above)
            other = home if self.to(home) is not None and (home < 0) != (self.value() < 0) else \
                (self.xmin + 1 if self.value() >= 0 else self.xmax - 1)
            d0 = self.to(other)
            assert d0 is not None, (self.cfg, self.value(), other)
            keep = self.x
            self.x = step(self.x, d0, self.bps, self.flags)
            d = self.to(target)
            self.x = keep
            vals = [d0]
        assert d is not None and d > self.xmax - self.xmin, (self.cfg, self.value(), target, d)
        avail = self.bs - (1 if first else 0)
        lead = self.n % max(1, avail - len(vals) - 1)
        self.block(([0] if first else []) + [0] * lead + vals + [d], kind="split", ref=ref)
        assert self.value() == target, (self.cfg, self.value(), target)

    def dist_out(self):
        v = self.value()
        return v - self.xmax if v > self.xmax else (self.xmin - v if v < self.xmin else 0)

    def drift(self, down):
        """a block that stays outside the range: a few steps of one towards the range (down) or away from it"""
        assert self.dist_out() >= 1
        above = self.value() > self.xmax
        cnt = min(self.bs, 1 + self.n % 3, self.dist_out() - 1 if down else 40 - self.dist_out())
        r = 1 if (above == down) else 2                      # residual 1: a step of -1, residual 2: a step of +1
        lead = self.n % max(1, self.bs - cnt) if cnt > 0 else 0
        if cnt <= 0 and self.n % 2:
            return self.zeros(1)
        self.block([0] * lead + [r] * max(cnt, 0))
        assert 1 <= self.dist_out() <= 40

    def back(self, j=0, c=0):
        """the block that returns: a two-sided step across the end of the range to j inside it, then a step of j + 1 + c
        towards the end, which the reference takes one-sided (and a running sum takes to 1 + c outside again)"""
        above = self.value() > self.xmax
        edge = self.xmax - j if above else self.xmin + j
        d1 = self.to(edge)
        if d1 is None:                                       # (from far outside: 2^32 - 1 is the largest residual)
            j, edge = 0, self.xmax if above else self.xmin
            d1 = self.to(edge)
        assert d1 is not None, (self.cfg, self.value())
        half = j + 1 + c
        d2 = 2 * half if above else 2 * half - 1
        lead = self.n % max(1, self.bs - 2)
        self.block([0] * lead + [d1, d2])
        assert self.dist_out() == 0, (self.cfg, self.value())


def _homes(cfg, side):
    """reference samples for the RSIs of a vector: well inside the range, on the half from which `side` can be left for"""
    bps, bs, rsi, flags = cfg
    xmin, xmax = limits(bps, flags)
    q = max(1, (xmax - xmin + 1) // 4)
    if flags & SGN:
        return [xmin + q] if side == "above" else [xmax - q]
    return [xmin + q, xmax - q]


def _rsi_sizes(cfg, n_full, tail):
    return [cfg[2]] * n_full + ([tail] if tail else [])


def _short_tail(rsi):
    """blocks of the short last RSI: more than a round where the RSI has more than one"""
    return 1 if rsi < 16 else (5 if rsi <= 64 else min(rsi - 1, 70))


def _excursions(cfg, side, targets, n_back, drift_rounds=False):
    """RSIs that leave the range at the end of a round (a block of split residuals, one of them above xmax) and come back
    at the start of the next (Build.back); RSIs of at most 64 blocks: leave in the last block but one, come back in the
    last.  `targets`: function(i) -> how far outside excursion i goes (a number: the state).  With drift_rounds the state
    leaves in the first block of the RSI and stays outside until the RSI's last round."""
    bps, bs, rsi, flags = cfg
    b = Build(cfg)
    homes = _homes(cfg, side)
    per = 1 if rsi <= 64 else len(range(64, rsi, 128))
    if drift_rounds:
        per = 1
    n_full = -(-n_back // per) + 1
    i = 0
    for r, n in enumerate(_rsi_sizes(cfg, n_full, _short_tail(rsi))):
        home = homes[r % len(homes)]
        raw = home & ((1 << bps) - 1)
        if n <= 64:
            leave_at, back_at = ({n - 2}, {n - 1}) if n >= 2 else (set(), set())
        elif drift_rounds:
            leave_at, back_at = {0}, {(n - 1) // 64 * 64}
        else:
            back_at = set(range(64, n, 128))                 # (the round of a return holds no block that leaves)
            leave_at = {q - 1 for q in back_at}
        if drift_rounds and n >= 2:
            leave_at = {0}
        while b.blk < sum(_rsi_sizes(cfg, n_full, _short_tail(rsi))[:r + 1]):
            at = b.at()
            ref = raw if at == 0 else None
            if at in leave_at:
                b.leave(targets(i), home, ref=ref)
            elif at in back_at and b.dist_out():
                if drift_rounds:
                    assert b.dist_out() <= 6, b.dist_out()
                b.back(j=(i % 3) if b.xmax - b.xmin >= 64 else 0, c=((i // 3) % 3) if b.xmax - b.xmin >= 64 else 0)
                i += 1
            elif b.dist_out():
                nxt = min(q for q in back_at if q > at) if any(q > at for q in back_at) else n
                # away from the range up to 32 outside, back towards it in time for the return
                down = b.dist_out() >= 32 or nxt - at <= 24 or (b.dist_out() > 3 and (at // 24) % 2 == 1)
                b.drift(down)
            else:
                b.calm(home, ref=ref)
    return b.cds


def leave_and_return(bps, bs, rsi, flags):
    """out through the upper end by 1 .. 40, back across xmax in the next round's first block, whose second step is
    one-sided in the reference"""
    xmin, xmax = limits(bps, flags)
    far = min(40, (xmax - xmin) // 4)            # (the return's sum, twice the way back and a little, must fit x0 - xmin)
    return _excursions((bps, bs, rsi, flags), "above", lambda i: xmax + 1 + (7 * i) % far, 10)


def below(bps, bs, rsi, flags):
    """the signed mirror: out below xmin by 1 .. 40 (first by exactly one) and back"""
    assert flags & SGN
    xmin = limits(bps, flags)[0]
    return _excursions((bps, bs, rsi, flags), "below", lambda i: xmin - 1 - (7 * i) % 40, 10)


def hover(bps, bs, rsi, flags):
    """the state leaves in the first block of every RSI, stays 1 .. 40 outside through blocks whose residuals sum to
    less than 64 -- every one passes the present test on a wrapped subtraction, and rightly takes the running sum -- and
    returns in the first block of the RSI's last round (the module's docstring: why no block can do both)"""
    xmin, xmax = limits(bps, flags)
    side = "below" if (flags & SGN and bs == 16) else "above"
    per = (rsi - 1) if rsi <= 64 else (rsi - 1) // 64 * 64
    n_back = max(9, -(-310 // per))
    far = (lambda i: xmin - 2 - i % 5) if side == "below" else (lambda i: xmax + 2 + i % 5)
    return _excursions((bps, bs, rsi, flags), side, far, n_back, drift_rounds=True)


def edge_out(bps, bs, rsi, flags):
    """the states xmax + 1, 2^bps and the largest value of the container (signed: also xmin - 1) in front of the block
    that returns"""
    xmin, xmax = limits(bps, flags)
    nb = H.bytes_per_sample(bps, flags)
    t = [xmax + 1]
    if 8 * nb > bps:
        t.append(1 << bps)
        if nb < 4 or (bps == 31 and not flags & SGN):        # (4 bytes: a residual that returns from there exists for 31 bits only)
            t.append((1 << (8 * nb)) - 1)
    return _excursions((bps, bs, rsi, flags), "above", lambda i: t[i % len(t)], max(9, 3 * len(t)))


def edge_in(bps, bs, rsi, flags):
    """the control: the state in front of the block is exactly xmax, xmax - sum, xmin or xmin + sum; the test passes and
    the running sum is the predictor"""
    cfg = (bps, bs, rsi, flags)
    xmin, xmax = limits(bps, flags)
    b = Build(cfg)
    s = max(2, min(2 * ((bs - 1) // 2), (xmax - xmin) // 2 // 2 * 2, 40))
    starts = [(xmax, []), (xmax - s, [2] * (s // 2)), (xmin, []), (xmin + s, [1] * min(s, bs)), (xmax - s, [1, 2] * (s // 3)),
              (xmin + s, [2, 1] * (s // 3))]
    n_rsi = 13
    for r in range(n_rsi):
        v, vals = starts[r % len(starts)]
        if len(vals) > bs:
            vals = vals[:bs]
        n = rsi if r + 1 < n_rsi else _short_tail(rsi)
        raw = v & ((1 << bps) - 1)
        for at in range(n):
            if b.at() != at:
                continue
            if at == 0 and n > 1:
                b.zeros(1, ref=raw)
            elif at == 0:
                b.block([0] + vals[:bs - 1], ref=raw)
            elif at == 1 or at % 64 == 0:
                # (behind the first: the sum that is left; the state has moved, the room on that side with it)
                room = b.room()
                vv = vals if at == 1 else ([1 if b.value() > (xmin + xmax) // 2 else 2] * min(room, bs, 3))
                if sum(vv) > room and at != 1:
                    vv = []
                b.block(vv) if any(vv) else b.zeros(1)
            else:
                left = min(n - at, 64 - at % 64, 3 + r % 4)
                b.zeros(left)
    return b.cds


def no_pp(bps, bs, rsi, flags):
    """no preprocessor: split residuals above 2^bps in a container wider than bps; the low container bytes are stored"""
    assert not flags & PP and 8 * H.bytes_per_sample(bps, flags) > bps
    cfg = (bps, bs, rsi, flags)
    b = Build(cfg)
    rng = np.random.default_rng(100 * bps + bs)
    n = 2 * rsi + _short_tail(rsi) if rsi <= 130 else rsi + 70
    top = min(6 << bps, M32)
    for i in range(n):
        if i % 3 == 0:
            vals = [int(v) for v in rng.integers(0, top + 1, bs)]
            vals[i % bs] = min(top, (1 << bps) + i)
            b.block(vals, kind="split")
        elif i % 3 == 1:
            b.block([int(v) for v in rng.integers(0, 1 << bps, bs)], kind="uncomp")
        else:
            b.block([int(v) for v in rng.integers(0, 4, bs)])
    return b.cds


def sum_wraps(bps, bs, rsi, flags):
    """Containers of less than 4 bytes, where store_block had nothing like the `any >> 26` guard of 4-byte ones: one
    block whose residuals, 2^31 and 2^31 + 6, sum to 2^32 + 6.  In 2-byte containers (k at most 13) that is two
    fundamental sequences of 2^18 zeros each, a coded data set of 64 KiB, which outgrows every ring and goes to the
    sequential decoder; in 3-byte containers (k up to 29) it is a coded data set of a few dozen bits that reaches the
    per-block test with a sum of 6.  (8-bit samples: k is at most 5, the same sum takes 16 MiB; left out.)"""
    nb = H.bytes_per_sample(bps, flags)
    assert nb in (2, 3)
    cfg = (bps, bs, rsi, flags)
    xmin, xmax = limits(bps, flags)
    b = Build(cfg)
    home = xmin + (xmax - xmin + 1) // 2
    raw = home & ((1 << bps) - 1)
    wrap_at = 64 if rsi > 64 else min(1, rsi - 1)            # (the first block of a round of the wave kernel)
    for r in range(3):
        for at in range(rsi if r < 2 else 1):
            if b.at() != at:
                continue
            if r == 1 and at == wrap_at:
                b.cds.append(("split", max_k(bps, flags), ([raw] if at == 0 else []) + [1 << 31, (1 << 31) + 6] + [0] * (bs - 2 - (at == 0))))
                for v in (1 << 31, (1 << 31) + 6):
                    b.x = step(b.x, v, bps, flags)
                b.blk += 1
            elif at == 0:
                b.zeros(1, ref=raw)
            elif b.room() >= 0 and b.dist_out() == 0 and r == 0:
                b.calm(home)
            else:
                b.zeros(1)
    return b.cds


FAMILIES = {"leave_and_return": leave_and_return, "below": below, "hover": hover, "edge_in": edge_in, "edge_out": edge_out,
            "no_pp": no_pp, "sum_wraps": sum_wraps}

# (bps, bs, rsi, flags).  Containers of 1, 2, 3 and 4 bytes; bps equal to the container (8, 16) and below it (5, 12, 20 and
# 31 in 4 bytes, 24 in 3); unsigned and signed, LSB and MSB; the templated block sizes and 24 (generic store, as is every
# output 4 bytes behind a 16-byte boundary).  rsi 2: a lane per RSI; rsi 16 and 100 (short last RSI): a wavefront per RSI;
# rsi 130: three segments per RSI (segment decode); rsi 512 of 8-sample blocks: eight segments, the bare decode by segments;
# 4100 RSIs of 16 blocks of 8 samples (big_table): the lane kernel at an RSI length that otherwise goes to the wave kernel.
# The wave kernel steps back behind a table of more than WAVE_MAX_ITEMS = 8192 entries (aec_dec.hip: dec_wave_wanted; not
# 4096), and 8193 such RSIs are 1 048 704 samples, beyond the limit of 600 000 for a vector.  What sizes the launch is the
# BOUND of the table, though, not what it holds: aec_gpu_index_async + aec_gpu_decode_indexed_async with a bound of
# LANE_TABLE_BOUND RSIs send the 4100 RSIs to the lane kernel (as the libaec ABI does, whose bound is the room of a call
# and never below 4 MiB).  aec_gpu_decode_async from a table of 4100 entries is the wave kernel, where no RSI of 16
# blocks can show a wrong block (required()).
_OUT = [(16, 8, 2, PP), (8, 8, 2, PP | SGN), (5, 16, 16, PP | MSB), (12, 16, 100, PP | SGN), (16, 32, 100, PP | MSB),
        (20, 64, 100, PP | MSB | SGN), (24, 16, 100, PP | B3), (31, 8, 100, PP), (16, 16, 130, PP), (12, 32, 130, PP | SGN | MSB),
        (16, 8, 512, PP), (8, 8, 512, PP | SGN), (16, 24, 100, PP | NE), (24, 8, 2, PP | B3 | MSB | SGN), (8, 64, 100, PP)]
_BIG = (16, 8, 16, PP)                     # with 4100 RSIs (leave_and_return only)
N_BIG_RSI = 4100
WAVE_MAX_ITEMS = 8192                      # aec_dec.hip: AEC_DEC_WAVE_MAX, the most items the wave kernel takes (rsi 16 .. 63)
LANE_TABLE_BOUND = WAVE_MAX_ITEMS + 8      # a table bound that sends RSIs of 16 .. 63 blocks to the lane kernel
CONFIGS = {
    "leave_and_return": _OUT,
    "below": [c for c in _OUT if c[3] & SGN],
    "hover": [(16, 8, 512, PP), (8, 8, 512, PP | SGN), (16, 16, 130, PP), (12, 16, 100, PP | SGN), (16, 8, 2, PP),
              (31, 8, 100, PP), (5, 16, 16, PP | MSB), (24, 16, 100, PP | B3)],
    "edge_in": _OUT + [(32, 8, 100, PP), (32, 16, 2, PP | SGN)],
    "edge_out": [(16, 8, 2, PP), (12, 16, 100, PP | SGN), (20, 64, 100, PP | MSB | SGN), (24, 16, 100, PP | B3), (31, 8, 100, PP),
                 (5, 16, 16, PP | MSB), (12, 32, 130, PP | SGN | MSB), (16, 8, 512, PP), (20, 8, 2, PP)],
    "no_pp": [(5, 16, 16, MSB), (12, 16, 100, SGN), (20, 64, 100, MSB), (31, 8, 2, 0), (12, 8, 512, 0), (12, 24, 100, NE)],
    "sum_wraps": [(16, 8, 2, PP), (12, 16, 100, PP | MSB), (16, 8, 512, PP), (24, 16, 100, PP | B3), (24, 8, 2, PP | B3 | MSB | SGN),
                  (20, 64, 130, PP | B3 | SGN)],
}


def big_table(bps, bs, rsi, flags):
    """the RSIs of leave_and_return, N_BIG_RSI of them, every one leaving in its last block but one and returning in its
    last: under the lane kernel (the comment above CONFIGS) every wavefront meets the wrong block in all its lanes"""
    xmax = limits(bps, flags)[1]
    one = _excursions((bps, bs, rsi, flags), "above", lambda i: xmax + 1 + (7 * i) % 40, 40)
    per, whole, blk = [], [], 0
    for c in one:                                            # (the coded data sets of every whole RSI)
        assert c[1] != "ros"
        whole.append(c)
        blk += c[1] if c[0] == "zero" else 1
        if blk % rsi == 0:
            per.append(whole)
            whole = []
    out = []
    for r in range(N_BIG_RSI):
        out += per[r % len(per)]
    return out


FAMILIES["big_table"] = big_table
CONFIGS["big_table"] = [_BIG]

# the issue's stream: 16 bit, block 8, rsi 2, preprocessor; block 0 = split k 13, reference 0xFFF0, residual 0x1FFFA; block
# 1 = split k 0, residuals 11, 2, 0 ...
ISSUE_CFG = (16, 8, 2, PP)
ISSUE_STREAM = bytes.fromhex("efff00001ffff40000000000000000000080 09fc".replace(" ", ""))
ISSUE_SAMPLES = [0xFFF0] + [0x0005] * 7 + [0xFFFF] + [0xFFFD] * 7


def case_id(family, cfg):
    return "%s-n%d-j%d-r%d-f%d" % ((family,) + tuple(cfg))


def cases():
    return [(f, c) for f in FAMILIES for c in CONFIGS[f]]


_vectors = {}


def vector(family, cfg):
    """the written stream of a case (write_stream's dictionary) with the walk's results: "front", "bytes"; built once"""
    key = (family, tuple(cfg))
    if key not in _vectors:
        v = write_stream(cfg, FAMILIES[family](*cfg))
        assert v["nblk"] * cfg[1] <= MAX_SAMPLES, (key, v["nblk"] * cfg[1])
        v["front"], _, v["bytes"] = walk(cfg, v["d"])
        for a in (v["d"], v["front"], v["rsi_bits"], v["seg_bits"]):
            a.setflags(write=False)
        _vectors[key] = v
    return _vectors[key]


def out_block_range(v, cfg):
    """(first, last) block of the longest stretch of blocks with the state in front outside the range, or None"""
    bps, bs, rsi, flags = cfg
    if not flags & PP:
        return None
    xmin, xmax = limits(bps, flags)
    xi = v["front"].astype(np.int64)
    if flags & SGN:
        xi = np.where(xi >= 1 << 31, xi - (1 << 32), xi)
    out = ((xi < xmin) | (xi > xmax)) & (np.arange(xi.size) % rsi != 0)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], out.astype(np.int8), [0]])))
    if not edges.size:
        return None
    k = int(np.argmax(edges[1::2] - edges[::2]))
    return int(edges[2 * k]), int(edges[2 * k + 1]) - 1


def digest(data):
    return {"len": len(data), "sha256": hashlib.sha256(data).hexdigest()}


_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(GOLDEN_JSON) as f:
            _golden = json.load(f)
    return _golden
