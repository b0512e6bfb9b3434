"""The cases of tests/test_sz_estimate_emul.py and tests/test_gpu_sz_estimate.py (aec_gpu_sz_estimate_async: the length of
SZ_BufftoBuffCompress's stream per pixels-per-block in one pass), and of the fixture tests/golden/sz_estimate.json, in which
tests/golden/make_golden_sz_estimate.py stores the lengths of the streams the reference's shim made of every chunk under
every candidate.  A case: name, options mask, bits per pixel, the four candidates' pixels per scan line (0: not asked) and
the chunks."""
import json
import os

import numpy as np

import helpers
import sz_chunks_cases
from sz_chunks_cases import unit_of
from sz_device_cases import MSB, NN, RAW
from test_sz_layout import np_marshal, py_layout

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sz_estimate.json")

# shorter than every block; around one piece; lines of two pieces with a short last one; three pieces; three segments of
# blocks of 8 (138 blocks); 4096 blocks of 8, the limit
LINES = [5, 63, 64, 65, 100, 130, 1100, 32768]
PIXELS = [(8, 0), (12, 0), (16, MSB), (24, 0), (32, 0), (64, MSB)]


def pack(values, bpp, opts):
    """pixel values (uint64) -> the bytes of a chunk"""
    unit = unit_of(bpp)
    v = np.asarray(values, dtype=np.uint64)
    out = np.empty((v.size, unit), dtype=np.uint8)
    for b in range(unit):
        shift = 8 * (unit - 1 - b) if opts & MSB else 8 * b
        out[:, b] = (v >> np.uint64(shift)) & np.uint64(0xFF)
    return out.reshape(-1)


def pixels(rng, kind, count, bpp, opts):
    """constant: zero blocks in runs, across segment borders and into the padding (zero without NN, whose fill is zero and
    whose samples go out as they are); walk: one step in 16 pixels; noise: the uncompressed option"""
    top = np.uint64((1 << bpp) - 1)
    if kind == "constant":
        v = np.full(count, (0x5A5A5A5A5A5A5A5A & int(top)) if opts & NN else 0, dtype=np.uint64)
    elif kind == "walk":
        v = sz_chunks_cases.steps(rng, count, min(bpp, 40)).astype(np.uint64) & top
    else:
        v = ((rng.integers(0, 1 << 62, size=count, dtype=np.uint64) << np.uint64(2)) ^
             rng.integers(0, 4, size=count, dtype=np.uint64)) & top
    return pack(v, bpp, opts)


def recipe(rng, bpp, opts, pps, flip):
    """one pixel; a partial last line (with planes, lines that straddle them); a trailing fraction of a pixel; an odd
    pixel count; whole lines (eligible for a fast path where the scan line allows one)"""
    unit = unit_of(bpp)
    chunks = [pixels(rng, "noise", 1, bpp, opts),
              pixels(rng, "constant", pps + pps // 2 + 1, bpp, opts),
              pixels(rng, "walk", pps + 3, bpp, opts),
              pixels(rng, "noise" if flip else "walk", 2 * pps + 1, bpp, opts),
              pixels(rng, "walk" if flip else "constant", 2 * pps, bpp, opts)]
    if unit > 1:
        chunks[2] = np.concatenate([chunks[2], np.full(unit - 1, 0xC3, dtype=np.uint8)])
    return chunks


def cases():
    out = []
    k = 0
    for pps in LINES:
        for bpp, order in PIXELS:
            for nn in (NN, 0):
                opts = nn | order | RAW
                rng = np.random.default_rng(100000 * pps + 100 * bpp + nn)
                out.append((f"{pps}-{bpp}bpp-{'nn' if nn else 'zero'}", opts, bpp, [pps] * 4, recipe(rng, bpp, opts, pps, k & 1)))
                k += 1
    # a scan line per candidate: two passes, one size left out
    rng = np.random.default_rng(17)
    out.append(("per-candidate-16bpp", NN | RAW, 16, [100, 100, 128, 0], recipe(rng, 16, NN | RAW, 100, 1)))
    out.append(("per-candidate-32bpp", NN | RAW, 32, [0, 60, 64, 24], recipe(rng, 32, NN | RAW, 64, 0)))
    # the unequal batches of the chunk calls
    for name, prm, sizes, chunks in sz_chunks_cases.batches():
        if name.startswith("beyond"):
            continue
        opts, bpp, _, pps = prm
        out.append((name, opts, bpp, [pps] * 4, [np.ascontiguousarray(c).view(np.uint8).reshape(-1) for c in chunks]))
    return out


_CASES = None


def all_cases():
    """the cases, made once and shared (nobody writes to the chunks)"""
    global _CASES
    if _CASES is None:
        _CASES = cases()
        for c in _CASES:
            for chunk in c[4]:
                chunk.setflags(write=False)
    return _CASES


def asked(pps):
    return [i for i in range(4) if pps[i]]


def oracle_bits(opts, bpp, pps, chunk):
    """per size asked: the oracle's total_bits of the padded coder input that py_layout + NumPy padding build"""
    bits = [None] * 4
    for i in asked(pps):
        L = py_layout(opts, bpp, 8 << i, pps[i], chunk.size)
        rc, _, _, _, total = helpers.oracle_encode(np_marshal(chunk, opts, bpp, 8 << i, pps[i]), L["bps"], L["bs"], L["rsi"], L["flags"])
        assert rc == helpers.AEC_OK
        bits[i] = total
    return bits


def golden():
    """{case name: per chunk, per size: the length of the reference shim's stream, or None}"""
    with open(GOLDEN) as f:
        return json.load(f)


def place(chunks, how, skew=0):
    """the chunks in one buffer -> (buffer, offsets, order).  aligned: every chunk at a 16-byte boundary, in order;
    shuffled: odd gaps, so that most chunks lie off a boundary, and the chunks in reverse order in the buffer."""
    n = len(chunks)
    order = list(range(n)) if how == "aligned" else list(range(n - 1, -1, -1))
    offs, at = [0] * n, skew
    for k, c in enumerate(order):
        offs[c] = at
        at += chunks[c].size
        at = (at + 15) // 16 * 16 if how == "aligned" else at + 3 + 13 * (k % 3)
    buf = np.full(at + 16, 0x3C, dtype=np.uint8)
    for o, c in zip(offs, chunks):
        buf[o:o + c.size] = c
    return buf, np.array(offs, dtype=np.uint64), np.array([c.size for c in chunks], dtype=np.uint64)
