"""Batches of bare streams for the tests of the every-bit index scheme over a batch (libaec_amd/csrc/aec_bsmall.h):
tests/test_bsmall_emul.py runs them through the CPU emulation, tests/test_gpu_index_chunks.py through the device --
the same helper with the same seeds, so what the emulation delivers is what the device has to.  Every expected value
comes from the oracle's encoder (helpers.oracle_encode), never from the product."""
import numpy as np

import helpers

PP, MSB, SGN = helpers.AEC_DATA_PREPROCESS, helpers.AEC_DATA_MSB, helpers.AEC_DATA_SIGNED
RESTRICTED, PAD_RSI = helpers.AEC_RESTRICTED, helpers.AEC_PAD_RSI

# the scheme's limits (include/aec_gpu.h)
MIN_BITS, MAX_BITS, MAX_RSI = 64, 1 << 24, 256

# name: (bps, block size, rsi, flags, scale, zero_frac, RSI counts of the streams, blocks of a short last RSI for some)
# The RSI counts put rsis + 1 around the powers of four (3, 4, 5, 15, 16, 17), one RSI beside several hundred, and a
# chunk without a sample (0).
CASES = {
    "8/8/4 PP": (8, 8, 4, PP, 1.0, 0.3, [3, 4, 5, 1, 15, 16, 17, 0, 2, 300, 63, 64, 65, 7], 3),
    "16/16/16 PP|MSB short last": (16, 16, 16, PP | MSB, 60.0, 0.3, [3, 4, 5, 15, 16, 17, 1, 40, 2, 64, 9], 5),
    "16/8/64 PP zero runs": (16, 8, 64, PP, 0.3, 0.7, [3, 4, 5, 1, 15, 16, 17, 30, 2], 17),
    "16/16/128 no PP": (16, 16, 128, 0, 8.0, 0.5, [3, 1, 4, 5, 2, 15, 1], 70),
    "32/16/5 PP|SIGNED": (32, 16, 5, PP | SGN, 400.0, 0.1, [3, 4, 5, 15, 16, 17, 1, 250, 2, 33], 2),
    "4 bits restricted": (4, 8, 8, PP | RESTRICTED, 0.6, 0.3, [3, 4, 5, 15, 16, 17, 1, 300, 2, 21], 3),
    "PAD_RSI": (16, 16, 8, PP | PAD_RSI, 3.0, 0.2, [3, 4, 5, 1, 15, 16, 17, 80, 2], 3),
    "rsi 300": (8, 8, 300, PP, 1.0, 0.3, [1, 2, 3], 100),
}


class Batch:
    """buf: the streams back to back behind `lead` bytes of 0xFF (uint8 array, padded with 0xFF to a multiple of 4 and
    16 more); in_off / in_sizes / out_sizes: uint64 arrays; starts[i]: the oracle's RSI starts of stream i as absolute
    bits of buf; raw[i]: the bytes stream i decodes to; rsis[i] / last_blocks[i]: what chunk i announces."""


def encode_stream(raw, bps, bs, rsi, flags):
    """-> (stream bytes, RSI starts in bits): with AEC_PAD_RSI the RSIs are coded as streams of their own, back to back
    (as tests/test_gpu_offsets.py builds them)"""
    if not flags & PAD_RSI:
        rc, enc, _, offs, _ = helpers.oracle_encode(raw, bps, bs, rsi, flags)
        assert rc == helpers.AEC_OK
        return enc, [int(o) for o in offs] if len(raw) else []
    rb = bs * rsi * helpers.bytes_per_sample(bps, flags)
    parts = []
    for i in range(0, len(raw), rb):
        rc, enc, _, _, _ = helpers.oracle_encode(raw[i:i + rb], bps, bs, rsi, flags & ~PAD_RSI)
        assert rc == helpers.AEC_OK
        parts.append(enc)
    starts = [8 * int(x) for x in np.cumsum([0] + [len(p) for p in parts[:-1]])] if parts else []
    return b"".join(parts), starts


def make_batch(name, seed=0, lead=3, pad_zero_bytes=None):
    """pad_zero_bytes: {stream: k} -- in_sizes of that stream counts k zero bytes behind it (they are in buf)"""
    bps, bs, rsi, flags, scale, zero_frac, counts, short = CASES[name]
    rng = np.random.default_rng(1000 * seed + sum(ord(ch) for ch in name))
    nb = helpers.bytes_per_sample(bps, flags)
    b = Batch()
    b.params = (bps, bs, rsi, flags)
    b.raw, b.starts, b.rsis, b.last_blocks = [], [], [], []
    pieces, in_off, in_sizes, out_sizes = [bytes([0xFF] * lead)], [], [], []
    pos = lead
    for k, r in enumerate(counts):
        # every third stream of more than one RSI ends on a short RSI, with a last block that is not whole
        blocks = r * rsi if (k % 3 or r < 2) else (r - 1) * rsi + short
        n = blocks * bs - (3 if (blocks and k % 3 == 0) else 0)
        vals = helpers.random_walk_samples(rng, n, bps, flags, scale=scale, zero_frac=zero_frac) if n else np.zeros(0, dtype=np.int64)
        raw = helpers.pack_samples(vals, bps, flags).tobytes()
        enc, starts = encode_stream(raw, bps, bs, rsi, flags) if n else (b"\x00" * 9, [])
        extra = (pad_zero_bytes or {}).get(k, 0)
        pieces.append(enc + b"\x00" * extra)
        in_off.append(pos)
        in_sizes.append(len(enc) + extra)
        out_sizes.append(n * nb)
        b.raw.append(raw)
        b.starts.append([8 * pos + s for s in starts])
        b.rsis.append((blocks + rsi - 1) // rsi)
        b.last_blocks.append(blocks - (b.rsis[-1] - 1) * rsi if blocks else 0)
        pos += len(enc) + extra
    body = b"".join(pieces)
    body += b"\xFF" * ((-len(body)) % 4 + 16)
    b.buf = np.frombuffer(body, dtype=np.uint8).copy()
    b.in_bytes = pos
    b.in_off = np.array(in_off, dtype=np.uint64)
    b.in_sizes = np.array(in_sizes, dtype=np.uint64)
    b.out_sizes = np.array(out_sizes, dtype=np.uint64)
    b.n = len(counts)
    return b


def within(b, i, round_bits=1 << 24):
    """is stream i of the batch within the every-bit scheme's limits?"""
    nbits = 8 * int(b.in_sizes[i])
    slot = (nbits + 1 + 1023) // 1024 * 1024
    return MIN_BITS <= nbits <= MAX_BITS and b.params[2] <= MAX_RSI and slot <= round_bits


def expected_record(b, i):
    """(n_rsi, tail_blocks) of a whole stream: all RSIs where the last is full, else the short one as the tail"""
    rsi = b.params[2]
    if b.rsis[i] == 0:
        return 0, 0
    full = b.last_blocks[i] == rsi
    return (b.rsis[i], 0) if full else (b.rsis[i] - 1, b.last_blocks[i])


def table_entry0(b, i):
    """first table entry of chunk i: the sum of rsis_j + 1 in front"""
    return sum(r + 1 for r in b.rsis[:i])
