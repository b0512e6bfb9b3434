"""aec_buffer_decode_batch / aec_buffer_encode_batch at the edges of their staged transfers (libaec_amd/csrc/aec_abi.cpp:
stage_up, stage_down): the smallest batches on either side of every condition under which a batch goes through the
pinned staging buffer, in pieces, in two halves, or chunk by chunk.  Config 5 (8-bit, blocks of 8, RSIs of 128 blocks,
preprocessor) unless a shape needs samples of two bytes.  What is expected comes from the oracle -- its stream of every
chunk, byte for byte, and the samples that went in -- never from the product's own single-chunk calls.

A call of 8 chunks and more than 8 MiB is split into parts of n / parts chunks each, every part a batch of its own
(run_parts): the 9 chunks of 1 MiB are one batch of 4 and one of 5."""
import numpy as np
import pytest

from helpers import AEC_DATA_PREPROCESS as PP, AEC_OK, AEC_STREAM_ERROR, oracle_encode

pytestmark = pytest.mark.gpu

MIB, KIB = 1 << 20, 1 << 10
C5 = (8, 8, 128, PP)
C16 = (16, 16, 64, PP)

# name, parameters, chunk sizes in bytes
SHAPES = {
    # decode: a slot of 1 MiB, pieces of 4 slots through the two halves of the staging buffer, the last piece short
    "9x1MiB": (C5, [MIB] * 9),
    # decode: a slot above the piece size -- a chunk per piece, four pieces
    "4x5MiB": (C5, [5 * MIB] * 4),
    # fewer than 4 chunks: no staging in either direction
    "3x256KiB": (C5, [256 * KIB] * 3),
    # unequal chunks of 16-bit samples, one of them empty
    "6-unequal": (C16, [300000, 0, 70002, 2048, 1 << 19, 99998]),
    # encode, unequal chunks of at most 256 KiB: staged both ways from 16 chunks on
    "17-unequal": (C5, [256 * KIB, 1000, 77777, 8, 131072, 200001, 1024, 1023, 1025, 50000, 256 * KIB, 3, 90000, 65536, 12345,
                        256 * KIB - 1, 180000]),
    "15-unequal": (C5, [256 * KIB, 1000, 77777, 8, 131072, 200001, 1024, 1023, 1025, 50000, 256 * KIB, 3, 90000, 65536, 12345]),
}

# name, shape, decode (else encode), chunk with a short output buffer (or None) and by how many bytes
CASES = [
    ("decode-9x1MiB", "9x1MiB", True, None, 0),
    ("decode-4x5MiB", "4x5MiB", True, None, 0),
    ("decode-3-unstaged", "3x256KiB", True, None, 0),
    ("decode-6-unequal-one-empty-one-short", "6-unequal", True, 4, 1025),
    ("encode-9x1MiB-uniform", "9x1MiB", False, None, 0),
    ("encode-17-unequal-staged", "17-unequal", False, None, 0),
    ("encode-15-unequal-unstaged", "15-unequal", False, None, 0),
    ("encode-17-one-output-a-byte-short", "17-unequal", False, 5, 1),
    ("encode-9x1MiB-one-output-a-byte-short", "9x1MiB", False, 7, 1),
]

_made = {}


def shape(name):
    """the chunks of a shape and the oracle's stream of each: made once, shared by the cases, never written"""
    if name not in _made:
        from test_gpu_parity import gen
        (bps, bs, rsi, flags), sizes = SHAPES[name]
        data = gen(2 if bps == 8 else 0, sum(sizes) + 64)
        chunks, at = [], 0
        for s in sizes:                                  # (every chunk its own piece of the data: a chunk in the wrong place shows)
            chunks.append(np.ascontiguousarray(data[at:at + s]))
            at += s
        streams = []
        for c in chunks:
            rc, enc = (AEC_OK, b"") if not c.size else oracle_encode(c, bps, bs, rsi, flags)[:2]     # (no input: no stream)
            assert rc == AEC_OK
            streams.append(np.frombuffer(enc, dtype=np.uint8).copy())
        for a in chunks + streams:
            a.setflags(write=False)
        _made[name] = (chunks, streams)
    return _made[name]


@pytest.mark.parametrize("name,shape_name,decode,short,by", CASES, ids=[c[0] for c in CASES])
def test_batches_at_the_edges_of_the_staged_transfers(name, shape_name, decode, short, by):
    import torch
    assert torch.cuda.is_available()
    from fuzz_batch_gpu import batch
    from libaec_amd import api
    lib = api.library()
    params, sizes = SHAPES[shape_name]
    chunks, streams = shape(shape_name)
    n, nb = len(sizes), 1 if params[0] <= 8 else 2
    if decode:
        caps = list(sizes)
        if short is not None:
            caps[short] -= by                            # an odd number of bytes: the last sample has no room
        rc, got, st = batch(lib, "aec_buffer_decode_batch", params, streams, caps)
        assert rc == AEC_OK and st == [AEC_OK] * n, (rc, st)
        for i in range(n):
            want = chunks[i][:caps[i] - caps[i] % nb]    # (a whole number of samples)
            assert got[i].size == want.size and np.array_equal(got[i], want), f"chunk {i} of {n}: {got[i].size} bytes"
    else:
        caps = [s.size + 64 for s in streams]
        if short is not None:
            caps[short] = streams[short].size - by
        rc, got, st = batch(lib, "aec_buffer_encode_batch", params, chunks, caps)
        want_st = [AEC_STREAM_ERROR if i == short else AEC_OK for i in range(n)]
        assert st == want_st and rc == (AEC_OK if short is None else AEC_STREAM_ERROR), (rc, st)
        for i in range(n):
            want = streams[i][:caps[i]]                  # (too small a buffer: the prefix that fits)
            assert got[i].size == want.size and np.array_equal(got[i], want), f"chunk {i} of {n}: {got[i].size} bytes"
