"""The unequal batches of tests/test_sz_chunks_layout.py and tests/test_gpu_sz_chunks_device.py, and of the fixture
tests/golden/sz_chunks_vectors.npz (tests/golden/make_golden_sz_chunks.py stores, per batch, these inputs and the streams
the reference's SZ_BufftoBuffCompress made of them)."""
import os

import numpy as np

from sz_device_cases import MSB, NN, RAW
from test_sz_layout import SYNTHETIC, py_layout, synthetic_chunks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sz_chunks_vectors.npz")


def unit_of(bpp):
    """bytes of a pixel as the chunk holds it"""
    return bpp // 8 if bpp in (32, 64) else (4 if bpp > 16 else (2 if bpp > 8 else 1))


def size_list(case):
    """the sizes every synthetic batch holds: one pixel; the set's own size; whole lines of whole quads (with byte planes:
    eligible for the plane path); a trailing fraction of a pixel (where a pixel has more than one byte); shorter than one
    scan line"""
    opts, bpp, ppb, pps, own = case
    u = unit_of(bpp)
    sizes = [u, own, 2 * pps * u]
    if u > 1:
        sizes.append(10 * u + u - 1)
    sizes.append(max(1, pps // 10) * u)
    return sizes


def eligible(case, size):
    """sz_planes_fast of a chunk of this size (its address apart)"""
    opts, bpp, ppb, pps, _ = case
    L = py_layout(opts, bpp, ppb, pps, size)
    return bool(L["word"] and L["coded_bytes"] == size and size % 16 == 0 and (size // L["word"]) % 4 == 0 and
                L["line"] % 4 == 0 and L["padded_line"] % 4 == 0)


def synthetic_batch(case, seed=0):
    opts, bpp, ppb, pps, _ = case
    sizes = size_list(case)
    return sizes, [synthetic_chunks((opts, bpp, ppb, pps, s), 1, seed=seed + 10 * i)[0] for i, s in enumerate(sizes)]


def steps(rng, count, bits, every=16):
    """a walk that moves one step in `every` samples: long runs, short streams"""
    move = rng.integers(-1, 2, size=count) * (rng.integers(0, every, size=count) == 0)
    return ((1 << (bits - 1)) + np.cumsum(move)).astype(np.int64)


def beyond_batch(pps):
    """two chunks of 300 KiB and one of 10 KiB, 8 bpp / 2 pixels per block: with 127 pixels per scan line each large chunk
    is 2419 RSIs of one segment, more than the uniform batch takes; with 128 the chunks are the coder's input as they lie"""
    rng = np.random.default_rng(127)
    sizes = [300 << 10, 10 << 10, 300 << 10]
    return (NN | RAW, 8, 2, pps), sizes, [steps(rng, s, 8).astype(np.uint8) for s in sizes]


def small_batch():
    """300 chunks of 1..2000 pixels, 16 bpp / 16 / 100"""
    rng = np.random.default_rng(300)
    sizes = [2 * int(v) for v in rng.integers(1, 2001, size=300)]
    return (NN | RAW, 16, 16, 100), sizes, [steps(rng, s // 2, 16, 8).astype("<u2").view(np.uint8) for s in sizes]


def mixed_batch(bpp):
    """chunk 0: eligible for the plane path; 1: an odd pixel count; 2: eligible (the tests put it at an unaligned
    offset); 3: eligible, with a partial last line"""
    rng = np.random.default_rng(bpp)
    if bpp == 32:
        prm, pixels = (NN | RAW, 32, 16, 1024), [2048, 1001, 1024, 3000]
        chunks = [np.cumsum(rng.standard_normal(p)).astype("<f4").view(np.uint8) for p in pixels]
    else:
        prm, pixels = (NN | MSB | RAW, 64, 8, 24), [96, 101, 48, 260]
        chunks = [(steps(rng, p, 40, 2) * 1000003).astype(">u8").view(np.uint8) for p in pixels]
    return prm, [c.size for c in chunks], chunks


def batches():
    """(name, (options, bits per pixel, pixels per block, pixels per scan line), sizes, chunks) of every fixture batch"""
    for case in SYNTHETIC:
        sizes, chunks = synthetic_batch(case)
        yield f"synthetic-{case[1]}", case[:4], sizes, chunks
    for pps in (127, 128):
        prm, sizes, chunks = beyond_batch(pps)
        yield f"beyond-{pps}", prm, sizes, chunks
    yield ("small-300",) + small_batch()
    for bpp in (32, 64):
        yield (f"mixed-{bpp}",) + mixed_batch(bpp)


def golden_batches():
    """the fixture: (name, params, sizes, chunks, streams) per batch"""
    z = np.load(GOLDEN)
    c = 0
    for b, name in enumerate(z["names"]):
        n = int(z["n_chunks"][b])
        sizes = [int(v) for v in z["sizes"][c:c + n]]
        lens = [int(v) for v in z["stream_bytes"][c:c + n]]
        i0, o0 = int(z["in_off"][b]), int(z["out_off"][b])
        chunks, streams = [], []
        for s, k in zip(sizes, lens):
            chunks.append(z["inputs"][i0:i0 + s])
            streams.append(z["outputs"][o0:o0 + k].tobytes())
            i0, o0 = i0 + s, o0 + k
        c += n
        yield str(name), tuple(int(v) for v in z["params"][b]), sizes, chunks, streams
