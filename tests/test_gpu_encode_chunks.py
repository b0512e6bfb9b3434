"""aec_gpu_encode_chunks_async (include/aec_gpu.h): a batch of unequal chunks as one launch set.  Every chunk's stream must
be, byte for byte, the oracle's stream of that chunk alone; the streams lie back to back in chunk order, an empty chunk is
one zero byte.  The chunks sit at shuffled 16-byte aligned offsets of the input with 0xA5 between them, and the output is
0xFF before the call: the call clears what it has to clear itself, and behind the last stream nothing is touched but the
zero padding of its last word and of the word after it.

Run as a program (`python tests/test_gpu_encode_chunks.py abi`) the file is the child process of the ABI test: it codes
batches through aec_buffer_encode_batch and SZ_BatchCompress, compares them with the oracle and with
SZ_BufftoBuffCompress, and leaves the AEC_ABI_TRACE lines on stderr for the parent to read."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import helpers  # noqa: E402
from helpers import (AEC_DATA_3BYTE, AEC_DATA_MSB, AEC_DATA_PREPROCESS as PP, AEC_DATA_SIGNED, AEC_NOT_ENFORCE, AEC_OK,  # noqa: E402
                     oracle_encode)

pytestmark = pytest.mark.gpu

C5 = (8, 8, 128, PP)
PARAM_SETS = [
    C5,
    (16, 16, 64, PP),
    (16, 16, 128, 0),
    (32, 32, 100, PP | AEC_DATA_MSB | AEC_DATA_SIGNED),      # an rsi that is no multiple of 64
    (24, 64, 17, PP | AEC_DATA_3BYTE),
    (12, 24, 5, PP | AEC_NOT_ENFORCE),                       # the generic block size
    (16, 8, 1, PP),                                          # rsi 1
]
GUARD = 256


def make_chunk(rng, kind, samples, prm, extra_bytes=0):
    """`samples` samples of a kind, as bytes, with `extra_bytes` of a further sample behind them"""
    bps, bs, rsi, flags = prm
    nb = helpers.bytes_per_sample(bps, flags)
    lo, hi = (-(1 << (bps - 1)), (1 << (bps - 1)) - 1) if flags & AEC_DATA_SIGNED else (0, (1 << bps) - 1)
    if samples == 0:
        return rng.integers(0, 256, size=extra_bytes, dtype=np.uint8)
    if kind == "walk":
        vals = helpers.random_walk_samples(rng, samples, bps, flags)
    elif kind == "const":
        vals = np.full(samples, int(rng.integers(lo, hi + 1)), dtype=np.int64)
    elif kind == "zero":
        vals = np.zeros(samples, dtype=np.int64)
    else:
        vals = rng.integers(lo, hi + 1, size=samples, dtype=np.int64)
    raw = np.frombuffer(helpers.pack_samples(vals, bps, flags), dtype=np.uint8)
    assert raw.size == samples * nb
    return np.concatenate([raw, rng.integers(0, 256, size=extra_bytes, dtype=np.uint8)]) if extra_bytes else raw.copy()


_big = []


def big_data():
    """8-bit samples for the large batches of config 5: made once, shared, never written"""
    if not _big:
        from test_gpu_parity import gen
        a = gen(2, 33 << 20)
        a.setflags(write=False)
        _big.append(a)
    return _big[0]


def awkward_batch(rng, prm):
    bps, bs, rsi, flags = prm
    nb = helpers.bytes_per_sample(bps, flags)
    S = bs * rsi
    frac = nb - 1                                            # (8-bit samples have no fractions: an empty chunk then)
    spec = [("walk", 0, 0), ("walk", 1, 0), ("walk", 0, frac), ("walk", bs - 1, 0), ("walk", 64 * bs, 0), ("walk", 65 * bs, 0),
            ("walk", S, 0), ("walk", S + 1, frac)]
    spec += [("const", 3 * bs, 0)] * 5 + [("const", 1, 0)] * 3   # streams of a few bytes: several chunks in one 32-bit word
    spec += [("zero", 2 * S + 3, 0)]
    spec += [("walk", 0, 0)] * 10                            # ten empty chunks: words no neighbour's rule covers
    spec += [("noise", S + 3 * bs, 0), ("walk", 3 * S + 7, 0), ("const", 2, 0), ("walk", 0, frac), ("walk", 129 * bs + 5, 0)]
    return [make_chunk(rng, kind, n, prm, extra) for kind, n, extra in spec]


def expected(chunk, prm):
    """(stream, bits, RSI offsets) of a chunk alone; an empty chunk: one zero byte"""
    nb = helpers.bytes_per_sample(prm[0], prm[3])
    if chunk.size < nb:
        return b"\0", 0, []
    rc, enc, _, offs, bits = oracle_encode(chunk, *prm)
    assert rc == AEC_OK and len(enc) == (bits + 7) // 8
    return enc, int(bits), [int(o) for o in offs]


def run_batch(prm, chunks, rng, want=None, decode=True, out_cap=None, codec=None):
    """codes the chunks as one batch and checks everything the call promises; returns (codec, expected streams)"""
    import torch
    from libaec_amd import gpu
    bps, bs, rsi, flags = prm
    nb = helpers.bytes_per_sample(bps, flags)
    n = len(chunks)
    want = want or [expected(c, prm) for c in chunks]
    # the chunks in shuffled order at 16-byte aligned offsets, gaps of 0 to 48 bytes, 0xA5 wherever no chunk is
    order = rng.permutation(n)
    offsets, at = np.zeros(n, dtype=np.uint64), 16 * int(rng.integers(0, 3))
    for i in order:
        offsets[i] = at
        at += (chunks[i].size + 15) // 16 * 16 + 16 * int(rng.integers(0, 4))
    host = np.full(at + 16, 0xA5, dtype=np.uint8)
    for i in range(n):
        host[int(offsets[i]):int(offsets[i]) + chunks[i].size] = chunks[i]
    sizes = np.array([c.size for c in chunks], dtype=np.uint64)
    d_in = torch.from_numpy(host).cuda()
    codec = codec or gpu.Codec(*prm)
    plan = codec.encode_chunks_plan(sizes)
    need = sum(len(w[0]) for w in want)
    cap = plan["out_bound"] if out_cap is None else out_cap
    assert need <= plan["out_bound"]
    d_buf = torch.full((cap + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    d_out, rec, d_tab, res = codec.encode_chunks(d_in, offsets, sizes, want_offsets=True, out_cap=cap, d_out=d_buf)
    out = d_buf.cpu().numpy()
    tab = d_tab.cpu().numpy()
    assert int(res["total_bits"]) == need * 8, (int(res["total_bits"]), need * 8)
    assert int(res["overflow"]) == (1 if need > cap else 0)
    assert np.all(out[cap:] == 0xFF), "bytes at or beyond out_cap were written"
    at, entry = 0, 0
    for i in range(n):
        enc, bits, offs = want[i]
        assert int(rec[i][0]) == at * 8 and int(rec[i][1]) == bits, (i, rec[i], at * 8, bits)
        if at + len(enc) <= cap:                                       # (a stream that fits is intact)
            got = out[at:at + len(enc)].tobytes()
            assert got == enc, f"chunk {i} of {n} ({chunks[i].size} bytes): stream differs from the oracle's"
        assert tab[entry:entry + len(offs) + 1].tolist() == [at * 8 + o for o in offs] + [at * 8 + bits], f"RSI table, chunk {i}"
        if decode and offs and need <= cap:
            blocks = (chunks[i].size // nb + bs - 1) // bs
            d_dec, status = codec.decode(d_buf, need, d_tab[entry:], len(offs), blocks)
            whole = chunks[i].size - chunks[i].size % nb
            assert status == 0 and d_dec[:whole].cpu().numpy().tobytes() == chunks[i][:whole].tobytes(), f"round trip, chunk {i}"
        at += len(enc)
        entry += len(offs) + 1
    assert entry == plan["rsi_entries"]
    if need <= cap:
        # behind the last stream: its zero padding up to the end of the next 32-bit word at the most, then nothing
        pad_end = min((need // 4 + 2) * 4, cap)
        assert np.all((out[need:pad_end] == 0) | (out[need:pad_end] == 0xFF)) and np.all(out[pad_end:cap] == 0xFF), \
            "bytes behind the last stream were written"
    return codec, want


@pytest.mark.parametrize("prm", PARAM_SETS, ids=lambda p: "-".join(str(x) for x in p))
def test_one_batch_of_every_awkward_chunk_size(prm):
    rng = np.random.default_rng(sum(prm))
    chunks = awkward_batch(rng, prm)
    codec, want = run_batch(prm, chunks, rng)
    # the same context again, the batch reversed: descriptors and tables of the call before are gone
    run_batch(prm, chunks[::-1], rng, want=want[::-1], decode=False, codec=codec)
    codec.close()


def test_chunks_of_2049_and_4100_segments_next_to_small_ones():
    rng = np.random.default_rng(5)
    seg = 64 * 8
    sizes = [700, 2049 * seg, 0, 3, 4100 * seg - 5, 1000, 2048 * seg, 12]
    chunks, at = [], 0
    for size in sizes:
        chunks.append(big_data()[at:at + size])
        at += size
    codec, _ = run_batch(C5, chunks, rng)
    codec.close()


@pytest.mark.parametrize("thresh,spw", [(16384, 2), (32768, 4), (65536, 8)])
def test_every_number_of_segments_a_wave_walks(thresh, spw):
    """config 5 hands a wave 2 / 4 / 8 segments from 16384 / 32768 / 65536 segments in the batch on (8 / 16 / 32 MiB);
    the chunks' segment counts are no multiples of any of them"""
    from libaec_amd import gpu
    rng = np.random.default_rng(thresh)
    segs, total = [], 0
    for k in [4101, 2051, 1027, 515, 259, 131, 7, 3, 1] * 40:
        if total >= thresh:
            break
        segs.append(k)
        total += k
    assert total >= thresh and gpu.encode_chunks_plan(*C5, [k * 512 for k in segs])["waves"] == sum(-(-k // spw) for k in segs)
    chunks, at = [], 0
    for k in segs:                                       # (every chunk its own piece of the data)
        size = k * 512 - int(rng.integers(0, 8))
        chunks.append(big_data()[at:at + size])
        at += size
    codec, _ = run_batch(C5, chunks, rng, decode=False)
    codec.close()


def test_out_cap_one_word_short():
    """the capacity is a multiple of 16, so the batch is made to need 16 k + 4 bytes: a last chunk of noise is chosen for
    its stream's length"""
    rng = np.random.default_rng(11)
    chunks = awkward_batch(rng, C5)
    want = [expected(c, C5) for c in chunks]
    need = sum(len(w[0]) for w in want)
    for blocks in range(4, 80):
        last = make_chunk(rng, "noise", blocks * 8, C5)
        w = expected(last, C5)
        if (need + len(w[0])) % 16 == 4:
            break
    else:
        raise AssertionError("no last chunk found")
    chunks.append(last)
    want.append(w)
    need += len(w[0])
    assert len(w[0]) > 4
    codec, _ = run_batch(C5, chunks, rng, want=want, out_cap=need - 4)
    run_batch(C5, chunks, rng, want=want, out_cap=need + 12, codec=codec)          # ... and just enough: no overflow
    codec.close()


def test_refusals_and_the_empty_batch():
    import ctypes as C
    import torch
    from libaec_amd import gpu
    codec = gpu.Codec(*C5)
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(8, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    off, siz = np.array([0, 1000], dtype=np.uint64), np.array([100, 100], dtype=np.uint64)

    def call(p, offsets, n, cap=4096):
        return codec.lib.aec_gpu_encode_chunks_async(codec.ctx, C.byref(p), C.c_void_p(d.data_ptr()), C.c_void_p(offsets.ctypes.data),
                                                     C.c_void_p(siz.ctypes.data), n, C.c_void_p(d.data_ptr()), cap,
                                                     C.c_void_p(d_rec.data_ptr()), None, C.c_void_p(d_res.data_ptr()), codec._stream(None))
    assert call(codec.p, off, 0) == 0
    assert call(gpu.Params(8, 10, 128, PP), off, 0) == helpers.AEC_CONF_ERROR
    assert call(gpu.Params(8, 10, 128, PP), off, 2) == helpers.AEC_CONF_ERROR
    assert call(codec.p, off, 2) == helpers.AEC_CONF_ERROR            # an offset that is no multiple of 16
    assert call(codec.p, np.array([0, 1008], dtype=np.uint64), 2, cap=4090) == helpers.AEC_CONF_ERROR
    assert call(codec.p, np.array([0, 1008], dtype=np.uint64), 2) == 0
    torch.cuda.synchronize()
    codec.close()


def test_through_the_abi_the_batches_take_the_chunks_path():
    env = dict(os.environ, AEC_ABI_TRACE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "abi"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    paths = [line.rsplit("path ", 1)[1].strip() for line in r.stderr.splitlines() if "encode batch:" in line]
    assert paths and all(p == "chunks" for p in paths), paths
    assert r.stdout.count("same as the") == 3, r.stdout


def abi_child():
    import torch
    assert torch.cuda.is_available()
    from fuzz_batch_gpu import batch
    from sz_device_cases import NN, RAW
    from libaec_amd import api, szip
    lib = api.library()
    rng = np.random.default_rng(3)
    for name, prm, sizes in (("9 x 100000 bytes of 16-bit samples", (16, 16, 64, PP), [100000] * 9),
                             ("3 x 1.5 MiB of config 5", C5, [3 << 19] * 3)):
        nb = helpers.bytes_per_sample(prm[0], prm[3])
        chunks = [make_chunk(rng, "walk", s // nb, prm) for s in sizes]
        want = [expected(c, prm)[0] for c in chunks]
        rc, got, st = batch(lib, "aec_buffer_encode_batch", prm, chunks, [len(w) + 64 for w in want])
        assert rc == AEC_OK and st == [AEC_OK] * len(chunks), (name, rc, st)
        for i, w in enumerate(want):
            assert got[i].tobytes() == w, (name, i)
        print(name + ": same as the oracle's streams")
    # the geometry of test_gpu_sz_device.py's chunk beyond the uniform batch: 8 / 8 / 1000, 2000 lines, 4000 segments
    opts, bpp, ppb, pps, size = NN | RAW, 8, 8, 1000, 2000 * 1000
    chunks = [(128 + np.cumsum(rng.integers(-2, 3, size=size)) % 64).astype(np.uint8) for _ in range(2)]
    rc, got, st = szip.compress_batch(chunks, [size * 2 + 4096] * 2, opts, bpp, ppb, pps)
    assert rc == szip.SZ_OK and st == [szip.SZ_OK] * 2, (rc, st)
    for i, c in enumerate(chunks):
        rc1, one = szip.compress(c, size * 2 + 4096, opts, bpp, ppb, pps)
        assert rc1 == szip.SZ_OK and got[i] == one, i
    print("SZ_BatchCompress of two chunks of 4000 segments: same as the single calls")
    return 0


if __name__ == "__main__":
    sys.exit(abi_child() if sys.argv[1:] == ["abi"] else 2)
