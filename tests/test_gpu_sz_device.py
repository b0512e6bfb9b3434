"""SZIP chunks that stay on the device (include/aec_gpu_sz.h, libaec_amd/szgpu.py): byte planes, scan-line padding and
the batch coder in one enqueue, against vectors the reference's shim produced (tests/golden/sz_vectors.npz), against the
host path (szip.compress per chunk, which tests/test_gpu_szip.py pins to the reference) and, when oracle/_ref travelled,
against the reference shim itself."""
import ctypes as C

import numpy as np
import pytest

from helpers import REF_SO, have_ref
from sz_device_cases import MSB, NN, RAW, chunk_data, sweep_cases
from test_sz_layout import SYNTHETIC, golden, np_marshal, synthetic_chunks

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import gpu, szgpu, szip
    szip.library()
    return torch, gpu, szgpu, szip


def host_streams(szip, chunks, opts, bpp, ppb, pps):
    out = []
    ref = szip.bind(C.CDLL(REF_SO)) if have_ref() else None
    for c in chunks:
        rc, enc = szip.compress(c, c.size * 2 + 4096, opts, bpp, ppb, pps)
        assert rc == szip.SZ_OK
        if ref is not None:
            assert szip.compress(c, c.size * 2 + 4096, opts, bpp, ppb, pps, lib=ref) == (rc, enc)
        out.append(enc)
    return out


def guarded(torch, nbytes, skew=0):
    """(whole tensor, the nbytes in its middle): 64 bytes of a fixed pattern on either side; skew moves the middle off
    its 16-byte boundary"""
    whole = torch.empty(GUARD + skew + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    whole[:] = torch.arange(whole.numel(), device="cuda") % 251
    return whole, whole[GUARD + skew:GUARD + skew + nbytes]


def guards_intact(torch, whole, nbytes, skew=0):
    want = (torch.arange(whole.numel(), device="cuda") % 251).to(torch.uint8)
    lo = GUARD + skew
    return torch.equal(whole[:lo], want[:lo]) and torch.equal(whole[lo + nbytes:], want[lo + nbytes:])


def repack(torch, streams):
    """the streams at 16-byte aligned offsets of one device buffer (the repacking itself done on the device)"""
    offs = [0]
    for s in streams:
        offs.append(offs[-1] + (len(s) + 15) // 16 * 16)
    d_in = torch.zeros(offs[-1] + 16, dtype=torch.uint8, device="cuda")
    for s, o in zip(streams, offs):
        d_in[o:o + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    return d_in, torch.tensor(offs, dtype=torch.int64, device="cuda")


def round_trip(mods, chunks, opts, bpp, ppb, pps, skew=0):
    """compress on the device (one call, or marshal + chunk-wise encode where the batch is not for one call), compare with
    the host path, decompress on the device into guarded buffers"""
    torch, gpu, szgpu, szip = mods
    n, size = chunks.shape
    codec = szgpu.SzCodec(opts, bpp, ppb, pps)
    L = codec.layout(size)
    want = host_streams(szip, chunks, opts, bpp, ppb, pps)
    # chunk bases at size * i from a base that is `skew` off a 16-byte boundary
    src_whole, d_src = guarded(torch, n * size, skew)
    d_src.copy_(torch.from_numpy(np.ascontiguousarray(chunks).reshape(-1)).cuda())
    work_whole, d_work = guarded(torch, n * L.coder_bytes)
    if codec.batch_ok(size, n):
        cap = codec.encode_bound(size) * n
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
        d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
        assert codec.compress_batch_async(d_src, size, n, None if L.passthrough else d_work, d_out, d_rec, d_res) == 0
        rec = d_rec.cpu().numpy().reshape(n, 2)
        assert d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["overflow"] == 0
        out = d_out.cpu().numpy()
        got = [out[int(b) // 8:int(b) // 8 + (int(bits) + 7) // 8].tobytes() for b, bits in rec]
    else:
        slot = codec.encode_bound(size)
        d_out = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
        assert codec.marshal_async(d_src, size, n, d_work) == 0
        assert codec.encode_chunks_async(d_work, L.coder_bytes, n, d_out, slot, d_res) == 0
        res = d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)
        out = d_out.cpu().numpy()
        got = [out[i * slot:i * slot + (int(res[i]["total_bits"]) + 7) // 8].tobytes() for i in range(n)]
    assert guards_intact(torch, work_whole, n * L.coder_bytes)
    if not L.passthrough:
        want_in = np.stack([np_marshal(c, opts, bpp, ppb, pps) for c in chunks]).reshape(-1)
        assert np.array_equal(d_work.cpu().numpy(), want_in), "coder input differs from sz_abi.cpp's"
    for i in range(n):
        assert got[i] == want[i], f"stream {i} of {n}: {len(got[i])} vs {len(want[i])} bytes"
    # and back
    d_in, d_offs = repack(torch, want)
    work_whole, d_work = guarded(torch, n * L.coder_bytes)
    dst_whole, d_dst = guarded(torch, n * size, skew)
    d_rsi = torch.zeros(n * L.lines, dtype=torch.int64, device="cuda")
    d_results = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
    assert codec.decompress_batch_async(d_in, d_in.numel(), d_offs, n, size, d_rsi, d_work, d_dst, d_results, d_result) == 0
    res = d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)
    assert np.all(res["status"] == 0) and np.all(res["n_rsi"] == L.lines), res
    back = d_dst.cpu().numpy().reshape(n, size)
    assert np.array_equal(back[:, :L.coded_bytes], chunks[:, :L.coded_bytes])
    assert not back[:, L.coded_bytes:].any()
    assert guards_intact(torch, work_whole, n * L.coder_bytes) and guards_intact(torch, dst_whole, n * size, skew)
    assert guards_intact(torch, src_whole, n * size, skew)
    codec.close()
    return L


def test_golden_vectors_as_batches_of_one(mods):
    torch, gpu, szgpu, szip = mods
    for name, opts, bpp, ppb, pps, data, comp in golden():
        codec = szgpu.SzCodec(opts, bpp, ppb, pps)
        assert codec.batch_ok(data.size, 1), name
        d_src = torch.from_numpy(data.copy()).cuda()
        assert codec.compress_batch(d_src, data.size, 1) == [comp], name
        padded = comp + bytes(-len(comp) % 16)
        d_in = torch.frombuffer(bytearray(padded), dtype=torch.uint8).cuda()
        d_offs = torch.tensor([0, len(padded)], dtype=torch.int64, device="cuda")
        d_dst, res, overall = codec.decompress_batch(d_in, d_offs, 1, data.size)
        assert res[0]["status"] == 0 and overall["status"] == 0, name
        assert d_dst.cpu().numpy().tobytes() == data.tobytes(), name
        codec.close()


@pytest.mark.parametrize("case", SYNTHETIC, ids=lambda c: f"{c[1]}bpp-{c[2]}-{c[3]}-{c[4]}B")
def test_synthetic_shapes_as_batches_of_five(mods, case):
    opts, bpp, ppb, pps, size = case
    round_trip(mods, synthetic_chunks(case, 5, seed=3), opts, bpp, ppb, pps)


def smooth(n, size, seed):
    rng = np.random.default_rng(seed)
    return (128 + np.cumsum(rng.integers(-2, 3, size=n * size)) % 64).astype(np.uint8).reshape(n, size)


def test_unaligned_chunk_bases(mods):
    """7 chunks of 1001 bytes, 8 / 8 / 1000 NN: no chunk but the first starts on a 16-byte boundary, and the batch itself
    starts 3 bytes off one"""
    L = round_trip(mods, smooth(7, 1001, 1), NN | RAW, 8, 8, 1000, skew=3)
    assert (L.lines, L.padded_line, L.passthrough) == (2, 1000, 0)


def test_passthrough_chunks(mods):
    """6 chunks of 64 KiB, 8 / 8 / 1024 NN: the chunk as it lies is the coder's input; aligned and not"""
    for skew in (0, 8):
        L = round_trip(mods, smooth(6, 65536, 2), NN | RAW, 8, 8, 1024, skew=skew)
        assert L.passthrough == 1


def test_float32_like_chunks_take_the_register_path(mods):
    """4 chunks of 256 KiB of float32-like data, 32 / 16 / 1024: planes split and merged in registers"""
    rng = np.random.default_rng(3)
    x = np.cumsum(rng.standard_normal(4 * 65536)).astype("<f4")
    L = round_trip(mods, x.view(np.uint8).reshape(4, -1), NN | RAW, 32, 16, 1024)
    assert (L.word, L.lines, L.coder_bytes) == (4, 256, 262144)


def test_a_damaged_stream_spoils_its_own_chunk_only(mods):
    torch, gpu, szgpu, szip = mods
    opts, bpp, ppb, pps, size = NN | RAW, 16, 16, 1000, 6000
    rng = np.random.default_rng(4)
    chunks = (1000 + np.cumsum(rng.integers(-9, 10, size=8 * size // 2))).astype("<u2").view(np.uint8).reshape(8, size)
    streams = host_streams(szip, chunks, opts, bpp, ppb, pps)
    streams[5] = streams[5][:len(streams[5]) // 2]
    codec = szgpu.SzCodec(opts, bpp, ppb, pps)
    d_in, d_offs = repack(torch, streams)
    d_dst, res, overall = codec.decompress_batch(d_in, d_offs, 8, size)
    L = codec.layout(size)
    assert res[5]["status"] != 0 or res[5]["n_rsi"] < L.lines
    back = d_dst.cpu().numpy().reshape(8, size)
    for i in (0, 1, 2, 3, 4, 6, 7):
        assert res[i]["status"] == 0 and res[i]["n_rsi"] == L.lines and np.array_equal(back[i], chunks[i]), i
    codec.close()


def test_a_chunk_beyond_the_uniform_batch(mods):
    """8 / 8 / 1000 in chunks of 2000 lines: 4000 segments of 64 blocks, about twice what the uniform batch takes per chunk.
    aec_gpu_sz_batch_ok says so, the one-call form refuses, marshal + aec_gpu_encode_batch_async gives the host path's
    stream."""
    torch, gpu, szgpu, szip = mods
    opts, bpp, ppb, pps, size = NN | RAW, 8, 8, 1000, 2000 * 1000
    codec = szgpu.SzCodec(opts, bpp, ppb, pps)
    L = codec.layout(size)
    assert L.lines * ((L.coder.rsi + 63) // 64) > 2048 and codec.batch_ok(size, 2) == 0
    d_src = torch.zeros(2 * size, dtype=torch.uint8, device="cuda")
    d_work = torch.empty(2 * L.coder_bytes, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(2 * codec.encode_bound(size), dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    assert codec.compress_batch_async(d_src, size, 2, d_work, d_out, d_rec, d_res) == szgpu.AEC_CONF_ERROR
    codec.close()
    round_trip(mods, smooth(1, size, 5), opts, bpp, ppb, pps)


def test_random_sweep_against_the_host_path(mods):
    torch, gpu, szgpu, szip = mods
    skipped = 0
    for case in sweep_cases():
        if szgpu.layout(case["opts"], case["bpp"], case["ppb"], case["pps"], case["chunk_bytes"]) is None:
            skipped += 1
            continue
        round_trip(mods, chunk_data(case), case["opts"], case["bpp"], case["ppb"], case["pps"], skew=case["seed"] % 3 * 4)
    assert skipped * 4 <= 30
