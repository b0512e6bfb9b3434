"""The decoder's launch layer (aec_dec.hip: one host entry for table, segment, bare, batch and window decodes): every
kernel family, block size and container width it dispatches to, through the device seam of libaec_amd/gpu.py.  Every
expected byte and status comes from the oracle decoding the same stream."""
import ctypes as C

import numpy as np
import pytest

from helpers import (AEC_DATA_3BYTE, AEC_DATA_MSB, AEC_DATA_PREPROCESS, AEC_DATA_SIGNED, AEC_NOT_ENFORCE, AEC_OK,
                     oracle_decode, oracle_encode, pack_samples, random_walk_samples)

pytestmark = pytest.mark.gpu

PP, MSB, SGN = AEC_DATA_PREPROCESS, AEC_DATA_MSB, AEC_DATA_SIGNED
DEC_OK, DEC_DATA_ERROR = 0, 2


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import gpu as g
    lib = g._lib()
    vp, u64 = C.c_void_p, C.c_uint64
    lib.aec_gpu_decode_range_async.restype = C.c_int
    lib.aec_gpu_decode_range_async.argtypes = [vp, C.POINTER(g.Params), vp, C.c_size_t, vp, u64, u64, u64, vp, vp, vp]
    lib.aec_gpu_decode_batch_async.restype = C.c_int
    lib.aec_gpu_decode_batch_async.argtypes = [vp, C.POINTER(g.Params), vp, C.c_size_t, vp, u64, u64, vp, vp, vp, vp, vp]
    return g


def walk(seed, nblk, bps, bs, flags):
    rng = np.random.default_rng(seed)
    return pack_samples(random_walk_samples(rng, nblk * bs, bps, flags, scale=3.0, zero_frac=0.1), bps, flags)


def coded(data, bps, bs, rsi, flags):
    """(stream, RSI start bits, decoded bytes) of `data`, all three the oracle's"""
    rc, stream, _, offs, _ = oracle_encode(data, bps, bs, rsi, flags)
    assert rc == AEC_OK
    rc, full, _ = oracle_decode(stream, bps, bs, rsi, flags, data.size)
    assert rc == AEC_OK and len(full) == data.size
    return stream, offs.astype(np.uint64), full


def on_device(stream):
    import torch
    d = torch.zeros(len(stream) + 16, dtype=torch.uint8, device="cuda")
    d[:len(stream)] = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    return d


def record(gpu, d_res, i=0):
    return d_res.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[i]


def table_decode(gpu, shape, nblk, seed, off=0):
    """aec_gpu_decode_async from the oracle's table into a buffer `off` bytes behind a 16-byte boundary"""
    import torch
    bps, bs, rsi, flags = shape
    data = walk(seed, nblk, bps, bs, flags)
    stream, offs, full = coded(data, bps, bs, rsi, flags)
    codec = gpu.Codec(bps, bs, rsi, flags)
    d_off = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_out = torch.zeros(len(full) + 32, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    codec.decode_async(on_device(stream), len(stream), d_off, offs.size, nblk, d_out[off:], d_res)
    res = record(gpu, d_res)
    assert res["status"] == DEC_OK, (shape, res)
    assert d_out[off:off + len(full)].cpu().numpy().tobytes() == full, shape
    codec.close()


# every templated block size and the generic one, every container width, no flag set twice: rsi = 4 stays on the lane
# kernel (the wave kernel wants 16 blocks per RSI), 70 RSIs fill one wavefront and six lanes of a second
LANE = [(8, 8, 4, PP), (16, 16, 4, PP | MSB), (24, 32, 4, PP | AEC_DATA_3BYTE), (32, 64, 4, PP | SGN), (16, 24, 4, AEC_NOT_ENFORCE)]
# the wave kernel, 3 RSIs with a short last one: 1 block, and 65 blocks of 100 (a second round of one block)
WAVE = [(16, 16, 16, PP, 33), (8, 8, 100, PP | MSB, 265), (24, 64, 16, PP | AEC_DATA_3BYTE | MSB, 33), (32, 32, 100, PP | SGN, 265)]


@pytest.mark.parametrize("off", [0, 4], ids=["aligned", "off4"])
@pytest.mark.parametrize("shape", LANE, ids=lambda s: f"{s[0]}b-bs{s[1]}")
def test_lane_kernel(gpu, shape, off):
    """off4: blocks that are not 16-byte aligned take the generic kernel, same bytes"""
    table_decode(gpu, shape, 4 * 70, 11, off)


@pytest.mark.parametrize("off", [0, 4], ids=["aligned", "off4"])
@pytest.mark.parametrize("shape", WAVE, ids=lambda s: f"{s[0]}b-bs{s[1]}-rsi{s[2]}")
def test_wave_kernel(gpu, shape, off):
    table_decode(gpu, shape[:4], shape[4], 12, off)


def test_segment_decode(gpu):
    """rsi = 130: three segments per RSI, the last with 2 blocks; the table is the encoder's"""
    import torch
    bps, bs, rsi, flags = 16, 16, 130, PP
    nblk = 130 * 2 + 67
    data = walk(13, nblk, bps, bs, flags)
    codec = gpu.Codec(bps, bs, rsi, flags)
    nseg = codec.segment_count(data.size)
    assert nseg == 3 + 3 + 2
    d_tab = torch.zeros(nseg * 16, dtype=torch.uint8, device="cuda")
    codec.set_segment_table(d_tab)
    d_enc, nbytes, _, _, _ = codec.encode(torch.from_numpy(data.copy()).cuda())
    codec.set_segment_table(None)
    stream = d_enc[:nbytes].cpu().numpy().tobytes()
    rc, full, _ = oracle_decode(stream, bps, bs, rsi, flags, data.size)
    assert rc == AEC_OK and full == data.tobytes()
    d_out = torch.zeros(data.size + 16, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    codec.decode_segments_async(on_device(stream), nbytes, d_tab, nseg, nblk, d_out, d_res)
    assert record(gpu, d_res)["status"] == DEC_OK
    assert d_out[:data.size].cpu().numpy().tobytes() == full
    codec.close()


def test_bare_decode(gpu):
    """rsi = 512 of 8-sample blocks (eight segments per RSI), 3 RSIs; the middle one sits at the top of the range, where
    the predictor clips: its sums do not hold and it is decoded from the list, a lane for the whole RSI"""
    import torch
    bps, bs, rsi, flags = 8, 8, 512, PP
    rng = np.random.default_rng(14)
    n = bs * rsi
    mid = np.clip(128 + np.cumsum(rng.integers(-2, 3, n)), 64, 192)
    top = np.clip(250 + np.cumsum(rng.integers(-4, 5, n)), 0, 255)
    data = pack_samples(np.concatenate([mid, top, mid[::-1]]), bps, flags)
    stream, offs, full = coded(data, bps, bs, rsi, flags)
    codec = gpu.Codec(bps, bs, rsi, flags)
    spr = codec.segments_per_rsi()
    assert spr == 8
    d_in = on_device(stream)
    d_idx = torch.zeros(3 + 2, dtype=torch.int64, device="cuda")
    d_sb = torch.zeros((3 + 2) * spr, dtype=torch.int64, device="cuda")
    d_ires = torch.zeros(40, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(data.size + 64 * bs, dtype=torch.uint8, device="cuda")
    codec.index_segments_async(d_in, len(stream), 0, d_idx, d_sb, 4, d_ires)
    codec.decode_bare_async(d_in, len(stream), d_idx, d_sb, 4, 3 * rsi, d_ires, d_out, d_res)
    ires, res = record(gpu, d_ires), record(gpu, d_res)
    assert int(ires["n_rsi"]) * rsi + int(ires["tail_blocks"]) == 3 * rsi, ires
    assert np.array_equal(d_idx[:3].cpu().numpy().astype(np.uint64), offs)
    assert res["status"] == DEC_OK, res
    assert d_out[:data.size].cpu().numpy().tobytes() == full
    codec.close()


def _bits(s):
    s += "0" * (-len(s) % 8)
    return bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))


def test_batch_decode(gpu):
    """aec_gpu_decode_batch_async, 5 streams of 4 RSIs; stream 2 holds a second-extension code beyond the table (m > 90
    is a data error, for the oracle as for the decoder): its record says so, the other four stay DEC_OK and whole"""
    import torch
    bps, bs, rsi, flags = 8, 8, 128, PP
    rpc, chunk = 4, 4 * 128 * 8
    datas = [walk(20 + s, rpc * rsi, bps, bs, flags) for s in range(5)]
    cod = [coded(d, bps, bs, rsi, flags) for d in datas]
    streams = [c[0] for c in cod]
    streams[2] = _bits("000" + "1" + "10000000" + "0" * 95 + "1" + "1" * 67) + bytes(64)
    rc_o, _, _ = oracle_decode(streams[2], bps, bs, rsi, flags, chunk)
    assert rc_o != AEC_OK
    choff, blob = [0], b""
    for s in streams:
        blob += s + bytes(-len(s) % 16)
        choff.append(len(blob))
    codec = gpu.Codec(bps, bs, rsi, flags)
    d_choff = torch.tensor(choff, dtype=torch.int64, device="cuda")
    d_off = torch.zeros(5 * rpc, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(5 * chunk + 16, dtype=torch.uint8, device="cuda")
    d_recs = torch.zeros(5 * 40, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    rc = gpu._lib().aec_gpu_decode_batch_async(codec.ctx, C.byref(codec.p), on_device(blob).data_ptr(), len(blob),
                                               d_choff.data_ptr(), 5, rpc, d_off.data_ptr(), d_out.data_ptr(),
                                               d_recs.data_ptr(), d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    out = d_out.cpu().numpy()
    for s in range(5):
        rec = record(gpu, d_recs, s)
        if s == 2:
            assert rec["status"] == DEC_DATA_ERROR, rec
            continue
        assert rec["status"] == DEC_OK and int(rec["n_rsi"]) * rsi + int(rec["tail_blocks"]) == rpc * rsi, (s, rec)
        assert out[s * chunk:(s + 1) * chunk].tobytes() == cod[s][2], s
    assert record(gpu, d_res)["status"] == DEC_DATA_ERROR
    codec.close()


@pytest.mark.parametrize("off", [0, 4], ids=["aligned", "off4"])
@pytest.mark.parametrize("shape", [(16, 16, 4, PP), (16, 16, 16, PP)], ids=["lane", "wave"])
def test_window_decode(gpu, shape, off):
    """aec_gpu_decode_range_async: one byte in the last block of an RSI; a window from the middle of an RSI to the middle
    of a block of the next; whole RSIs in place; and a table whose entry behind RSI 3 is another stream's"""
    import torch
    bps, bs, rsi, flags = shape
    nblk = rsi * 5
    data = walk(15, nblk, bps, bs, flags)
    stream, offs, full = coded(data, bps, bs, rsi, flags)
    other = data.copy()                                   # the same first three RSIs, then incompressible samples
    r3 = 3 * rsi * bs * 2
    other[r3:] = np.random.default_rng(16).integers(0, 256, other.size - r3, dtype=np.uint8)
    offs_other = coded(other, bps, bs, rsi, flags)[1]
    assert np.array_equal(offs_other[:3], offs[:3]) and offs_other[4] != offs[4]
    codec = gpu.Codec(bps, bs, rsi, flags)
    lib = gpu._lib()
    d_in = on_device(stream)
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    blk, R = bs * 2, rsi * bs * 2

    def window(table, pos, size):
        d_off = torch.from_numpy(table.astype(np.int64)).cuda()
        d_out = torch.full((size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = lib.aec_gpu_decode_range_async(codec.ctx, C.byref(codec.p), d_in.data_ptr(), len(stream), d_off.data_ptr(),
                                            table.size, pos, size, d_out.data_ptr() + off, d_res.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        o = d_out.cpu().numpy()
        assert (o[:off] == 0xA5).all() and (o[off + size:] == 0xA5).all(), "write outside the window"
        return record(gpu, d_res), o[off:off + size].tobytes()

    for pos, size in ((2 * R - 3, 1), (R + R // 2 + 5, R // 2 + blk + 7), (R, 2 * R), (0, len(full))):
        res, got = window(offs, pos, size)
        assert res["status"] == DEC_OK and got == full[pos:pos + size], (pos, size, res)
    # RSIs 0 .. 3 of this stream with the other stream's table: RSI 3 does not end where entry 4 says
    res, _ = window(offs_other.copy(), 0, 4 * R)
    assert res["status"] == DEC_DATA_ERROR and res["bad_rsi"] == 3, res
    codec.close()
