"""RSI offset tables, aec_buffer_seek and aec_decode_range (libaec 1.1's offsets API) on the MI355X: every expected
value comes from the oracle (oracle_encode's rsi_bit_off, oracle_decode's bytes), never from the product."""
import ctypes as C

import numpy as np
import pytest

from helpers import (AEC_DATA_3BYTE, AEC_DATA_MSB, AEC_DATA_PREPROCESS, AEC_DATA_SIGNED, AEC_FLUSH, AEC_MEM_ERROR,
                     AEC_NO_FLUSH, AEC_NOT_ENFORCE, AEC_OK, AEC_PAD_RSI, AEC_RESTRICTED, AEC_STREAM_ERROR, ROOT,
                     bytes_per_sample, craft_overlong_stream, oracle_decode, oracle_encode, pack_samples,
                     random_walk_samples)

pytestmark = pytest.mark.gpu

PP, MSB, SGN = AEC_DATA_PREPROCESS, AEC_DATA_MSB, AEC_DATA_SIGNED
AEC_DATA_ERROR = -3
CANARY = 4096

# (bps, block, rsi, flags, samples): every container width, LSB / MSB, signed, with and without the preprocessor,
# the templated block sizes and a generic one, rsi 1 .. 4096, short last RSIs, a restricted low-bps set
SHAPES = [
    (8, 8, 128, PP, 8 * 128 * 40 + 77),
    (16, 16, 128, PP, 16 * 128 * 50 + 5),
    (24, 16, 4, PP | AEC_DATA_3BYTE | MSB, 16 * 4 * 300 + 9),
    (32, 32, 4096, PP | MSB | SGN, 32 * 4096 * 2 + 1000),
    (16, 64, 1, 0, 64 * 700 + 3),
    (12, 10, 4, PP | AEC_NOT_ENFORCE, 10 * 4 * 400 + 7),
    (32, 8, 128, SGN, 8 * 128 * 20 + 1),
    (4, 16, 16, PP | AEC_RESTRICTED, 16 * 16 * 200 + 11),
    (16, 32, 4096, PP | MSB, 32 * 4096 + 32 * 100),
    (16, 16, 128, PP | MSB, 16 * 128 * 1200 + 13),      # 4.7 MiB: streamed encoder pieces above 1 MiB too
]


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import api as a
    a.library()
    return a


@pytest.fixture(scope="module")
def gpu():
    import torch  # noqa: F401
    from libaec_amd import gpu as g
    return g


def make(shape, seed):
    bps, bs, rsi, flags, n = shape
    rng = np.random.default_rng(seed)
    vals = random_walk_samples(rng, n, bps, flags, scale=3.0 if bps > 4 else 0.5, zero_frac=0.1)
    return pack_samples(vals, bps, flags)


def expected(data, bps, bs, rsi, flags):
    rc, want, _, offs, _ = oracle_encode(data, bps, bs, rsi, flags)
    assert rc == AEC_OK
    nb = bytes_per_sample(bps, flags)
    nblk = (data.size // nb + bs - 1) // bs
    rc, full, _ = oracle_decode(want, bps, bs, rsi, flags, nblk * bs * nb)
    assert rc == AEC_OK and len(full) == nblk * bs * nb
    return want, offs.astype(np.uint64), full


def range_on(api, dec, stream_arr, offs_arr, pos, size, flags_check=True):
    """aec_decode_range into a buffer with a canary on either side; returns (rc, bytes, stream fields)."""
    buf = np.full(size + 2 * CANARY, 0xA5, dtype=np.uint8)
    s = dec.s
    s.next_in, s.avail_in = stream_arr.ctypes.data, stream_arr.size
    s.next_out, s.avail_out = buf.ctypes.data + CANARY, size
    before = (s.total_in, s.total_out)
    rc = dec.lib.aec_decode_range(C.byref(s), offs_arr.ctypes.data_as(C.POINTER(C.c_size_t)), offs_arr.size, pos, size)
    assert (buf[:CANARY] == 0xA5).all() and (buf[CANARY + size:] == 0xA5).all(), "write outside the window"
    assert s.next_in == stream_arr.ctypes.data and s.avail_in == stream_arr.size and s.total_in == before[0]
    if rc == AEC_OK:
        assert s.next_out == buf.ctypes.data + CANARY + size and s.avail_out == 0 and s.total_out == before[1] + size
    else:
        assert s.next_out == buf.ctypes.data + CANARY and s.avail_out == size and s.total_out == before[1]
    return rc, buf[CANARY:CANARY + size].tobytes()


def random_windows(rng, total, rsi_bytes, count):
    w = [(0, 1), (0, total), (total - 1, 1), (total - rsi_bytes // 2 - 3, rsi_bytes // 2 + 3)]
    for b in range(1, min(total // rsi_bytes, 4) + 1):
        w.append((b * rsi_bytes - 5, 11))                 # across an RSI border
    while len(w) < count:
        pos = int(rng.integers(0, total))
        size = int(rng.choice([1, 2, 3, 7, 64, 4096, rsi_bytes, 3 * rsi_bytes + 5, total]))
        w.append((pos, max(1, min(size, total - pos))))
    return [(p, s) for p, s in w if 0 <= p and s >= 1 and p + s <= total]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}b-bs{s[1]}-rsi{s[2]}-f{s[3]}")
def test_offsets_seek_and_ranges(api, shape):
    bps, bs, rsi, flags, _ = shape
    data = make(shape, hash(shape) & 0xFFFF)
    want, offs, full = expected(data, bps, bs, rsi, flags)
    rsi_bytes = rsi * bs * bytes_per_sample(bps, flags)
    rng = np.random.default_rng(7)

    # 1. encoder offsets: one-shot, and streamed in random pieces (the count never decreases)
    rc, enc, eo = api.encode_with_offsets(data, bps, bs, rsi, flags)
    assert rc == AEC_OK and enc == want and np.array_equal(eo, offs)
    e = api.Encoder(bps, bs, rsi, flags)
    assert e.enable_offsets() == AEC_OK
    out, at, last, big = [], 0, 0, 0
    nb = bytes_per_sample(bps, flags)
    while at < data.size:
        # (pieces of up to 64 KiB, and of 1.5 MiB: those are coded as batches of their own, rebased on what came before)
        step = int(rng.integers(1, 65536)) if rng.random() < 0.6 else 1536 << 10
        step = step // nb * nb or nb
        big += step > (1 << 20) and at + step < data.size
        rc, used, got = e.call(data[at:at + step], len(want) + 64, AEC_NO_FLUSH)
        assert rc == AEC_OK
        at += used
        out.append(got)
        rc, o = e.offsets()
        assert rc == AEC_OK and o.size >= last and np.array_equal(o, offs[:o.size])
        last = o.size
    rc, _, got = e.call(b"", len(want) + 64, AEC_FLUSH)
    out.append(got)
    rc, o = e.offsets()
    assert rc == AEC_OK and b"".join(out) == want and np.array_equal(o, offs)
    assert e.enable_offsets() == api.AEC_RSI_OFFSETS_ERROR        # (too late)
    assert big or data.size < (3 << 20)
    e.end()

    # 2. decoder offsets, the input cut into random pieces
    wa = np.frombuffer(want, dtype=np.uint8)
    d = api.Decoder(bps, bs, rsi, flags)
    assert d.enable_offsets() == AEC_OK
    at, got = 0, []
    while at < wa.size:
        step = int(rng.integers(1, max(2, wa.size // 4)))
        rc, used, o = d.call(wa[at:at + step], len(full), AEC_NO_FLUSH)
        assert rc == AEC_OK
        at += used
        got.append(o)
    rc, _, o = d.call(b"", len(full), AEC_FLUSH)
    got.append(o)
    assert b"".join(got) == full
    rc, do = d.offsets()
    assert rc == AEC_OK and np.array_equal(do, offs)
    d.end()

    # 3. ranges: many on one state, canaries, the stream fields
    d = api.Decoder(bps, bs, rsi, flags)
    for pos, size in random_windows(rng, len(full), rsi_bytes, 200):
        rc, b = range_on(api, d, wa, offs, pos, size)
        assert rc == AEC_OK and b == full[pos:pos + size], (pos, size)
    d.end()

    # 4. seek to an RSI start, then aec_decode: the output from that RSI on
    for i in sorted({0, 1, offs.size // 2, offs.size - 1}):
        if i >= offs.size:
            continue
        d = api.Decoder(bps, bs, rsi, flags)
        rc, skipped = d.buffer_seek(wa, int(offs[i]))
        assert rc == AEC_OK and skipped == int(offs[i]) // 8 and d.s.total_in == 0
        rc, _, o = d.call(wa[skipped:], len(full) - i * rsi_bytes, AEC_FLUSH)
        assert rc == AEC_OK and o == full[i * rsi_bytes:], i
        d.end()


def test_error_returns(api):
    shape = (16, 16, 8, PP, 16 * 8 * 30 + 3)
    bps, bs, rsi, flags, _ = shape
    data = make(shape, 5)
    want, offs, full = expected(data, bps, bs, rsi, flags)
    wa = np.frombuffer(want, dtype=np.uint8)
    rsi_bytes = rsi * bs * 2
    d = api.Decoder(bps, bs, rsi, flags)
    # count / get without offsets enabled
    n = C.c_size_t(99)
    assert d.lib.aec_decode_count_offsets(C.byref(d.s), C.byref(n)) == api.AEC_RSI_OFFSETS_ERROR and n.value == 0
    buf = (C.c_size_t * 4)()
    assert d.lib.aec_decode_get_offsets(C.byref(d.s), buf, 4) == api.AEC_RSI_OFFSETS_ERROR
    # size 0, beyond the table, no room
    assert range_on(api, d, wa, offs, 5, 0)[0] == AEC_OK
    assert range_on(api, d, wa, offs[:3], 3 * rsi_bytes, 4)[0] == AEC_DATA_ERROR
    s = d.s
    s.next_in, s.avail_in, s.next_out, s.avail_out = wa.ctypes.data, wa.size, C.addressof(buf), 3
    assert d.lib.aec_decode_range(C.byref(s), offs.ctypes.data_as(C.POINTER(C.c_size_t)), offs.size, 0, 8) == AEC_MEM_ERROR
    # tables that are not this stream's
    bad = offs.copy(); bad[2] = bad[1]
    assert range_on(api, d, wa, bad, rsi_bytes, 3 * rsi_bytes)[0] == AEC_DATA_ERROR              # not increasing
    bad = offs.copy(); bad[3] = 8 * wa.size + 100
    assert range_on(api, d, wa, bad, 2 * rsi_bytes, 2 * rsi_bytes)[0] == AEC_DATA_ERROR          # beyond the input
    bad = offs.copy(); bad[4] += 1
    assert range_on(api, d, wa, bad, 3 * rsi_bytes, rsi_bytes + 10)[0] == AEC_DATA_ERROR       # shifted by one bit
    other = make(shape, 6)
    _, oo, _ = expected(other, bps, bs, rsi, flags)
    # another stream's table: the whole window decodes RSI 0 whole, which cannot end at the other stream's entry 1
    assert range_on(api, d, wa, oo, 0, len(full))[0] == AEC_DATA_ERROR
    rc, b = range_on(api, d, wa, oo, rsi_bytes * 5 + 3, rsi_bytes * 4)
    assert rc in (AEC_OK, AEC_DATA_ERROR)
    # the stream ends before the window: a table with one entry too many
    cut = wa[: int(offs[-1]) // 8 + 2].copy()
    rc, _ = range_on(api, d, cut, offs, len(full) - 20, 20)
    assert rc == AEC_DATA_ERROR
    # after aec_decode: AEC_STREAM_ERROR; enable / seek too late
    rc, _, _ = d.call(wa, len(full), AEC_FLUSH)
    assert rc == AEC_OK
    assert range_on(api, d, wa, offs, 0, 4)[0] == AEC_STREAM_ERROR
    assert d.enable_offsets() == api.AEC_RSI_OFFSETS_ERROR
    d.end()
    # get into a buffer that is too short; seek beyond the input
    d = api.Decoder(bps, bs, rsi, flags)
    assert d.enable_offsets() == AEC_OK
    assert d.call(wa, len(full), AEC_FLUSH)[0] == AEC_OK
    n = C.c_size_t(0)
    assert d.lib.aec_decode_count_offsets(C.byref(d.s), C.byref(n)) == AEC_OK and n.value == offs.size
    small = (C.c_size_t * 2)(7, 7)
    assert d.lib.aec_decode_get_offsets(C.byref(d.s), small, 2) == AEC_MEM_ERROR and list(small) == [7, 7]
    d.end()
    d = api.Decoder(bps, bs, rsi, flags)
    assert d.buffer_seek(wa, 8 * wa.size + 3)[0] == AEC_MEM_ERROR and d.s.avail_in == wa.size
    d.end()


def test_foreign_streams(api):
    """Coded data sets longer than any libaec encoder writes (the windowed sequential fallback), and AEC_PAD_RSI."""
    rng = np.random.default_rng(21)
    bps, bs, rsi = 16, 16, 8
    stream = craft_overlong_stream(rng, bps, bs, rsi, 12, 4, 0.05, 3000)
    nblk = rsi * 12
    rc, full, _ = oracle_decode(stream, bps, bs, rsi, PP, nblk * bs * 2)
    assert rc == AEC_OK and len(full) == nblk * bs * 2
    # RSI k starts where the oracle's decode of the first k RSIs stops reading
    starts = np.array([0] + [oracle_decode(stream, bps, bs, rsi, PP, k * rsi * bs * 2)[2] for k in range(1, 12)],
                      dtype=np.uint64)
    d = api.Decoder(bps, bs, rsi, PP)
    assert d.enable_offsets() == AEC_OK
    assert d.call(stream, len(full), AEC_FLUSH)[0] == AEC_OK
    rc, offs = d.offsets()
    d.end()
    assert rc == AEC_OK and np.array_equal(offs, starts)
    sa = np.frombuffer(stream, dtype=np.uint8)
    d = api.Decoder(bps, bs, rsi, PP)
    for pos, size in random_windows(rng, len(full), rsi * bs * 2, 40):
        rc, b = range_on(api, d, sa, offs, pos, size)
        assert rc == AEC_OK and b == full[pos:pos + size], (pos, size)
    d.end()
    # AEC_PAD_RSI: RSIs coded as streams of their own, back to back
    vals = random_walk_samples(rng, bs * rsi * 9, bps, PP, scale=3.0, zero_frac=0.2)
    data = pack_samples(vals, bps, PP)
    rb = bs * rsi * 2
    parts = [oracle_encode(data[i:i + rb], bps, bs, rsi, PP)[1] for i in range(0, data.size, rb)]
    stream = b"".join(parts)
    starts = np.cumsum([0] + [len(p) for p in parts[:-1]]) * 8
    d = api.Decoder(bps, bs, rsi, PP | AEC_PAD_RSI)
    assert d.enable_offsets() == AEC_OK
    rc, _, o = d.call(stream, data.size, AEC_FLUSH)
    assert rc == AEC_OK and o == data.tobytes()
    rc, offs = d.offsets()
    d.end()
    assert rc == AEC_OK and np.array_equal(offs, starts.astype(np.uint64))
    sa = np.frombuffer(stream, dtype=np.uint8)
    d = api.Decoder(bps, bs, rsi, PP | AEC_PAD_RSI)
    for pos, size in random_windows(rng, data.size, rsi * bs * 2, 60):
        rc, b = range_on(api, d, sa, offs, pos, size)
        assert rc == AEC_OK and b == data.tobytes()[pos:pos + size], (pos, size)
    d.end()


def test_device_seam(api, gpu):
    import torch
    bps, bs, rsi, flags, _ = shape = SHAPES[1]
    data = make(shape, 3)
    want, offs, full = expected(data, bps, bs, rsi, flags)
    lib = gpu._lib()
    lib.aec_gpu_decode_range_async.restype = C.c_int
    lib.aec_gpu_decode_range_async.argtypes = [C.c_void_p, C.POINTER(gpu.Params), C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    codec = gpu.Codec(bps, bs, rsi, flags)
    d_in = torch.zeros(len(want) + 16, dtype=torch.uint8, device="cuda")
    d_in[:len(want)] = torch.frombuffer(bytearray(want), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(9)
    for pos, size in random_windows(rng, len(full), rsi * bs * 2, 60):
        d_out = torch.full((size + 2 * CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = lib.aec_gpu_decode_range_async(codec.ctx, C.byref(codec.p), d_in.data_ptr(), len(want), d_off.data_ptr(),
                                            offs.size, pos, size, d_out.data_ptr() + CANARY, d_res.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        res = d_res.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0]
        o = d_out.cpu().numpy()
        assert res["status"] == 0 and (o[:CANARY] == 0xA5).all() and (o[CANARY + size:] == 0xA5).all()
        assert o[CANARY:CANARY + size].tobytes() == full[pos:pos + size], (pos, size)
    codec.close()


def _gen(kind, nbytes):
    lib = C.CDLL(f"{ROOT}/libaec_amd/lib/libaec_datagen.so")
    a = np.empty(nbytes, dtype=np.uint8)
    bpsb = {0: 2, 1: 4, 2: 1}[kind]
    lib.aec_gen_fill_parallel(C.c_uint(kind), C.c_uint64(0), C.c_void_p(a.ctypes.data), C.c_size_t(nbytes // bpsb),
                              C.c_uint(8))
    return a


@pytest.mark.parametrize("cfg,scheme_want", [((0, 16, 16, 128, PP), 2), ((1, 32, 32, 4096, PP | MSB | SGN), 3)],
                         ids=["c2-window-tables", "c3-trunk-segments"])
def test_large_streams(api, gpu, cfg, scheme_want):
    """Decoder offsets of a 256 MiB stream through the index schemes for large streams, and a 1 GiB round trip
    through aec_decode_range with the encoder's offsets (the oracle checks the first 64 MiB of the stream)."""
    kind, bps, bs, rsi, flags = cfg
    data = _gen(kind, 256 << 20)
    rc, want, _, offs, _ = oracle_encode(data, bps, bs, rsi, flags)
    assert rc == AEC_OK
    scheme = gpu.index_scheme(bps, bs, rsi, flags, len(want), len(want) * 8 // max(offs.size, 1), 0)
    # (config 2: the window tables; config 3: the trunk, which also leaves the segment starts the decoder takes a lane
    # per segment from -- 64 segments per RSI)
    assert scheme == scheme_want, gpu.INDEX_SCHEMES[scheme]
    d = api.Decoder(bps, bs, rsi, flags)
    assert d.enable_offsets() == AEC_OK
    rc, _, o = d.call(want, data.size, AEC_FLUSH)
    assert rc == AEC_OK and len(o) == data.size
    rc, do = d.offsets()
    d.end()
    assert rc == AEC_OK and np.array_equal(do, offs.astype(np.uint64))
    del o, want
    # 1 GiB: encode with offsets, decode everything back through the offsets
    data = _gen(kind, 1 << 30)
    rc, enc, eo = api.encode_with_offsets(data, bps, bs, rsi, flags)
    assert rc == AEC_OK
    head = 64 << 20
    rc, want_head, _, offs_head, _ = oracle_encode(data[:head], bps, bs, rsi, flags)
    assert rc == AEC_OK and enc[:len(want_head) - 1] == want_head[:-1]
    assert np.array_equal(eo[:offs_head.size], offs_head.astype(np.uint64))
    out = np.empty(data.size, dtype=np.uint8)
    rc, _, s = api.decode_range(enc, eo, 0, data.size, bps, bs, rsi, flags, out=out)
    assert rc == AEC_OK and s.total_out == data.size
    assert np.array_equal(out, data)
