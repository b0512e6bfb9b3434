"""The narrow cases (tests/narrow_cases.py: generic block sizes from 2 to 62, samples of 1 to 7 bits, restricted code sets
with block headers of one and two bits, 3-byte and 31-bit containers) on the device.  Every expected byte, offset and count
is the oracle's (tests/test_narrow_emul.py holds the oracle to the compiled reference on the same streams).

  a. every decode family on every case: the encoder's stream and RSI table, then the table decode (aligned and at +4), the
     segment decode from the encoder's segment table, the bare decode behind the segment index, the indexed decode behind
     the plain index pass, the batch decode of five streams, windows of the stream between canaries, and batches of chunks
     of 0 samples, 1 sample, an RSI and a sample, three blocks -- with the table and bare;
  b. tests/cross_scheme.py --narrow: every index scheme that admits a shape forced on it (tuning build, child process);
  c. the shipped dispatch: per class the streams whose chain begins with the phase-locked chains, the window tables, the
     trunk (tests/golden/narrow_chain.json), through aec_gpu_index_async and aec_buffer_decode;
  d. the encoder on the inputs of c (aec_buffer_encode, aec_encode in random pieces) and SZIP chunks of 1-bit pixels in
     blocks of 2 and 5-bit pixels in blocks of 10 against the reference shim's bytes (tests/golden/narrow_sz.json).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import narrow_cases as N
from test_gpu_dec_modes import DEC_OK, gpu, on_device, record  # noqa: F401
from test_gpu_decode_chunks import decode_both_ways

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def geometry(c):
    nb = H.bytes_per_sample(c.bps, c.flags)
    return nb, c.bs * nb, c.rsi * c.bs * nb


def found_blocks(res, c):
    return int(res["n_rsi"]) * c.rsi + int(res["tail_blocks"])


# ---- a. the decode families --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", N.CASES, ids=N.case_id)
def test_encode_then_every_decode_of_one_stream(gpu, c):  # noqa: F811
    import torch
    k = N.family(c)
    nb, blk, R = geometry(c)
    n_rsi, nblk, full = len(k.offs), k.nblk, k.decoded
    codec = gpu.Codec(*N.prm(c))
    assert codec.rsi_count(k.data.size) == n_rsi and codec.block_count(k.data.size) == nblk
    # the encoder: stream, RSI table, and (RSIs of more than one segment) the segment table
    nseg = codec.segment_count(k.data.size)
    d_tab = torch.zeros(nseg * 16, dtype=torch.uint8, device="cuda")
    if c.rsi > 64:
        codec.set_segment_table(d_tab)
    d_enc, nbytes, bits, _, d_off = codec.encode(torch.from_numpy(k.data.copy()).cuda())
    codec.set_segment_table(None)
    assert bits == k.bits and d_enc[:nbytes].cpu().numpy().tobytes() == k.stream, "stream differs from the oracle's"
    assert np.array_equal(d_off.cpu().numpy()[:n_rsi].astype(np.uint64), k.offs), "RSI table differs from the oracle's"
    d_in = on_device(k.stream)
    d_offs = torch.from_numpy(k.offs.astype(np.int64)).cuda()
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")

    # 1. from the table, aligned and 4 bytes behind a 16-byte boundary
    for off in (0, 4):
        d_out = torch.zeros(len(full) + 32, dtype=torch.uint8, device="cuda")
        codec.decode_async(d_in, len(k.stream), d_offs, n_rsi, nblk, d_out[off:], d_res)
        assert record(gpu, d_res)["status"] == DEC_OK, off
        assert d_out[off:off + len(full)].cpu().numpy().tobytes() == full, ("table decode", off)
    # 2. a lane per segment, from the encoder's segment table
    if c.rsi > 64:
        d_out = torch.zeros(len(full) + 32, dtype=torch.uint8, device="cuda")
        codec.decode_segments_async(d_in, len(k.stream), d_tab, nseg, nblk, d_out, d_res)
        assert record(gpu, d_res)["status"] == DEC_OK
        assert d_out[:len(full)].cpu().numpy().tobytes() == full, "segment decode"
    # 3. bare: segment index, then a lane per segment where the index found the starts.  (A run of zero blocks that closes
    # a short last RSI reads as one to the end of its segment: up to 63 blocks more than were coded.)
    room = (n_rsi + 1) * R + 64 * blk
    spr = codec.segments_per_rsi()
    d_idx = torch.zeros(n_rsi + 3, dtype=torch.int64, device="cuda")
    d_sb = torch.zeros((n_rsi + 3) * spr, dtype=torch.int64, device="cuda")
    d_ires = torch.zeros(40, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(room, dtype=torch.uint8, device="cuda")
    codec.index_segments_async(d_in, len(k.stream), 0, d_idx, d_sb, n_rsi + 1, d_ires)
    codec.decode_bare_async(d_in, len(k.stream), d_idx, d_sb, n_rsi + 1, n_rsi * c.rsi, d_ires, d_out, d_res)
    ires, res = record(gpu, d_ires), record(gpu, d_res)
    assert nblk <= found_blocks(ires, c) <= min(nblk + 63, n_rsi * c.rsi) and int(ires["end_bit"]) == k.bits, ires
    assert np.array_equal(d_idx[:n_rsi].cpu().numpy().astype(np.uint64), k.offs), "segment index: RSI starts"
    assert res["status"] == DEC_OK, res
    assert d_out[:len(full)].cpu().numpy().tobytes() == full, "bare decode"
    # 4. the plain index pass and the decode that takes its counts on the device
    d_idx = torch.full((n_rsi + 3,), -1, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(room, dtype=torch.uint8, device="cuda")
    codec.index_async(d_in, len(k.stream), 0, d_idx, n_rsi + 1, d_ires)
    codec.decode_indexed_async(d_in, len(k.stream), d_idx, n_rsi + 1, d_ires, d_out, d_res)
    ires, res = record(gpu, d_ires), record(gpu, d_res)
    assert int(ires["status"]) == 0 and nblk <= found_blocks(ires, c) <= min(nblk + 63, n_rsi * c.rsi), ires
    assert int(ires["end_bit"]) == k.bits
    assert np.array_equal(d_idx[:n_rsi].cpu().numpy().astype(np.uint64), k.offs), "index pass: RSI starts"
    assert res["status"] == DEC_OK, res
    assert d_out[:len(full)].cpu().numpy().tobytes() == full, "indexed decode"
    # 5. windows of the decoded stream, 0xA5 on both sides (the four of test_window_decode, inside this stream)
    lib = gpu._lib()
    total = len(full)
    mid = min(R + R // 2 + 5, total - 1)
    windows = [(min(2 * R, total) - 3, 1), (mid, min(R // 2 + blk + 7, total - mid)),
               (R, min(2 * R, (total - R) // blk * blk)), (0, total)]
    for off in (0, 4):
        for pos, size in windows:
            d_win = torch.full((size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            rc = lib.aec_gpu_decode_range_async(codec.ctx, C.byref(codec.p), d_in.data_ptr(), len(k.stream), d_offs.data_ptr(),
                                                n_rsi, pos, size, d_win.data_ptr() + off, d_res.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert rc == 0, (pos, size)
            o = d_win.cpu().numpy()
            assert (o[:off] == 0xA5).all() and (o[off + size:] == 0xA5).all(), ("write outside the window", pos, size, off)
            assert record(gpu, d_res)["status"] == DEC_OK and o[off:off + size].tobytes() == full[pos:pos + size], (pos, size, off)
    codec.close()


@pytest.mark.parametrize("c", N.CASES, ids=N.case_id)
def test_batch_decode_of_five_streams(gpu, c):  # noqa: F811
    """aec_gpu_decode_batch_async: the case's samples rotated by 0 to 4 RSIs and a block, five streams of the same count"""
    import torch
    nb, blk, R = geometry(c)
    n = N.family_samples(c)
    base = N.case_data(c, n)
    datas = [np.ascontiguousarray(np.roll(base, s * (R + blk))) for s in range(5)]
    want = []
    for d in datas:
        rc, stream, _, offs, bits = H.oracle_encode(d, *N.prm(c))
        assert rc == H.AEC_OK
        nblk = -(-n // c.bs)
        rc, full, _ = H.oracle_decode(stream, *N.prm(c), nblk * blk)
        assert rc == H.AEC_OK and len(full) == nblk * blk
        want.append((stream, full))
    rpc = -(-nblk // c.rsi)
    choff, blob = [0], b""
    for stream, _ in want:
        blob += stream + bytes(-len(stream) % 16)
        choff.append(len(blob))
    codec = gpu.Codec(*N.prm(c))
    d_choff = torch.tensor(choff, dtype=torch.int64, device="cuda")
    d_off = torch.zeros(5 * rpc, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(5 * rpc * R + 64 * blk, dtype=torch.uint8, device="cuda")
    d_recs = torch.zeros(5 * 40, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    rc = gpu._lib().aec_gpu_decode_batch_async(codec.ctx, C.byref(codec.p), on_device(blob).data_ptr(), len(blob), d_choff.data_ptr(),
                                               5, rpc, d_off.data_ptr(), d_out.data_ptr(), d_recs.data_ptr(), d_res.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    out = d_out.cpu().numpy()
    for s, (stream, full) in enumerate(want):
        rec = record(gpu, d_recs, s)
        assert rec["status"] == DEC_OK and nblk <= found_blocks(rec, c) <= min(nblk + 63, rpc * c.rsi), (s, rec)
        assert out[s * rpc * R:s * rpc * R + len(full)].tobytes() == full, s
    assert record(gpu, d_res)["status"] == DEC_OK
    codec.close()


@pytest.mark.parametrize("c", N.CASES, ids=N.case_id)
def test_chunks_encode_and_decode_with_the_table_and_bare(gpu, c):  # noqa: F811
    """aec_gpu_encode_chunks_async on chunks of 0 samples, 1 sample, an RSI and a sample, three blocks (and two RSIs and a
    half): streams, records and table are the oracle's per chunk; aec_gpu_decode_chunks_async gives the chunks back from
    the table and from the bare streams (tests/test_gpu_decode_chunks.py: decode_both_ways)."""
    import torch
    from test_gpu_decode_chunks import expected
    nb, blk, R = geometry(c)
    S = c.rsi * c.bs
    data = N.case_data(c, 4 * S + 8 * c.bs, salt=1)
    chunks, at = [], 0
    for samples in (0, 1, S + 1, 3 * c.bs, 2 * S + S // 2 + 1):
        chunks.append(np.ascontiguousarray(data[at * nb:(at + samples) * nb]))
        at += samples
    want = [expected(ch, N.prm(c)) for ch in chunks]
    sizes = np.array([ch.size for ch in chunks], dtype=np.uint64)
    offsets = np.zeros(len(chunks), dtype=np.uint64)
    offsets[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16 + 16)
    host = np.full(int(offsets[-1] + sizes[-1]) + 32, 0xA5, dtype=np.uint8)
    for o, ch in zip(offsets, chunks):
        host[int(o):int(o) + ch.size] = ch
    codec = gpu.Codec(*N.prm(c))
    d_enc, rec, d_tab, res = codec.encode_chunks(torch.from_numpy(host).cuda(), offsets, sizes, want_offsets=True)
    need = sum(len(w[0]) for w in want)
    assert not int(res["overflow"]) and int(res["total_bits"]) == need * 8
    out, tab = d_enc.cpu().numpy(), d_tab.cpu().numpy()
    at = entry = 0
    for i, (enc, bits, offs) in enumerate(want):
        assert (int(rec[i][0]), int(rec[i][1])) == (at * 8, bits), (i, rec[i])
        assert out[at:at + len(enc)].tobytes() == enc, f"chunk {i}: stream differs from the oracle's"
        assert tab[entry:entry + len(offs) + 1].tolist() == [at * 8 + o for o in offs] + [at * 8 + bits], f"RSI table, chunk {i}"
        at += len(enc)
        entry += len(offs) + 1
    # ... and back: from the table (the oracle's offsets) and bare
    decode_both_ways(N.prm(c), chunks, np.random.default_rng(c.bps * 100 + c.bs), codec=codec)
    codec.close()


# ---- b. every scheme forced ---------------------------------------------------------------------------------------------

def test_every_index_scheme_on_the_narrow_shapes():
    """tests/cross_scheme.py --narrow on the tuning library: the shapes of narrow_cases.FORCED, each through EVERY scheme
    the table names for it -- whole, cut short, with the caller's bound, resumed inside an RSI"""
    e = dict(os.environ, AEC_AMD_LIB=os.path.join(ROOT, "libaec_amd", "lib", "tuning", "libaec.so.0"))
    assert os.path.exists(e["AEC_AMD_LIB"])
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cross_scheme.py"), "--narrow"], env=e, capture_output=True,
                         text=True, timeout=600)
    print(out.stdout[-4000:], out.stderr[-4000:])
    assert out.returncode == 0 and "cross scheme ok" in out.stdout, (out.stdout[-3000:], out.stderr[-3000:])


# ---- c., d. the shipped dispatch and the encoder on its inputs --------------------------------------------------------------

GOLDEN = N.golden_chains()["dispatch"]
ROWS = [(c, n, first, row) for (c, n, first), row in zip(N.DISPATCH, GOLDEN)]
ROW_IDS = [f"{N.case_id(c)}-scheme{first}" for c, _, first, _ in ROWS]


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import api as a
    a.library()
    return a


@pytest.mark.parametrize("c,n,first,row", ROWS, ids=ROW_IDS)
def test_shipped_dispatch(gpu, api, c, n, first, row):  # noqa: F811
    """the stream's chain is the one the table claims (aec_gpu_index_plan on what the oracle coded here); the index pass
    finds the oracle's RSI starts, its end and its counts; aec_buffer_decode gives the oracle's bytes"""
    import torch
    k = N.coded(c, n)
    n_rsi = len(k.offs)
    ids = gpu.index_plan(*N.prm(c), len(k.stream), N.rsi_bits_hint(k))[0]
    assert ids == row["chain"] and ids[0] == first, (ids, row)
    codec = gpu.Codec(*N.prm(c))
    d_in = on_device(k.stream)
    d_idx = torch.full((n_rsi + 3,), -1, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    codec.index_async(d_in, len(k.stream), 0, d_idx, n_rsi + 1, d_res)
    torch.cuda.synchronize()
    res = record(gpu, d_res)
    got = d_idx.cpu().numpy()[:n_rsi].astype(np.uint64)
    assert np.array_equal(got, k.offs), ("RSI starts", int(np.argmax(got != k.offs)))
    assert int(res["status"]) == 0 and int(res["end_bit"]) == k.bits, res
    assert k.nblk <= found_blocks(res, c) <= min(k.nblk + 63, n_rsi * c.rsi), res
    assert int(res["n_rsi"]) >= k.nblk // c.rsi
    codec.close()
    rc, dec = api.aec_buffer_decode(k.stream, *N.prm(c), len(k.decoded))
    assert rc == H.AEC_OK and dec == k.decoded


@pytest.mark.parametrize("c,n,first,row", ROWS, ids=ROW_IDS)
def test_encoder_on_the_dispatch_inputs(api, c, n, first, row):
    """aec_buffer_encode, and aec_encode fed in random pieces with random room: the oracle's stream"""
    k = N.coded(c, n)
    rc, got = api.aec_buffer_encode(k.data, *N.prm(c))
    assert rc == H.AEC_OK and got == k.stream, (rc, len(got), len(k.stream))
    rng = np.random.default_rng(n)
    nb = H.bytes_per_sample(c.bps, c.flags)
    e = api.Encoder(*N.prm(c))
    out, pos = bytearray(), 0
    while pos < k.data.size:
        step = int(rng.choice([nb, 7 * nb, 4096 * nb, 1 << 16, 1 << 19, 1 << 20])) // nb * nb
        piece, off = k.data[pos:pos + step], 0
        while off < piece.size:
            rc, used, part = e.call(piece[off:], int(rng.choice([4096, 1 << 16, 1 << 21])), H.AEC_NO_FLUSH)
            assert rc == H.AEC_OK
            out += part
            off += used
            if used == 0 and not part:
                break
        pos += step
    while True:
        rc, used, part = e.call(b"", 1 << 20, H.AEC_FLUSH)
        assert rc == H.AEC_OK
        out += part
        if not part:
            break
    assert e.end() == H.AEC_OK
    assert bytes(out) == k.stream, (len(out), len(k.stream))


@pytest.mark.parametrize("i", range(len(N.SZ_SHAPES)), ids=[s[0] for s in N.SZ_SHAPES])
def test_szip_chunks_of_narrow_pixels(api, i):
    """SZ_BufftoBuffCompress / SZ_BufftoBuffDecompress on one chunk of 1 MiB: the reference shim's bytes (by length and
    SHA-256, tests/golden/narrow_sz.json), and the pixels back"""
    import hashlib
    from libaec_amd import szip
    name, prm, data, want_len, want_sha = N.sz_golden()[i]
    assert (name, prm) == (N.SZ_SHAPES[i][0], N.SZ_SHAPES[i][1]) and data.size == 1 << 20
    rc, comp = szip.compress(data, data.size * 2 + 4096, *prm)
    assert rc == szip.SZ_OK and len(comp) == want_len, (rc, len(comp), want_len)
    assert hashlib.sha256(comp).hexdigest() == want_sha, "stream differs from the reference shim's"
    rc, dec = szip.decompress(comp, data.size, *prm)
    assert rc == szip.SZ_OK and dec == data.tobytes(), (rc, len(dec))
