"""Streams whose predictor state leaves the sample range (tests/foreign_predictor.py: the writer, the exact walk, the
families and the model that shows what they hit) through every decode entry that can take them: the table decode at a
16-byte aligned output (lane or wave kernel) and 4 bytes behind the boundary (generic store), the indexed decode behind
a table bound that sends RSIs of 16 blocks to the lane kernel, the segment decode, the bare decode by segments, the chunk
batches with the table and bare between two valid neighbours, windows that start and end in the stretch outside the
range, and the libaec ABI in one shot, with the input cut inside the stretch and with the room handed out block by
block.  Expected bytes and status are always the oracle's, pinned to the reference by the hashes in
tests/golden/foreign_predictor.json; tests/test_foreign_predictor.py checks on the CPU that every vector reaches the
conditions it is meant for.

Which kernel sees what.  The wave kernel takes RSIs of 16 blocks and more from a table of up to 8192 entries
(aec_dec.hip: dec_wave_wanted), and an RSI of 16 to 64 blocks is one round of it, in which the block that leaves the
range makes the whole round take the exact steps: at rsi 16 -- (5, 16, 16) and the 4100 RSIs of big_table -- the table
decode can show no wrong block, with the old per-block test or the new.  A vector of more than 8192 such RSIs would
exceed the 600 000 samples a vector may have, so these configs reach the lane kernel through the BOUND of the table
instead, which is what sizes the launch: aec_gpu_index_async + aec_gpu_decode_indexed_async with a bound of 8200 RSIs,
and the libaec ABI, whose bound comes from the room of the call.  Elsewhere the lane kernel is covered by the rsi-2
configs and the wave kernel by rsi 100 and more.

The segment table: SegEntry.prev is unsigned 32 bits and the kernel takes it as the state for unsigned samples, so the
table built from the exact walk carries a state outside the range and the decode must be the oracle's.  For signed
samples the kernel sign-extends the low bps bits of prev -- a sample, which a state outside the range is not: the
interface cannot say it, and what it promises for such a stream is DEC_OK and exact bytes for every
segment whose predecessor is a sample; the bytes of the others are not compared.

These vectors are for a library whose per-block test has its precondition.  One from before it (AEC_AMD_LIB) does not
return from the wave kernel on the vectors that come back into the range at the start of a round
(test_foreign_predictor.py::test_the_wave_kernels_correction_ends): do not run this file against such a library."""
import ctypes as C

import numpy as np
import pytest
import torch

import foreign_predictor as F
import helpers as H
from libaec_amd import api, gpu

pytestmark = pytest.mark.gpu

CASES = F.cases()


def _lib():
    """the library with the prototype of aec_gpu_decode_range_async, which libaec_amd.gpu does not wrap"""
    lib = gpu._lib()
    if lib.aec_gpu_decode_range_async.argtypes is None:
        lib.aec_gpu_decode_range_async.restype = C.c_int
        lib.aec_gpu_decode_range_async.argtypes = [C.c_void_p, C.POINTER(gpu.Params), C.c_void_p, C.c_size_t, C.c_void_p,
                                                   C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib

DEC_OK = 0
ONE_BLOCK_CALLS = 6400      # the streaming ABI with room for one block per call: at most so many such calls per vector


def _first_diff(got, want, nb, bs):
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    m = min(g.size, w.size)
    first = int(np.argmax(g[:m] != w[:m])) if (g[:m] != w[:m]).any() else m
    return "%d of %d bytes, first wrong byte %d, sample %d, block %d" % (g.size, w.size, first, first // nb, first // nb // bs)


_neighbours = {}


def valid_chunk(cfg, seed):
    """(stream, RSI start bits, bits, decoded bytes) of a valid stream of the same parameters: two RSIs and three blocks,
    the oracle's"""
    key = (tuple(cfg), seed)
    if key not in _neighbours:
        bps, bs, rsi, flags = cfg
        rng = np.random.default_rng(seed)
        nblk = 2 * rsi + 3 if rsi <= 130 else rsi + 3
        data = H.pack_samples(H.random_walk_samples(rng, nblk * bs, bps, flags, scale=3.0, zero_frac=0.1), bps, flags)
        rc, enc, _, offs, bits = H.oracle_encode(data, bps, bs, rsi, flags)
        assert rc == H.AEC_OK
        rc, full, _ = H.oracle_decode(enc, bps, bs, rsi, flags, data.size)
        assert rc == H.AEC_OK and len(full) == data.size
        _neighbours[key] = (enc, offs.astype(np.uint64), int(bits), full)
    return _neighbours[key]


def gpu_paths(family, cfg):
    """One vector through every decode entry that can take it; expected bytes and status are the oracle's.  Returns
    (paths run, failures): a failure is (path, what) and does not stop the other paths."""
    bps, bs, rsi, flags = cfg
    tag = F.case_id(family, cfg)
    v = F.vector(family, cfg)
    stream, nblk = v["stream"], v["nblk"]
    nb = H.bytes_per_sample(bps, flags)
    blk_bytes = bs * nb
    out_bytes = nblk * blk_bytes
    rc, full, _ = H.oracle_decode(stream, bps, bs, rsi, flags, out_bytes)
    assert rc == H.AEC_OK and len(full) == out_bytes and full == v["bytes"], tag
    ran, fails = [], []

    def rec(d_res, i=0):
        return d_res.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[i]

    def check(what, status, got, want=full):
        ran.append(what)
        if int(status) != DEC_OK:
            fails.append((what, "status %d" % int(status)))
        elif got != want:
            fails.append((what, _first_diff(got, want, nb, bs)))

    def on_device(b):
        d = torch.zeros(len(b) + 16, dtype=torch.uint8, device="cuda")
        d[:len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
        return d

    codec = gpu.Codec(bps, bs, rsi, flags)
    lib = _lib()
    d_in = on_device(stream)
    offs = v["rsi_bits"]
    n_rsi = offs.size
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()

    # aec_gpu_decode_async from the writer's RSI table: 16-byte aligned (lane or wave kernel, vector stores) and 4 bytes
    # behind the boundary (the generic store, which takes the exact step for every sample)
    for off in (0, 4):
        d_out = torch.zeros(out_bytes + 32, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
        assert d_out.data_ptr() % 16 == 0
        codec.decode_async(d_in, len(stream), d_offs, n_rsi, nblk, d_out[off:], d_res)
        check("table decode, output offset %d" % off, rec(d_res)["status"], d_out[off:off + out_bytes].cpu().numpy().tobytes())

    # aec_gpu_index_async + aec_gpu_decode_indexed_async with a table bound above what the wave kernel takes: the launch is
    # sized by the bound, so RSIs of 16 blocks go to the lane kernel (foreign_predictor.py: the comment above CONFIGS)
    if 16 <= rsi < 64:
        bound = F.LANE_TABLE_BOUND
        what = "indexed decode, table bound %d" % bound
        d_idx = torch.full((bound + 2,), -1, dtype=torch.int64, device="cuda")
        d_ires = torch.zeros(40, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((bound * rsi + 1) * blk_bytes + 64, dtype=torch.uint8, device="cuda")
        codec.index_async(d_in, len(stream), 0, d_idx, bound, d_ires)
        codec.decode_indexed_async(d_in, len(stream), d_idx, bound, d_ires, d_out, d_res)
        ires = rec(d_ires)
        found = int(ires["n_rsi"]) * rsi + int(ires["tail_blocks"])
        if int(ires["status"]) != DEC_OK or found != nblk:
            ran.append(what)
            fails.append((what, "index pass: status %d, %d blocks of %d" % (int(ires["status"]), found, nblk)))
        elif not np.array_equal(d_idx[:n_rsi].cpu().numpy().astype(np.uint64), offs):
            ran.append(what)
            fails.append((what, "index pass: RSI starts"))
        else:
            check(what, rec(d_res)["status"], d_out[:out_bytes].cpu().numpy().tobytes())

    # aec_gpu_decode_segments_async (rsi 130), the table from the exact walk: start bit and the state in front of the segment
    if rsi == 130 and flags & F.PP:
        spr = codec.segments_per_rsi()
        nseg = n_rsi * spr
        tab = np.zeros(nseg, np.dtype([("bit", "<u8"), ("prev", "<u4"), ("pad", "<u4")]))
        tab["bit"] = v["seg_bits"]
        exact = np.ones(nseg, bool)                          # segments whose predecessor the table can hold
        xmin, xmax = F.limits(bps, flags)
        for r in range(n_rsi):
            for j in range(1, spr):
                b = r * rsi + 64 * j
                if b < nblk:
                    x = int(v["front"][b])
                    if flags & F.SGN:
                        # (SegEntry.prev is a sample: the kernel sign-extends its low bps bits; a state outside the range is
                        # not one, and the segment behind it is not promised)
                        exact[r * spr + j] = xmin <= F.as_int(x, flags) <= xmax
                        x &= (1 << bps) - 1
                    tab["prev"][r * spr + j] = x
        nseg_used = (n_rsi - 1) * spr + (nblk - (n_rsi - 1) * rsi + 63) // 64
        d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
        d_out = torch.zeros(out_bytes + 16, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
        codec.decode_segments_async(d_in, len(stream), d_tab, nseg_used, nblk, d_out, d_res)
        got = np.frombuffer(d_out[:out_bytes].cpu().numpy().tobytes(), np.uint8).copy()
        want = np.frombuffer(full, np.uint8)
        for s in np.flatnonzero(~exact):                     # (unspecified bytes: not compared)
            r, j = divmod(int(s), spr)
            lo, hi = (r * rsi + 64 * j) * blk_bytes, min(nblk, r * rsi + min(rsi, 64 * (j + 1))) * blk_bytes
            got[lo:hi] = want[lo:hi]
        check("segment decode" + (", %d segments not promised" % int((~exact).sum()) if not exact.all() else ""),
              rec(d_res)["status"], got.tobytes())

    # the bare stream: index pass with segment starts, decode by segments (rsi 512) -- RSIs whose sums do not hold go to the
    # list and are decoded exactly, a lane per RSI
    if rsi == 512:
        spr = codec.segments_per_rsi()
        for with_record in (True, False):
            d_idx = torch.zeros(n_rsi + 2, dtype=torch.int64, device="cuda")
            d_sb = torch.zeros((n_rsi + 2) * spr, dtype=torch.int64, device="cuda")
            d_ires = torch.zeros(40, dtype=torch.uint8, device="cuda")
            d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
            d_out = torch.zeros((n_rsi + 2) * rsi * blk_bytes + 64 * blk_bytes, dtype=torch.uint8, device="cuda")
            codec.index_segments_async(d_in, len(stream), 0, d_idx, d_sb, n_rsi + 1, d_ires)
            ires = rec(d_ires)
            what = "bare decode" + (", index record" if with_record else "")
            found = int(ires["n_rsi"]) * rsi + int(ires["tail_blocks"])
            if int(ires["status"]) != DEC_OK or not nblk <= found <= nblk + 63:
                ran.append(what)
                fails.append((what, "index pass: status %d, %d blocks of %d" % (int(ires["status"]), found, nblk)))
                continue
            if not np.array_equal(d_idx[:n_rsi].cpu().numpy().astype(np.uint64), offs):
                ran.append(what)
                fails.append((what, "index pass: RSI starts"))
                continue
            if with_record:
                codec.decode_bare_async(d_in, len(stream), d_idx, d_sb, n_rsi + 1, nblk, d_ires, d_out, d_res)
            else:
                codec.decode_bare_async(d_in, len(stream), d_idx, d_sb, n_rsi, nblk, None, d_out, d_res)
            check(what, rec(d_res)["status"], d_out[:out_bytes].cpu().numpy().tobytes())

    # aec_gpu_decode_chunks_async: valid chunk, this stream, valid chunk -- with the table and bare
    if nblk * bs <= 120000:
        left, right = valid_chunk(cfg, 31), valid_chunk(cfg, 32)
        parts = [(left[0], left[1], left[2], left[3]), (stream, offs, v["bits"], full), (right[0], right[1], right[2], right[3])]
        blob, in_off, table = b"", [], []
        for enc, o, bits, _ in parts:
            in_off.append(len(blob))
            table += [8 * len(blob) + int(x) for x in o] + [8 * len(blob) + bits]
            blob += enc
        out_sizes = [len(p[3]) for p in parts]
        d_blob = on_device(blob)
        for have_table in (True, False):
            what = "chunks, " + ("table" if have_table else "bare")
            d_tab = torch.tensor(table, dtype=torch.int64, device="cuda") if have_table else None
            d_out, ooff, recs, res = codec.decode_chunks(d_blob, len(blob), out_sizes, d_table=d_tab, in_offsets=in_off,
                                                         in_sizes=[len(p[0]) for p in parts])
            out = d_out.cpu().numpy()
            ran.append(what)
            for i, p in enumerate(parts):
                got = out[int(ooff[i]):int(ooff[i]) + out_sizes[i]].tobytes()
                name = what + (": the chunk" if i == 1 else ": neighbour %d" % i)
                blocks = out_sizes[i] // blk_bytes
                if int(recs[i]["status"]) != DEC_OK:
                    fails.append((name, "record status %d" % int(recs[i]["status"])))
                elif int(recs[i]["n_rsi"]) * rsi + int(recs[i]["tail_blocks"]) < blocks:
                    fails.append((name, "record: %d RSIs + %d blocks of %d blocks" % (int(recs[i]["n_rsi"]), int(recs[i]["tail_blocks"]), blocks)))
                elif got != p[3]:
                    fails.append((name, _first_diff(got, p[3], nb, bs)))
            if int(res["status"]) != DEC_OK:
                fails.append((what, "overall status %d" % int(res["status"])))

    # aec_gpu_decode_range_async: a window that starts in the middle of the stretch outside the range, one that ends there
    span = F.out_block_range(v, cfg)
    if span is not None:
        mid = (span[0] + span[1]) // 2 * blk_bytes + blk_bytes // 2 + 1
        R = rsi * blk_bytes
        windows = [(mid, min(out_bytes - mid, R + 2 * blk_bytes + 5)), (max(0, mid - R - 3), mid - max(0, mid - R - 3))]
        d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
        for k, (pos, size) in enumerate(windows):
            what = "range decode, window %s in the stretch" % ("starts", "ends")[k]
            d_out = torch.full((size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            rc = lib.aec_gpu_decode_range_async(codec.ctx, C.byref(codec.p), d_in.data_ptr(), len(stream), d_offs.data_ptr(), n_rsi,
                                                pos, size, d_out.data_ptr() + 16, d_res.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            o = d_out.cpu().numpy()
            if rc != 0 or not ((o[:16] == 0xA5).all() and (o[16 + size:] == 0xA5).all()):
                ran.append(what)
                fails.append((what, "rc %d, or a write outside the window" % rc))
                continue
            check(what, rec(d_res)["status"], o[16:16 + size].tobytes(), full[pos:pos + size])
    codec.close()

    # the libaec ABI: one shot; streaming with the input cut inside the stretch, and with the room handed out block by block
    rc, dec = api.aec_buffer_decode(stream, bps, bs, rsi, flags, out_bytes)
    check("aec_buffer_decode", 0 if rc == H.AEC_OK else 100 - rc, dec)

    def pieces(plan):
        """aec_decode with plan = [(input bytes offered, room offered), ...], the last entry again and again; until
        nothing comes any more"""
        dec = api.Decoder(bps, bs, rsi, flags)
        src, out, pos, rc, k = np.frombuffer(stream, np.uint8), bytearray(), 0, H.AEC_OK, 0
        while rc == H.AEC_OK and len(out) < out_bytes:
            n_in, room = plan[min(k, len(plan) - 1)]
            k += 1
            n_in = min(n_in, src.size - pos)
            room = min(room, out_bytes - len(out))
            rc, used, got = dec.call(src[pos:pos + n_in], room, H.AEC_FLUSH if pos + n_in >= src.size else H.AEC_NO_FLUSH)
            pos += used
            out += got
            if pos >= src.size and n_in == 0 and not got:
                break
        dec.end()
        return rc, bytes(out)

    # every vector: the input cut at a byte of the block in the middle of the stretch outside (three calls)
    mid_blk = nblk // 2 if span is None else (span[0] + span[1] + 1) // 2
    cut = min(len(stream) - 1, max(1, (int(v["blk_bits"][mid_blk]) + 9) // 8))
    rc, dec = pieces([(cut, out_bytes), (len(stream) - cut, out_bytes), (0, out_bytes)])
    check("aec_decode, input cut", 0 if rc == H.AEC_OK else 100 - rc, dec)
    # every vector: room for one block per call -- through the whole vector where it has at most ONE_BLOCK_CALLS blocks,
    # else through so many blocks around the middle of the stretch (the blocks in front in one call, the rest in another)
    lo = 0 if nblk <= ONE_BLOCK_CALLS else min(max(0, mid_blk - ONE_BLOCK_CALLS // 2), nblk - ONE_BLOCK_CALLS)
    plan = [(1 << 30, lo * blk_bytes)] if lo else []
    plan += [(1 << 30, blk_bytes)] * min(nblk, ONE_BLOCK_CALLS) + [(1 << 30, out_bytes)]
    rc, dec = pieces(plan)
    check("aec_decode, room of one block per call", 0 if rc == H.AEC_OK else 100 - rc, dec)
    return ran, fails


@pytest.mark.parametrize("family,cfg", CASES, ids=[F.case_id(f, c) for f, c in CASES])
def test_every_decode_entry(family, cfg):
    """The sum_wraps vectors in 2-byte containers hold one coded data set of 64 KiB (two fundamental sequences of 2^18
    zeros).  It outgrows every ring, so the sequential decoder behind the kernels gives the oracle's bytes and such a
    block never reaches the per-block test; the index walker, whose window of the stream holds 16 KiB, reads it from
    the stream where it lies (aec_idx.hip: k_index; before that it took the end of its window for the end of the
    input, and aec_buffer_decode returned AEC_OK with 62 of 80, 5278 of 6432 and 9230 of 16400 bytes).  The 3-byte
    sum_wraps vectors, whose wrapping block is a few dozen bits long, do reach the test.

    Room for one block per call costs a call of aec_decode per block (some 40 us), so it is bounded by calls:
    ONE_BLOCK_CALLS, which takes every vector whole (the largest has 6214 blocks) except big_table's 65 600 blocks; of
    those it takes 6400 around the middle, the blocks in front in one call and the rest in another -- every RSI of that
    vector leaves and returns, 400 of them block by block.  The cut input is three calls and runs on every vector.

    Run time of the whole file on an MI355X: 4.9 s for its 72 tests (this one: 0.53 s for big_table, 0.27 s and less
    for every other case)."""
    ran, fails = gpu_paths(family, cfg)
    print(F.case_id(family, cfg), ran)
    assert "table decode, output offset 0" in ran and "table decode, output offset 4" in ran and "aec_buffer_decode" in ran
    assert "aec_decode, input cut" in ran and "aec_decode, room of one block per call" in ran
    if 16 <= cfg[2] < 64:
        assert "indexed decode, table bound %d" % F.LANE_TABLE_BOUND in ran
    if cfg[2] == 130 and cfg[3] & F.PP:
        assert any(p.startswith("segment decode") for p in ran)
    if cfg[2] == 512:
        assert "bare decode" in ran and "bare decode, index record" in ran
    if family != "big_table":
        assert "chunks, table" in ran and "chunks, bare" in ran
    if family in ("leave_and_return", "below", "hover", "edge_out", "big_table"):
        assert sum(p.startswith("range decode") for p in ran) == 2
    assert not fails, fails


LONG = [c for c in F.CONFIGS["sum_wraps"] if H.bytes_per_sample(c[0], c[3]) == 2]


@pytest.mark.parametrize("cfg", LONG, ids=[F.case_id("sum_wraps", c) for c in LONG])
def test_input_that_ends_in_a_coded_data_set_longer_than_the_index_window(cfg):
    """The 64 KiB coded data set of a 2-byte sum_wraps vector, cut 40 KiB behind its start: the index walker's window of
    16 KiB ends in front of the end of the input, so the walker reads on from the stream and meets the end there.  The
    record says "the input ended" (pad 1) at the start of that coded data set, with the blocks in front of it; the
    libaec ABI returns what the oracle returns for the same bytes."""
    bps, bs, rsi, flags = cfg
    v = F.vector("sum_wraps", cfg)
    starts = v["blk_bits"].astype(np.int64)
    b = int(np.argmax(np.diff(np.append(starts, v["bits"]))))          # the block of the longest coded data set
    assert (v["bits"] if b + 1 == v["nblk"] else int(starts[b + 1])) - int(starts[b]) > 8 * 60000
    cut = int(starts[b]) // 8 + 40 * 1024
    part = v["stream"][:cut]
    cap = v["nblk"] * bs * H.bytes_per_sample(bps, flags)
    rc_o, dec_o, _ = H.oracle_decode(part, bps, bs, rsi, flags, cap)
    assert rc_o == H.AEC_OK and dec_o == v["bytes"][:len(dec_o)] and len(dec_o) >= b * bs * 2
    codec = gpu.Codec(bps, bs, rsi, flags)
    d_in = torch.zeros(cut + 16, dtype=torch.uint8, device="cuda")
    d_in[:cut] = torch.frombuffer(bytearray(part), dtype=torch.uint8).cuda()
    n_rsi = v["rsi_bits"].size
    d_idx = torch.full((n_rsi + 3,), -1, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    codec.index_async(d_in, cut, 0, d_idx, n_rsi + 1, d_res)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0]
    codec.close()
    print(F.case_id("sum_wraps", cfg), "block", b, "cut", cut, res)
    assert int(res["status"]) == DEC_OK and int(res["pad"]) == 1
    assert int(res["n_rsi"]) * rsi + int(res["tail_blocks"]) == b and int(res["end_bit"]) == int(starts[b])
    rc, dec = api.aec_buffer_decode(part, bps, bs, rsi, flags, cap)
    assert rc == rc_o and dec == dec_o, (rc, len(dec), len(dec_o))


def test_the_issues_stream():
    """the 20 bytes of the issue through the table decode (a lane per RSI) at both alignments and through the ABI"""
    bps, bs, rsi, flags = F.ISSUE_CFG
    want = H.pack_samples(F.ISSUE_SAMPLES, 16, 0).tobytes()
    codec = gpu.Codec(bps, bs, rsi, flags)
    d_in = torch.zeros(36, dtype=torch.uint8, device="cuda")
    d_in[:20] = torch.frombuffer(bytearray(F.ISSUE_STREAM), dtype=torch.uint8).cuda()
    d_offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    for off in (0, 4):
        d_out = torch.zeros(64, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
        codec.decode_async(d_in, 20, d_offs, 1, 2, d_out[off:], d_res)
        assert d_res.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0]["status"] == 0
        got = d_out[off:off + 32].cpu().numpy()
        assert got.tobytes() == want, (off, np.frombuffer(got.tobytes(), "<u2").tolist())
    codec.close()
    rc, dec = api.aec_buffer_decode(F.ISSUE_STREAM, bps, bs, rsi, flags, 32)
    assert rc == 0 and dec == want
