"""aec_gpu_index_chunks_async / aec_gpu_set_chunks_index (include/aec_gpu.h): the index pass of a batch of bare streams,
with the every-bit scheme over the batch (libaec_amd/csrc/aec_bsmall.h) in front of the serial walker.  The batches are
those of tests/test_bsmall_emul.py (tests/bsmall_cases.py, same seeds): oracle-encoded streams back to back at odd byte
offsets.  Whichever scheme delivers a stream, its record and the specified entries of its part of the table must be
byte for byte the same and the oracle's; under EVERY_BIT every stream within the limits must have been delivered by the
every-bit scheme -- d_how says so -- and none outside them."""
import numpy as np
import pytest

import bsmall_cases as cases
import helpers

pytestmark = pytest.mark.gpu

SENTINEL = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import gpu, szgpu
    return torch, gpu, szgpu


@pytest.fixture(scope="module")
def batches():
    return {name: cases.make_batch(name) for name in cases.CASES}


def index(mods, codec, b, how, round_bits=0, d_in=None):
    """-> (table as uint64 with SENTINEL where nothing was written, records, how per stream)"""
    torch, gpu, _ = mods
    codec.set_chunks_index(how, round_bits)
    d_in = torch.from_numpy(b.buf).cuda() if d_in is None else d_in
    entries = sum(r + 1 for r in b.rsis)
    d_table = torch.full((entries + 8,), SENTINEL, dtype=torch.int64, device="cuda")
    d_rec = torch.full((40 * b.n,), 0xA5, dtype=torch.uint8, device="cuda")
    d_how = torch.full((b.n,), 7, dtype=torch.int32, device="cuda")
    assert codec.index_chunks_async(d_in, b.in_bytes, b.in_off, b.in_sizes, b.out_sizes, d_table, d_rec, d_how) == 0
    torch.cuda.synchronize()
    return d_table.cpu().numpy(), d_rec.cpu().numpy().view(gpu.DEC_RESULT_DTYPE), d_how.cpu().numpy()


def specified(b, table, rec, i):
    """the entries of chunk i the contract specifies: 0 .. n_rsi - 1, and n_rsi where there is a tail"""
    e0 = cases.table_entry0(b, i)
    return table[e0:e0 + int(rec[i]["n_rsi"]) + (1 if rec[i]["tail_blocks"] else 0)]


def assert_same(b, a, other, what):
    """records byte for byte, specified entries, nothing outside the chunks' entries"""
    (ta, ra, _), (tb, rb, _) = a, other
    assert ra.tobytes() == rb.tobytes(), what
    for i in range(b.n):
        assert np.array_equal(specified(b, ta, ra, i), specified(b, tb, rb, i)), (what, i)
    entries = sum(r + 1 for r in b.rsis)
    assert np.all(ta[entries:] == SENTINEL) and np.all(tb[entries:] == SENTINEL), what


def assert_oracle(b, got, streams):
    table, rec, _ = got
    for i in streams:
        n_rsi, tail = cases.expected_record(b, i)
        assert (int(rec[i]["n_rsi"]), int(rec[i]["tail_blocks"]), int(rec[i]["status"]), int(rec[i]["pad"])) == (n_rsi, tail, 0, 0), i
        assert int(rec[i]["bad_rsi"]) == (1 << 64) - 1
        assert [int(x) for x in specified(b, table, rec, i)] == b.starts[i][:n_rsi + (1 if tail else 0)], i


@pytest.mark.parametrize("name", list(cases.CASES))
def test_three_ways_one_result(mods, batches, name):
    torch, gpu, _ = mods
    b = batches[name]
    codec = gpu.Codec(*b.params)
    serial = index(mods, codec, b, gpu.CHUNKS_INDEX_SERIAL)
    every = index(mods, codec, b, gpu.CHUNKS_INDEX_EVERY_BIT)
    planned = index(mods, codec, b, gpu.CHUNKS_INDEX_PLANNED)
    assert_oracle(b, serial, range(b.n))
    assert_same(b, every, serial, "every bit / serial")
    assert_same(b, planned, serial, "planned / serial")
    want = [1 if cases.within(b, i) else 0 for i in range(b.n)]
    assert every[2].tolist() == want                       # no stream has quietly gone to the walker
    assert not serial[2].any()
    assert all(p <= w for p, w in zip(planned[2].tolist(), want))
    plan = codec.index_chunks_plan(b.in_sizes, b.out_sizes, gpu.CHUNKS_INDEX_EVERY_BIT, 0)
    assert plan["taken"] == sum(want) and plan["rsi_entries"] == sum(r + 1 for r in b.rsis)
    assert int(planned[2].sum()) == codec.index_chunks_plan(b.in_sizes, b.out_sizes, gpu.CHUNKS_INDEX_PLANNED, 0)["taken"]
    # many rounds: identical results
    for rb in (4096, max((8 * int(s) + 1 + 1023) // 1024 * 1024 for s in b.in_sizes)):
        rounds = index(mods, codec, b, gpu.CHUNKS_INDEX_EVERY_BIT, rb)
        assert_same(b, rounds, serial, f"rounds of {rb}")
        assert rounds[2].tolist() == [1 if cases.within(b, i, rb) else 0 for i in range(b.n)]
        plan = codec.index_chunks_plan(b.in_sizes, b.out_sizes, gpu.CHUNKS_INDEX_EVERY_BIT, rb)
        assert plan["table_bits"] <= rb and (rb == 4096 or plan["taken"] < 2 or plan["rounds"] > 1)
    codec.close()


def test_damaged_streams_are_the_walkers_and_spoil_no_neighbour(mods, batches):
    """a flipped bit in a coded data set's header, a stream cut inside a coded data set, a stream shorter than announced"""
    import copy
    torch, gpu, _ = mods
    b = copy.deepcopy(batches["16/16/16 PP|MSB short last"])
    flipped, cut, short = 4, 7, 9
    # (the header of the coded data set RSI 2 of the stream begins with: its option id)
    at = b.starts[flipped][2]
    b.buf[at // 8] ^= 0x80 >> (at % 8)
    b.in_sizes[cut] -= 5
    b.out_sizes[short] *= 2
    announced = (int(b.out_sizes[short]) // 2 + 15) // 16
    b.rsis[short] = (announced + 15) // 16
    codec = gpu.Codec(*b.params)
    serial = index(mods, codec, b, gpu.CHUNKS_INDEX_SERIAL)
    every = index(mods, codec, b, gpu.CHUNKS_INDEX_EVERY_BIT)
    planned = index(mods, codec, b, gpu.CHUNKS_INDEX_PLANNED)
    assert_same(b, every, serial, "every bit / serial")
    assert_same(b, planned, serial, "planned / serial")
    # what the walker says of the three
    rec = serial[1]
    whole = copy.deepcopy(batches["16/16/16 PP|MSB short last"])
    assert int(rec[cut]["n_rsi"]) < whole.rsis[cut] and int(rec[cut]["status"]) == 0
    assert (int(rec[short]["n_rsi"]), int(rec[short]["tail_blocks"])) == cases.expected_record(whole, short)
    assert int(rec[flipped]["n_rsi"]) != whole.rsis[flipped] or int(rec[flipped]["status"]) != 0 or \
        [int(x) for x in specified(b, serial[0], rec, flipped)] != whole.starts[flipped][:len(specified(b, serial[0], rec, flipped))]
    good = [i for i in range(b.n) if i not in (flipped, cut, short)]
    assert_oracle(b, every, good)
    assert all(every[2][i] == 1 for i in good)
    codec.close()


def test_bare_decode_and_the_table_fed_back(mods, batches):
    torch, gpu, _ = mods
    for name in ("16/16/16 PP|MSB short last", "16/8/64 PP zero runs", "PAD_RSI"):
        b = batches[name]
        bps, bs, rsi, flags = b.params
        nb = helpers.bytes_per_sample(bps, flags)
        codec = gpu.Codec(*b.params)
        codec.set_chunks_index(gpu.CHUNKS_INDEX_EVERY_BIT)
        d_in = torch.from_numpy(b.buf).cuda()
        d_out, ooff, rec, res = codec.decode_chunks(d_in, b.in_bytes, b.out_sizes, in_offsets=b.in_off, in_sizes=b.in_sizes)
        assert int(res["status"]) == 0 and not rec["status"].any()
        out = d_out.cpu().numpy()
        for i in range(b.n):
            assert out[int(ooff[i]):int(ooff[i]) + len(b.raw[i])].tobytes() == b.raw[i], (name, i)
        # index once, read with the table ever after
        d_table, irec, how = codec.index_chunks(d_in, b.in_bytes, b.out_sizes, b.in_off, b.in_sizes)
        assert how.tolist() == [1 if cases.within(b, i) else 0 for i in range(b.n)]
        # (the entry behind a chunk's last RSI is not read; a short last RSI is the chunk's last item)
        d_out2, ooff2, rec2, res2 = codec.decode_chunks(d_in, b.in_bytes, b.out_sizes, d_table=d_table)
        assert int(res2["status"]) == 0 and np.array_equal(ooff, ooff2)
        out2 = d_out2.cpu().numpy()
        for i in range(b.n):
            assert out2[int(ooff[i]):int(ooff[i]) + len(b.raw[i])].tobytes() == b.raw[i], (name, i)
        codec.close()


def test_szip_float32_chunks_without_a_table(mods):
    """float32 pixels in byte planes, lines of 1000 pixels, every chunk with a partial last line"""
    torch, gpu, szgpu = mods
    NN, RAW = 32, 128
    rng = np.random.default_rng(18)
    sizes = [2501 * 4, 1203 * 4, 40000, 777 * 4, 16 * 4, 9001 * 4]
    chunks = [np.cumsum(rng.normal(0, 0.01, size=s // 4)).astype("<f4").view(np.uint8) for s in sizes]
    src_off = np.zeros(len(sizes), dtype=np.uint64)
    src_off[1:] = np.cumsum(sizes[:-1])
    d_src = torch.from_numpy(np.concatenate(chunks)).cuda()
    codec = szgpu.SzCodec(NN | RAW, 32, 16, 1000)
    d_enc, rec, d_table, _ = codec.compress_chunks(d_src, src_off, np.array(sizes, dtype=np.uint64), want_table=True)
    in_off = (rec["base_bits"] // 8).astype(np.uint64)
    in_sizes = np.maximum((rec["bits"] + 7) // 8, 1).astype(np.uint64)
    in_bytes = int((in_off + in_sizes).max())
    results = {}
    for how in (gpu.CHUNKS_INDEX_SERIAL, gpu.CHUNKS_INDEX_EVERY_BIT):
        codec.set_chunks_index(how)
        d_dst, recs, res = codec.decompress_chunks(d_enc, in_bytes, np.array(sizes, dtype=np.uint64), in_offsets=in_off, in_sizes=in_sizes)
        assert int(res["status"]) == 0 and not recs["status"].any()
        assert d_dst.cpu().numpy().tobytes() == b"".join(c.tobytes() for c in chunks)
        results[how] = recs
    assert results[gpu.CHUNKS_INDEX_SERIAL].tobytes() == results[gpu.CHUNKS_INDEX_EVERY_BIT].tobytes()
    codec.close()


def test_what_the_context_holds_and_the_argument_checks(mods, batches):
    torch, gpu, _ = mods
    b = batches["32/16/5 PP|SIGNED"]
    codec = gpu.Codec(*b.params)
    assert codec.held_bytes() == 0
    d_in = torch.from_numpy(b.buf).cuda()
    for how, rb in ((gpu.CHUNKS_INDEX_EVERY_BIT, 0), (gpu.CHUNKS_INDEX_EVERY_BIT, 1 << 16), (gpu.CHUNKS_INDEX_SERIAL, 0)):
        codec.trim(0)
        index(mods, codec, b, how, rb, d_in)
        plan = codec.index_chunks_plan(b.in_sizes, b.out_sizes, how, rb)
        desc = (40 * (b.n + 1) + 255) // 256 * 256                 # the descriptors, with the room the context adds
        assert plan["workspace_bytes"] <= codec.held_bytes() <= (desc + desc // 4 + 255) // 256 * 256 + plan["workspace_bytes"]
        assert (plan["workspace_bytes"] == 0) == (how == gpu.CHUNKS_INDEX_SERIAL)
    codec.trim(0)
    assert codec.held_bytes() == 0
    # n_chunks == 0: AEC_OK, nothing enqueued; the checks of the bare decode
    empty = np.zeros(0, dtype=np.uint64)
    d_table = torch.zeros(8, dtype=torch.int64, device="cuda")
    d_rec = torch.zeros(40 * b.n, dtype=torch.uint8, device="cuda")
    assert codec.index_chunks_async(d_in, b.in_bytes, empty, empty, empty, d_table, d_rec) == 0
    assert codec.held_bytes() == 0
    beyond = b.in_sizes.copy()
    beyond[-1] += 1
    assert codec.index_chunks_async(d_in, b.in_bytes, b.in_off, beyond, b.out_sizes, d_table, d_rec) == helpers.AEC_CONF_ERROR
    assert codec.index_chunks_async(d_in[1:], b.in_bytes - 1, b.in_off, b.in_sizes, b.out_sizes, d_table, d_rec) == helpers.AEC_CONF_ERROR
    assert codec.index_chunks_async(d_in, b.in_bytes, b.in_off, b.in_sizes, b.out_sizes, None, d_rec) == helpers.AEC_CONF_ERROR
    assert codec.index_chunks_async(d_in, b.in_bytes, b.in_off, b.in_sizes, b.out_sizes, d_table, None) == helpers.AEC_CONF_ERROR
    codec.close()
