"""aec_gpu_decode_chunks_async (include/aec_gpu.h): a batch of streams of unequal decoded sizes as one decode launch.  The
streams are the oracle's, one per chunk, laid back to back at byte granularity; every chunk's blocks land in a room of its
own at a shuffled 16-byte aligned offset of an output that is 0xA5 before the call, and what comes out must be the input
that was encoded: byte for byte inside the rooms (the real samples of a padded last block), 0xA5 everywhere else.  With
the table built from the oracle's RSI offsets no index pass runs; without it (bare streams) the call finds the same table.

Run as a program (`python tests/test_gpu_decode_chunks.py abi`) the file is the child process of the ABI test: it decodes
batches through aec_buffer_decode_batch and SZ_BatchDecompress and leaves the AEC_ABI_TRACE lines on stderr for the parent
to read."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import helpers  # noqa: E402
from helpers import (AEC_DATA_3BYTE, AEC_DATA_ERROR, AEC_DATA_MSB, AEC_DATA_PREPROCESS as PP, AEC_DATA_SIGNED,  # noqa: E402
                     AEC_NOT_ENFORCE, AEC_OK, craft_overlong_stream, oracle_decode, oracle_encode)

pytestmark = pytest.mark.gpu

C5 = (8, 8, 128, PP)
PARAM_SETS = [                                               # (those of tests/test_gpu_encode_chunks.py)
    C5,
    (16, 16, 64, PP),
    (16, 16, 128, 0),
    (32, 32, 100, PP | AEC_DATA_MSB | AEC_DATA_SIGNED),      # an rsi that is no multiple of 64
    (24, 64, 17, PP | AEC_DATA_3BYTE),
    (12, 24, 5, PP | AEC_NOT_ENFORCE),                       # the generic block size
    (16, 8, 1, PP),                                          # rsi 1
]
GUARD = 256
NONE = (1 << 64) - 1
REDO = 1 << 31


def make_chunk(rng, kind, samples, prm, extra_bytes=0):
    """`samples` samples of a kind, as bytes, with `extra_bytes` of a further sample behind them"""
    bps, bs, rsi, flags = prm
    lo, hi = (-(1 << (bps - 1)), (1 << (bps - 1)) - 1) if flags & AEC_DATA_SIGNED else (0, (1 << bps) - 1)
    if samples == 0:
        return rng.integers(0, 256, size=extra_bytes, dtype=np.uint8)
    if kind == "walk":
        vals = helpers.random_walk_samples(rng, samples, bps, flags)
    elif kind == "fast":                                     # (vectorised: the large batches)
        walk = (lo + hi) // 2 + np.cumsum(rng.integers(-3, 4, size=samples))
        # (held at the ends of the range -- runs of zero blocks -- or wrapped around it -- a rare full-range jump)
        vals = np.clip(walk, lo, hi) if rng.random() < 0.5 else lo + (walk - lo) % (hi - lo + 1)
    elif kind == "const":
        vals = np.full(samples, int(rng.integers(lo, hi + 1)), dtype=np.int64)
    elif kind == "zero":
        vals = np.zeros(samples, dtype=np.int64)
    else:
        vals = rng.integers(lo, hi + 1, size=samples, dtype=np.int64)
    raw = np.frombuffer(helpers.pack_samples(vals, bps, flags), dtype=np.uint8)
    return np.concatenate([raw, rng.integers(0, 256, size=extra_bytes, dtype=np.uint8)]) if extra_bytes else raw.copy()


def awkward_batch(rng, prm):
    """the chunk list of tests/test_gpu_encode_chunks.py's awkward_batch"""
    bps, bs, rsi, flags = prm
    nb = helpers.bytes_per_sample(bps, flags)
    S = bs * rsi
    frac = nb - 1                                            # (8-bit samples have no fractions: an empty chunk then)
    spec = [("walk", 0, 0), ("walk", 1, 0), ("walk", 0, frac), ("walk", bs - 1, 0), ("walk", 64 * bs, 0), ("walk", 65 * bs, 0),
            ("walk", S, 0), ("walk", S + 1, frac)]
    spec += [("const", 3 * bs, 0)] * 5 + [("const", 1, 0)] * 3
    spec += [("zero", 2 * S + 3, 0)]
    spec += [("walk", 0, 0)] * 10
    spec += [("noise", S + 3 * bs, 0), ("walk", 3 * S + 7, 0), ("const", 2, 0), ("walk", 0, frac), ("walk", 129 * bs + 5, 0)]
    return [make_chunk(rng, kind, n, prm, extra) for kind, n, extra in spec]


def expected(chunk, prm):
    """(stream, bits, RSI offsets) of a chunk alone, from the oracle; a chunk without a sample: one zero byte"""
    nb = helpers.bytes_per_sample(prm[0], prm[3])
    if chunk.size < nb:
        return b"\0", 0, []
    rc, enc, _, offs, bits = oracle_encode(chunk, *prm)
    assert rc == AEC_OK and len(enc) == (bits + 7) // 8
    return enc, int(bits), [int(o) for o in offs]


def counts(size, prm):
    bps, bs, rsi, flags = prm
    nb = helpers.bytes_per_sample(bps, flags)
    blocks = (size // nb + bs - 1) // bs
    return blocks, (blocks + rsi - 1) // rsi, bs * nb


class Batch:
    """streams back to back at byte granularity, the table of the oracle's offsets, rooms at shuffled aligned offsets"""

    def __init__(self, prm, chunks, want, rng, announce=None):
        self.prm, self.chunks, self.want = prm, chunks, want
        n = self.n = len(chunks)
        self.out_sizes = np.array([c.size for c in chunks] if announce is None else announce, dtype=np.uint64)
        self.in_sizes = np.array([len(w[0]) for w in want], dtype=np.uint64)
        self.in_off = np.zeros(n, dtype=np.uint64)
        if n:
            self.in_off[1:] = np.cumsum(self.in_sizes[:-1], dtype=np.uint64)
        self.in_bytes = int(self.in_sizes.sum())
        blob = np.frombuffer(b"".join(w[0] for w in want), dtype=np.uint8)
        self.blob = np.concatenate([blob, np.zeros((-blob.size) % 4 + 16, dtype=np.uint8)])
        self.table, self.entry0, self.item0 = [], [], []
        items = 0
        for i in range(n):
            rsis = counts(int(self.out_sizes[i]), prm)[1]
            offs = want[i][2]
            self.entry0.append(len(self.table))
            self.item0.append(items)
            base = 8 * int(self.in_off[i])
            # (a chunk that announces more RSIs than its stream holds: the entries of the missing ones are never read)
            self.table += [base + o for o in offs][:rsis] + [0] * (rsis - len(offs)) + [base + want[i][1]]
            items += rsis
        self.items = items
        # rooms: shuffled, 16-byte aligned, gaps of 0 to 48 bytes
        self.out_off, at = np.zeros(n, dtype=np.uint64), 16 * int(rng.integers(0, 3))
        for i in rng.permutation(n):
            self.out_off[i] = at
            blocks, _, blk = counts(int(self.out_sizes[i]), prm)
            at += (blocks * blk + 15) // 16 * 16 + 16 * int(rng.integers(0, 4))
        self.out_len = at + GUARD

    def run(self, codec, have_table):
        import torch
        from libaec_amd import gpu
        d_in = torch.from_numpy(self.blob).cuda()
        tab = np.array(self.table if have_table else [0] * len(self.table), dtype=np.int64)
        d_tab = torch.from_numpy(tab).cuda()
        d_out = torch.full((self.out_len,), 0xA5, dtype=torch.uint8, device="cuda")
        d_rec = torch.full((max(self.n, 1) * 40,), 0xEE, dtype=torch.uint8, device="cuda")
        d_res = torch.full((40,), 0xEE, dtype=torch.uint8, device="cuda")
        plan = codec.decode_chunks_plan(self.out_sizes)
        assert plan["items"] == self.items and plan["rsi_entries"] == len(self.table)
        rc = codec.decode_chunks_async(d_in, self.in_bytes, None if have_table else self.in_off, None if have_table else self.in_sizes,
                                       self.out_off, self.out_sizes, d_tab, have_table, d_out, d_rec, d_res)
        assert rc == 0
        torch.cuda.synchronize()
        return (d_out.cpu().numpy(), d_rec.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[:self.n],
                d_res.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0], d_tab.cpu().numpy())

    def check_output(self, out, skip=()):
        """every chunk's real samples, and 0xA5 wherever no room is"""
        nb = helpers.bytes_per_sample(self.prm[0], self.prm[3])
        untouched = np.ones(out.size, dtype=bool)
        for i, c in enumerate(self.chunks):
            blocks, _, blk = counts(int(self.out_sizes[i]), self.prm)
            at = int(self.out_off[i])
            untouched[at:at + blocks * blk] = False
            if i in skip:
                continue
            whole = c.size - c.size % nb
            assert out[at:at + whole].tobytes() == c[:whole].tobytes(), f"chunk {i} of {self.n} ({c.size} bytes)"
        assert np.all(out[untouched] == 0xA5), "bytes outside the chunks' rooms were written"

    def stream_blocks(self, i):
        """the complete blocks chunk i's stream holds within the RSIs the chunk announces, by the oracle's decoder: a stream
        that ends in a run of zero blocks coded as "the rest of the segment" holds more than were encoded"""
        blocks, rsis, blk = counts(int(self.out_sizes[i]), self.prm)
        if not blocks:
            return 0
        rc, dec, _ = oracle_decode(self.want[i][0], *self.prm, rsis * self.prm[2] * blk)
        return len(dec) // blk

    def check_records(self, rec, res, skip=(), redo=False, bare=False):
        """with the table: what the chunks announce; bare: what the streams hold"""
        rsi = self.prm[2]
        for i, c in enumerate(self.chunks):
            if i in skip:
                continue
            blocks = self.stream_blocks(i) if bare else counts(c.size, self.prm)[0]
            assert (int(rec[i]["n_rsi"]), int(rec[i]["tail_blocks"]), int(rec[i]["status"])) == (blocks // rsi, blocks % rsi, 0), (i, rec[i])
        if not skip:
            assert int(res["status"]) == 0 and int(res["bad_rsi"]) == NONE, res
        if redo is not None:
            assert bool(int(res["pad"]) & REDO) == redo


def decode_both_ways(prm, chunks, rng, codec=None, modes=(1, 0)):
    from libaec_amd import gpu
    want = [expected(c, prm) for c in chunks]
    b = Batch(prm, chunks, want, rng)
    codec = codec or gpu.Codec(*prm)
    for have_table in modes:
        out, rec, res, tab = b.run(codec, have_table)
        b.check_output(out)
        b.check_records(rec, res, bare=not have_table)
        if not have_table:
            # the table the call leaves: the oracle's offsets shifted by the chunk's base (the closing entries are not written)
            for i in range(b.n):
                k = len(want[i][2])
                assert tab[b.entry0[i]:b.entry0[i] + k].tolist() == b.table[b.entry0[i]:b.entry0[i] + k], f"RSI table, chunk {i}"
    return codec, b


@pytest.mark.parametrize("prm", PARAM_SETS, ids=lambda p: "-".join(str(x) for x in p))
def test_awkward_batch_with_the_table_and_bare(prm):
    rng = np.random.default_rng(sum(prm))
    chunks = awkward_batch(rng, prm)
    codec, _ = decode_both_ways(prm, chunks, rng)
    decode_both_ways(prm, chunks[::-1], rng, codec=codec)      # the same context again: the descriptors of the call before are gone
    codec.close()


@pytest.mark.parametrize("prm", [C5, (16, 16, 64, PP), (16, 8, 1, PP)], ids=lambda p: "-".join(str(x) for x in p))
def test_a_bare_stream_shorter_than_announced(prm):
    """a chunk announces two RSIs and three blocks more than its stream holds: its record says what was found, the blocks
    found are exact, and the neighbours -- whose streams begin on the byte behind it -- come out exact"""
    from libaec_amd import gpu
    rng = np.random.default_rng(7 + sum(prm))
    bps, bs, rsi, flags = prm
    nb = helpers.bytes_per_sample(bps, flags)
    chunks = awkward_batch(rng, prm)
    want = [expected(c, prm) for c in chunks]
    liars = [6, 7, 17, 28]                                   # one RSI exactly; one RSI and a sample; none; three RSIs and seven samples
    announce = [c.size for c in chunks]
    for i in liars:
        announce[i] += (2 * rsi + 3) * bs * nb
    b = Batch(prm, chunks, want, rng, announce=announce)
    codec = gpu.Codec(*prm)
    out, rec, res, _ = b.run(codec, 0)
    b.check_output(out)                                      # (every chunk's real samples, the liars' too)
    b.check_records(rec, res, bare=True)                     # (n_rsi / tail_blocks of what the streams hold: below the announced)
    for i in liars:
        blocks, rsis, _ = counts(announce[i], prm)
        assert counts(chunks[i].size, prm)[0] <= int(rec[i]["n_rsi"]) * rsi + int(rec[i]["tail_blocks"]) < blocks
    codec.close()


def test_round_trip_from_the_encoders_output_and_table():
    """encode_chunks(want_offsets=True) -> decode_chunks with that table, straight from the encoder's buffers"""
    import torch
    from libaec_amd import gpu
    prm = (16, 16, 64, PP)
    rng = np.random.default_rng(21)
    S = prm[1] * prm[2]
    chunks = [make_chunk(rng, "fast", int(rng.integers(0, 3 * S + 8)) if rng.random() > 0.1 else 0, prm, int(rng.integers(0, 2)))
              for _ in range(300)]
    sizes = np.array([c.size for c in chunks], dtype=np.uint64)
    offsets = np.zeros(len(chunks), dtype=np.uint64)
    offsets[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    host = np.zeros(int(offsets[-1] + sizes[-1]) + 32, dtype=np.uint8)
    for o, c in zip(offsets, chunks):
        host[int(o):int(o) + c.size] = c
    codec = gpu.Codec(*prm)
    d_enc, rec, d_tab, res = codec.encode_chunks(torch.from_numpy(host).cuda(), offsets, sizes, want_offsets=True)
    assert not int(res["overflow"])
    d_out, out_off, recs, one = codec.decode_chunks(d_enc, int(res["total_bits"]) // 8, sizes, d_table=d_tab)
    out = d_out.cpu().numpy()
    for i, c in enumerate(chunks):
        whole = c.size - c.size % 2
        assert out[int(out_off[i]):int(out_off[i]) + whole].tobytes() == c[:whole].tobytes(), i
    assert np.all(recs["status"] == 0) and int(one["status"]) == 0 and int(one["bad_rsi"]) == NONE
    # ... and bare, from the records' stream positions
    d_out2, _, recs2, one2 = codec.decode_chunks(d_enc, int(res["total_bits"]) // 8, sizes, in_offsets=rec[:, 0] // 8,
                                                 in_sizes=np.maximum((rec[:, 1] + 7) // 8, 1))
    assert torch.equal(d_out2, d_out) and np.all(recs2["status"] == 0) and int(one2["status"]) == 0
    codec.close()


def ragged_batch(rng, prm, n, max_rsis):
    bps, bs, rsi, flags = prm
    S = bs * rsi
    return [make_chunk(rng, "fast", int(rng.integers(1, max_rsis + 1)) * S - int(rng.integers(0, S)), prm) for _ in range(n)]


def test_the_lane_kernel_of_config_5_above_8192_items():
    """dec_wave_wanted hands batches of at most 8192 items with rsi >= 16 to the wave kernel: 8200 items and more of config 5
    (chunks of 1 to 40 RSIs with ragged tails, about 9 MB) take k_decode<CHUNKS> with the templated block size"""
    rng = np.random.default_rng(40)
    chunks = ragged_batch(rng, C5, 430, 40)
    while sum(counts(c.size, C5)[1] for c in chunks) < 8200:
        chunks += ragged_batch(rng, C5, 10, 40)
    codec, b = decode_both_ways(C5, chunks, rng)
    assert b.items >= 8200
    codec.close()


@pytest.mark.parametrize("prm", [(16, 16, 5, PP), (12, 24, 5, PP | AEC_NOT_ENFORCE)], ids=lambda p: "-".join(str(x) for x in p))
def test_the_lane_kernel_with_short_rsis(prm):
    """rsi 5: the lane kernel whatever the number of items, with a templated block size and with the generic one"""
    rng = np.random.default_rng(5 + prm[1])
    chunks = ragged_batch(rng, prm, 400, 9) + [make_chunk(rng, "walk", 0, prm)] * 3
    codec, _ = decode_both_ways(prm, [chunks[i] for i in rng.permutation(len(chunks))], rng)
    codec.close()


@pytest.mark.parametrize("bps,bs,rsi,n_rsi,long_hi,redo", [(16, 16, 8, 30, 400, True), (8, 8, 128, 3, 200, None)])
def test_overlong_coded_data_sets_in_one_chunk_of_a_batch(bps, bs, rsi, n_rsi, long_hi, redo):
    """one chunk is a stream like those of test_overlong_coded_data_sets_of_a_foreign_encoder (helpers.craft_overlong_stream).
    With rsi 8 the lane kernel takes the batch: coded data sets of 3000 bits on average (15 fundamental sequences of up to
    400 zeros) outgrow a lane's ring of 1024 bits, so the batch goes through k_decode_redo<CHUNKS>, comes out exact, and
    bit 31 of the overall record's pad says so.  With rsi 128 the wave kernel takes it, whose window of the stream holds
    such coded data sets: exact either way, the bit is not asserted."""
    from libaec_amd import gpu
    prm = (bps, bs, rsi, PP)
    rng = np.random.default_rng(bps + bs)
    enc = craft_overlong_stream(rng, bps, bs, rsi, n_rsi, {8: 3, 16: 4}[bps], 0.05, long_hi)
    nbytes = n_rsi * rsi * bs * helpers.bytes_per_sample(bps, PP)
    rc, dec, _ = oracle_decode(enc, bps, bs, rsi, PP, nbytes)
    assert rc == AEC_OK and len(dec) == nbytes
    chunks = awkward_batch(rng, prm)[:12]
    want = [expected(c, prm) for c in chunks]
    chunks.insert(5, np.frombuffer(dec, dtype=np.uint8))
    want.insert(5, (enc, 8 * len(enc), [0] * n_rsi))           # (the crafted stream comes without RSI offsets: bare mode finds them)
    b = Batch(prm, chunks, want, rng)
    codec = gpu.Codec(*prm)
    out, rec, res, _ = b.run(codec, 0)
    b.check_output(out)
    b.check_records(rec, res, redo=redo, bare=True)
    codec.close()


def test_a_damaged_chunk_is_named_and_its_neighbours_are_exact():
    """the damage is chosen on the CPU so that the oracle's decoder says AEC_DATA_ERROR for that chunk: bytes of its last RSI
    are cleared until it does.  One batch, run once."""
    from libaec_amd import gpu
    prm = C5
    rng = np.random.default_rng(66)
    chunks = awkward_batch(rng, prm)
    victim = 28                                              # three RSIs and seven samples
    want = [expected(c, prm) for c in chunks]
    enc, bits, offs = want[victim]
    assert len(offs) == 4
    lo, hi = offs[2] // 8 + 2, offs[3] // 8 - 40
    for trial in range(400):
        at = int(rng.integers(lo, hi))
        bad = bytearray(enc)
        bad[at:at + 32] = bytes(32)
        rc, _, _ = oracle_decode(bytes(bad), *prm, chunks[victim].size)
        if rc == AEC_DATA_ERROR:
            break
    else:
        raise AssertionError("no damage found that the oracle's decoder calls a data error")
    want[victim] = (bytes(bad), bits, offs)
    b = Batch(prm, chunks, want, rng)
    codec = gpu.Codec(*prm)
    out, rec, res, _ = b.run(codec, 1)
    b.check_output(out, skip=(victim,))
    b.check_records(rec, res, skip=(victim,))
    assert int(rec[victim]["status"]) == 2
    assert int(res["status"]) == 2 and b.item0[victim] <= int(res["bad_rsi"]) < b.item0[victim] + 4, res
    # the RSIs of the damaged chunk in front of the damage are exact as well
    at = int(b.out_off[victim])
    assert out[at:at + 2 * 1024].tobytes() == chunks[victim][:2 * 1024].tobytes()
    codec.close()


def test_refusals_and_the_empty_batch():
    import torch
    from libaec_amd import gpu
    codec = gpu.Codec(*C5)
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d_tab = torch.zeros(16, dtype=torch.int64, device="cuda")
    d_rec = torch.zeros(80, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    sizes = np.array([100, 100], dtype=np.uint64)

    def call(c, out_off, n_sizes):
        return c.decode_chunks_async(d, 64, None, None, np.array(out_off, dtype=np.uint64), n_sizes, d_tab, 1, d, d_rec, d_res)
    assert call(codec, [0, 112], sizes[:0]) == 0
    assert call(codec, [0, 104], sizes) == helpers.AEC_CONF_ERROR            # an offset that is no multiple of 16
    bad = gpu.Codec(*C5)
    bad.p = gpu.Params(8, 7, 128, PP)                        # (an odd block size: refused for decoding as well)
    assert call(bad, [0, 112], sizes[:0]) == helpers.AEC_CONF_ERROR
    assert call(bad, [0, 112], sizes) == helpers.AEC_CONF_ERROR
    torch.cuda.synchronize()
    bad.close()
    codec.close()


def test_through_the_abi_unequal_batches_take_the_chunks_path_and_equal_ones_the_old():
    env = dict(os.environ, AEC_ABI_TRACE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "abi"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    paths = [line.rsplit("path ", 1)[1].strip() for line in r.stderr.splitlines() if "decode batch:" in line]
    assert paths == ["chunks", "batch", "chunks", "batch"], paths
    assert r.stdout.count("same as the inputs") == 4, r.stdout


def abi_child():
    import torch
    assert torch.cuda.is_available()
    from fuzz_batch_gpu import batch
    from libaec_amd import api, szip
    lib = api.library()
    rng = np.random.default_rng(3)
    prm = (16, 16, 64, PP)
    rsi_b = 16 * 64 * 2
    for name, sizes in (("unequal", [int(rng.integers(2, 6 * rsi_b)) // 2 * 2 for _ in range(80)]), ("equal", [3 * rsi_b - 64] * 80)):
        chunks = [make_chunk(rng, "fast", s // 2, prm) for s in sizes]
        streams = [np.frombuffer(expected(c, prm)[0], dtype=np.uint8) for c in chunks]
        rc, got, st = batch(lib, "aec_buffer_decode_batch", prm, streams, sizes)
        assert rc == AEC_OK and st == [AEC_OK] * len(chunks), (name, rc, st)
        for i, c in enumerate(chunks):
            assert got[i].tobytes() == c.tobytes(), (name, i)
        print(f"aec_buffer_decode_batch, 80 {name} chunks: same as the inputs")
    # SZIP: 8-bit pixels, 8 per block, scan lines of 256 (an RSI of 32 blocks), chunks of whole scan lines
    opts, sz_prm = szip.SZ_NN_OPTION_MASK | szip.SZ_RAW_OPTION_MASK, (8, 8, 32, PP)
    for name, lines in (("unequal", [int(rng.integers(1, 40)) for _ in range(96)]), ("equal", [12] * 96)):
        chunks = [make_chunk(rng, "fast", 256 * k, sz_prm) for k in lines]
        streams = [expected(c, sz_prm)[0] for c in chunks]
        rc, got, st = szip.decompress_batch(streams, [c.size for c in chunks], opts, 8, 8, 256)
        assert rc == szip.SZ_OK and st == [szip.SZ_OK] * len(chunks), (name, rc, st)
        for i, c in enumerate(chunks):
            assert got[i] == c.tobytes(), (name, i)
        print(f"SZ_BatchDecompress, 96 {name} chunks: same as the inputs")
    return 0


if __name__ == "__main__":
    sys.exit(abi_child() if sys.argv[1:] == ["abi"] else 2)
