"""The device memory an aec_gpu context holds for its own purposes (include/aec_gpu.h: aec_gpu_held_bytes, aec_gpu_trim):
it grows with the need of a call alone, a call that finds room reallocates nothing, a trim to the total frees nothing, a
trim to 0 frees everything, and whatever was grown, kept, trimmed or grown again the streams and the decoded bytes are
exact.  One sequence of calls, sequence(), walks a context through the chunk calls (whose descriptors go through two pinned
buffers taken in turn), the batch decodes and a window decode through the context's workspace; run as a program the file
prints the held bytes after every step of it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import AEC_DATA_PREPROCESS as PP  # noqa: E402
from test_gpu_decode_chunks import NONE, expected, make_chunk  # noqa: E402

pytestmark = pytest.mark.gpu

WIDE = (16, 16, 64, PP)
TINY = (8, 8, 1, PP)              # a few bytes per chunk


def bind(lib):
    vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
    lib.aec_gpu_held_bytes.restype = sz
    lib.aec_gpu_held_bytes.argtypes = [vp]
    lib.aec_gpu_trim.restype = None
    lib.aec_gpu_trim.argtypes = [vp, sz]
    lib.aec_gpu_decode_range_async.restype = C.c_int
    lib.aec_gpu_decode_range_async.argtypes = [vp, vp, vp, sz, vp, u64, u64, u64, vp, vp, vp]


class Chunks:
    """chunks back to back at 16-byte aligned offsets on the device, and the oracle's stream of each alone"""

    def __init__(self, prm, chunks):
        import torch
        self.prm, self.chunks = prm, chunks
        self.want = [expected(c, prm) for c in chunks]
        self.sizes = np.array([c.size for c in chunks], dtype=np.uint64)
        self.offsets = np.zeros(len(chunks), dtype=np.uint64)
        self.offsets[1:] = np.cumsum((self.sizes[:-1] + 15) // 16 * 16)
        host = np.zeros(int(self.offsets[-1] + self.sizes[-1]) + 32, dtype=np.uint8)
        for o, c in zip(self.offsets, chunks):
            host[int(o):int(o) + c.size] = c
        self.d_in = torch.from_numpy(host).cuda()

    def encode(self, codec):
        """one encode_chunks call; the streams are the oracle's.  Returns what the call returned."""
        got = codec.encode_chunks(self.d_in, self.offsets, self.sizes, want_offsets=True)
        d_out, rec, d_tab, res = got
        need = sum(len(w[0]) for w in self.want)
        assert not int(res["overflow"]) and int(res["total_bits"]) == need * 8
        assert d_out[:need].cpu().numpy().tobytes() == b"".join(w[0] for w in self.want)
        assert rec[:, 1].tolist() == [w[1] for w in self.want]
        return got

    def decode(self, codec, d_enc, rec, d_tab, res):
        """decode_chunks of the encoder's output, with its table and bare: the chunks' whole samples come back"""
        nb = 2 if self.prm[0] > 8 else 1
        in_bytes = int(res["total_bits"]) // 8
        for bare in (False, True):
            kw = dict(in_offsets=rec[:, 0] // 8, in_sizes=np.maximum((rec[:, 1] + 7) // 8, 1)) if bare else dict(d_table=d_tab)
            d_out, out_off, recs, one = codec.decode_chunks(d_enc, in_bytes, self.sizes, **kw)
            out = d_out.cpu().numpy()
            for i, c in enumerate(self.chunks):
                whole = c.size - c.size % nb
                assert out[int(out_off[i]):int(out_off[i]) + whole].tobytes() == c[:whole].tobytes(), (bare, i)
            assert np.all(recs["status"] == 0) and int(one["status"]) == 0 and int(one["bad_rsi"]) == NONE


def three_chunks(rng, prm):
    """no byte, one RSI and one sample, three blocks"""
    bps, bs, rsi, _ = prm
    return Chunks(prm, [make_chunk(rng, "fast", n, prm) for n in (0, bs * rsi + 1, 3 * bs)])


def encode_alone(codec, batch):
    """Codec.encode of every chunk that holds a sample, alone, through the same context: the batch's streams again"""
    for i, c in enumerate(batch.chunks):
        if c.size:
            at = int(batch.offsets[i])
            d_out, nbytes, bits, _, _ = codec.encode(batch.d_in[at:at + c.size])
            assert bits == batch.want[i][1] and d_out[:nbytes].cpu().numpy().tobytes() == batch.want[i][0], i


def window(codec, batch, i):
    """aec_gpu_decode_range_async over chunk i's stream: from the middle of a block of its first RSI to the middle of a block
    of its third, so that the blocks go through the context's workspace"""
    import torch
    bps, bs, rsi, _ = batch.prm
    enc, _, offs = batch.want[i]
    assert len(offs) >= 3 and batch.chunks[i].size == len(offs) * rsi * bs * 2
    blk, R = bs * 2, rsi * bs * 2
    pos, size = 5 * blk + 6, 2 * R + 3 * blk + 1
    stream = np.frombuffer(enc, dtype=np.uint8)
    d_in = torch.from_numpy(np.concatenate([stream, np.zeros((-stream.size) % 4 + 16, dtype=np.uint8)])).cuda()
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_out = torch.full((size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    rc = codec.lib.aec_gpu_decode_range_async(codec.ctx, C.byref(codec.p), d_in.data_ptr(), len(enc), d_off.data_ptr(), len(offs),
                                              pos, size, d_out.data_ptr(), d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == 0 and out[:size].tobytes() == batch.chunks[i][pos:pos + size].tobytes() and np.all(out[size:] == 0xA5)


def sequence(say=lambda step, held: None):
    """the calls of the test, in order; say(step, held bytes) after each"""
    from libaec_amd import gpu
    bind(gpu._lib())

    def held(codec, step):
        h = int(codec.lib.aec_gpu_held_bytes(codec.ctx))
        say(step, h)
        return h

    rng = np.random.default_rng(9)
    codec = gpu.Codec(*WIDE)
    assert held(codec, "16/16/64: created") == 0
    three = three_chunks(rng, WIDE)
    three.encode(codec)
    h1 = held(codec, "three chunks")
    assert h1 > 0
    S = WIDE[1] * WIDE[2]
    forty = Chunks(WIDE, [make_chunk(rng, "fast", int(rng.integers(1, 6)) * S, WIDE) for _ in range(40)])
    forty.encode(codec)
    h2 = held(codec, "40 chunks")
    assert h2 >= h1
    # room for both by now: nothing is reallocated, and the pinned buffers' turn comes round again
    enc40 = forty.encode(codec)
    assert held(codec, "40 chunks again") == h2
    three.encode(codec)
    assert held(codec, "three chunks again") == h2
    forty.decode(codec, *enc40)
    h3 = held(codec, "40 chunks decoded, with the table and bare")
    assert h3 >= h2
    window(codec, forty, next(i for i, w in enumerate(forty.want) if len(w[2]) >= 3))
    h4 = held(codec, "window decode")
    assert h4 >= h3
    codec.lib.aec_gpu_trim(codec.ctx, h4)                     # no single buffer is larger than all of them together
    assert held(codec, "trim to the total") == h4
    codec.lib.aec_gpu_trim(codec.ctx, 0)
    assert held(codec, "trim to 0") == 0
    three.encode(codec)
    assert held(codec, "three chunks after the trim") == h1   # growth depends on the need alone
    codec.close()

    codec = gpu.Codec(*TINY)
    assert held(codec, "8/8/1: created") == 0
    three = three_chunks(rng, TINY)
    three.encode(codec)
    encode_alone(codec, three)
    h1 = held(codec, "three chunks, then each alone")
    assert h1 > 0
    codec.lib.aec_gpu_trim(codec.ctx, 0)
    assert held(codec, "trim to 0") == 0
    three.encode(codec)
    encode_alone(codec, three)
    assert held(codec, "three chunks, then each alone, after the trim") == h1
    codec.close()


def test_held_bytes_follow_the_need_and_the_outputs_stay_exact():
    sequence()


if __name__ == "__main__":
    sequence(lambda step, h: print(f"{h:10d}  {step}", flush=True))
