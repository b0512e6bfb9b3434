"""The encoder route that codes every block once (libaec_amd/csrc/aec_enc_local.h) against the oracle: the cases of
tests/test_gpu_encode_local.py, run as a program on the tuning library so that AEC_ENC_LOCAL, AEC_ENC_LOCAL_SPW and
AEC_ENC_LOCAL_GUESS reach it (the library reads them at every call).
    python tests/enc_local_cases.py sweep <segments per wavefront>
    python tests/enc_local_cases.py plateau <segments per wavefront>
    python tests/enc_local_cases.py edges <segments per wavefront>
    python tests/enc_local_cases.py threshold           (the library as shipped)
Stream, RSI offsets, total_bits and the segment table must be the oracle's byte for byte; k_out must be what the
analyze / scan / pack kernels of the same library leave (AEC_ENC_LOCAL=0; the oracle does not report it)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import AEC_DATA_MSB as MSB, AEC_DATA_PREPROCESS as PP, AEC_DATA_SIGNED as SGN  # noqa: E402
from helpers import OPT_ZERO_CONT, OPT_ZERO, bytes_per_sample, oracle_encode, pack_samples  # noqa: E402

DIRECT = [(16, 16, 128, PP), (8, 8, 128, PP), (16, 16, 64, PP | MSB | SGN)]
ONE_BLOCK_RSI = (16, 8, 1, PP)
NOT_DIRECT = (32, 32, 100, PP | MSB | SGN)
AT_THRESHOLD = (16, 16, 128, PP)         # the shape the shipped library takes the route for: whole segments
T_SEGMENTS = 131072                      # kLocalMinSegs (aec_enc.hip)


def seg_blocks(prm):
    """blocks of a full segment (RSIs of 100 blocks have one of 64 and one of 36: sizes are then in units of 64)"""
    return min(64, prm[2])


def sizes(prm, spw):
    """(name, blocks, extra bytes): one block, one segment, 8 segments and one block less and more, 17 segments and part
    of a block with a cut-off sample behind it, 33 wavefronts"""
    S = seg_blocks(prm)
    nb = bytes_per_sample(prm[0], prm[3])
    part = (prm[1] // 2 + 1) * nb + (nb - 1)            # half a block and a sample, then a sample cut off (if it has 2 bytes)
    out = [("one block", 1, 0), ("one segment", S, 0), ("8 segments", 8 * S, 0), ("8 segments + 1 block", 8 * S + 1, 0),
           ("17 segments and a part", 17 * S, part), ("33 wavefronts", 33 * spw * S, 0)]
    if 8 * S > 1:
        out.insert(2, ("8 segments - 1 block", 8 * S - 1, 0))
    return out


def values(kind, n, prm, rng, spw=1):
    bps, bs, _, flags = prm
    lo, hi = (-(1 << (bps - 1)), (1 << (bps - 1)) - 1) if flags & SGN else (0, (1 << bps) - 1)
    mid = (lo + hi) // 2
    if kind == "zero":
        return np.zeros(n, dtype=np.int64)
    if kind == "constant":
        return np.full(n, mid + 3, dtype=np.int64)
    if kind == "noise":
        return rng.integers(lo, hi + 1, n)
    if kind == "walk":
        step = np.rint(rng.standard_normal(n) * rng.choice([0.3, 1, 6, 90], size=n, p=[0.4, 0.4, 0.15, 0.05])).astype(np.int64)
        for at in rng.integers(0, n, max(1, n // 600)):
            step[at:at + int(rng.integers(1, 3 * bs * 8))] = 0               # constant stretches: zero blocks and runs
        return np.clip(mid + np.cumsum(step), lo, hi)
    if kind == "islands":
        # zeros with short busy stretches between stretches of zero blocks of every length up to 40 segments: wavefronts
        # of a few bits each, several of them in one word of the stream (reaches_edge)
        v, seg, pos = np.zeros(n, dtype=np.int64), 64 * bs, 0
        while pos < n:
            pos += int(rng.integers(1, 40 * seg))
            b = int(rng.integers(1, 3 * bs))
            v[pos:pos + b] = rng.integers(0, 1 << min(bps - 1, 9), size=len(v[pos:pos + b]))
            pos += b
        return v
    assert kind in ("plateau", "late")
    # mid + {0, 1} everywhere; the first block of every wavefront is a ramp of +1 per sample (every mapped residual 2: the
    # plateau [0, 2]); the block in front of it mid + {0, 1} (carries k = 0) for odd wavefronts and
    # mid + [0, 2^(bps / 2)) (carries a large k) for even ones
    v = mid + rng.integers(0, 2, n)
    W = spw * seg_blocks(prm) * bs                                           # samples per wavefront
    for w in range(1, (n + W - 1) // W):
        at = w * W
        if w % 2 == 0:
            v[at - bs:at] = mid + rng.integers(0, 1 << (bps // 2), bs)
        if kind == "late":
            # the wavefront's first segment is constant (zero blocks: no k), the ramp opens its SECOND segment, at a
            # bit of the slot that is on no word border as a rule: the redo starts behind the run's first segment
            S = seg_blocks(prm) * bs
            v[at:at + S] = v[at - 1]
            at += S
        m = min(bs, n - at)
        v[at:at + m] = v[at - 1] + 1 + np.arange(m)
    return v


def segment_blocks(prm, nblk):
    """the first block of every segment"""
    rsi = prm[2]
    return [r + s for r in range(0, nblk, rsi) for s in range(0, min(rsi, nblk - r), 64)]


def segment_table(data, prm, trace):
    """start bit and the raw sample in front of every segment, from the oracle's per-block trace"""
    bps, bs, rsi, flags = prm
    nb = bytes_per_sample(bps, flags)
    first = segment_blocks(prm, len(trace))
    start = np.concatenate([[0], np.cumsum(trace["bits"].astype(np.uint64))])[first]
    prev = []
    nsamp = data.size // nb
    for b in first:
        if b % rsi == 0:
            prev.append(0)
            continue
        i = min(b * bs - 1, nsamp - 1)
        raw = data[i * nb:(i + 1) * nb]
        prev.append(int.from_bytes(raw.tobytes(), "big" if flags & MSB else "little"))
    return start, np.array(prev, dtype=np.uint64)


def reaches_edge(prm, spw, trace, bits):
    """What "islands" is for, read off the oracle's per-block trace.  Wavefronts of one segment: a 32-bit word of the
    stream holds bits of three or more of them.  Longer ones: a word is shared by two wavefronts of zero blocks only."""
    first = segment_blocks(prm, len(trace))[::spw]               # the first block of every wavefront
    ends = np.concatenate([[0], np.cumsum(trace["bits"].astype(np.int64))])
    ws = np.append(ends[first], np.int64(bits))                  # its first bit, and the end of the stream
    if spw == 1:
        # wavefronts w, w + 1, w + 2: the last bit of w and the first of w + 2 lie in one word
        return bool(np.any((ws[1:-2] - 1) >> 5 == ws[2:-1] >> 5))
    zero = np.isin(trace["option"], (OPT_ZERO, OPT_ZERO_CONT))
    only = np.array([zero[a:b].all() for a, b in zip(first, first[1:] + [len(trace)])])
    return bool(np.any(only[:-1] & only[1:] & (ws[1:-1] & 31 != 0)))


class Device:
    def __init__(self):
        import torch
        from libaec_amd import gpu
        self.torch, self.gpu = torch, gpu
        self.codecs = {}

    def encode(self, data, prm, fill=None, out_cap=None):
        """(stream bytes, offsets, result record, segment table, the whole output buffer)"""
        torch, gpu = self.torch, self.gpu
        codec = self.codecs.get(prm) or self.codecs.setdefault(prm, gpu.Codec(*prm))
        d_in = torch.from_numpy(np.ascontiguousarray(data)).cuda()
        n = data.size
        cap = codec.encode_bound(n) if out_cap is None else out_cap
        d_out = torch.full((cap + 64,), 0 if fill is None else fill, dtype=torch.uint8, device="cuda")
        d_off = torch.zeros(codec.rsi_count(n) + 1, dtype=torch.int64, device="cuda")
        d_res = torch.zeros(gpu.ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_tab = torch.zeros(codec.segment_count(n) * 16, dtype=torch.uint8, device="cuda")
        codec.set_segment_table(d_tab)
        codec.encode_async(d_in, n, d_out[:cap], d_off, d_res)
        torch.cuda.synchronize()
        codec.set_segment_table(None)
        res = d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]
        return d_out.cpu().numpy(), d_off.cpu().numpy().astype(np.uint64), res, d_tab.cpu().numpy().view(gpu.SEG_ENTRY_DTYPE)


def check(dev, data, prm, what, fill=None, edge_spw=None):
    """one input through the device encoder with the route on, against the oracle and the three-kernel route
    (edge_spw: the input must reach the edge of wavefronts of that many segments, reaches_edge)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    rc, want, trace, offs, bits = oracle_encode(data, *prm, want_trace=True)
    assert rc == 0, what
    assert edge_spw is None or reaches_edge(prm, edge_spw, trace, bits), (what, "does not reach its edge")
    out, off, res, tab = dev.encode(data, prm, fill=fill)
    nbytes = (bits + 7) // 8
    assert not int(res["overflow"]) and int(res["total_bits"]) == bits, (what, int(res["total_bits"]), bits)
    got = out[:nbytes].tobytes()
    if got != want[:nbytes]:
        bad = next(i for i in range(nbytes) if got[i] != want[i])
        raise AssertionError((what, "stream differs at byte", bad, "of", nbytes))
    assert np.array_equal(off[:-1], offs) and int(off[-1]) == bits, what
    start, prev = segment_table(data, prm, trace)
    assert np.array_equal(tab["bit"], start) and np.array_equal(tab["prev"].astype(np.uint64), prev), what
    if fill is not None:
        # the words the stream ends in (the open one and one of padding) are the encoder's; nothing behind them is
        end = ((bits >> 5) + 2) * 4
        assert np.all(out[end:] == fill), (what, "bytes behind the stream were written")
    os.environ["AEC_ENC_LOCAL"] = "0"
    try:
        out0, off0, res0, tab0 = dev.encode(data, prm)
    finally:
        os.environ["AEC_ENC_LOCAL"] = "1"
    assert int(res["k_out"]) == int(res0["k_out"]) and out0[:nbytes].tobytes() == got, what
    return trace


def inputs(prm, spw, kinds, rng):
    bps, bs, _, flags = prm
    nb = bytes_per_sample(bps, flags)
    for name, blocks, extra in sizes(prm, spw):
        for kind in kinds:
            v = values(kind, blocks * bs + (extra + nb - 1) // nb, prm, rng, spw)
            data = pack_samples(v, bps, flags)[:blocks * bs * nb + extra]
            yield f"{prm} spw {spw} {name} {kind}", data, (name, kind)


def sweep_inputs(spw):
    """(shape, segments per wavefront, name, input, its size and kind) of sweep()"""
    rng = np.random.default_rng(1210 + spw)
    for prm in DIRECT + [ONE_BLOCK_RSI, NOT_DIRECT]:
        # (the shape that keeps the analyze / scan / pack kernels: wavefronts of one segment, which keeps it small)
        w = 1 if prm == NOT_DIRECT else spw
        for what, data, tag in inputs(prm, w, ("walk", "zero", "constant", "noise", "islands"), rng):
            yield prm, w, what, data, tag


def sweep(spw):
    dev, n = Device(), 0
    for prm, w, what, data, tag in sweep_inputs(spw):
        # the largest input of "islands" is the one that has to reach the edge of its wavefronts, for every shape
        check(dev, data, prm, what, edge_spw=w if tag == ("33 wavefronts", "islands") else None)
        n += 1
    return n


def plateau(spw):
    """every wavefront starts with a block whose plateau is [0, 2], and the carried k in front is 0 for half of them
    and beyond 2 for the other half: whatever the guess, runs are coded a second time -- asserted on the oracle's trace
    first, then with the guess fixed to 0, to 31 and left to the rule"""
    dev, rng, n = Device(), np.random.default_rng(77 + spw), 0
    for prm in DIRECT:
        bps, bs, _, flags = prm
        blocks = 33 * spw * seg_blocks(prm)
        data = pack_samples(values("plateau", blocks * bs, prm, rng, spw), bps, flags)
        for guess in ("0", "31", None):
            os.environ.pop("AEC_ENC_LOCAL_GUESS", None)
            if guess is not None:
                os.environ["AEC_ENC_LOCAL_GUESS"] = guess
            trace = check(dev, data, prm, f"{prm} spw {spw} plateau guess {guess}")
            n += 1
        os.environ.pop("AEC_ENC_LOCAL_GUESS", None)
        k = trace["k"][spw * seg_blocks(prm)::spw * seg_blocks(prm)]
        assert len(k) == 32 and np.sum(k == 0) >= 12 and np.sum(k == 2) >= 12, (prm, spw, k.tolist())
        if spw > 1 and prm[2] % 64 == 0:
            # the same with the first miss in the run's second segment (rsi 64: behind an RSI border, rsi 128: inside one)
            data = pack_samples(values("late", blocks * bs, prm, rng, spw), bps, flags)
            trace = check(dev, data, prm, f"{prm} spw {spw} miss in the second segment")
            W, S = spw * seg_blocks(prm), seg_blocks(prm)
            k = trace["k"][W + S::W]
            assert np.all(np.isin(trace["option"][W:W + S], (OPT_ZERO, OPT_ZERO_CONT)))
            assert len(k) == 32 and np.sum(k == 0) >= 12 and np.sum(k == 2) >= 12, (prm, spw, k.tolist())
            n += 1
    return n


def edges(spw):
    """the output buffer filled with 0xFF: nothing behind the stream's last word is touched; a capacity one word short:
    overflow is reported and nothing is written beyond the capacity"""
    dev, rng, n = Device(), np.random.default_rng(5 + spw), 0
    for prm in DIRECT:
        bps, bs, _, flags = prm
        for kind in ("walk", "zero"):
            blocks = 17 * seg_blocks(prm) + 3
            data = pack_samples(values(kind, blocks * bs, prm, rng, spw), bps, flags)
            check(dev, data, prm, f"{prm} spw {spw} {kind} into 0xFF", fill=0xFF)
            rc, want, _, _, bits = oracle_encode(data, *prm)
            cap = ((bits + 7) // 8 + 3) // 4 * 4 - 4          # one word short
            cap -= cap % 16                                    # (the call wants whole 16 bytes)
            if cap >= 16:
                out, _, res, _ = dev.encode(data, prm, fill=0xEE, out_cap=cap)
                assert int(res["overflow"]) == 1 and int(res["total_bits"]) == bits
                assert np.all(out[cap:] == 0xEE) and out[:cap].tobytes() == want[:cap], (prm, kind, "overflow")
            n += 2
    return n


def held(dev, prm):
    codec = dev.codecs[prm]
    codec.lib.aec_gpu_held_bytes.restype = C.c_size_t
    codec.lib.aec_gpu_held_bytes.argtypes = [C.c_void_p]
    return int(codec.lib.aec_gpu_held_bytes(codec.ctx))


def threshold():
    """The library as shipped one segment below the size from which it takes the route, and at it: both exact, and the
    context's held bytes show which kernels ran -- the route's image area is 1.09 x the input, the old kernels' workspace
    an eighth of it.  Then a shape with RSIs of one block at the same number of segments: it keeps the old kernels."""
    dev, rng, n = Device(), np.random.default_rng(3), 0
    prm = AT_THRESHOLD
    bps, bs, rsi, flags = prm
    seg_bytes = 64 * bs * 2
    tile = pack_samples(values("walk", (1 << 20) // 2, prm, rng), bps, flags)
    data = np.tile(np.ascontiguousarray(tile, dtype=np.uint8), T_SEGMENTS * seg_bytes // tile.size)
    data[-seg_bytes:] = data[-seg_bytes - 1]        # the last segment constant: no k behind segment T - 1
    k_out = []
    for segs, route in ((T_SEGMENTS - 1, False), (T_SEGMENTS, True)):
        part = data[:segs * seg_bytes]
        rc, want, trace, offs, bits = oracle_encode(part, *prm, want_trace=True)
        out, off, res, tab = dev.encode(part, prm)
        assert int(res["total_bits"]) == bits and not int(res["overflow"]) and out[:(bits + 7) // 8].tobytes() == want, segs
        assert np.array_equal(off[:-1], offs) and int(off[-1]) == bits, segs
        start, prev = segment_table(part, prm, trace)
        assert np.array_equal(tab["bit"], start) and np.array_equal(tab["prev"].astype(np.uint64), prev), segs
        k_out.append(int(res["k_out"]))
        h = held(dev, prm)
        print(f"{prm} {segs} segments ({part.size} bytes): held {h} bytes", flush=True)
        assert (h > part.size) == route and (route or h < part.size // 4), (segs, h)
        dev.codecs[prm].lib.aec_gpu_trim(dev.codecs[prm].ctx, C.c_size_t(0))
        n += 1
    assert k_out[0] == k_out[1]                     # (the oracle reports no k; the old kernels coded the first)
    # RSIs shorter than a segment: the old kernels at any size.  A segment is one block here: 4 B of summary and 15 B of
    # scan arrays each, 16 B of scan partial per 2048 of them, every array rounded up to 256 B
    small = (16, 16, 1, PP)
    part = data[:T_SEGMENTS * 32]
    rc, want, _, offs, bits = oracle_encode(part, *small)
    out, off, res, _ = dev.encode(part, small)
    assert int(res["total_bits"]) == bits and out[:(bits + 7) // 8].tobytes() == want
    h = held(dev, small)
    print(f"{small} {T_SEGMENTS} segments ({part.size} bytes): held {h} bytes", flush=True)
    assert h < T_SEGMENTS * (4 + 15) + (T_SEGMENTS // 2048 + 2) * 16 + 8 * 256, h      # (the route's area alone: 291 MB)
    return n + 1


def main():
    mode = sys.argv[1]
    if mode == "threshold":
        n = threshold()
    else:
        os.environ["AEC_ENC_LOCAL"] = "1"
        os.environ["AEC_ENC_LOCAL_SPW"] = sys.argv[2]
        n = {"sweep": sweep, "plateau": plateau, "edges": edges}[mode](int(sys.argv[2]))
    print("encode local ok:", mode, n, "cases; AEC_AMD_LIB=%s" % os.environ.get("AEC_AMD_LIB"))


if __name__ == "__main__":
    main()
