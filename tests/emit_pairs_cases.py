"""The small-block emitter on sample pairs (libaec_amd/csrc/aec_lane.h emit_small_pairs, aec_enc.hip emit_segment) on the
device against the oracle: the cases of tests/test_gpu_emit_pairs.py, run as a program on the tuning library with
AEC_ENC_LOCAL=1 (every block coded once: k_encode_local) and, inside check(), with AEC_ENC_LOCAL=0 (analyze / scan / pack:
k_pack runs the same emitter).
    python tests/emit_pairs_cases.py classes      (no device: the inputs hold the classes below)
    python tests/emit_pairs_cases.py run <shape index>
Stream, RSI offsets, total_bits and the segment table are the oracle's byte for byte on both routes, and the stream decodes
to the input.  Every input holds, read off the oracle's per-block trace (an input that lacks one is refused):
  a segment of second-extension blocks only; a segment with second-extension, split and zero-run blocks;
  a split block at k = kmax; a block the pair emitter does not take because its fields pass 64 bits, and one whose
  header and unary region pass 64 bits (a zero run of 59 - 63 blocks: a code of 60 - 64 bits behind its header -- the
  encoder's own choice of k leaves no split or second-extension code of 64 zeros); an uncompressed block;
  the first block of an RSI as each of split, second extension and zero run."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import AEC_DATA_PREPROCESS as PP  # noqa: E402
from helpers import OPT_ZERO, bytes_per_sample, id_len_of, oracle_encode, pack_samples  # noqa: E402
import enc_local_cases as elc  # noqa: E402

OPT_SE, OPT_SPLIT, OPT_UNCOMP = 1, 2, 3
SHAPES = [(16, 16, 128, PP), (16, 8, 128, PP), (8, 8, 128, PP), (8, 16, 64, PP), (16, 16, 100, PP)]
SEGMENTS = (70, 2049)          # a last workgroup that is not full; more than one run per wavefront
SEG_KINDS = 5


def block(kind, bs, bps, rng):
    """one block's samples; every kind but the noisy ones starts and ends on `mid`"""
    mid, kmax = 1 << (bps - 1), (1 << id_len_of(bps, PP)) - 3
    v = np.full(bs, mid, dtype=np.int64)
    if kind == "se":                       # mapped residuals 1 and 2 in a block of zeros
        v[2:4] = mid - 1
    elif kind == "split":
        v += rng.integers(-3, 4, bs)
        v[-1] = mid
    elif kind == "kmax":
        v += rng.integers(-(1 << (kmax - 1)), 1 << (kmax - 1), bs)
    elif kind == "noise":
        v = rng.integers(0, 1 << bps, bs)
    else:
        assert kind == "zero"
    return v


def segment_kinds(t, nv):
    """block kinds of segment kind t (nv blocks)"""
    if t == 0:
        return ["se"] * nv
    if t == 1:
        return (["se", "split", "zero", "zero", "se", "split", "split", "zero"] * 8)[:nv]
    if t == 2:
        return (["split", "split", "kmax", "kmax", "split", "noise", "noise", "split"] * 8)[:nv]
    if t == 3:                             # a zero block, then a run of 60 that does not close the segment
        return (["zero", "se"] + ["zero"] * 60 + ["se", "se"])[:nv]
    return ["split"] * nv


def make_input(prm, segments, seed, extra_blocks=0, extra_bytes=0):
    bps, bs, rsi, flags = prm
    rng = np.random.default_rng(seed)
    nb = bytes_per_sample(bps, flags)
    per_rsi = [min(64, rsi - s) for s in range(0, rsi, 64)]
    vals, s = [], 0
    while s < segments:
        for nv in per_rsi:
            if s == segments:
                break
            for kind in segment_kinds(s % SEG_KINDS, nv):
                vals.append(block(kind, bs, bps, rng))
            s += 1
    for _ in range(extra_blocks + 1):
        vals.append(block("split", bs, bps, rng))
    v = np.concatenate(vals)
    nbytes = (len(v) - bs) * nb + extra_bytes
    return np.ascontiguousarray(pack_samples(v, bps, flags)[:nbytes], dtype=np.uint8)


def classes(prm, trace):
    """the classes of the module's text that the oracle's trace of an input holds"""
    bps, bs, rsi, flags = prm
    idl = id_len_of(bps, flags)
    kmax = (1 << idl) - 3
    opt, k, bits = trace["option"], trace["k"].astype(np.int64), trace["bits"].astype(np.int64)
    first = elc.segment_blocks(prm, len(trace))
    ends = first[1:] + [len(trace)]
    emits = opt != elc.OPT_ZERO_CONT
    ref = (np.arange(len(trace)) % rsi == 0).astype(np.int64)
    n = bs - ref
    head = idl + np.where(opt == OPT_SPLIT, 0, 1) + ref * bps
    fbits = np.where(opt == OPT_SPLIT, n * k, 0)
    ubits = bits - head - fbits
    small = np.isin(opt, (OPT_ZERO, OPT_SE, OPT_SPLIT))
    has = {
        "segment of SE only": any(np.all(opt[a:b] == OPT_SE) for a, b in zip(first, ends) if b - a >= 32),
        "segment of SE, split and zero run": any(all(np.any(opt[a:b] == o) for o in (OPT_SE, OPT_SPLIT, OPT_ZERO))
                                                 for a, b in zip(first, ends)),
        "k = kmax": bool(np.any((opt == OPT_SPLIT) & (k == kmax))),
        # (8-bit samples in blocks of 8 have no such block: 8 fields of kmax = 5 bits)
        "fields beyond 64 bits": bool(np.any(small & (fbits > 64))) or bs * kmax <= 64,
        "header and unary region beyond 64 bits": bool(np.any(small & emits & (fbits <= 64) & (head + ubits > 64))),
        "eligible": bool(np.any(small & emits & (fbits <= 64) & (head + ubits <= 64))),
        "uncompressed": bool(np.any(opt == OPT_UNCOMP)),
    }
    for name, o in (("split", OPT_SPLIT), ("SE", OPT_SE), ("zero run", OPT_ZERO)):
        has["reference block as " + name] = bool(np.any(opt[::rsi] == o))
    return has


def inputs(prm):
    for segments in SEGMENTS:
        # (the shorter input goes on with five blocks and part of one: segments the kernels feed through the LDS rows)
        extra = (5, prm[1] // 2 * bytes_per_sample(prm[0], prm[3]) + 1) if segments == SEGMENTS[0] else (0, 0)
        yield f"{prm} {segments} segments", make_input(prm, segments, 1900 + segments + prm[0] + prm[1], *extra)


def checked_trace(prm, what, data):
    rc, _, trace, _, _ = oracle_encode(data, *prm, want_trace=True)
    assert rc == 0, what
    missing = [name for name, ok in classes(prm, trace).items() if not ok]
    assert not missing, (what, "the input lacks", missing)
    return trace


def decode_check(dev, data, prm, what):
    """encode and decode on the device: the input comes back (the last block padded with its last sample)"""
    torch = dev.torch
    codec = dev.codecs[prm]
    d_in = torch.from_numpy(data).cuda()
    d_out, nbytes, _, _, d_off = codec.encode(d_in)
    nblk = codec.block_count(data.size)
    d_dec, status = codec.decode(d_out, nbytes, d_off, codec.rsi_count(data.size), nblk)
    nb = bytes_per_sample(prm[0], prm[3])
    whole = data.size // nb * nb
    assert status == 0 and d_dec[:whole].cpu().numpy().tobytes() == data[:whole].tobytes(), (what, "decoded")


def encode_at(dev, data, prm, start_bit):
    """(stream bytes, segment table) of an encode that starts `start_bit` bits into the buffer's first byte"""
    torch, gpu = dev.torch, dev.gpu
    codec = dev.codecs[prm]
    d_in = torch.from_numpy(data).cuda()
    d_out = torch.zeros(codec.encode_bound(data.size) + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(codec.rsi_count(data.size) + 1, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(gpu.ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_tab = torch.zeros(codec.segment_count(data.size) * 16, dtype=torch.uint8, device="cuda")
    codec.set_segment_table(d_tab)
    codec.encode_async(d_in, data.size, d_out[:-64], d_off, d_res, start_bit=start_bit)
    torch.cuda.synchronize()
    codec.set_segment_table(None)
    bits = int(d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["total_bits"])
    return d_out[:(start_bit + bits + 7) // 8].cpu().numpy(), d_tab.cpu().numpy().view(gpu.SEG_ENTRY_DTYPE), d_off.cpu().numpy()


def table_check(dev, data, prm, what):
    """the segment table, the RSI offsets and the stream the route leaves are those of the analyze / scan / pack route, at
    start bit 0 -- check() has compared them with the oracle's -- and at start bit 5, where every entry lies 5 bits
    behind"""
    got = {}
    for start_bit in (0, 5):
        for local in ("1", "0"):
            os.environ["AEC_ENC_LOCAL"] = local
            got[start_bit, local] = encode_at(dev, data, prm, start_bit)
        os.environ["AEC_ENC_LOCAL"] = "1"
        (s1, t1, o1), (s0, t0, o0) = got[start_bit, "1"], got[start_bit, "0"]
        assert np.array_equal(t1["bit"], t0["bit"]) and np.array_equal(t1["prev"], t0["prev"]), (what, start_bit, "table")
        assert np.array_equal(o1, o0) and np.array_equal(s1[1:-1], s0[1:-1]), (what, start_bit, "stream")
    assert np.array_equal(got[5, "1"][1]["bit"], got[0, "1"][1]["bit"] + 5), (what, "start bit")
    assert np.array_equal(got[5, "1"][1]["prev"], got[0, "1"][1]["prev"]), (what, "start bit")


def run(index):
    prm = SHAPES[index]
    dev, n = elc.Device(), 0
    for what, data in inputs(prm):
        checked_trace(prm, what, data)
        for spw in ("8", "32") if "2049" in what else ("8",):
            os.environ["AEC_ENC_LOCAL_SPW"] = spw
            elc.check(dev, data, prm, what + " spw " + spw)      # the route, the oracle, the analyze / scan / pack route
            n += 1
        table_check(dev, data, prm, what)
        decode_check(dev, data, prm, what)
        os.environ["AEC_ENC_LOCAL"] = "0"
        try:
            decode_check(dev, data, prm, what + " (pack)")
        finally:
            os.environ["AEC_ENC_LOCAL"] = "1"
    return n


def main():
    if sys.argv[1] == "classes":
        for prm in SHAPES:
            for what, data in inputs(prm):
                checked_trace(prm, what, data)
                print("classes ok:", what, data.size, "bytes")
        return
    os.environ["AEC_ENC_LOCAL"] = "1"
    n = run(int(sys.argv[2]))
    print("emit pairs ok:", SHAPES[int(sys.argv[2])], n, "cases; AEC_AMD_LIB=%s" % os.environ.get("AEC_AMD_LIB"))


if __name__ == "__main__":
    main()
