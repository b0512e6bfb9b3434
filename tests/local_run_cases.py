"""k_encode_local's walk over a run (libaec_amd/csrc/aec_enc.hip: segments as 32-bit indices from the run's first one, the
parameters' derived values computed per segment, analyze_segment's length scan handed to emit_segment) on the device
against the oracle: the cases of tests/test_gpu_local_run.py, run as a program on the tuning library with AEC_ENC_LOCAL=1.
    python tests/local_run_cases.py properties     (no device: the inputs drive what they are meant to)
    python tests/local_run_cases.py run <case index>
16-bit samples in blocks of 16; every input ends in a segment of 37 blocks.  Per case and run length two inputs, each at
start bit 0 and 5, each compared with the oracle (stream, RSI offsets, segment table) and decoded back:
  "drive"      every run opens with a block whose plateau is [0, 2] behind a carried k of 0 or of a large one, every fourth
               run behind a first segment of zero blocks: the guess misses, k_encode_local<REDO> codes the run again from
               the first to the last miss and joins the last word with what stays in the slot (merge_tail); a block of
               noise (uncompressed: an emit_block lane); a zero run across a segment end.  properties() reads that off a
               model of the k chain (the plateau of assess_split_with, the guess and the miss test of aec_enc_local.h),
               which it first holds against the k of the oracle's trace.
  "unaligned"  a walk in a buffer 2 bytes off a 16-byte border: no segment takes the direct path, the rows come from
               feed_now (the loop's first copy of the segment body)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import AEC_DATA_PREPROCESS as PP  # noqa: E402
from helpers import OPT_ZERO, OPT_ZERO_CONT, oracle_encode  # noqa: E402
import enc_local_cases as elc  # noqa: E402

BPS, BS, KMAX, MID = 16, 16, 13, 1 << 15
OPT_SPLIT, OPT_UNCOMP = 2, 3
LAST = 37                      # blocks of every input's last segment
# (rsi, segments, run lengths): one full run of 32 and a run of one | a tail run of 6, and with runs of one segment the
# second segment of an RSI first in a run | more than one tile of the scan (2048 segments)
CASES = [(64, 33, (32,)), (128, 70, (32, 1)), (128, 2049, (32, 8))]


def prm_of(case):
    return (BPS, BS, case[0], PP)


def blocks_of(case):
    return (case[1] - 1) * 64 + LAST


def drive_values(case, spw, rng):
    n, seg, run = blocks_of(case) * BS, 64 * BS, spw * 64 * BS
    v = MID + rng.integers(0, 2, n)
    for w in range(1, (n + run - 1) // run):
        at = w * run
        if w % 2 == 1:
            v[at - BS:at] = MID + rng.integers(0, 1 << 8, BS)        # carries a large k into the run
        if w % 4 == 3 and spw > 1 and at + seg < n:
            v[at:at + seg] = v[at - 1]                               # first segment: zero blocks, no k
            at += seg
        m = min(BS, n - at)
        v[at:at + m] = v[at - 1] + 1 + np.arange(m)                  # every mapped residual 2: plateau [0, 2]
    # a block of noise in the third segment of every run of 4 and more segments (or in every fifth segment)
    for at in range(2 * seg + 5 * BS, n - BS, run if spw >= 4 else 5 * seg):
        v[at:at + BS] = rng.integers(0, 1 << BPS, BS)
    # constant from block 61 of segment 2 to block 3 of segment 3 (rsi 128: inside an RSI; rsi 64: across its border)
    at = 2 * seg + 61 * BS
    v[at:at + 6 * BS] = v[at - 1]
    return v


def inputs(case, spw):
    """(name, bytes, bytes the device buffer is shifted by)"""
    rng = np.random.default_rng(2100 + case[0] + case[1] + spw)
    n = blocks_of(case) * BS
    yield "drive", elc.pack_samples(drive_values(case, spw, rng), BPS, PP), 0
    yield "unaligned", elc.pack_samples(elc.values("walk", n, prm_of(case), rng), BPS, PP), 2


# ---- the k chain of an input, modelled ---------------------------------------------------------------------------------------
def plateaus(case, data):
    """per block (klo, khi) of the split option (aec_lane.h assess_split_with) and whether the block is all zero; the
    mapped residuals as aec_lane.h pp_unsigned has them"""
    x = np.frombuffer(data.tobytes(), dtype="<u2").astype(np.int64)
    prev = np.concatenate([x[:1], x[:-1]])
    dist, room = np.abs(x - prev), np.minimum(prev, (1 << BPS) - 1 - prev)
    r = np.where(dist <= room, 2 * dist - (x < prev), room + dist).reshape(-1, BS)
    ref = np.arange(len(r)) % case[0] == 0
    r[ref, 0] = 0
    n = BS - ref.astype(np.int64)
    fs = np.stack([(r >> k).sum(axis=1) for k in range(KMAX + 1)], axis=1)
    g = fs[:, :-1] - fs[:, 1:]                                       # g(k), k < kmax
    first = lambda ok: np.where(ok.any(axis=1), ok.argmax(axis=1), KMAX)      # noqa: E731
    return first(g <= n[:, None]), first(g < n[:, None]), ~r.any(axis=1)


def chain(lo, hi, zero, k, out=None):
    for b in range(len(lo)):
        if not zero[b]:
            k = min(max(k, lo[b]), hi[b])
        if out is not None:
            out[b] = k
    return k


def properties(case, spw, data, trace):
    """what the "drive" input makes the kernels do, from the model; returns a line for the log"""
    lo, hi, zero = plateaus(case, data)
    k_true = np.zeros(len(lo), dtype=np.int64)
    chain(lo, hi, zero, 0, k_true)
    split = trace["option"] == OPT_SPLIT
    assert np.array_equal(k_true[split], trace["k"][split]), "the model of the k chain is not the oracle's"
    assert np.array_equal(zero, np.isin(trace["option"], (OPT_ZERO, OPT_ZERO_CONT)))
    first = elc.segment_blocks(prm_of(case), len(lo)) + [len(lo)]
    nseg = len(first) - 1
    redo = merged = late = 0
    for s0 in range(0, nseg, spw):
        k, have, missed = 0, s0 == 0, []
        for s in range(s0, min(s0 + spw, nseg)):
            a, b = first[s], first[s + 1]
            upd = [i for i in range(a, b) if not zero[i]]
            if not have and upd:
                k, have = lo[upd[0]], True                           # local_guess: the plateau's lower end
            k_in_true = k_true[a - 1] if a else 0
            if upd:                                                  # local_missed
                c1 = lambda kk: min(max(kk, lo[upd[0]]), hi[upd[0]])     # noqa: E731
                missed.append(c1(k) != c1(k_in_true))
            else:
                missed.append(False)
            k = chain(lo[a:b], hi[a:b], zero[a:b], k)
        if any(missed):
            redo += 1
            last = max(i for i, m in enumerate(missed) if m)
            merged += last + 1 < len(missed)
            late += missed.index(True) > 0
    ends = np.array(first[1:-1])
    across = bool(np.any(zero[ends - 1] & zero[ends]))
    assert redo >= 1 and across and np.any(trace["option"] == OPT_UNCOMP), (case, spw, redo, across)
    if spw > 1 and nseg > spw + 1:          # (the call's first run has the true k; a run of one ends where it ends)
        assert merged >= 1, (case, spw, "no run is coded again up to a segment that stays")
    if spw > 1 and case[1] > 4 * spw + 1:
        assert late >= 1, (case, spw, "no run is coded again from behind its first segment")
    return f"runs coded again {redo}, of them ending in front of the run's end {merged}, starting behind its start {late}"


# ---- the device --------------------------------------------------------------------------------------------------------------
def encode_at(dev, data, prm, start_bit, shift):
    """(stream bits from start_bit on, RSI offsets, segment table, total bits) with the input `shift` bytes into its buffer"""
    torch, gpu = dev.torch, dev.gpu
    codec = dev.codecs.get(prm) or dev.codecs.setdefault(prm, gpu.Codec(*prm))
    d_buf = torch.zeros(data.size + 16, dtype=torch.uint8, device="cuda")
    d_in = d_buf[shift:shift + data.size]
    d_in.copy_(torch.from_numpy(data))
    assert d_in.data_ptr() % 16 == shift
    cap = codec.encode_bound(data.size)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(codec.rsi_count(data.size) + 1, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(gpu.ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_tab = torch.zeros(codec.segment_count(data.size) * 16, dtype=torch.uint8, device="cuda")
    codec.set_segment_table(d_tab)
    codec.encode_async(d_in, data.size, d_out[:cap], d_off, d_res, start_bit=start_bit)
    torch.cuda.synchronize()
    codec.set_segment_table(None)
    res = d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]
    assert not int(res["overflow"])
    bits = int(res["total_bits"])
    # decoded back (the decoder takes a stream from bit 0: the call that starts there)
    if start_bit == 0:
        nblk = codec.block_count(data.size)
        d_dec, status = codec.decode(d_out, (bits + 7) // 8, d_off, codec.rsi_count(data.size), nblk)
        assert status == 0 and d_dec[:data.size].cpu().numpy().tobytes() == data.tobytes(), "decoded"
    stream = np.unpackbits(d_out[:(start_bit + bits + 7) // 8].cpu().numpy())[start_bit:start_bit + bits]
    return stream, d_off.cpu().numpy().astype(np.uint64), d_tab.cpu().numpy().view(gpu.SEG_ENTRY_DTYPE), bits


def check(dev, case, spw, name, data, shift):
    prm = prm_of(case)
    what = f"{case} spw {spw} {name}"
    rc, want, trace, offs, bits = oracle_encode(data, *prm, want_trace=True)
    assert rc == 0, what
    note = properties(case, spw, data, trace) if name == "drive" else ""
    want_bits = np.unpackbits(np.frombuffer(want, dtype=np.uint8))[:bits]
    start, prev = elc.segment_table(data, prm, trace)
    for start_bit in (0, 5):
        stream, off, tab, got_bits = encode_at(dev, data, prm, start_bit, shift)
        assert got_bits == bits, (what, start_bit, got_bits, bits)
        if not np.array_equal(stream, want_bits):
            raise AssertionError((what, start_bit, "stream differs at bit", int(np.argmax(stream != want_bits)), "of", bits))
        assert np.array_equal(off[:-1], offs + start_bit) and int(off[-1]) == bits + start_bit, (what, start_bit, "RSI offsets")
        assert np.array_equal(tab["bit"], start + np.uint64(start_bit)), (what, start_bit, "segment table: bit")
        assert np.array_equal(tab["prev"].astype(np.uint64), prev), (what, start_bit, "segment table: sample")
    print(what, "ok", note, flush=True)


def run(index):
    case = CASES[index]
    dev, n = elc.Device(), 0
    for spw in case[2]:
        os.environ["AEC_ENC_LOCAL_SPW"] = str(spw)
        for name, data, shift in inputs(case, spw):
            check(dev, case, spw, name, np.ascontiguousarray(data, dtype=np.uint8), shift)
            n += 1
    return n


def main():
    if sys.argv[1] == "properties":
        for case in CASES:
            for spw in case[2]:
                name, data, _ = next(inputs(case, spw))
                data = np.ascontiguousarray(data, dtype=np.uint8)
                rc, _, trace, _, _ = oracle_encode(data, *prm_of(case), want_trace=True)
                print(case, "spw", spw, properties(case, spw, data, trace))
        return
    os.environ["AEC_ENC_LOCAL"] = "1"
    n = run(int(sys.argv[2]))
    print("local run ok:", CASES[int(sys.argv[2])], n, "inputs; AEC_AMD_LIB=%s" % os.environ.get("AEC_AMD_LIB"))


if __name__ == "__main__":
    main()
