"""The placement of the route that codes every block once (aec_enc.hip k_place) at the borders of its rounds and
groups: the cases of tests/test_gpu_place_rounds.py, run as a program on the tuning library (AEC_ENC_LOCAL=1).
    python tests/place_rounds_cases.py runs       wavefronts of 8 segments: stream, offsets, segment table; decode round trip
    python tests/place_rounds_cases.py again      the same input with other run lengths, into 0xFF, and into short buffers
    python tests/place_rounds_cases.py past       a stream of more than 2^31 bits
    python tests/place_rounds_cases.py list       (no device) the runs the input has, from the oracle's RSI offsets
k_place moves a run (what one wavefront of k_encode_local coded: AEC_ENC_LOCAL_SPW segments) in rounds of 256 slot words,
kPlaceRounds rounds loaded at a time.  The input sets the lengths of the runs of 8 segments: 16-bit samples, blocks of
16, RSIs of 128 blocks, so a run is 512 blocks, four RSIs, and is coded the same wherever it stands.  A run holds some
blocks of noise (260 bits each, uncompressed, or a few less), then blocks of 16 residuals of which the first
j are -1 and the rest 0, which move the length by a few bits each, then zeros.  Which blocks a run needs for a wanted
length is found by coding candidates with the oracle; what the runs ARE is then read off the RSI offsets the oracle
reports for the whole input, and the case fails unless every length of required() is there."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import AEC_DATA_PREPROCESS as PP, ROOT, oracle_encode, pack_samples  # noqa: E402

PRM = (16, 16, 128, PP)
BS, RSI = PRM[1], PRM[2]
SPW = 8                               # segments per run of the input's design
RUN_BLOCKS = SPW * 64
RUN_BYTES = RUN_BLOCKS * BS * 2
ROUND = 256                           # slot words per round: 64 lanes of four
MID = 32768


def place_constants():
    """kPlaceSlots, kPlaceRounds as the kernel has them"""
    text = open(os.path.join(ROOT, "libaec_amd", "csrc", "aec_enc.hip")).read()
    m = re.search(r"constexpr uint32_t kPlaceSlots = (\d+), kPlaceRounds = (\d+);", text)
    assert m, "kPlaceSlots / kPlaceRounds not found in aec_enc.hip"
    return int(m.group(1)), int(m.group(2))


def run_values(noise, trim, rng):
    """the samples of one run: `noise` blocks of noise (the last sample MID), a block per entry j of `trim` whose first
    j samples go down by one each, then the last value for the rest"""
    v = np.empty(RUN_BLOCKS * BS, dtype=np.int64)
    n = noise * BS
    v[:n] = rng.integers(0, 1 << 16, n)
    if n:
        v[n - 1] = MID
    step = np.zeros(v.size - n, dtype=np.int64)
    for b, j in enumerate(trim):
        step[b * BS:b * BS + j] = -1
    v[n:] = MID + np.cumsum(step)
    return v


def run_bits(v):
    rc, _, _, _, bits = oracle_encode(pack_samples(v, PRM[0], PRM[3]), *PRM)
    assert rc == 0
    return bits


def trims():
    """candidates in rising order of what they add: up to 11 blocks, all but the last one full"""
    yield ()
    for full in range(11):
        for j in range(1, BS + 1):
            yield (BS,) * full + (j,)


def fit(fits, most_noise, rng):
    """a run with at most most_noise blocks of noise whose length in bits satisfies fits(bits)"""
    for noise in range(most_noise, max(most_noise - 2, -1), -1):
        seed = int(rng.integers(1 << 31))
        for trim in trims():
            if noise + len(trim) > RUN_BLOCKS:
                break
            v = run_values(noise, trim, np.random.default_rng(seed))
            if fits(run_bits(v)):
                return v
    raise AssertionError(("no run found", most_noise))


def words_wanted(rounds):
    """slot-word counts at the borders of the rounds and of the first group (1 comes from the short last run)"""
    w = [ROUND - 1, ROUND, ROUND + 1]
    for k in range(2, rounds + 2):
        w += [ROUND * k - 1, ROUND * k, ROUND * k + 1]
    return w


def build(rounds):
    """the input: a run of whole words at bit 0, a run for every count of words_wanted(), run i = 0 .. 512 with i
    blocks of noise and i % 40 residuals behind them, and a last run of one constant block"""
    rng = np.random.default_rng(1500)
    runs = [fit(lambda bits: bits % 32 == 0, 3, rng)]
    for w in words_wanted(rounds):
        runs.append(fit(lambda bits: 32 * (w - 1) < bits <= 32 * w, (32 * w) // 260, rng))
    for i in range(RUN_BLOCKS + 1):
        j = i % 40
        trim = ((BS,) * (j // BS) + ((j % BS,) if j % BS else ()))[:RUN_BLOCKS - i]
        runs.append(run_values(i, trim, rng))
    runs.append(np.full(BS, MID, dtype=np.int64))
    return pack_samples(np.concatenate(runs), PRM[0], PRM[3]), len(runs)


def run_table(offs, bits, spw=SPW):
    """(start bit, length in bits) of every run of spw segments, from the RSI offsets (spw 8: four RSIs a run)"""
    assert spw % 2 == 0
    starts = np.append(offs[::spw // 2].astype(np.int64), np.int64(bits))
    return starts[:-1], np.diff(starts)


def required(slots, rounds, start, length):
    """every length and position the placement can go wrong at: missing ones, as a list of words"""
    nslot = (length + 31) >> 5
    lead = start & 31
    head = lead != 0
    tail = (lead + length) & 31 != 0
    missing = [f"{w} slot words" for w in [1] + words_wanted(rounds) if not np.any(nslot == w)]
    if not np.any(length >= RUN_BLOCKS * 257):          # (a block of noise: 260 bits, or a split that saves one to three)
        missing.append("a run of noise alone, which fills its slot")
    if not np.any(~head & ~tail):
        missing.append("a run of whole words")
    if np.sum(head & tail) < 8:
        missing.append("runs with both ends shared")
    if not np.any(nslot > rounds * ROUND * 2):
        missing.append("a run of three groups")
    if len(length) % (4 * slots) == 0:
        missing.append("a last workgroup that is not full")
    return missing


def reference(rounds):
    data, nruns = build(rounds)
    rc, want, trace, offs, bits = oracle_encode(data, *PRM, want_trace=True)
    assert rc == 0 and len(offs) == 4 * (nruns - 1) + 1
    return data, want, trace, offs, bits


def middle_round_cap(start, length):
    """bytes of a buffer that ends in the second round of a run of three or more, and of one that ends with the word a
    run starts in (which it shares): whole 16 bytes both"""
    nslot, word0 = (length + 31) >> 5, start >> 5
    g = int(np.flatnonzero(nslot > 2 * ROUND + 8)[0])
    mid = (int(word0[g]) + ROUND + 101) // 4 * 16
    assert int(word0[g]) + ROUND < mid // 4 < int(word0[g]) + 2 * ROUND
    f = int(np.flatnonzero((word0 % 4 == 3) & (start & 31 != 0) & (nslot > 8))[0])
    return mid, (int(word0[f]) + 1) * 4


def past_bit_31():
    """264 MiB of noise: the stream is longer than 2^31 bits, so run edges have bit 31 of their low word set.  The
    reference is the analyze / scan / pack route of the same library (the oracle would take as long as all other
    cases together); the stream decodes to the input."""
    import torch
    from libaec_amd import gpu
    n = 264 << 20
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    d_in = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    codec = gpu.Codec(*PRM)
    os.environ["AEC_ENC_LOCAL_SPW"] = str(SPW)
    got = {}
    for route in ("0", "1"):
        os.environ["AEC_ENC_LOCAL"] = route
        got[route] = codec.encode(d_in)
    (out0, nbytes0, bits0, k0, off0), (out1, nbytes1, bits1, k1, off1) = got["0"], got["1"]
    assert bits1 == bits0 and bits1 > 1 << 31 and k1 == k0, (bits0, bits1)
    assert torch.equal(off1, off0), "RSI offsets differ"
    assert torch.equal(out1[:nbytes1], out0[:nbytes0]), "stream differs"
    d_dec, status = codec.decode(out1, nbytes1, off1, codec.rsi_count(n), codec.block_count(n))
    assert status == 0 and torch.equal(d_dec[:n], d_in), "decode round trip"
    return 1


def main():
    mode = sys.argv[1]
    if mode == "past":
        print("place rounds ok:", mode, past_bit_31(), "cases; AEC_AMD_LIB=%s" % os.environ.get("AEC_AMD_LIB"))
        return
    slots, rounds = place_constants()
    data, want, trace, offs, bits = reference(rounds)
    start, length = run_table(offs, bits)
    missing = required(slots, rounds, start, length)
    if mode == "list":
        nslot = (length + 31) >> 5
        print(f"{data.size} bytes, {len(length)} runs, {bits} bits; slot words {sorted(set(nslot.tolist()))[:12]} ...")
        print("capacities", middle_round_cap(start, length), "missing", missing)
    assert not missing, missing
    if mode == "list":
        return
    from enc_local_cases import Device, check
    os.environ["AEC_ENC_LOCAL"] = "1"
    os.environ["AEC_ENC_LOCAL_SPW"] = str(SPW)
    dev, n = Device(), 0
    nbytes = (bits + 7) // 8
    if mode == "runs":
        check(dev, data, PRM, "runs of 8 segments")
        # the stream back through the decoder
        torch, codec = dev.torch, dev.codecs[PRM]
        d_out, got_bytes, got_bits, _, d_off = codec.encode(torch.from_numpy(data).cuda())
        assert got_bits == bits and d_out[:nbytes].cpu().numpy().tobytes() == want[:nbytes]
        d_dec, status = codec.decode(d_out, got_bytes, d_off, codec.rsi_count(data.size), len(trace))
        assert status == 0 and d_dec.cpu().numpy()[:data.size].tobytes() == data.tobytes(), "decode round trip"
        n += 2
    else:
        for spw in (1, 32, SPW):
            os.environ["AEC_ENC_LOCAL_SPW"] = str(spw)
            check(dev, data, PRM, f"runs of {spw} segments into 0xFF", fill=0xFF)
            n += 1
        for spw in (SPW, 1, 32):
            os.environ["AEC_ENC_LOCAL_SPW"] = str(spw)
            for cap in middle_round_cap(start, length):
                out, _, res, _ = dev.encode(data, PRM, fill=0xFF, out_cap=cap)
                assert int(res["overflow"]) == 1 and int(res["total_bits"]) == bits, (spw, cap)
                assert np.all(out[cap:] == 0xFF), (spw, cap, "bytes behind the capacity were written")
                if out[:cap].tobytes() != want[:cap]:
                    bad = next(i for i in range(cap) if out[i] != want[i])
                    raise AssertionError((spw, cap, "stream differs at byte", bad))
                n += 1
    print("place rounds ok:", mode, n, "cases; AEC_AMD_LIB=%s" % os.environ.get("AEC_AMD_LIB"))


if __name__ == "__main__":
    main()
