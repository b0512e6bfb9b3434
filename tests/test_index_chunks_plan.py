"""aec_gpu_index_chunks_plan (include/aec_gpu.h; host arithmetic, no device): which streams of a batch of bare chunks
the every-bit scheme takes under the three ways an index pass can run, in how many rounds and with what workspace --
against a restatement of the limits in Python; refusals and rsi_entries are those of aec_gpu_decode_chunks_plan."""
import ctypes as C

import numpy as np
import pytest

from helpers import AEC_DATA_MSB, AEC_DATA_PREPROCESS as PP, AEC_DATA_SIGNED, AEC_NOT_ENFORCE, AEC_RESTRICTED
import helpers

from libaec_amd import gpu

PLANNED, SERIAL, EVERY_BIT = gpu.CHUNKS_INDEX_PLANNED, gpu.CHUNKS_INDEX_SERIAL, gpu.CHUNKS_INDEX_EVERY_BIT
DEFAULT_ROUND = 1 << 24
PARAM_SETS = [(8, 8, 128, PP), (16, 16, 64, PP), (16, 16, 128, 0), (32, 32, 100, PP | AEC_DATA_MSB | AEC_DATA_SIGNED),
              (16, 8, 1, PP), (8, 8, 256, PP), (8, 8, 257, PP), (8, 8, 300, PP)]


def slot(in_bytes):
    return (8 * in_bytes + 1 + 1023) // 1024 * 1024


def within(prm, in_bytes, round_bits=DEFAULT_ROUND):
    return 64 <= 8 * in_bytes <= (1 << 24) and prm[2] <= 256 and slot(in_bytes) <= round_bits


def rounds_of(slots, round_bits):
    """whole streams in the order of the chunks: a stream that does not fit opens the next round"""
    rounds, cur, largest = 0, 0, 0
    for s in slots:
        if cur == 0 or cur + s > round_bits:
            rounds += 1
            cur = 0
        cur += s
        largest = max(largest, cur)
    return rounds, largest


def blocks_of(prm, out_bytes):
    return (out_bytes // helpers.bytes_per_sample(prm[0], prm[3]) + prm[1] - 1) // prm[1]


IN_SIZES = [0, 1, 7, 8, 9, 100, 127, 128, 511, 512, 4000, 65536, 300000, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, 5 << 20]


@pytest.mark.parametrize("prm", PARAM_SETS, ids=lambda p: "-".join(str(x) for x in p))
def test_the_three_ways(prm):
    rng = np.random.default_rng(prm[0] + prm[2])
    for trial in range(6):
        n = int(rng.integers(1, 60))
        in_sizes = rng.choice(IN_SIZES, size=n).tolist()
        out_sizes = [int(rng.integers(0, 1 << 22)) for _ in range(n)]
        entries = gpu.decode_chunks_plan(*prm, out_sizes)["rsi_entries"]
        for round_bits in (0, 4096, 1 << 20):
            rb = round_bits or DEFAULT_ROUND
            serial = gpu.index_chunks_plan(*prm, in_sizes, out_sizes, SERIAL, round_bits)
            assert serial == {"taken": 0, "rounds": 0, "table_bits": 0, "rsi_entries": entries, "workspace_bytes": 0}
            every = gpu.index_chunks_plan(*prm, in_sizes, out_sizes, EVERY_BIT, round_bits)
            ok = [s for s in in_sizes if within(prm, s, rb)]
            rounds, largest = rounds_of([slot(s) for s in ok], rb)
            assert (every["taken"], every["rounds"], every["table_bits"], every["rsi_entries"]) == (len(ok), rounds, largest, entries)
            # 8 bytes per table entry at the least (12 with the hops) -- and not more than 16 and the chains
            assert (every["workspace_bytes"] == 0) == (not ok)
            if ok:
                assert every["workspace_bytes"] >= (12 if prm[2] > 16 else 8) * largest
                assert every["workspace_bytes"] <= 16 * largest + 16 * sum(8 * s for s in ok) + 64 * n + 4096
            planned = gpu.index_chunks_plan(*prm, in_sizes, out_sizes, PLANNED, round_bits)
            assert planned["taken"] <= every["taken"] and planned["rounds"] <= MOST_ROUNDS
            assert planned["rsi_entries"] == entries


MOST_ROUNDS = 16       # (kBsR of libaec_amd/csrc/aec_bsmall.h)
LEAST_BLOCKS = 128     # (kBsB0)


def test_planned_takes_few_long_streams_and_at_most_r_rounds():
    prm = (8, 8, 128, PP)
    out = lambda blocks: 8 * blocks
    # a few long streams: taken, with the short ones beside them left to the walker -- the rows of
    # profiles/r18/bench_index_chunks.txt in small: 16 chunks of up to 128 KiB, 64 x 1 MiB
    sizes = [40000] * 16 + [300] * 50
    outs = [out(16384)] * 16 + [out(LEAST_BLOCKS - 1)] * 50
    assert gpu.index_chunks_plan(*prm, sizes, outs, PLANNED)["taken"] == 16
    assert gpu.index_chunks_plan(*prm, sizes, outs, EVERY_BIT)["taken"] == 66
    mib = gpu.index_chunks_plan(*prm, [380000] * 64, [1 << 20] * 64, PLANNED)
    assert mib["taken"] == 64 and mib["rounds"] == 13
    # a thousand streams as long as the longest: the walk takes as long as one of them, the scheme as long as all
    assert gpu.index_chunks_plan(*prm, [40000] * 1024, [out(16384)] * 1024, PLANNED)["taken"] == 0
    # chunks below LEAST_BLOCKS blocks are never taken, nor streams outside the limits, however many blocks they announce
    assert gpu.index_chunks_plan(*prm, [300] * 4, [out(LEAST_BLOCKS - 1)] * 4, PLANNED)["taken"] == 0
    assert gpu.index_chunks_plan(*prm, [7, 5 << 20], [out(1 << 16)] * 2, PLANNED)["taken"] == 0
    assert gpu.index_chunks_plan(8, 8, 300, PP, [3000] * 4, [out(1 << 12)] * 4, PLANNED)["taken"] == 0
    # more rounds than R: only a threshold whose streams fit R rounds is chosen
    sizes = [2000] * 40                                    # a slot of 16384 each
    outs = [out(LEAST_BLOCKS * 16)] * 30 + [out(LEAST_BLOCKS * 1024)] * 10
    every = gpu.index_chunks_plan(*prm, sizes, outs, EVERY_BIT, 16384)
    planned = gpu.index_chunks_plan(*prm, sizes, outs, PLANNED, 16384)
    assert (every["taken"], every["rounds"]) == (40, 40)
    assert 0 < planned["taken"] == planned["rounds"] <= MOST_ROUNDS
    # ... and with room for all in one round all of them are taken
    assert gpu.index_chunks_plan(*prm, sizes, outs, PLANNED, 16384 * 40)["taken"] == 40


def test_round_bits_is_clamped():
    prm = (16, 16, 16, PP)
    sizes, outs = [511, 512, 100000], [1 << 16] * 3
    at = lambda rb: gpu.index_chunks_plan(*prm, sizes, outs, EVERY_BIT, rb)
    assert at(1) == at(4096) == at(100)                     # the minimum
    assert at(4096)["taken"] == 1 and at(4096)["table_bits"] == 4096
    assert at(5120)["taken"] == 2 and at(5120)["rounds"] == 2
    assert at(0) == at(1 << 24) == at(1 << 30) == at((1 << 64) - 1)      # the default, and everything above it
    assert at(0)["taken"] == 3 and at(0)["rounds"] == 1


def test_no_chunks_is_a_plan_of_nothing():
    got = gpu.index_chunks_plan(8, 8, 128, PP, [], [], EVERY_BIT)
    assert got == {"taken": 0, "rounds": 0, "table_bits": 0, "rsi_entries": 0, "workspace_bytes": 0}


def test_refusals_are_those_of_the_decode_plan():
    prm = (8, 8, 1, PP)
    most = (1 << 31) - 1
    for how in (PLANNED, SERIAL, EVERY_BIT):
        assert gpu.index_chunks_plan(*prm, [100], [8 * most], how)["rsi_entries"] == most + 1
        assert gpu.index_chunks_plan(*prm, [100, 100], [8 * most, 1], how) is None
        assert gpu.index_chunks_plan(*prm, [100], [8 * (most + 1)], how) is None
        for bad in [(0, 8, 128, PP), (33, 8, 128, PP), (8, 7, 128, PP | AEC_NOT_ENFORCE), (8, 8, 0, PP), (8, 8, 4097, PP),
                    (6, 8, 16, AEC_RESTRICTED)]:
            assert gpu._lib().aec_gpu_check_params(C.byref(gpu.Params(*bad)), 0) != 0
            assert gpu.decode_chunks_plan(*bad, [1000, 2000]) is None
            assert gpu.index_chunks_plan(*bad, [100, 100], [1000, 2000], how) is None
            assert gpu.index_chunks_plan(*bad, [], [], how) is None
