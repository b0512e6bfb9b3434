"""tests/foreign_predictor.py on the CPU: the streams really take the predictor's state outside the sample range and bring
it back where the per-block test of the decoder kernels is blind (coverage is a condition, not a hope); the reference's
step restated in Python integers gives the oracle's bytes for every one of them and -- where it is built -- the compiled
reference's, with AEC_OK; the hashes of the reference's bytes in tests/golden/foreign_predictor.json are the oracle's."""
import os

import numpy as np
import pytest

import foreign_predictor as F
from helpers import AEC_OK, bytes_per_sample, have_ref, oracle_decode, pack_samples, ref_decode

CASES = F.cases()
IDS = [F.case_id(f, c) for f, c in CASES]


def test_step_is_the_predictor_of_valid_streams():
    """on states and residuals inside the range step() is the inverse of the standard's mapping (predictor_edges.fwd)"""
    import predictor_edges as E
    for bps, flags in ((3, 0), (3, F.SGN), (5, 0), (5, F.SGN)):
        xmin, xmax = F.limits(bps, flags)
        for prev in range(xmin, xmax + 1):
            for cur in range(xmin, xmax + 1):
                d = E.fwd(prev, cur, xmin, xmax)
                assert F.as_int(F.step(prev & F.M32, d, bps, flags), flags) == cur, (bps, flags, prev, cur)
    # and outside it: the issue's two blocks, step by step
    assert F.step(0xFFF0, 0x1FFFA, 16, 0) == 0x10005
    assert F.step(0x10005, 11, 16, 0) == 0xFFFF and F.step(0xFFFF, 2, 16, 0) == 0xFFFD
    # signed: out below by one, back in by a two-sided step, then one-sided at xmin
    assert F.as_int(F.step(5, 256 + 0, 8, F.SGN), F.SGN) == 127 - 256 == -129
    assert F.as_int(F.step(-129 & F.M32, 2, 8, F.SGN), F.SGN) == -128
    assert F.as_int(F.step(-128 & F.M32, 3, 8, F.SGN), F.SGN) == 3 - 128


def test_the_issues_stream():
    """the 20 bytes of the issue, verbatim: the writer produces them from the coded data sets it names, the walk, the
    oracle and the reference give its 16 samples"""
    cfg = F.ISSUE_CFG
    v = F.write_stream(cfg, [("split", 13, [0xFFF0, 0x1FFFA, 0, 0, 0, 0, 0, 0]), ("split", 0, [11, 2, 0, 0, 0, 0, 0, 0])])
    assert v["stream"] == F.ISSUE_STREAM and len(F.ISSUE_STREAM) == 20
    want = pack_samples(F.ISSUE_SAMPLES, 16, 0).tobytes()
    front, _, got = F.walk(cfg, v["d"])
    assert got == want and int(front[1]) == 0x10005
    rc, dec, _ = oracle_decode(F.ISSUE_STREAM, *cfg, 32)
    assert rc == AEC_OK and dec == want
    assert F.golden()["issue"]["decoded"] == F.digest(want)
    m = F.measure(cfg, v["d"])
    assert m["passes_wrapped"] == 1 and m["differs_uniform"] == 1 and m["state_out"] == 1, m
    if have_ref():
        rc, dec = ref_decode(F.ISSUE_STREAM, *cfg, 32)
        assert rc == AEC_OK and dec == want


@pytest.mark.parametrize("family,cfg", CASES, ids=IDS)
def test_vector_reaches_its_conditions(family, cfg):
    v = F.vector(family, cfg)
    have = F.measure(cfg, v["d"])
    need = F.required(family, cfg)
    assert need
    print(F.case_id(family, cfg), v["nblk"] * cfg[1], "samples", len(v["stream"]), "bytes",
          {k: have.get(k) for k in need})
    short = F.reaches(have, need)
    assert not short, short
    assert v["nblk"] * cfg[1] <= (F.MAX_SAMPLES if family == "big_table" else 100000)


@pytest.mark.parametrize("family,cfg", CASES, ids=IDS)
def test_walk_oracle_reference_and_golden_hash(family, cfg):
    """the oracle decodes the stream with AEC_OK to exactly the bytes of the Python walk; the compiled reference, where
    built, returns the same; the golden file holds the hash of the reference's bytes"""
    bps, bs, rsi, flags = cfg
    v = F.vector(family, cfg)
    cap = v["nblk"] * bs * bytes_per_sample(bps, flags)
    rc, dec, _ = oracle_decode(v["stream"], bps, bs, rsi, flags, cap)
    assert rc == AEC_OK and dec == v["bytes"]
    g = F.golden()[F.case_id(family, cfg)]
    assert F.digest(v["stream"]) == g["stream"], "the generated stream is not the one the reference was given"
    assert F.digest(dec) == g["decoded"]
    if have_ref():
        rc, r_dec = ref_decode(v["stream"], bps, bs, rsi, flags, cap)
        assert rc == AEC_OK and r_dec == dec


WAVE = [(f, c) for f, c in CASES if c[2] >= 16 and c[3] & F.PP and c[1] != 24 and f != "big_table"]


@pytest.mark.parametrize("family,cfg", WAVE, ids=[F.case_id(f, c) for f, c in WAVE])
def test_the_wave_kernels_correction_ends(family, cfg):
    """k_decode_wave puts the lanes of a round right one after the other, which ends only if a block's samples are the
    same whichever way the wavefront went (F.wave_rounds).  With the sum test alone, the vectors that return into the range
    at the start of a round send that loop round for ever -- on the device: a kernel that does not return; with the
    state in front inside the range as part of the test, every round of every vector ends."""
    v = F.vector(family, cfg)
    rounds, endless = F.wave_rounds(cfg, v["d"], True)
    assert rounds and endless == 0
    _, endless_before = F.wave_rounds(cfg, v["d"], False)
    print(F.case_id(family, cfg), rounds, "rounds;", endless_before, "would not end with the sum test alone")
    if family in ("leave_and_return", "below", "edge_out") and cfg[2] > 64:
        assert endless_before >= 8
    if family == "edge_in":
        assert endless_before == 0


def test_golden_file_lists_exactly_the_cases():
    assert sorted(F.golden()) == sorted(IDS + ["issue"])


def test_configs_cover_the_store_forms_and_kernel_families():
    out = [c for f in ("leave_and_return", "below", "hover", "edge_out") for c in F.CONFIGS[f]]
    assert {bytes_per_sample(c[0], c[3]) for c in out} == {1, 2, 3, 4}
    assert {c[0] for c in out} >= {5, 8, 12, 16, 20, 24, 31}
    assert {c[1] for c in out} >= {8, 16, 24, 32, 64}
    assert {c[2] for c in out} >= {2, 16, 100, 130, 512}
    for flag in (F.SGN, F.MSB, F.B3, F.NE):
        assert any(c[3] & flag for c in out) and any(not c[3] & flag for c in out)
    # more than 4096 RSIs of 16 blocks of 8 samples, all of one layout, and the table bound that sends them to the lane
    # kernel: above the most items the wave kernel takes, which as many RSIs as that could not be within the sample limit
    assert F.N_BIG_RSI > 4096 and F.CONFIGS["big_table"] == [(16, 8, 16, F.PP)]
    assert F.LANE_TABLE_BOUND > F.WAVE_MAX_ITEMS == 8192 and (F.WAVE_MAX_ITEMS + 1) * 16 * 8 > F.MAX_SAMPLES
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "libaec_amd", "csrc", "aec_dec.hip")) as f:
        assert 'tune("AEC_DEC_WAVE_MAX", %du)' % F.WAVE_MAX_ITEMS in f.read()
    for f in ("leave_and_return", "below", "hover", "edge_out"):       # both kernels see wrong blocks in every family
        assert any(c[2] < 16 for c in F.CONFIGS[f]) and any(c[2] > 64 for c in F.CONFIGS[f]), f


def test_segment_starts_of_the_writer():
    """the writer's segment starts: one entry per 64 blocks of an RSI, the first the RSI's own start, rising, and none
    for the segments a short last RSI does not have"""
    v = F.vector("leave_and_return", (16, 16, 130, F.PP))
    spr = 3
    assert v["seg_bits"].size == v["rsi_bits"].size * spr
    assert np.array_equal(v["seg_bits"][::spr], v["rsi_bits"])
    sb = v["seg_bits"].reshape(-1, spr)
    assert (np.diff(sb[:-1].astype(np.int64), axis=1) > 0).all()
    last = v["nblk"] - (sb.shape[0] - 1) * 130                   # blocks of the short last RSI
    assert [int(x != 0xFFFFFFFFFFFFFFFF) for x in sb[-1]] == [1, int(last > 64), int(last > 128)]
    assert np.array_equal(v["blk_bits"][::130], v["rsi_bits"]) and (np.diff(v["blk_bits"].astype(np.int64)) >= 0).all()


# the first ten cases of tests/fuzz_corrupt_gpu.py, seed 13, recorded before the sweep had its `containers` switch:
# (bps, bs, rsi, flags, room, length of the damaged stream, first 16 hex digits of its SHA-256)
SEED_13 = [(32, 64, 1024, 8, 8000000, 101654, "43de0053c4a92df6"), (32, 32, 1024, 8, 160000, 15340, "76a58861b8665ed1"),
           (32, 8, 16, 8, 8000, 1815, "25de1e6150b79bac"), (16, 8, 16, 8, 4000, 887, "9d698dbf34ff9b97"),
           (16, 32, 128, 8, 80000, 40553, "c5f51edf92ac0385"), (16, 64, 1024, 8, 600064, 156230, "4b3b113683c97900"),
           (32, 16, 16, 8, 8000000, 491638, "82d0e0fa69ef540f"), (16, 8, 1, 8, 4000000, 819681, "4e07b800f3eea01e"),
           (32, 16, 128, 8, 1200000, 198307, "89590fc094e51f8e"), (16, 64, 128, 8, 4096, 890, "d3d4f909ac2b2e3f")]


class _Enough(Exception):
    pass


def _sweep_cases(args, count):
    """the first `count` streams tests/fuzz_corrupt_gpu.py hands to the decoder (the oracle stands in for it)"""
    import hashlib

    import fuzz_corrupt_gpu
    seen = []

    def decode(enc, bps, bs, rsi, flags, room):
        seen.append((bps, bs, rsi, flags, room, len(enc), hashlib.sha256(bytes(enc)).hexdigest()[:16]))
        if len(seen) == count:
            raise _Enough
        rc, dec, _ = oracle_decode(enc, bps, bs, rsi, flags, room)
        return rc, dec

    with pytest.raises(_Enough):
        fuzz_corrupt_gpu.run(args, decode=decode)
    return seen


def test_the_corrupt_sweep_draws_what_it_drew():
    """without the switch -- a Namespace that has no such attribute, as the existing callers pass -- every draw of seed 13
    is unchanged: parameters, sizes and the damaged bytes of its first ten cases"""
    import argparse
    assert _sweep_cases(argparse.Namespace(cases=60, seed=13), 10) == SEED_13


def test_the_corrupt_sweep_with_containers():
    """with the switch: bps 5, 12, 20, 24 in 3-byte containers and 31, MSB and signed at random, at most 40 000 samples"""
    import argparse
    seen = _sweep_cases(argparse.Namespace(cases=40, seed=14, containers=True), 40)
    assert {c[0] for c in seen} == {5, 12, 20, 24, 31}
    for bps, bs, rsi, flags, room, _, _ in seen:
        assert bool(flags & F.B3) == (bps == 24) and flags & F.PP
        assert room <= (40000 + bs) * bytes_per_sample(bps, flags)
    assert {bool(c[3] & F.MSB) for c in seen} == {False, True} and {bool(c[3] & F.SGN) for c in seen} == {False, True}
