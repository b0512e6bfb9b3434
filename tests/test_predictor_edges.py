"""tests/predictor_edges.py on the CPU: the vectors really sit on the thresholds they are meant for (coverage is a
condition, not a hope), the predictor written from the standard agrees with the oracle and -- where it is built -- with
the compiled reference on every one of them, the lane functions code them as the oracle does, and the reference's
hashes in tests/golden/predictor_edges.json are the oracle's."""
import numpy as np
import pytest

import predictor_edges as E
from helpers import AEC_OK, bytes_per_sample, have_ref, oracle_decode, oracle_encode, ref_decode, ref_encode
from test_lane_emul import check_case, emul  # noqa: F401  (emul: the fixture that builds tests/emul)

CASES = E.cases()
IDS = [E.case_id(f, c) for f, c in CASES]


def test_the_predictor_is_its_own_inverse():
    """fwd and inv over every ordered pair of a small range, unsigned and signed, and at the ends of a 32-bit one"""
    for xmin, xmax in ((0, 7), (-4, 3), (0, 31), (-16, 15)):
        for prev in range(xmin, xmax + 1):
            seen = set()
            for cur in range(xmin, xmax + 1):
                d = E.fwd(prev, cur, xmin, xmax)
                assert 0 <= d <= xmax - xmin and d not in seen
                seen.add(d)
                assert E.inv(prev, d, xmin, xmax) == cur
    xmin, xmax = E.limits(32, E.SGN)
    for prev in (xmin, xmin + 1, -1, 0, xmax - 1, xmax):
        for cur in (xmin, xmin + 1, -1, 0, 1, xmax - 1, xmax):
            assert E.inv(prev, E.fwd(prev, cur, xmin, xmax), xmin, xmax) == cur
    assert E.fwd(1 << 31, 0, 0, (1 << 32) - 1) == (1 << 32) - 1            # the issue's example: 2^31 -> 0 -> 1 -> 1
    assert E.walk([0, (1 << 32) - 1, 1, 0], 1 << 31, 0, (1 << 32) - 1) == [1 << 31, 0, 1, 1]


@pytest.mark.parametrize("family,cfg", CASES, ids=IDS)
def test_vector_sits_on_its_thresholds(family, cfg):
    x, _ = E.vector(family, cfg)
    have = E.measure(x, *cfg)
    need = E.required(family, cfg)
    assert need
    print(E.case_id(family, cfg), x.size, "samples", {k: have[k] for k in need})
    short = {k: (have.get(k, 0), n) for k, n in need.items() if have.get(k, 0) < n}
    assert not short, short
    # the vectorised residuals of the model are fwd(), sample by sample (a slice of a large vector, every clipping step)
    d, clip = E.residuals(x, *cfg)
    xmin, xmax = E.limits(cfg[0], cfg[3])
    per_rsi = cfg[1] * cfg[2]
    pick = np.unique(np.concatenate([np.arange(min(x.size, 3000)), np.flatnonzero(clip)[:3000], np.flatnonzero(clip)[-500:]]))
    for i in pick:
        i = int(i)
        if i % per_rsi == 0:
            assert d[i] == 0
            continue
        p, c = int(x[i - 1]), int(x[i])
        assert int(d[i]) == E.fwd(p, c, xmin, xmax), (i, p, c)
        assert bool(clip[i]) == (abs(c - p) > min(p - xmin, xmax - p)), i
        assert E.inv(p, int(d[i]), xmin, xmax) == c, i


@pytest.mark.parametrize("family,cfg", CASES, ids=IDS)
def test_oracle_reference_and_golden_hash(family, cfg):
    """decode(encode(v)) is v (sign-extended containers for signed samples); the compiled reference, where built, writes
    and reads the same bytes; the hash of the reference's stream in the golden file is the hash of the oracle's"""
    bps, bs, rsi, flags = cfg
    x, data = E.vector(family, cfg)
    rc, enc, *_ = oracle_encode(data, bps, bs, rsi, flags)
    assert rc == AEC_OK
    nblk = (x.size + bs - 1) // bs
    cap = nblk * bs * bytes_per_sample(bps, flags)
    rc, dec, _ = oracle_decode(enc, bps, bs, rsi, flags, cap)
    assert rc == AEC_OK and dec == E.expected_decode(x, cfg)
    assert E.digest(enc) == E.golden()[E.case_id(family, cfg)]
    if have_ref():
        rc, r_enc = ref_encode(data, bps, bs, rsi, flags)
        assert rc == AEC_OK and r_enc == enc
        rc, r_dec = ref_decode(enc, bps, bs, rsi, flags, cap)
        assert rc == AEC_OK and r_dec == dec


def test_every_path_is_reached():
    """the decode paths that depend on the shape alone: each family has a configuration for the lane kernel (rsi < 16)
    and for the wave kernel -- but for the families bound to other RSI lengths"""
    for family, cfgs in E.CONFIGS.items():
        rsis = {c[2] for c in cfgs}
        assert any(r >= 16 for r in rsis), family
        if family not in ("inactive_lanes",) + E.BY_SEGMENTS:
            assert any(r < 16 for r in rsis), family


@pytest.mark.parametrize("family,cfg", [fc for fc in CASES if fc[0] in E.BY_SEGMENTS],
                         ids=[E.case_id(f, c) for f, c in CASES if f in E.BY_SEGMENTS])
def test_the_index_pass_will_leave_segment_starts(family, cfg):
    """The bare decode sums per segment only behind an index pass that leaves segment starts: the trunk or the regions
    (launch_index), which take a stream by its coded length per RSI.  A shape alone (rsi 512) does not reach it: the
    vectors that are about the segments' intervals must be coded long enough, by the library's own plan for them."""
    from libaec_amd import gpu
    bps, bs, rsi, flags = cfg
    _, data = E.vector(family, cfg)
    rc, enc, _, offs, _ = oracle_encode(data, bps, bs, rsi, flags)
    assert rc == AEC_OK
    hint = len(enc) * 8 // (offs.size + 1)                   # (what the pass assumes when called for offs.size + 1 RSIs)
    chain = gpu.index_plan(bps, bs, rsi, flags, len(enc), hint, 0, True)[0]
    assert set(chain) & {3, 5}, [gpu.INDEX_SCHEMES[s] for s in chain]


def test_golden_file_lists_exactly_the_cases():
    assert sorted(E.golden()) == sorted(IDS)


@pytest.mark.parametrize("family", list(E.FAMILIES))
def test_lane_functions_on_the_vectors(emul, family):  # noqa: F811
    for cfg in E.CONFIGS[family]:
        bps, bs, rsi, flags = cfg
        _, data = E.vector(family, cfg)
        rc, enc, *_ = oracle_encode(data, bps, bs, rsi, flags)
        assert rc == AEC_OK
        check_case(emul, E.case_id(family, cfg), bps, bs, rsi, flags, np.asarray(data), enc)
