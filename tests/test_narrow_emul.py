"""The narrow cases (tests/narrow_cases.py: generic block sizes, samples below 8 bits, restricted code sets, odd containers)
on the CPU: the oracle's streams against the compiled reference, what the traces must hold, every CPU emulation of the
device code that applies to a case, and the table of schemes the GPU tests claim to exercise.

  * the oracle's stream of every case is the reference's, and both decode it to the same bytes at exact capacity;
  * per class the traces hold every code option and both kinds of zero run, and the "short" cases have coded data sets
    of fewer than 8 bits on average;
  * the every-bit scheme (small_emul), the trunk (trunk_emul) and the lane coder with the window tables (emul.cpp) run on
    every case; the region index (region_emul) and the entries by plausibility (plaus_emul) where their plans admit the
    stream -- NOT_APPLICABLE names the rest with the rule that keeps them out;
  * tests/golden/narrow_chain.json is what aec_gpu_index_plan says today for the streams of tests/test_gpu_narrow.py and
    what aec_gpu_index_scheme of the tuning build says for the shapes of tests/cross_scheme.py --narrow: a threshold that
    moves fails here, not by quietly routing every narrow stream back to the every-bit scheme.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import narrow_cases as N
from libaec_amd import gpu
from test_lane_emul import check_case, emul as lane_emul  # noqa: F401
from test_plaus_emul import emul as plaus_emul  # noqa: F401
from test_region_emul import emul as region_emul  # noqa: F401
from test_small_emul import emul as small_emul  # noqa: F401
from test_trunk_emul import emul as trunk_emul, run as trunk_run  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = N.golden_chains()


def emul_stream(c):
    """a stream of the case for the emulations that work bit by bit: two RSIs and a short third, 1500 blocks at least"""
    blocks = max(2 * c.rsi + max(1, c.rsi // 3), 1500)
    return N.coded(c, min(N.family_samples(c), blocks * c.bs) if c.rsi < 16 else blocks * c.bs - c.bs // 2)


# ---- the oracle's streams are the reference's --------------------------------------------------------------------

@pytest.mark.skipif(not H.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("cls", N.CLASSES)
def test_streams_are_the_references(cls):
    for c in N.of_class(cls):
        k = N.family(c)
        rc, enc = H.ref_encode(k.data, *N.prm(c))
        assert rc == H.AEC_OK and enc == k.stream, N.case_id(c)
        rc, dec = H.ref_decode(k.stream, *N.prm(c), len(k.decoded))
        assert rc == H.AEC_OK and dec == k.decoded, N.case_id(c)
        nb = H.bytes_per_sample(c.bps, c.flags)
        if not (c.flags & N.SGN and c.bps % 8):     # (signed samples come back sign-extended into their container)
            assert k.decoded[:k.data.size] == k.data.tobytes(), N.case_id(c)
        assert len(k.decoded) == k.nblk * c.bs * nb


# ---- what the traces hold ------------------------------------------------------------------------------------------

def test_the_case_list_is_the_one_the_classes_ask_for():
    assert 28 <= len(N.CASES) <= 40 and len(set(N.CASES)) == len(N.CASES)
    by = {cls: N.of_class(cls) for cls in N.CLASSES}
    assert {c.bs for c in by["generic"]} == {2, 4, 6, 10, 24, 62} and {c.bps for c in by["generic"]} == {1, 5, 8, 12, 16, 31}
    assert all(c.flags & N.NE for c in by["generic"])
    assert {c.bps for c in by["narrow"]} == {1, 2, 3, 5, 7} and not any(c.flags & N.R for c in by["narrow"])
    assert {8, 16} < {c.bs for c in by["narrow"]} and any(c.flags & N.NE for c in by["narrow"])
    assert {c.bps for c in by["restricted"]} == {1, 2, 3, 4} and {c.bs for c in by["restricted"]} == {2, 4, 16, 64}
    assert all(c.flags & N.R for c in by["restricted"])
    assert {H.id_len_of(c.bps, c.flags) for c in by["restricted"]} == {1, 2}
    assert {c.bps for c in by["odd"]} == {12, 20, 24, 31} and all(c.flags & N.B3 for c in by["odd"] if c.bps < 31)
    for cls, cases in by.items():
        # short, medium and multi-segment RSIs in every class; every RSI length of the list somewhere
        assert min(c.rsi for c in cases) <= 5 and max(c.rsi for c in cases) == 4096, cls
        assert any(16 <= c.rsi <= 64 for c in cases) and any(64 < c.rsi < 4096 for c in cases), cls
        assert {c.kind for c in cases} >= {"walk", "noise"}, cls
    assert {c.rsi for c in N.CASES} == set(N.RSIS)
    assert {c.kind for c in N.CASES} == set(N.KINDS)
    # signed only where samples come back as they went in
    assert all(c.bps % 8 == 0 for c in N.CASES if c.flags & N.SGN)


@pytest.mark.parametrize("cls", N.CLASSES)
def test_traces_hold_every_option_and_run(cls):
    seen = set()
    for c in N.of_class(cls):
        k = N.family(c)
        seen |= N.features(c, k.trace)
        mean = N.mean_cds_bits(k.trace)
        print(N.case_id(c), f"{len(k.stream)} bytes, {mean:.2f} bits per coded data set")
        if c.short:
            assert mean < 8.0, (N.case_id(c), mean)
    assert any(c.short for c in N.of_class(cls)) or cls == "odd"
    assert seen == set(N.FEATURES), (cls, sorted(set(N.FEATURES) - seen))


# ---- the emulations -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", N.CASES, ids=N.case_id)
def test_every_bit_scheme(small_emul, c):  # noqa: F811
    """tests/test_small_emul.py on the case: the chain of RSI starts is the oracle's, the walk through the hop tables is
    the walk without them at every bit"""
    k = emul_stream(c)
    want = np.asarray(k.offs, dtype=np.uint64)
    enc_a = np.frombuffer(k.stream, dtype=np.uint8)
    whole = k.nblk // c.rsi
    p = (C.c_uint32 * 4)(*N.prm(c))
    for hops in (0, 1, 2):
        stats = np.zeros(4, dtype=np.uint64)
        rc = small_emul.emul_small(p, C.c_void_p(enc_a.ctypes.data), C.c_size_t(enc_a.size), C.c_void_p(want.ctypes.data),
                                   C.c_uint64(len(want)), C.c_uint32(hops), C.c_void_p(stats.ctypes.data))
        m, bad, differ, _ = (int(x) for x in stats)
        assert rc == 0 and bad == 0 and differ == 0, (hops, m, bad, differ)
        assert m >= min(len(want), whole + (1 if k.nblk % c.rsi else 0)), (hops, m, len(want), whole)


@pytest.mark.parametrize("c", N.CASES, ids=N.case_id)
def test_trunk(trunk_emul, c):  # noqa: F811
    """tests/test_trunk_emul.py on the case: every record at a true RSI start is the serial walk's, with short and long
    windows, walks in memory and on staged stretches"""
    k = emul_stream(c)
    for L, lead, staged, budget in ((1024, 0, 0, 64), (4096, 8192, 1, 32768), (16384, 1024, 3, 4096)):
        trunk_run(trunk_emul, k.stream, k.offs, k.bits, *N.prm(c), L=L, lead=lead, staged=staged, budget=budget)


@pytest.mark.parametrize("c", N.CASES, ids=N.case_id)
def test_lane_coder_and_window_tables(lane_emul, c):  # noqa: F811
    """tests/test_lane_emul.py: check_case -- the lane encoder's stream, trace and offsets, the lane decoder, the serial
    index walk and the speculative tables at every true RSI start"""
    k = emul_stream(c)
    check_case(lane_emul, N.case_id(c), *N.prm(c), k.data, k.stream)


def region_admits(c, row):
    """aec_region.hip: region_plan -- the preprocessor's reference samples, block headers of three bits and more, RSIs of 48
    blocks and more, coded data sets of 8 bits and more on average; the rest is the size of the stream"""
    if not c.flags & N.PP:
        return "no preprocessor: no reference sample to look for"
    if H.id_len_of(c.bps, c.flags) < 3:
        return "block headers of fewer than three bits"
    if c.rsi < 48:
        return "RSIs of fewer than 48 blocks"
    if row["rsi_bits"] // c.rsi < 8:
        return "coded data sets of fewer than 8 bits on average"
    raw = c.rsi * (H.id_len_of(c.bps, c.flags) + c.bs * c.bps)
    if row["rsi_bits"] + raw // 32 >= raw and row["rsi_bits"] <= raw + 64:
        return "RSIs as long as uncompressed ones (aec_cfg.h: index_incompressible)"
    return None


FORCED_ROWS = [(c, nbytes, GOLDEN["forced"][N.case_id(c)]) for c, nbytes in N.FORCED]
REGION_OK = [(c, nbytes) for c, nbytes, row in FORCED_ROWS if N.REGIONS in row["schemes"]]
NOT_APPLICABLE = {
    "region_emul": {N.case_id(c): region_admits(c, row) for c, nbytes, row in FORCED_ROWS if N.REGIONS not in row["schemes"]},
}


def test_the_region_index_admits_what_the_table_says():
    """every shape of FORCED either runs through region_emul below or is named in NOT_APPLICABLE with the rule of
    region_plan that keeps it out (a shape the plan keeps out for its size alone would have no rule to name)"""
    assert len(REGION_OK) >= 3 and {c.cls for c, _ in REGION_OK} == {"generic", "narrow", "odd"}
    for c, nbytes, row in FORCED_ROWS:
        why = region_admits(c, row)
        if N.REGIONS in row["schemes"]:
            assert why is None, (N.case_id(c), why)
        else:
            assert why is not None and NOT_APPLICABLE["region_emul"][N.case_id(c)] == why, N.case_id(c)
    # every restricted shape is out for its header, whatever else
    assert all(NOT_APPLICABLE["region_emul"][N.case_id(c)] for c, _ in N.FORCED if c.cls == "restricted")


@pytest.mark.parametrize("c,nbytes", REGION_OK, ids=[N.case_id(c) for c, _ in REGION_OK])
def test_region_index(region_emul, c, nbytes):  # noqa: F811
    """tests/test_region_emul.py: the whole pass -- guesses, walks, mending passes -- delivers the oracle's table, with the
    guesses as they are and with every third one 7 bits off"""
    k = N.coded(c, N.forced_samples(c, nbytes))
    enc = np.frombuffer(k.stream, dtype=np.uint8)
    offs = np.ascontiguousarray(k.offs)
    p = (C.c_uint32 * 4)(*N.prm(c))
    cds = N.rsi_bits_hint(k) // c.rsi
    # (region_plan's budget: RSIs of up to 512 blocks are verified, three-bit options say less)
    budget = ((4 if H.id_len_of(c.bps, c.flags) <= 3 else 3) if c.rsi <= 512 else 2) * c.rsi + 384 + 3 * cds
    region = (max(N.rsi_bits_hint(k), 16384) + 63) // 64 * 64      # (region_plan: an RSI at least, 16 kbit at least)
    for sabotage_every, shift, passes in ((0, 0, 12), (3, -7, 400)):
        stats = np.zeros(16, dtype=np.uint64)
        out = np.zeros(offs.size + 8, dtype=np.uint64)
        rc = region_emul.emul_region_index(p, C.c_void_p(enc.ctypes.data), C.c_size_t(enc.size), C.c_uint64(region), C.c_uint32(budget),
                                           C.c_uint32(passes), C.c_uint32(sabotage_every), C.c_int64(shift),
                                           C.c_void_p(out.ctypes.data), C.c_uint64(out.size), C.c_void_p(stats.ctypes.data))
        nreg, kept, differ, busy, delivered = (int(x) for x in stats[:5])
        print(N.case_id(c), "regions", nreg, "kept", kept, "differ", differ, "passes with work", busy, "delivered", delivered)
        assert rc == 0 and nreg >= 16
        # A pass that does not deliver leaves the stream to the schemes behind it (speed, not bytes): what the scheme
        # promises is that a table it does deliver is exact.  (As written: RSIs of 65 and 128 blocks of 16 deliver, with
        # and without the sabotage; with RSIs of 300 generic blocks one guess in ten is kept, walks between kept regions
        # outrun their 16 regions and the pass gives the stream up.)
        if delivered:
            assert np.array_equal(out[: offs.size], offs), (N.case_id(c), sabotage_every)


def plaus_admits(c, row):
    """aec_idx.hip: lock_plan -- entries by plausibility need the preprocessor's reference samples, and coded data sets
    long enough for their options to say something (32 bits with headers of four bits and RSIs of up to 44 blocks, 96
    else); where the 64 agreeing chains serve the stream (mode 0) no entry is guessed"""
    if not c.flags & N.PP:
        return "no preprocessor: no reference sample to look for"
    cds, idl = row["rsi_bits"] // c.rsi, H.id_len_of(c.bps, c.flags)
    if cds < (32 if c.rsi <= 44 and idl >= 4 else 96):
        return "coded data sets too short for their options to tell"
    return None


DISPATCH_ROWS = [(c, n, first, row) for (c, n, first), row in zip(N.DISPATCH, GOLDEN["dispatch"])]
# the streams whose shipped chain guesses entries: the phase-locked chains with another scheme enqueued behind them
PLAUS_OK = [(c, n) for c, n, first, row in DISPATCH_ROWS if row["chain"][0] == N.LOCKED and len(row["chain"]) > 1]
NOT_APPLICABLE["plaus_emul"] = {N.case_id(c): plaus_admits(c, row) or "the chain is not the plausibility scheme's: %s" % row["chain"]
                                for c, n, first, row in DISPATCH_ROWS if (c, n) not in PLAUS_OK}


def test_the_plausibility_scheme_admits_what_the_table_says():
    assert PLAUS_OK and all(plaus_admits(c, row) is None for c, n, _, row in DISPATCH_ROWS if (c, n) in PLAUS_OK)
    assert len(PLAUS_OK) + len(NOT_APPLICABLE["plaus_emul"]) == len(N.DISPATCH)
    assert all(NOT_APPLICABLE["plaus_emul"].values())
    for c, n, _, row in DISPATCH_ROWS:
        if not c.flags & N.PP:
            assert NOT_APPLICABLE["plaus_emul"][N.case_id(c)].startswith("no preprocessor")


@pytest.mark.parametrize("c,n", PLAUS_OK, ids=[N.case_id(c) for c, _ in PLAUS_OK])
def test_entries_by_plausibility(plaus_emul, c, n):  # noqa: F811
    """tests/test_plaus_emul.py: the model of k_lock_guess_p runs on the stream and classifies every region's guess as
    right, none or wrong against the true RSI starts.  Nothing rests on a guess in the product (every entry is checked and
    mended, a judge hands streams whose options say nothing to the scheme behind): what is asserted is that the model
    parses these streams and accounts for every region, the shares are printed."""
    k = N.coded(c, n)
    enc = np.frombuffer(k.stream, dtype=np.uint8)
    p = (C.c_uint32 * 4)(*N.prm(c))
    stats = np.zeros(4, dtype=np.uint64)
    rc = plaus_emul.emul_plaus(p, C.c_void_p(enc.ctypes.data), C.c_size_t(enc.size), C.c_uint32(1), C.c_void_p(stats.ctypes.data))
    regions, right, none, wrong = (int(x) for x in stats)
    print(N.case_id(c), "regions", regions, "right", right, "none", none, "wrong", wrong)
    assert rc == 0 and regions > 0 and right + none + wrong == regions


# ---- the table of schemes ---------------------------------------------------------------------------------------------

def test_the_table_covers_every_stream_and_every_class_meets_every_scheme():
    assert [r["case"] for r in GOLDEN["dispatch"]] == [N.case_id(c) for c, _, _ in N.DISPATCH]
    assert sorted(GOLDEN["forced"]) == sorted(N.case_id(c) for c, _ in N.FORCED)
    for cls in N.CLASSES:
        # the shipped dispatch: the chains, the tables and the trunk each come first for a stream of the class (no pair is
        # left to the forced schemes alone), none of more than 8 MiB
        rows = [r for r in GOLDEN["dispatch"] if r["class"] == cls]
        assert sorted(r["first_scheme"] for r in rows) == [N.LOCKED, N.TABLES, N.TRUNK], cls
        assert all(r["in_bytes"] <= 8 << 20 for r in rows)
        # forced: every scheme that admits the class
        legal = {s for c, _ in N.FORCED if c.cls == cls for s in GOLDEN["forced"][N.case_id(c)]["schemes"]}
        assert legal == ({1, 2, 3, 4} if cls == "restricted" else {1, 2, 3, 4, 5}), (cls, legal)
    assert any(c.short for c, _, _ in N.DISPATCH) and any(c.short for c, _ in N.FORCED)


@pytest.mark.parametrize("c,n,first,row", DISPATCH_ROWS, ids=[N.case_id(c) for c, _, _, _ in DISPATCH_ROWS])
def test_dispatch_chain(c, n, first, row):
    """the golden row is this stream's (size, mean coded RSI) and aec_gpu_index_plan gives its chain for them"""
    k = N.coded(c, n)
    assert (row["samples"], row["in_bytes"], row["rsi_bits"]) == (n, len(k.stream), N.rsi_bits_hint(k)), N.case_id(c)
    if c.short:
        assert N.mean_cds_bits(k.trace) < 8.0
    ids, asked, large, used = gpu.index_plan(*N.prm(c), row["in_bytes"], row["rsi_bits"])
    assert ids == row["chain"] and ids[0] == first == row["first_scheme"], (N.case_id(c), [gpu.INDEX_SCHEMES[i] for i in ids])
    assert gpu.index_scheme(*N.prm(c), row["in_bytes"], row["rsi_bits"], 0) == first
    assert used <= asked


def test_forced_schemes():
    """the schemes the tuning build names for the shapes of tests/cross_scheme.py --narrow as its switches take them away
    (host arithmetic in a child process: the switches are read from the environment of the tuning build only)"""
    env = dict(os.environ, AEC_AMD_LIB=os.path.join(ROOT, "libaec_amd", "lib", "tuning", "libaec.so.0"))
    assert os.path.exists(env["AEC_AMD_LIB"])
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "narrow_cases.py"), "forced"], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout) == GOLDEN["forced"]


# ---- the SZIP fixture ---------------------------------------------------------------------------------------------------

def test_szip_fixture_is_the_reference_shims():
    """tests/golden/narrow_sz.json: the inputs generated here are the fixture's (sz_golden asserts their digests), and --
    where the compiled reference is at hand -- its shim makes the fixture's streams of them"""
    import hashlib
    from libaec_amd import szip
    rows = N.sz_golden()
    assert [(r[0], r[1]) for r in rows] == [(s[0], s[1]) for s in N.SZ_SHAPES]
    if not H.have_ref():
        return
    ref = szip.bind(C.CDLL(H.REF_SO))
    for name, prm, data, want_len, want_sha in rows:
        rc, comp = szip.compress(data, data.size * 2 + 4096, *prm, lib=ref)
        assert rc == 0 and (len(comp), hashlib.sha256(comp).hexdigest()) == (want_len, want_sha), name
