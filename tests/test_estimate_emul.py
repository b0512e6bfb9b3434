"""CPU check of the size estimate's arithmetic (libaec_amd/csrc/aec_est.h) through the host harness
tests/emul/est_emul.cpp: what k_est_blocks does piece by piece and k_est_sum segment by segment, against the oracle
per block and per size, and against the reference's stream length where the reference is built."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import estimate_cases as ec
from helpers import OPT_ZERO, OPT_ZERO_CONT, ROOT, have_ref, ref_encode

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libest_emul.so")


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "est_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h)
                                                       for h in ("aec_est.h", "aec_lane.h", "aec_cfg.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", EMUL_SO, srcs[0]],
                       check=True)
    lib = C.CDLL(EMUL_SO)
    lib.est_emul.restype = C.c_int
    return lib


def run_emul(lib, data, bps, flags, vec):
    a = np.ascontiguousarray(data, dtype=np.uint8)
    n = ec.samples_of(a, bps, flags)
    nblk = [(n + (8 << i) - 1) // (8 << i) for i in range(4)]
    bits = [np.zeros(max(b, 1), np.uint32) for b in nblk]
    kind = [np.full(max(b, 1), 9, np.uint8) for b in nblk]
    total = (C.c_uint64 * 4)()
    best, mask = C.c_uint32(99), C.c_uint32(0)
    rsi = (C.c_uint * 4)(*vec) if vec is not None else None
    rc = lib.est_emul((C.c_uint32 * 2)(bps, flags), rsi, C.c_uint32(ec.RSI_ALL), C.c_void_p(a.ctypes.data),
                      C.c_size_t(a.size), total, C.byref(best), C.byref(mask),
                      (C.c_void_p * 4)(*[b.ctypes.data for b in bits]), (C.c_void_p * 4)(*[k.ctypes.data for k in kind]))
    return rc, list(total), best.value, mask.value, [b[:m] for b, m in zip(bits, nblk)], [k[:m] for k, m in zip(kind, nblk)]


def check(lib, key, data, bps, flags, vec):
    rc, total, best, mask, bits, kind = run_emul(lib, data, bps, flags, vec)
    assert rc == 0, key
    want, want_best = ec.expected(key, data, bps, flags, vec)
    assert mask == sum(1 << i for i in range(4) if ec.rsi_of(vec, i)), key
    for i in range(4):
        r = ec.rsi_of(vec, i)
        if not r:
            assert total[i] == (1 << 64) - 1, (key, i)
            continue
        o_bits, trace, o_len = ec.oracle_bits(key, data, bps, flags, i, r)
        if len(trace):
            bad = np.flatnonzero(bits[i] != trace["bits"])
            assert bad.size == 0, (key, vec, i, int(bad[0]), int(bits[i][bad[0]]), int(trace["bits"][bad[0]]))
            assert np.array_equal(kind[i] == 1, trace["option"] == OPT_ZERO), (key, vec, i)
            assert np.array_equal(kind[i] == 2, trace["option"] == OPT_ZERO_CONT), (key, vec, i)
        assert total[i] == o_bits, (key, vec, i)
        if have_ref():
            rc_r, enc = ref_encode(data, bps, 8 << i, r, flags)
            assert rc_r == 0 and len(enc) == max(1, (o_bits + 7) // 8), (key, vec, i)
    assert (total, best) == (want, want_best), (key, vec)


@pytest.mark.parametrize("bps,flags", ec.PARAMS, ids=[ec.param_id(p) for p in ec.PARAMS])
def test_every_block_of_every_size_is_the_oracles(emul, bps, flags):
    rng = np.random.default_rng(1000 + bps * 64 + flags)
    for kind in ec.KINDS:
        for n in ec.LENGTHS:
            data = ec.make_data(rng, kind, n, bps, flags)
            for vec in ec.RSI_VECTORS:
                check(emul, (kind, n), data, bps, flags, vec)


@pytest.mark.parametrize("bps,flags", ec.PARAMS, ids=[ec.param_id(p) for p in ec.PARAMS])
def test_crafted_zero_runs(emul, bps, flags):
    rng = np.random.default_rng(7 + bps)
    for vi, vec in enumerate(ec.RSI_VECTORS):
        data = ec.crafted_zero_runs(rng, bps, flags, vec)
        check(emul, ("crafted", vi), data, bps, flags, vec)
        # the runs are there: every size sees zero blocks that start a run and blocks inside one
        _, _, _, _, _, kind = run_emul(emul, data, bps, flags, vec)
        for i in range(4):
            if ec.rsi_of(vec, i):
                assert (kind[i] == 1).any() and ((kind[i] == 2).any() or ec.rsi_of(vec, i) == 1), (vec, i)


def test_a_trailing_fraction_of_a_sample_is_ignored(emul):
    rng = np.random.default_rng(5)
    for bps, flags in [(16, ec.PP), (24, ec.PP | ec.B3), (32, ec.PP)]:
        data = ec.make_data(rng, "walk", 130, bps, flags)
        for cut in (1, 2):
            check(emul, ("cut", cut), data[:-cut], bps, flags, [128] * 4)


def test_refused_parameter_sets(emul):
    data = np.zeros(64, np.uint8)
    for bps, flags, vec in [(0, ec.PP, None), (33, ec.PP, None), (1, ec.PP | ec.SIGNED, None), (6, ec.PP | ec.RESTRICTED, None),
                            (8, ec.PP, [128, 4097, 128, 128]), (8, ec.PP, [0, 0, 0, 0])]:
        a = np.ascontiguousarray(data)
        total = (C.c_uint64 * 4)()
        best, mask = C.c_uint32(), C.c_uint32()
        rsi = (C.c_uint * 4)(*vec) if vec is not None else None
        ptrs = (C.c_void_p * 4)()
        rc = emul.est_emul((C.c_uint32 * 2)(bps, flags), rsi, C.c_uint32(ec.RSI_ALL), C.c_void_p(a.ctypes.data),
                           C.c_size_t(a.size), total, C.byref(best), C.byref(mask), ptrs, ptrs)
        assert rc == -1, (bps, flags, vec)
