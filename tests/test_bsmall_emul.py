"""The every-bit index scheme over a BATCH of bare streams (libaec_amd/csrc/aec_bsmall.h) on the CPU:
tests/emul/bsmall_emul.cpp runs the plan, the slots and rounds, and entry by entry what the kernels of aec_idx.hip
(launch_index_chunks) compute -- with the functions those kernels call, and the per-bit functions of aec_small.h through
them -- over batches of oracle-encoded streams laid back to back at odd byte offsets.  Every stream's chain must be the
oracle's RSI offsets, whatever lies behind the stream; the inputs are those of tests/test_gpu_index_chunks.py (same
helper, same seeds), and here every stream within the limits must be DELIVERED, so that the device test's demand -- no
stream quietly handed to the walker -- is one the scheme has to meet."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bsmall_cases as cases
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libbsmall_emul.so")
PLANNED, SERIAL, EVERY_BIT = 0, 1, 2
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "bsmall_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h) for h in
                                                           ("aec_bsmall.h", "aec_small.h", "aec_dchunks.h", "aec_trunk.h",
                                                            "aec_spec.h", "aec_lane.h", "aec_cfg.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                        "-o", EMUL_SO, srcs[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.emul_bsmall.restype = C.c_int
    lib.emul_bsmall_plan.restype = C.c_int
    lib.emul_bsmall_slot_len.restype = C.c_uint32
    lib.emul_bsmall_slot_len.argtypes = [C.c_uint64]
    lib.emul_bsmall_round_bits.restype = C.c_uint64
    lib.emul_bsmall_round_bits.argtypes = [C.c_uint64]
    lib.emul_bsmall_within.restype = C.c_int
    lib.emul_bsmall_within.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    lib.emul_bsmall_consts.restype = C.c_uint32
    return lib


def run(emul, params, buf, in_off, in_sizes, out_sizes, entries, how=EVERY_BIT, round_bits=0):
    """-> (table, records[n, 4] = delivered / n_rsi / tail_blocks / end_bit, slots[taken, 4], plan[6])"""
    p = (C.c_uint32 * 4)(*params)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    in_off, in_sizes, out_sizes = (np.ascontiguousarray(a, dtype=np.uint64) for a in (in_off, in_sizes, out_sizes))
    n = in_off.size
    table = np.full(max(entries, 1), NONE, dtype=np.uint64)
    rec = np.zeros((max(n, 1), 4), dtype=np.uint64)
    slots = np.zeros((max(n, 1), 4), dtype=np.uint64)
    plan = np.zeros(6, dtype=np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    rc = emul.emul_bsmall(p, ptr(buf), C.c_size_t(buf.size), ptr(in_off), ptr(in_sizes), ptr(out_sizes), C.c_uint64(n),
                          C.c_int(how), C.c_uint64(round_bits), ptr(table), ptr(rec), ptr(slots), ptr(plan))
    assert rc == 0, rc
    return table, rec[:n], slots[:int(plan[0])], plan


def plan_of(emul, params, in_sizes, out_sizes, how, round_bits=0):
    p = (C.c_uint32 * 4)(*params)
    a, b = (np.ascontiguousarray(x, dtype=np.uint64) for x in (in_sizes, out_sizes))
    plan = np.zeros(6, dtype=np.uint64)
    assert emul.emul_bsmall_plan(p, C.c_int(how), C.c_uint64(round_bits), C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data),
                                 C.c_uint64(a.size), C.c_void_p(plan.ctypes.data)) == 0
    return dict(zip(("taken", "rounds", "table_bits", "bytes", "min_blocks", "units"), (int(x) for x in plan)))


def check_batch(b, table, rec, round_bits=1 << 24):
    """every stream within the limits delivered with the oracle's starts and the record of a whole stream; nothing
    written outside what a delivered stream owns"""
    entries = sum(r + 1 for r in b.rsis)
    owned = np.zeros(entries, dtype=bool)
    for i in range(b.n):
        e0 = cases.table_entry0(b, i)
        if not cases.within(b, i, round_bits):
            assert rec[i, 0] == 0, i
            continue
        assert rec[i, 0] == 1, (i, "not delivered", b.rsis[i], int(b.in_sizes[i]))
        n_rsi, tail = cases.expected_record(b, i)
        assert (int(rec[i, 1]), int(rec[i, 2])) == (n_rsi, tail), (i, rec[i], n_rsi, tail)
        nent = n_rsi + (1 if tail else 0)
        assert list(table[e0:e0 + nent]) == b.starts[i][:nent], i
        assert 8 * int(b.in_off[i]) <= int(rec[i, 3]) <= 8 * int(b.in_off[i] + b.in_sizes[i])
        owned[e0:e0 + b.rsis[i] + 1] = True
    assert np.all(table[:entries][~owned] == NONE)


@pytest.fixture(scope="module")
def batches():
    return {name: cases.make_batch(name) for name in cases.CASES}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_batch_chains_are_the_oracles_offsets(emul, batches, name):
    b = batches[name]
    entries = sum(r + 1 for r in b.rsis)
    table, rec, slots, plan = run(emul, b.params, b.buf, b.in_off, b.in_sizes, b.out_sizes, entries)
    want_taken = [i for i in range(b.n) if cases.within(b, i)]
    assert [int(s[0]) for s in slots] == want_taken            # (rsi 300: the limit says "not taken")
    if name == "rsi 300":
        assert plan[0] == 0 and not rec[:, 0].any()
        return
    check_batch(b, table, rec)
    # the slots: multiples of 1024, in the order of the chunks, one behind the other
    assert all(int(s[1]) % 1024 == 0 and int(s[2]) % 1024 == 0 for s in slots)
    assert all(int(s[2]) == (8 * int(b.in_sizes[int(s[0])]) + 1 + 1023) // 1024 * 1024 for s in slots)
    # many rounds -- of 4096 entries, and of the largest slot, which every stream fits: the same results for the streams
    # that fit a round
    largest = max(int(s[2]) for s in slots)
    for rb in (4096, largest):
        table4, rec4, slots4, plan4 = run(emul, b.params, b.buf, b.in_off, b.in_sizes, b.out_sizes, entries, round_bits=rb)
        assert plan4[2] <= rb and plan4[1] >= -(-sum(int(s[2]) for s in slots4) // rb)
        assert rb == 4096 or len(slots4) < 2 or plan4[1] > 1
        check_batch(b, table4, rec4, round_bits=rb)
        for i in range(b.n):
            if rec4[i, 0]:
                e0 = cases.table_entry0(b, i)
                assert np.array_equal(rec4[i], rec[i]) and np.array_equal(table4[e0:e0 + b.rsis[i] + 1], table[e0:e0 + b.rsis[i] + 1])
    assert len(slots4) == len(slots)


@pytest.mark.parametrize("name", ["8/8/4 PP", "16/8/64 PP zero runs", "16/16/128 no PP", "4 bits restricted", "PAD_RSI"])
def test_a_chain_does_not_depend_on_what_lies_behind_the_stream(emul, batches, name):
    b = batches[name]
    bps, bs, rsi, flags = b.params
    other = bytes(b.buf[int(b.in_off[1]):int(b.in_off[1] + b.in_sizes[1])])
    for i in (0, 4, b.n - 1):
        enc = bytes(b.buf[int(b.in_off[i]):int(b.in_off[i] + b.in_sizes[i])])
        results = []
        for behind in (other, b"\x00" * 64, b"\xFF" * 64):
            buf = np.frombuffer(b"\xFF" + enc + behind + b"\xFF" * 3, dtype=np.uint8)
            table, rec, _, _ = run(emul, b.params, buf, [1], [len(enc)], [b.out_sizes[i]], b.rsis[i] + 1)
            assert rec[0, 0] == 1
            results.append((table.copy(), rec.copy()))
        for t, r in results[1:]:
            assert np.array_equal(t, results[0][0]) and np.array_equal(r, results[0][1])
        n_rsi, tail = cases.expected_record(b, i)
        nent = n_rsi + (1 if tail else 0)
        shift = 8 * (int(b.in_off[i]) - 1)
        assert [int(x) + shift for x in results[0][0][:nent]] == b.starts[i][:nent]


def test_zero_bytes_counted_into_a_stream(emul, batches):
    """in_bytes_each padded with zero bytes: the record is that of the stream, and entries of nbits + 1 = 1017 and 1025
    (127 and 128 bytes: a slot of one unit and of two) come out the same"""
    name = "8/8/4 PP"
    b0 = batches[name]
    pads = {}
    for k in range(b0.n):
        if int(b0.in_sizes[k]) < 127:
            pads[k] = 127 - int(b0.in_sizes[k])
            break
    for k in range(b0.n):
        if int(b0.in_sizes[k]) < 128 and k not in pads:
            pads[k] = 128 - int(b0.in_sizes[k])
            break
    assert len(pads) == 2
    b = cases.make_batch(name, pad_zero_bytes=pads)
    assert sorted(int(b.in_sizes[k]) for k in pads) == [127, 128]
    entries = sum(r + 1 for r in b.rsis)
    table, rec, slots, _ = run(emul, b.params, b.buf, b.in_off, b.in_sizes, b.out_sizes, entries)
    check_batch(b, table, rec)
    lens = {int(s[0]): int(s[2]) for s in slots}
    assert sorted(lens[k] for k in pads) == [1024, 2048]


def test_slot_and_round_arithmetic_at_the_edges(emul):
    # entries nbits + 1 of 1023, 1024, 1025
    assert [emul.emul_bsmall_slot_len(n) for n in (1022, 1023, 1024)] == [1024, 1024, 2048]
    assert [emul.emul_bsmall_slot_len(n) for n in (0, 64, (1 << 24) - 1, 1 << 24)] == [1024, 1024, 1 << 24, (1 << 24) + 1024]
    # the budget of a round: 0 = the default, at least 4096, clamped to the default
    assert [emul.emul_bsmall_round_bits(n) for n in (0, 1, 4095, 4096, 4097, 1 << 24, (1 << 24) + 1, 1 << 40)] == \
        [1 << 24, 4096, 4096, 4096, 4097, 1 << 24, 1 << 24, 1 << 24]
    p = (C.c_uint32 * 4)(8, 8, 4, cases.PP)
    # streams of 56 and 64 bits; of 2^24 bits and a byte more (a slot beyond the default budget is not taken either way)
    assert [emul.emul_bsmall_within(p, nb, 0) for nb in (7, 8, (1 << 21) - 1, 1 << 21, (1 << 21) + 1)] == [0, 1, 1, 0, 0]
    # a round of 4096: 511 bytes fill it exactly (4089 entries), 512 bytes are one entry too many for it
    assert [emul.emul_bsmall_within(p, nb, 4096) for nb in (511, 512)] == [1, 0]
    p300 = (C.c_uint32 * 4)(8, 8, 300, cases.PP)
    assert emul.emul_bsmall_within(p300, 4096, 0) == 0
    # two slots of 2048 fill a round of 4096, a third stream opens the next
    out = [8 * 8 * 400] * 3
    assert plan_of(emul, (8, 8, 4, cases.PP), [255, 255], out[:2], EVERY_BIT, 4096)["rounds"] == 1
    three = plan_of(emul, (8, 8, 4, cases.PP), [255, 255, 127], out, EVERY_BIT, 4096)
    assert (three["taken"], three["rounds"], three["table_bits"], three["units"]) == (3, 2, 4096, 5)
    # SERIAL takes none; PLANNED takes streams of B0 blocks and more, and never more than R rounds
    b0, r = emul.emul_bsmall_consts(0), emul.emul_bsmall_consts(1)
    assert plan_of(emul, (8, 8, 4, cases.PP), [255, 255, 127], out, SERIAL)["taken"] == 0
    # (a few long streams beside short ones: the long ones; streams all alike: none -- the walk takes as long as one)
    sizes = [20000] * 4 + [2000] * 20
    outs = [8 * 16384] * 4 + [8 * (b0 - 1)] * 20
    planned = plan_of(emul, (8, 8, 4, cases.PP), sizes, outs, PLANNED)
    assert (planned["taken"], planned["rounds"], planned["min_blocks"]) == (4, 1, b0)
    assert plan_of(emul, (8, 8, 4, cases.PP), [2000] * 40, [8 * b0] * 40, PLANNED)["taken"] == 0
    sizes = [2000] * 40
    outs = [8 * b0 * 16] * 30 + [8 * b0 * 1024] * 10
    many = plan_of(emul, (8, 8, 4, cases.PP), sizes, outs, PLANNED, 16384)
    every = plan_of(emul, (8, 8, 4, cases.PP), sizes, outs, EVERY_BIT, 16384)
    assert every["taken"] == 40 and every["rounds"] == 40
    assert 0 < many["taken"] <= r and many["rounds"] <= r and many["min_blocks"] > b0
