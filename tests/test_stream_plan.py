"""The arithmetic of one streaming decode batch (libaec_amd/csrc/aec_stream_plan.h: plan_batch, judge_batch,
advance_stream), which tests/emul/abi_emul.cpp exposes over arrays of 64-bit values: no GPU, no HIP.

The verdict decides what of a batch is good, what is an error NOW, what is deferred to the next call and where the index
walker resumes (DESIGN.md §1 "Damaged streams", §5).  The expected values are worked out here from the rules as
aec_abi.cpp's decode_run stated them before they were separated from its launches, every one at the value where its
condition turns.  16-bit samples, blocks of 16, RSIs of 4 blocks: a block is 32 bytes, an RSI 128."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libabi_emul.so")

PREPROCESS = 8
CFG = (16, 16, 4, PREPROCESS)
BLK, RSI_BYTES = 32, 128
OK, NEED_INPUT, DATA_ERROR = 0, 1, 2
NONE = 2 ** 64 - 1                      # a decode record's tail_blocks when no block failed
MIN_BATCH_OUT, PIPE_OUT = 4 << 20, 64 << 20
WORST_RSI = (4 * (4 + 16 * 16) + 16 + 7) // 8 + 1          # bytes an encoder makes of an RSI at most: every block uncompressed

POS = ("base", "d_len", "rsi_start_bit", "rsi_bits_seen", "walk_bit", "walk_blocks", "delivered", "walked_len", "span_mul",
       "span_wide", "more")
PLAN = ("walk_rel", "rsi_rel", "skip", "hint", "pipe", "max_rsi", "in_bytes", "piece", "off_bytes", "out_bytes", "seg_bytes")
VERD = ("total", "part", "corrupt", "more_behind", "good_rsi", "tail_blocks", "res_rsi", "res_tail", "res_end", "fetch_off")
REC = ("n_rsi", "tail_blocks", "end_bit", "status", "pad", "bad_rsi")


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "abi_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h) for h in
                                                        ("aec_stream_plan.h", "aec_cfg.h", "aec_lane.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                        "-o", EMUL_SO, srcs[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.emul_advance.restype = C.c_int64
    lib.emul_worst_rsi_bytes.restype = C.c_uint64
    return lib


def arr(names, values):
    return np.array([int(values.get(n, 0)) for n in names], dtype=np.uint64)


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def rec(n_rsi=0, tail=0, end_bit=0, status=OK, pad=0, bad_rsi=0):
    return arr(REC, dict(n_rsi=n_rsi, tail_blocks=tail, end_bit=end_bit, status=status, pad=pad, bad_rsi=bad_rsi))


def pos(**kw):
    kw.setdefault("span_mul", 1)
    return arr(POS, kw)


def plan(emul, p, room, windowed, cfg=CFG):
    out = np.zeros(len(PLAN), dtype=np.uint64)
    assert emul.emul_plan(ptr(arr(range(4), dict(enumerate(cfg)))), ptr(p), C.c_uint64(room), C.c_int(windowed), ptr(out)) == 0
    return {n: int(v) for n, v in zip(PLAN, out)}


def verdict(emul, idx, dec, skip, want_out):
    out = np.zeros(len(VERD), dtype=np.uint64)
    assert emul.emul_verdict(ptr(arr(range(4), dict(enumerate(CFG)))), ptr(idx), ptr(dec), C.c_uint64(skip), C.c_uint64(want_out),
                             ptr(out)) == 0
    return {n: int(v) for n, v in zip(VERD, out)}


def advance(emul, p, b, v, idx, tail_start=0):
    """-> (the stream's new position, bytes dropped from the front of the resident stream)"""
    p = p.copy()
    drop = emul.emul_advance(ptr(arr(range(4), dict(enumerate(CFG)))), ptr(p), ptr(arr(PLAN, b)), ptr(arr(VERD, v)), ptr(idx),
                             C.c_uint64(tail_start))
    assert drop >= 0
    return {n: int(x) for n, x in zip(POS, p)}, drop


DEC_CLEAN = rec(tail=NONE)
BASE = 48                                                   # the resident stream starts at byte 48 of the stream
BASE_BITS = BASE * 8


def test_the_constants_are_the_ones_the_cases_below_assume(emul):
    out = np.zeros(3, dtype=np.uint64)
    emul.emul_constants(ptr(out))
    assert [int(v) for v in out] == [MIN_BATCH_OUT, PIPE_OUT, PIPE_OUT + PIPE_OUT // 2]
    assert emul.emul_worst_rsi_bytes(ptr(arr(range(4), dict(enumerate(CFG))))) == WORST_RSI == 133


# ---- verdict and advance ----------------------------------------------------------------------------------------------
def test_a_clean_batch(emul):
    E, rsi_rel = 2999, 40
    idx = rec(3, 0, E)
    v = verdict(emul, idx, DEC_CLEAN, 0, 1000)
    assert v == dict(total=384, part=0, corrupt=0, more_behind=0, good_rsi=3, tail_blocks=0, res_rsi=3, res_tail=0, res_end=E,
                     fetch_off=0)
    p = pos(base=BASE, d_len=1000, rsi_start_bit=BASE_BITS + rsi_rel, walk_bit=BASE_BITS + rsi_rel, delivered=7, walk_blocks=2)
    got, drop = advance(emul, p, dict(rsi_rel=rsi_rel, in_bytes=1000, max_rsi=4), v, idx)
    assert drop == 0
    assert got == dict(base=BASE, d_len=1000, rsi_start_bit=BASE_BITS + E, rsi_bits_seen=(E - rsi_rel) // 3, walk_bit=BASE_BITS + E,
                       walk_blocks=0, delivered=0, walked_len=1000, span_mul=1, span_wide=0, more=0)
    # stopped at the bound of RSIs, or with resident input beyond the span: there is more
    assert advance(emul, p, dict(rsi_rel=rsi_rel, in_bytes=1000, max_rsi=3), v, idx)[0]["more"] == 1
    assert advance(emul, p, dict(rsi_rel=rsi_rel, in_bytes=999, max_rsi=4), v, idx)[0]["more"] == 1
    # no whole RSI: the average of the batch in front stays
    p[POS.index("rsi_bits_seen")] = 777
    idx0 = rec(0, 0, rsi_rel)
    assert advance(emul, p, dict(rsi_rel=rsi_rel, in_bytes=1000, max_rsi=4), verdict(emul, idx0, DEC_CLEAN, 0, 1000), idx0)[0][
        "rsi_bits_seen"] == 777


def test_input_ends_inside_a_coded_data_set(emul):
    E, rsi_rel, tail_start = 2500, 8, 2100
    idx = rec(2, 1, E, NEED_INPUT, 1)
    dec = rec(tail=NONE, pad=0x80000005)                    # (bit 31: the sequential decoder ran -- informational)
    v = verdict(emul, idx, dec, 0, 1000)
    assert (v["part"], v["total"], v["corrupt"], v["more_behind"]) == (5, (2 * 4 + 1) * 32 + 10, 0, 0)
    p = pos(base=BASE, d_len=400, rsi_start_bit=BASE_BITS + rsi_rel, walk_bit=BASE_BITS + rsi_rel)
    got, drop = advance(emul, p, dict(rsi_rel=rsi_rel, in_bytes=400, max_rsi=9), v, idx, tail_start)
    assert drop == 0
    assert (got["walk_bit"], got["walk_blocks"], got["rsi_start_bit"], got["delivered"]) == \
           (BASE_BITS + E, 1, BASE_BITS + tail_start, 1 * 16 + 5)
    assert got["rsi_bits_seen"] == (E - rsi_rel) // 3       # (the RSI the batch ends in counts)
    assert got["more"] == 0
    # the walker stopped for another reason than the end of the input: nothing is released from an open coded data set
    assert verdict(emul, rec(2, 1, E, OK, 0), dec, 0, 1000)["part"] == 0


def test_a_walkers_error_behind_what_the_call_asked_for_is_deferred(emul):
    E = 3333
    idx = rec(2, 3, E, DATA_ERROR)
    total = (2 * 4 + 3) * 32
    assert total == 352
    for want_out, deferred in ((352, True), (353, False), (354, False), (0, True)):    # (no room: the finding waits for it)
        v = verdict(emul, idx, DEC_CLEAN, 0, want_out)
        assert (v["total"], v["corrupt"], v["more_behind"], v["fetch_off"]) == (total, int(not deferred), int(deferred), 0), want_out
        assert (v["res_rsi"], v["res_tail"], v["res_end"]) == (2, 3, E)
    # (what is already handed out of the current RSI does not count towards what the call asked for)
    assert verdict(emul, idx, DEC_CLEAN, 32, 320)["more_behind"] == 1
    assert verdict(emul, idx, DEC_CLEAN, 32, 321)["corrupt"] == 1
    v = verdict(emul, idx, DEC_CLEAN, 0, 352)
    p = pos(base=BASE, d_len=600, rsi_start_bit=BASE_BITS, walk_bit=BASE_BITS)
    got, _ = advance(emul, p, dict(rsi_rel=0, in_bytes=600, max_rsi=9), v, idx, 2900)
    assert (got["walk_bit"], got["walk_blocks"], got["rsi_start_bit"], got["delivered"], got["more"]) == \
           (BASE_BITS + E, 3, BASE_BITS + 2900, 48, 1)


def test_a_decoders_error_behind_what_the_call_asked_for_is_deferred(emul):
    idx = rec(3, 0, 4000)
    dec = rec(tail=1 * 4 + 2, status=DATA_ERROR, bad_rsi=1)
    v = verdict(emul, idx, dec, 0, 64)
    assert (v["good_rsi"], v["tail_blocks"], v["total"], v["part"]) == (1, 2, 192, 0)
    assert (v["corrupt"], v["more_behind"], v["fetch_off"], v["res_rsi"], v["res_tail"]) == (0, 1, 1, 1, 0)
    assert verdict(emul, idx, dec, 0, 192)["more_behind"] == 1
    assert verdict(emul, idx, dec, 0, 193)["corrupt"] == 1
    # a second-extension code beyond the table is not deferred by a call without room
    v0 = verdict(emul, idx, dec, 0, 0)
    assert (v0["corrupt"], v0["more_behind"], v0["fetch_off"]) == (1, 0, 0)
    # the caller completes res_end with entry good_rsi of the batch's RSI starts
    O = 1234
    v["res_end"] = O
    p = pos(base=BASE, d_len=700, rsi_start_bit=BASE_BITS + 16, walk_bit=BASE_BITS + 16, walk_blocks=1)
    got, _ = advance(emul, p, dict(rsi_rel=16, in_bytes=700, max_rsi=9), v, idx, 3999)
    assert (got["walk_bit"], got["walk_blocks"], got["rsi_start_bit"], got["delivered"], got["more"]) == \
           (BASE_BITS + O, 0, BASE_BITS + O, 2 * 16, 1)
    assert got["rsi_bits_seen"] == (O - 16) // 1


def test_a_decoders_error_beyond_the_walkers_rsis_or_without_a_failing_block(emul):
    idx = rec(3, 0, 4000)
    beyond = verdict(emul, idx, rec(tail=1 * 4 + 2, status=DATA_ERROR, bad_rsi=4), 0, 0)
    assert (beyond["corrupt"], beyond["good_rsi"], beyond["tail_blocks"], beyond["total"]) == (1, 3, 0, 384)
    at_the_end = verdict(emul, idx, rec(tail=3 * 4 + 1, status=DATA_ERROR, bad_rsi=3), 0, 1000)      # (bad_rsi == n_rsi: taken)
    assert (at_the_end["corrupt"], at_the_end["good_rsi"], at_the_end["tail_blocks"]) == (1, 3, 1)
    no_block = verdict(emul, idx, rec(tail=NONE, status=DATA_ERROR, bad_rsi=1), 0, 1000)
    assert (no_block["corrupt"], no_block["good_rsi"], no_block["tail_blocks"], no_block["total"]) == (1, 1, 0, 128)
    # the failing block lies in another RSI than the first bad one: no block of that RSI is good
    other = verdict(emul, idx, rec(tail=2 * 4 + 2, status=DATA_ERROR, bad_rsi=1), 0, 1000)
    assert (other["good_rsi"], other["tail_blocks"]) == (1, 0)


def test_the_span_widens_while_the_walker_runs_out_of_input_inside_it(emul):
    idx = rec(1, 0, 900, NEED_INPUT, 1)
    v = verdict(emul, idx, DEC_CLEAN, 0, 1000)

    def after(span_mul, span_wide, piece, in_bytes=500, d_len=501, pad=1):
        i = rec(1, 0, 900, NEED_INPUT, pad)
        p = pos(base=BASE, d_len=d_len, rsi_start_bit=BASE_BITS, walk_bit=BASE_BITS, span_mul=span_mul, span_wide=span_wide)
        got, _ = advance(emul, p, dict(rsi_rel=0, in_bytes=in_bytes, max_rsi=9, piece=piece), v, i)
        return got["span_mul"], got["span_wide"]

    assert after(1, 0, piece=1) == (1, 1)                   # a tight piece: first the worst case
    assert after(1, 1, piece=1) == (4, 1)
    assert after(1, 1, piece=0) == (4, 1)
    assert after(1, 0, piece=0) == (4, 0)
    assert after(4, 1, piece=0) == (16, 1)
    assert after(1 << 18, 0, piece=0) == (1 << 20, 0)
    assert after(1 << 20, 0, piece=0) == (1 << 20, 0)       # no wider than that
    assert after(16, 1, piece=0, in_bytes=501) == (1, 1)    # the span was all that is resident: more input is the cure
    assert after(16, 1, piece=0, pad=0) == (1, 1)


@pytest.mark.parametrize("start_byte,d_len,in_bytes,want", [
    (4100, 8192, 8192, (4096, 4096, 4096)),                 # (bytes dropped, d_len, walked_len)
    (4100, 8193, 8193, (0, 8193, 8193)),                    # the consumed front is not yet the larger part
    (4095, 8000, 8000, (0, 8000, 8000)),                    # ... or smaller than 4096 bytes
    (4111, 8192, 8192, (4096, 4096, 4096)),                 # the front is cut at a multiple of 16
    (4112, 8192, 8192, (4112, 4080, 4080)),
    (4100, 8192, 4097, (4096, 4096, 1)),                    # walked_len moves with the stream ...
    (4100, 8192, 1000, (4096, 4096, 0)),                    # ... and not below 0
])
def test_the_consumed_front_of_the_resident_stream_is_dropped(emul, start_byte, d_len, in_bytes, want):
    idx = rec(3, 0, start_byte * 8 + 3)
    v = verdict(emul, idx, DEC_CLEAN, 0, 1000)
    p = pos(base=BASE, d_len=d_len, rsi_start_bit=BASE_BITS, walk_bit=BASE_BITS)
    got, drop = advance(emul, p, dict(rsi_rel=0, in_bytes=in_bytes, max_rsi=9), v, idx)
    assert (drop, got["d_len"], got["walked_len"]) == want
    assert got["base"] == BASE + drop
    assert got["rsi_start_bit"] == got["walk_bit"] == BASE_BITS + start_byte * 8 + 3           # absolute bits: they stay


# ---- plan -----------------------------------------------------------------------------------------------------------
def test_pipelining_takes_room_and_a_windowed_index(emul):
    p = pos(base=BASE, d_len=32 << 20, rsi_start_bit=BASE_BITS, walk_bit=BASE_BITS, rsi_bits_seen=300)
    at = PIPE_OUT + PIPE_OUT // 2
    assert plan(emul, p, at, 1)["pipe"] == 1
    assert plan(emul, p, at - 1, 1)["pipe"] == 0
    for room in (at, at + 1, 1 << 31):
        assert plan(emul, p, room, 0)["pipe"] == 0
    # a pipelined batch is bounded by kPipeOut, any other by the room
    assert plan(emul, p, at, 1)["max_rsi"] == PIPE_OUT // RSI_BYTES + 2
    assert plan(emul, p, at - 1, 1)["max_rsi"] == (at - 1) // RSI_BYTES + 2


def test_the_bound_of_a_batch(emul):
    p = pos(base=BASE, d_len=1 << 20, rsi_start_bit=BASE_BITS + 24, walk_bit=BASE_BITS + 24)
    b = plan(emul, p, 1000, 0)
    assert (b["walk_rel"], b["rsi_rel"], b["skip"]) == (24, 24, 0)
    assert b["max_rsi"] == MIN_BATCH_OUT // RSI_BYTES + 2                       # the room is floored
    assert plan(emul, p, MIN_BATCH_OUT + RSI_BYTES - 1, 0)["max_rsi"] == MIN_BATCH_OUT // RSI_BYTES + 2
    assert plan(emul, p, MIN_BATCH_OUT + RSI_BYTES, 0)["max_rsi"] == MIN_BATCH_OUT // RSI_BYTES + 3
    # what is already handed out of the current RSI is room too
    p5 = pos(base=BASE, d_len=1 << 20, rsi_start_bit=BASE_BITS, walk_bit=BASE_BITS + 999, walk_blocks=2, delivered=37)
    b5 = plan(emul, p5, MIN_BATCH_OUT + RSI_BYTES - 74, 0)
    assert (b5["skip"], b5["max_rsi"]) == (74, MIN_BATCH_OUT // RSI_BYTES + 3)
    assert plan(emul, p5, MIN_BATCH_OUT + RSI_BYTES - 75, 0)["max_rsi"] == MIN_BATCH_OUT // RSI_BYTES + 2
    # the buffers
    assert (b["off_bytes"], b["out_bytes"], b["seg_bytes"]) == ((b["max_rsi"] + 2) * 8, b["max_rsi"] * RSI_BYTES + BLK + 64, 0)
    long_rsi = plan(emul, p, 1000, 0, cfg=(16, 16, 512, PREPROCESS))            # eight segments: their starts as well
    assert long_rsi["seg_bytes"] == (long_rsi["max_rsi"] + 2) * 8 * 8
    assert plan(emul, p, 1000, 0, cfg=(16, 16, 448, PREPROCESS))["seg_bytes"] == 0


def test_no_more_rsis_than_the_input_can_hold(emul):
    # the shortest RSI: an option and two bits per segment, and the reference sample
    p = pos(base=BASE, d_len=1000, rsi_start_bit=BASE_BITS, walk_bit=BASE_BITS)
    assert plan(emul, p, 1 << 20, 0)["max_rsi"] == 8000 // 22 + 2 == 365
    p = pos(base=BASE, d_len=1000, rsi_start_bit=BASE_BITS + 15, walk_bit=BASE_BITS + 15)
    assert plan(emul, p, 1 << 20, 0)["max_rsi"] == 7985 // 22 + 2 == 364
    assert plan(emul, p, 1 << 20, 0, cfg=(16, 16, 4, 0))["max_rsi"] == 7985 // 6 + 2
    assert plan(emul, p, 1 << 20, 0, cfg=(16, 16, 65, 0))["max_rsi"] == 7985 // 12 + 2     # two segments


def test_the_hint_is_measured_or_estimated_from_the_room(emul):
    p = pos(base=BASE, d_len=5000, rsi_start_bit=BASE_BITS + 80, walk_bit=BASE_BITS + 80, delivered=3)
    avail_bits = 5000 * 8 - 80
    assert plan(emul, p, 1280, 0)["hint"] == avail_bits // ((1280 + 6 + 127) // 128) == avail_bits // 11
    assert plan(emul, p, 1280 - 6, 0)["hint"] == avail_bits // 10
    assert plan(emul, p, RSI_BYTES, 0)["hint"] == avail_bits // 2
    assert plan(emul, p, RSI_BYTES - 1, 0)["hint"] == 0                         # less room than an RSI: no estimate
    p[POS.index("rsi_bits_seen")] = 640
    assert plan(emul, p, 1280, 0)["hint"] == 640                                # the batch in front measured it
    assert plan(emul, p, 0, 0)["hint"] == 640


def test_the_span_of_the_resident_stream_a_batch_is_given(emul):
    max_rsi = MIN_BATCH_OUT // RSI_BYTES + 2
    span = 100 + max_rsi * WORST_RSI + 64

    def p(d_len, **kw):
        return pos(base=BASE, d_len=d_len, rsi_start_bit=BASE_BITS, walk_bit=BASE_BITS + 807, rsi_bits_seen=200, **kw)

    assert plan(emul, p(span + 1), 1000, 0)["in_bytes"] == span
    assert plan(emul, p(span), 1000, 0)["in_bytes"] == span
    assert plan(emul, p(span - 1), 1000, 0)["in_bytes"] == span - 1
    assert plan(emul, p(32 << 20, span_mul=4), 1000, 0)["in_bytes"] == 100 + max_rsi * WORST_RSI * 4 + 64
    assert plan(emul, p(32 << 20, span_mul=4), 1000, 0)["piece"] == 0

    # pipelined: what the batch's RSIs need on average plus the look-ahead, if that is less than the worst case and
    # less than what is resident -- and only until it failed once
    at, H = PIPE_OUT + PIPE_OUT // 2, 200
    max_rsi = PIPE_OUT // RSI_BYTES + 2
    tight = 100 + (max_rsi * H + 8 * H) // 8 + 65536
    worst = 100 + max_rsi * WORST_RSI + 64
    assert tight < worst
    b = plan(emul, p(tight + 1), at, 1)
    assert (b["pipe"], b["piece"], b["in_bytes"], b["hint"], b["max_rsi"]) == (1, 1, tight, H, max_rsi)
    b = plan(emul, p(tight), at, 1)
    assert (b["piece"], b["in_bytes"]) == (0, tight)
    big = 128 << 20
    assert plan(emul, p(big), at, 1)["piece"] == 1
    assert plan(emul, p(big), at, 0)["piece"] == 0
    assert plan(emul, p(big), at - 1, 1)["piece"] == 0
    assert plan(emul, p(big, span_mul=4), at, 1)["piece"] == 0
    assert plan(emul, p(big, span_wide=1), at, 1) == dict(plan(emul, p(big), at, 1), piece=0, in_bytes=worst)
    # RSIs measured longer than an encoder's worst case: the tight span would be the wider one
    long_rsis = pos(base=BASE, d_len=big, rsi_start_bit=BASE_BITS, walk_bit=BASE_BITS + 807, rsi_bits_seen=WORST_RSI * 8 + 40)
    b = plan(emul, long_rsis, at, 1)
    assert (b["pipe"], b["piece"], b["in_bytes"]) == (1, 0, worst)
