"""CPU check of the simple-packing layer's arithmetic (libaec_amd/csrc/aec_gribbits.h) through the host harness
tests/emul/gribbits_emul.cpp, which runs the functions the kernels of aec_gribbits.hip call wavefront by wavefront and lane by
lane over the case list of tests/grib_simple_cases.py: the streams of a pack and the rooms of an unpack against the model
byte for byte (padding included), for the buffer's base at every address modulo 4; no store outside a field's S_i bytes, no
load outside the buffer, no misaligned word; every stream byte and every room byte stored exactly once.  The model is the WMO
definition stated twice (numpy.packbits over bit planes; a big integer), and the two are pinned to each other here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grib_cases as gc
import grib_simple_cases as sc
from helpers import ROOT

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libgribbits_emul.so")
NAMES = [c["name"] for c in sc.cases()]


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "gribbits_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h)
                                                            for h in ("aec_gribbits.h", "aec_grib.h", "aec_lane.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", EMUL_SO,
                        srcs[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    for f in (lib.gribbits_emul_pack, lib.gribbits_emul_unpack):
        f.restype = C.c_int64
    lib.gribbits_emul_wave_room.restype = C.c_uint32
    return lib


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def test_the_case_list_holds_what_it_is_for(emul):
    assert emul.gribbits_emul_wave_room() == gc.WAVE_ROOM
    cases = sc.cases()
    assert {c["tmpl"][0] for c in cases} == {1, 3, 7, 8, 9, 12, 16, 17, 24, 25, 31, 32}
    assert {gc.container(c["tmpl"][0]) for c in cases} == {1, 2, 4}
    assert all((4 * nbits) % 8 for nbits in (17, 25, 31))
    assert {c["tmpl"][2] for c in cases} == {8, 32, sc.ODD_BS}
    for nbits in sc.NBITS:
        c, s = sc.case(f"n{nbits}"), sc.span(nbits)
        sizes = set(sc.n_values(c))
        assert {1, 7, 8, 9, 63, 64, 65, s - 1, s, s + 1, 2 * s + 5} <= sizes
        assert any(n % c["tmpl"][2] for n in sizes), "no field has a padding"
        assert set(c["kinds"]) == set(sc.KINDS)
        offs, size = sc.placement(c)
        assert int(offs[0]) == (1 if nbits == 32 else 0) and all(int(offs[i]) + sc.stream_bytes(x.size, nbits) == int(offs[i + 1])
                                         for i, x in enumerate(c["X"][:-1])), "the streams do not lie back to back"
        assert any(int(o) % 4 for o in offs), "every stream starts on a word"
    assert {sc.span(n) for n in (8, 16, 31)} == {1024, 512, 256}
    for nbits in (8, 16, 31):
        assert 65 * sc.span(nbits) + 3 in sc.n_values(sc.case(f"n{nbits}"))
    assert [int(sc.placement(sc.case(name))[0][0]) for name in ("n17", "n17_at1", "n17_at2", "n17_at3")] == [0, 1, 2, 3]
    rev = [c for c in cases if c["rev"]]
    assert {gc.container(c["tmpl"][0]) for c in rev} == {1, 2, 4}
    for c in rev:
        offs, size = sc.placement(c)
        assert all(int(a) > int(b) for a, b in zip(offs, offs[1:])), "not in reversed order"
        buf, _ = sc.buffer_of(c)
        ends = [int(o) + sc.stream_bytes(x.size, c["tmpl"][0]) for o, x in zip(offs, c["X"])]
        assert all(buf[e] == sc.FILL for e in ends), "no gap behind a stream"
    odd = [c for c in cases if c["tmpl"][2] == sc.ODD_BS]
    assert {gc.container(c["tmpl"][0]) for c in odd} == {1, 2, 4}
    for c in odd:           # value n - 1 is the last of a wavefront's span, and its block goes on into the next wavefront's room
        s = sc.span(c["tmpl"][0])
        assert s % sc.ODD_BS and sc.ODD_BS % 2 == 0 and {s, 2 * s} <= set(sc.n_values(c))
    for name in sc.GARBAGE:
        assert sc.case(name)["tmpl"][0] < 8 * gc.container(sc.case(name)["tmpl"][0])
    for c in cases:
        for x, kind in zip(c["X"], c["kinds"]):
            M = 2 ** c["tmpl"][0] - 1
            assert int(x.max()) <= M
            if kind == "max":
                assert int(x.min()) == M
            if kind == "walking" and x.size >= c["tmpl"][0]:
                assert {int(v) for v in x} == {1 << k for k in range(c["tmpl"][0])}
    assert sum(x.size for c in cases for x in c["X"]) * 4 < 2 << 20


@pytest.mark.parametrize("name", NAMES)
def test_the_two_models_agree(name):
    c = sc.case(name)
    nbits = c["tmpl"][0]
    for x in c["X"]:
        a, b = sc.stream_numpy(x, nbits), sc.stream_bigint(x, nbits)
        assert a.size == sc.stream_bytes(x.size, nbits) and np.array_equal(a, b)
        assert int(a[-1]) & ((1 << (-x.size * nbits % 8)) - 1) == 0, "pad bits"


def run_pack(emul, c, mis, garbage=None):
    want, offs = sc.buffer_of(c, extra=5)
    work = sc.work_of(c, garbage=garbage)
    nv = np.array(sc.n_values(c), np.uint64)
    simple = np.full(want.size, sc.FILL, np.uint8)
    stores = np.zeros(want.size, np.uint32)
    outside = emul.gribbits_emul_pack((C.c_uint32 * 4)(*c["tmpl"]), ptr(nv), C.c_uint64(nv.size), ptr(work), C.c_uint64(work.size),
                                      ptr(sc.work_offsets(c)), ptr(simple), ptr(offs), C.c_uint32(mis), ptr(stores))
    return outside, simple, want, stores


@pytest.mark.parametrize("name", NAMES)
def test_pack_is_the_model(emul, name):
    c = sc.case(name)
    for mis in range(4):
        outside, simple, want, stores = run_pack(emul, c, mis)
        assert outside == 0, (name, mis)
        bad = np.flatnonzero(simple != want)
        assert bad.size == 0, (name, mis, int(bad[0]))
        in_stream = np.zeros(want.size, np.uint32)
        for o, x in zip(sc.placement(c)[0], c["X"]):
            in_stream[int(o):int(o) + sc.stream_bytes(x.size, c["tmpl"][0])] = 1
        assert np.array_equal(stores, in_stream), (name, mis, "a stream byte was not stored exactly once")


@pytest.mark.parametrize("name", sc.GARBAGE)
def test_pack_takes_x_modulo_two_to_the_nbits(emul, name):
    c = sc.case(name)
    assert not np.array_equal(sc.work_of(c), sc.work_of(c, garbage=7))
    outside, simple, want, stores = run_pack(emul, c, 1, garbage=7)
    assert outside == 0 and np.array_equal(simple, want)


@pytest.mark.parametrize("name", NAMES)
def test_unpack_is_the_model(emul, name):
    c = sc.case(name)
    simple, offs = sc.buffer_of(c)              # (the buffer ends with the last stream: nothing behind it may be loaded)
    want = sc.work_of(c)
    nv = np.array(sc.n_values(c), np.uint64)
    for mis in range(4):
        work = np.full(want.size, 0x5A, np.uint8)
        stores = np.zeros(want.size, np.uint32)
        outside = emul.gribbits_emul_unpack((C.c_uint32 * 4)(*c["tmpl"]), ptr(nv), C.c_uint64(nv.size), ptr(simple), C.c_uint64(simple.size),
                                            ptr(offs), C.c_uint32(mis), ptr(work), ptr(sc.work_offsets(c)), ptr(stores))
        assert outside == 0, (name, mis)
        bad = np.flatnonzero(work != want)
        assert bad.size == 0, (name, mis, int(bad[0]))
        in_room = np.zeros(want.size, np.uint32)
        for o, r in zip(sc.work_offsets(c), sc.rooms(c)):
            in_room[int(o):int(o) + r] = 1
        assert np.array_equal(stores, in_room), (name, mis, "a room byte was not stored exactly once")
