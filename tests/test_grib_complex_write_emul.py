"""CPU check of the complex-packing writer's arithmetic (libaec_amd/csrc/aec_gribcxw.h) through the host harness
tests/emul/gribcxw_emul.cpp, which runs the functions the kernels of aec_gribcxw.hip call launch by launch, wavefront by
wavefront and lane by lane over the case list of tests/grib_complex_write_cases.py: streams and records against the model byte
for byte; every stream byte stored exactly once and nothing else stored; no load outside the n values of a room (the samples
that pad the last block are poisoned).  The model is the writer's rule stated twice (a loop in Python integers; NumPy), pinned
to each other, to a fixture derived by hand, to the reader's two models (which give X back) and to the test writer of
tests/grib_complex_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grib_cases as gc
import grib_complex_cases as cc
import grib_complex_write_cases as wc
from helpers import ROOT

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libgribcxw_emul.so")
NAMES = [c["name"] for c in wc.cases()]
FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)       # (every test here is about the harness or about the model it is held against)
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "gribcxw_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h)
                                                           for h in ("aec_gribcxw.h", "aec_gribbits.h", "aec_grib.h", "aec_lane.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-D_GLIBCXX_ASSERTIONS", "-o",
                        EMUL_SO, srcs[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.gribcxw_emul_write.restype = C.c_int64
    lib.gribcxw_emul_tiles.restype = C.c_uint32
    lib.gribcxw_emul_bound.restype = C.c_uint64
    lib.gribcxw_emul_bound.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    return lib


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def every_field():
    return [(c, f, m) for c in wc.cases() for f, m in zip(c["fields"], wc.model(c))]


def test_the_hand_made_fixture_is_the_rule():
    h = wc.HAND
    assert h["stream"] == bytes([0x00, 0x0A, 0x80, 0x01, 0x18, 0x80, 0x0C, 0x52, 0x2B, 0x05, 0xD0, 0x5A, 0x12])
    for model in (wc.model_loop, wc.model_numpy):
        assert model(h["X"], h["nbits"], h["order"], h["G"]) == (h["stream"], h["desc"])
    assert cc.decode_loop(h["stream"], h["desc"], len(h["X"])) == h["X"]
    assert [int(v) for v in cc.decode_numpy(h["stream"], h["desc"], len(h["X"]))] == h["X"]


@pytest.mark.parametrize("name", NAMES)
def test_the_two_models_agree_and_read_back(name):
    """model_loop == model_numpy; the reader's models give X back; the stream is at most B_i bytes"""
    c = wc.case(name)
    nbits = c["tmpl"][0]
    for f, (stream, desc), B in zip(c["fields"], wc.model(c), wc.bounds(c)):
        assert wc.model_loop(f, nbits, c["order"], c["G"]) == (stream, desc)
        assert len(stream) <= B
        X = [int(v) for v in f]
        assert cc.decode_loop(stream, desc, f.size) == X
        assert [int(v) for v in cc.decode_numpy(stream, desc, f.size)] == X


def _cleared(stream, desc, n, G):
    """a stream with what cc.write fills with garbage cleared: the first `order` packed integers, and ival2 when n = 1"""
    o, ex = desc["order"], desc["extra_octets"]
    bits = np.unpackbits(np.frombuffer(stream, np.uint8)).copy()
    if o == 2 and n == 1:
        bits[8 * ex:16 * ex] = 0
    at = 8 * cc.head_bytes(desc)
    width0 = desc["width_ref"] + cc._take(stream, at - 8 * cc.table_bytes(desc["n_groups"], desc["width_bits"]), desc["width_bits"])
    bits[at:at + min(o, n) * width0] = 0          # (G >= 16 > order: they lie in the first group)
    return np.packbits(bits).tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_the_model_is_the_test_writer_under_fixed_groups(name):
    """cc.write(X, [G, .., G, last], order, extra = ceil((nbits + o) / 8), length_ref = G) follows the rule: byte-equal at order
    0, and at orders 1 and 2 once what it fills with garbage is cleared on both sides"""
    c = wc.case(name)
    nbits, o, G = c["tmpl"][0], c["order"], c["G"]
    for f, (stream, desc) in zip(c["fields"], wc.model(c)):
        if f.size > 5000:
            continue                              # (the test writer is a loop in Python; the large fields add no path to it)
        other, d2 = cc.write([int(v) for v in f], wc._lens(f.size, G), order=o, extra=wc.extra_octets(nbits, o), length_ref=G)
        assert d2 == desc
        if o == 0:
            assert other == stream
        else:
            assert _cleared(other, desc, f.size, G) == _cleared(stream, desc, f.size, G)


def test_the_case_list_holds_what_it_is_for(emul):
    assert emul.gribcxw_emul_tiles(0) == wc.TABLE_TILE and emul.gribcxw_emul_tiles(1) == wc.OUT_TILE
    cases, fields = wc.cases(), every_field()
    d = lambda m: m[1]
    assert {(c["tmpl"][0], c["order"]) for c in cases} >= {(nb, o) for nb in (8, 16, 30) for o in range(3)} | {(31, 1), (32, 0)}
    assert {c["G"] for c in cases} == set(wc.GROUP_LENGTHS)
    assert any(c["G"] == 256 and gc.container(c["tmpl"][0]) == 4 for c in cases), "a tile that is one group"
    for c in cases[:10]:
        assert {f.size for f in c["fields"]} == set(wc.sizes(c["tmpl"][0], c["G"]))
    # widths
    seen = set()
    for c, f, m in fields:
        seen |= set(wc.string_bits(*m)[1])
    assert seen >= set(cc.WIDTHS)
    assert any(c["order"] == 2 and 32 in wc.string_bits(*m)[1] for c, f, m in fields), "the swing gives widths of 32"
    assert any(d(m)["width_bits"] == 0 and d(m)["width_ref"] > 0 and d(m)["n_groups"] > 1 for c, f, m in fields)
    assert any(d(m)["ref_bits"] == 0 and d(m)["width_bits"] > 0 and d(m)["n_groups"] > 1 for c, f, m in fields)
    for o in range(3):
        const = [m for c, f, m in fields if c["name"] == f"constant_o{o}_n16_g32"]
        assert all(wc.string_bits(*m)[0] == 0 for m in const)
        assert any(len(m[0]) == 0 for m in const) == (o == 0), "S = 0: a field of zeros at order 0, and nowhere else"
    runs = wc.string_bits(*wc.model(wc.case("zero_runs_o0_n16_g16"))[0])[1]
    T = wc.tile(16) // 16
    zero = "".join("0" if w == 0 else "1" for w in runs)
    assert zero.startswith("000001") and zero.endswith("00") and "1" in zero[-16:] and "0" * (2 * T) in zero and "1001" in zero, "runs of width 0"
    # output ownership
    assert set(wc.string_bits(*wc.model(wc.case("width1_n8_g16"))[0])[1]) == {1} and set(wc.string_bits(*wc.model(wc.case("width2_n8_g16"))[0])[1]) == {2}
    assert [wc.string_bits(*m)[0] for m in wc.model(wc.case("string_ends_n8_g16"))] == [128, 129, 127, 64 * 128 + 8]
    # scans
    assert any(f.size == 65 * wc.tile(c["tmpl"][0]) + 3 and d(m)["n_groups"] > 64 * 64 for c, f, m in fields)
    # minsd and ival
    def minsd(m):
        return cc._sign_magnitude(m[0], d(m)["order"] * d(m)["extra_octets"], d(m)["extra_octets"])
    diff = [m for c, f, m in fields if c["order"] and f.size > c["order"]]
    assert any(minsd(m) < 0 for m in diff) and any(minsd(m) > 0 for m in diff) and any(minsd(m) == 0 for m in diff)
    assert all(m[0][d(m)["order"] * d(m)["extra_octets"]] != 0x80 or minsd(m) != 0 for m in diff), "minus zero"
    for o in (1, 2):
        firsts = {int(f[0]) for c, f, m in fields if c["order"] == o and c["tmpl"][0] == 16}
        assert firsts >= {0, (1 << 16) - 1}
    # placement
    assert [int(wc.placement(wc.case(f"at{k}_n16_g16"))[0][0]) for k in range(4)] == [0, 1, 2, 3]
    c = wc.case("at1_n16_g16")
    offs, size = wc.placement(c)
    assert all(int(o) + B == int(o2) for o, B, o2 in zip(offs, wc.bounds(c), offs[1:])), "neighbours do not touch"
    c = wc.case("rev_n16_g16")
    offs, size = wc.placement(c)
    assert all(int(a) > int(b) + B for a, b, B in zip(offs, offs[1:], wc.bounds(c)[1:])), "not reversed with gaps"
    assert sum(f.size for c in cases for f in c["fields"]) < 1 << 19


def test_the_bound_is_tight(emul):
    """B_i restated here is the header's, and one case reaches B_i - 1 or better"""
    for c in wc.cases():
        for f, B in zip(c["fields"], wc.bounds(c)):
            assert emul.gribcxw_emul_bound(f.size, c["tmpl"][0], c["order"], c["G"]) == B
    assert any(len(m[0]) >= B - 1 for c in wc.cases() for m, B in zip(wc.model(c), wc.bounds(c)))


def run(emul, c, mis):
    offs, size = wc.placement(c)
    nv = np.array(wc.n_values(c), np.uint64)
    work, wo = wc.work_of(c), wc.work_offsets(c)
    buf = np.full(size, FILL, np.uint8)
    stores = np.zeros(size, np.uint32)
    cxw = np.zeros(nv.size, wc.CXW_DTYPE)
    outside = emul.gribcxw_emul_write((C.c_uint32 * 4)(*c["tmpl"]), C.c_uint32(c["order"]), C.c_uint32(c["G"]), ptr(nv), C.c_uint64(nv.size),
                                      ptr(work), ptr(wo), ptr(buf), C.c_uint32(mis), ptr(offs), ptr(stores), ptr(cxw))
    return outside, buf, stores, cxw, offs


@pytest.mark.parametrize("name", NAMES)
def test_write_is_the_model(emul, name):
    c = wc.case(name)
    for mis in (0, 3):
        outside, buf, stores, cxw, offs = run(emul, c, mis)
        assert outside == 0, "a load left the values of its room, or a store its field's range, or a word was misaligned"
        want, once = np.full(buf.size, FILL, np.uint8), np.zeros(buf.size, np.uint32)
        for o, (stream, desc), rec in zip(offs, wc.model(c), cxw):
            want[int(o):int(o) + len(stream)] = np.frombuffer(stream, np.uint8)
            once[int(o):int(o) + len(stream)] = 1
            assert rec.tobytes() == wc.record_of(stream, desc).tobytes(), (name, desc, rec)
        assert np.array_equal(stores, once), "a stream byte was not stored exactly once, or a byte outside the streams was stored"
        bad = np.flatnonzero(buf != want)
        assert bad.size == 0, (name, mis, int(bad[0]))


def test_write_of_the_hand_made_fixture(emul):
    """the harness on the fixture derived by hand: its 13 bytes and its record"""
    h = wc.HAND
    c = dict(name="hand", tmpl=(h["nbits"], wc.PP, 8, 128), order=h["order"], G=h["G"], fields=[np.array(h["X"], np.uint32)], first=1, rev=False)
    outside, buf, stores, cxw, offs = run(emul, c, 1)
    assert outside == 0 and buf[1:14].tobytes() == h["stream"] and int(stores.sum()) == 13 and set(stores[1:14]) == {1}
    assert cxw[0].tobytes() == wc.record_of(h["stream"], h["desc"]).tobytes()
