"""CPU check of the complex-packing reader's arithmetic (libaec_amd/csrc/aec_gribcx.h) through the host harness
tests/emul/gribcx_emul.cpp, which runs the functions the kernels of aec_gribcx.hip call launch by launch, wavefront by
wavefront and lane by lane over the case list of tests/grib_complex_cases.py: rooms and records against the model byte for
byte (padding included); no load outside a stream's complex_bytes_each bytes; every room byte stored exactly once and nothing
else stored; damaged fields MALFORMED with their neighbours exact.  The reader does only byte loads from a stream, so there
is no word access that could be misaligned; the room is stored in the 16 bytes a lane owns.  The model is the definition
stated twice (a loop in Python integers; NumPy), pinned to each other and to a fixture derived by hand here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grib_cases as gc
import grib_complex_cases as cc
from helpers import ROOT

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libgribcx_emul.so")
NAMES = [c["name"] for c in cc.cases()]


@pytest.fixture(scope="module", autouse=True)       # (every test here is about the harness or about the model it is held against)
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "gribcx_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h)
                                                          for h in ("aec_gribcx.h", "aec_gribbits.h", "aec_grib.h", "aec_lane.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", EMUL_SO,
                        srcs[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.gribcx_emul_expand.restype = C.c_int64
    lib.gribcx_emul_group_tile.restype = C.c_uint32
    return lib


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def desc_array(c):
    return np.array([[f["desc"][k] for k in cc.DESC_KEYS] for f in c["fields"]], np.uint32)


def fields_where(pred):
    return [(c, f) for c in cc.cases() for f in c["fields"] if pred(c, f)]


def test_the_hand_made_fixture_decodes_as_derived():
    h = cc.HAND
    assert h["stream"] == bytes([0x0A, 0x0C, 0x87, 0x08, 0x00, 0x20, 0x30, 0x00, 0x12, 0x00])
    assert cc.decode_loop(h["stream"], h["desc"], h["n"]) == h["X"]
    assert [int(v) for v in cc.decode_numpy(h["stream"], h["desc"], h["n"])] == h["X"]


@pytest.mark.parametrize("name", NAMES)
def test_the_two_models_agree(name):
    for f in cc.case(name)["fields"]:
        if f["damaged"]:
            continue
        a, b = cc.decode_loop(f["stream"], f["desc"], f["n"]), cc.decode_numpy(f["stream"], f["desc"], f["n"])
        assert a == [int(v) for v in b] == [int(v) for v in f["X"]]


def test_the_case_list_holds_what_it_is_for(emul):
    assert emul.gribcx_emul_group_tile() == cc.GROUP_TILE
    cases = cc.cases()
    clean = fields_where(lambda c, f: not f["damaged"])
    d = lambda f: f["desc"]
    # orders and extra descriptors
    assert {d(f)["order"] for c, f in clean} == {0, 1, 2}
    assert {d(f)["extra_octets"] for c, f in clean if d(f)["order"]} >= {0, 1, 2, 4, 8}

    def minsd(f):
        return cc._sign_magnitude(f["stream"], d(f)["order"] * d(f)["extra_octets"], d(f)["extra_octets"])
    diff = [f for c, f in clean if d(f)["order"] and d(f)["extra_octets"]]
    assert any(minsd(f) < 0 for f in diff) and any(minsd(f) > 0 for f in diff)
    zeros = [f["stream"][d(f)["order"] * d(f)["extra_octets"]:][:d(f)["extra_octets"]] for f in diff if minsd(f) == 0]
    assert any(z[0] == 0x80 for z in zeros) and any(z[0] == 0 for z in zeros), "minsd zero and minus zero"
    # bit counts
    for key in ("ref_bits", "width_bits", "length_bits"):
        assert any(d(f)[key] == 0 and f["n"] > 1 for c, f in clean), key
    assert any(d(f)["ref_bits"] == 32 for c, f in clean)
    widths = set()
    for c, f in clean:
        s, dd = f["stream"], d(f)
        pos = 8 * ((dd["order"] + 1) * dd["extra_octets"] if dd["order"] else 0) + 8 * cc.table_bytes(dd["n_groups"], dd["ref_bits"])
        widths |= {dd["width_ref"] + cc._take(s, pos + g * dd["width_bits"], dd["width_bits"]) for g in range(dd["n_groups"])}
    assert widths >= {0, 1, 7, 8, 9, 25, 31, 32}
    assert {c["tmpl"][0] for c in cases} >= {8, 16, 31, 32} and {gc.container(c["tmpl"][0]) for c in cases} == {1, 2, 4}
    # field sizes
    for nbits in (8, 16, 31, 32):
        T = cc.tile(nbits)
        have = {f["n"] for c, f in clean if c["tmpl"][0] == nbits}
        assert have >= {1, 2, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5}, nbits
    assert any(f["n"] == 65 * cc.tile(c["tmpl"][0]) + 3 and d(f)["order"] == 2 for c, f in clean)
    # groupings
    assert any(d(f)["n_groups"] == 1 and f["n"] > 64 for c, f in clean)
    assert any(d(f)["n_groups"] == f["n"] and f["n"] > 64 for c, f in clean)
    assert any(d(f)["n_groups"] == 64 * cc.GROUP_TILE + 1 for c, f in clean)
    g = cc.case("groupings_n16")
    T, P = cc.tile(16), cc.per(16)
    ends = np.cumsum(g["fields"][0]["lengths"])
    starts = ends - g["fields"][0]["lengths"]
    assert any(e % P == 0 and s % P == 0 and e - s == P for s, e in zip(starts, ends)), "a group that is exactly one lane's"
    assert any(s // P != (e - 1) // P and e - s < 2 * P for s, e in zip(starts, ends)), "a group that crosses a lane's 16 bytes"
    assert any(s // T + 1 == (e - 1) // T for s, e in zip(starts, ends)), "a group that crosses a tile"
    assert any((e - 1) // T - s // T >= 2 for s, e in zip(starts, ends)), "a group that spans three tiles"
    assert any(ln[:3] == [20, 30, 3] for ln in [f["lengths"] for f in g["fields"]]), "runs of width 0"
    assert any(d(f)["order"] == 2 and f["lengths"][0] == 1 for f in g["fields"]), "a first group shorter than order"
    # placement
    assert [int(cc.placement(cc.case(f"at{k}_n16"))[0][0]) for k in range(4)] == [0, 1, 2, 3]
    offs, each, size = cc.placement(cc.case("at1_n16"))
    assert all(int(o) + int(e) == int(o2) for o, e, o2 in zip(offs, each, offs[1:])), "neighbours do not touch"
    offs, each, size = cc.placement(cc.case("rev_n16"))
    assert all(int(a) > int(b) + int(e) for a, b, e in zip(offs, offs[1:], each[1:])), "not reversed with gaps"
    # modular arithmetic
    wraps = cc.case("o2_n32_wraps")["fields"][0]
    assert d(wraps)["order"] == 2 and int(wraps["X"].max()) < 1 << 32
    dd = np.diff(wraps["X"].astype(object), 2)
    assert min(dd) < 0, "no sum of the decoder passes 2^64"
    over = cc.case("o2_n32_leaves_64")["fields"][1]
    assert int(over["X"].max()) >= 1 << 63 and cc.records(cc.case("o2_n32_leaves_64"))[1][2] == cc.RANGE
    rec = cc.records(cc.case("range_n8"))
    assert rec[0][0] >= 0 and rec[0][1:] == (300, cc.RANGE) and rec[1][2] == 0 and rec[2][0] == -5 and rec[2][2] == cc.RANGE
    # damaged streams, each between two clean fields
    dm = cc.case("damaged_n16")["fields"]
    assert [f["damaged"] for f in dm] == [None, "cut", None, "sum_low", None, "sum_high", None, "width33", None, "huge_lengths", None]
    cut = dm[1]
    assert cc.head_bytes(d(cut)) < cut["each"] < len(cut["stream"])
    assert d(dm[9])["length_bits"] == 32 and d(dm[9])["length_inc"] == 255
    assert sum(f["n"] for c in cases for f in c["fields"]) < 1 << 17


def run(emul, c):
    buf, offs, each = cc.buffer_of(c)
    nv = np.array(cc.n_values(c), np.uint64)
    wo = cc.work_offsets(c)
    work = np.full(int(wo[-1]), 0x5A, np.uint8)
    stores = np.zeros(work.size, np.uint32)
    cx = np.zeros(3 * nv.size, np.int64)
    descs = desc_array(c)
    outside = emul.gribcx_emul_expand((C.c_uint32 * 4)(*c["tmpl"]), ptr(nv), ptr(descs), C.c_uint64(nv.size), ptr(buf), ptr(offs), ptr(each),
                                      ptr(work), ptr(wo), ptr(stores), ptr(cx))
    return outside, work, stores, cx.reshape(-1, 3)


@pytest.mark.parametrize("name", NAMES)
def test_expand_is_the_model(emul, name):
    c = cc.case(name)
    outside, work, stores, cx = run(emul, c)
    assert outside == 0, "a load left its stream"
    in_room = np.zeros(work.size, np.uint32)
    for o, r in zip(cc.work_offsets(c), cc.rooms(c)):
        in_room[int(o):int(o) + r] = 1
    assert np.array_equal(stores, in_room), "a room byte was not stored exactly once, or a byte outside the rooms was stored"
    exact, loose = cc.room_regions(c)
    for o, want in exact:
        bad = np.flatnonzero(work[o:o + want.size] != want)
        assert bad.size == 0, (name, o, int(bad[0]))
    for f, want, got in zip(c["fields"], cc.records(c), cx):
        if f["damaged"]:
            assert int(got[2]) & cc.MALFORMED, f["damaged"]
        else:
            assert tuple(int(v) for v in got) == want
