"""CPU check of the bitmap layer's arithmetic (libaec_amd/csrc/aec_gribbm.h) through the host harness
tests/emul/gribbm_emul.cpp, which runs the functions the kernels of aec_gribbm.hip call wavefront by wavefront and lane by
lane and counts every access outside a field's elements, bitmap or room, over the case list of tests/grib_bitmap_cases.py:
the bitmap build against numpy.packbits, the tile bases against the NumPy prefix sum, the X rooms and records against
grib_cases.pack_model of y[mask] byte for byte (padding included), the expanded grids against grib_cases.dequantise
scattered by NumPy, and a count that is one more or one less than the bitmap's ones."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grib_bitmap_cases as bc
import grib_cases as gc
from helpers import ROOT

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libgribbm_emul.so")
NAMES = [b["name"] for b in bc.batches()]


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "gribbm_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h)
                                                          for h in ("aec_gribbm.h", "aec_grib.h", "aec_lane.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", EMUL_SO,
                        srcs[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    for f in (lib.gribbm_emul_build, lib.gribbm_emul_pack, lib.gribbm_emul_unpack):
        f.restype = C.c_int64
    lib.gribbm_emul_tile_points.restype = C.c_uint32
    return lib


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def batch(name):
    return next(b for b in bc.batches() if b["name"] == name)


def lay_out(b, grids=None, n_values=None):
    """(source bytes with 0xA5 between the grids, offsets, bitmap bytes, bitmap offsets, n_points, n_values, work offsets, rooms)"""
    offs, extent = bc.grid_placement(b)
    src = np.full(extent + 64, 0xA5, np.uint8)
    for o, g in zip(offs, b["grids"] if grids is None else grids):
        src[o:o + g.nbytes] = g.view(np.uint8)
    bitmap, bm_offs = bc.bitmaps(b)
    nbits, _, bs, _ = b["tmpl"]
    n_values = np.array([int(m.sum()) for m in b["masks"]] if n_values is None else n_values, np.uint64)
    rooms = [gc.room(int(n), bs, nbits) for n in n_values]
    work_offs = np.concatenate([[0], np.cumsum([gc.up16(r) for r in rooms])]).astype(np.uint64)
    return src, np.array(offs, np.uint64), bitmap, bm_offs, np.array([m.size for m in b["masks"]], np.uint64), n_values, work_offs, rooms


def test_the_case_list_holds_what_it_is_for(emul):
    assert emul.gribbm_emul_tile_points() == bc.T
    sizes = {n for n, kind in bc.GRIDS}
    assert {1, 7, 8, 9, 63, 64, 65, bc.T - 1, bc.T, bc.T + 1, 2 * bc.T + 5, 65 * bc.T + 3} == sizes
    for b in bc.batches():
        nbits, _, bs, _ = b["tmpl"]
        counts = [int(m.sum()) for m in b["masks"]]
        assert min(counts) >= 1
        assert any(c % bs for c in counts), "no field has a padding"
        odd = [bool((bc.tile_bases(m)[1:] % 2).any()) for m in b["masks"] if m.size > bc.T]
        assert any(odd), "no tile base is odd"
        kinds = dict((kind, m) for (n, kind), m in zip(bc.GRIDS, b["masks"]) if n == 65 * bc.T + 3)
        z = kinds["zero_mid"]
        assert not z[31 * bc.T:32 * bc.T].any() and z[:31 * bc.T].any() and z[32 * bc.T:].any()
        z = kinds["zero_tail2"]
        assert int(np.flatnonzero(z)[-1]) // bc.T == 62 and z.size // bc.T == 65
        offs, _ = bc.grid_placement(b)
        assert {o % 16 for o in offs} == {0, b["elem"]}
        bitmap, bm_offs = bc.bitmaps(b)
        assert int(bm_offs[0]) == b["bm0"] and len({int(o) % 2 for o in bm_offs}) == 2
        for g, m in zip(b["grids"], b["masks"]):
            if (~m).sum() >= 5:
                a = g[~m]
                assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any() and (a == 9999).any()
                assert b["elem"] == 4 or (a == 1e300).any()
    assert {b["tmpl"][0] for b in bc.batches()} == {8, 12, 24} and {b["tmpl"][2] for b in bc.batches()} == {8, 32}
    assert {(b["elem"], np.isnan(b["missing"])) for b in bc.batches()} == {(4, False), (4, True), (8, False), (8, True)}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("missing", [9999.0, float("nan")])
def test_build_is_packbits(emul, name, missing):
    b = batch(name)
    src, offs, want_bitmap, bm_offs, n_points, n_values, _, _ = lay_out(b, bc.build_grids(b, missing))
    bitmap = np.full(want_bitmap.size + 5, 0x5A, np.uint8)
    counts = np.zeros(n_points.size, np.uint64)
    outside = emul.gribbm_emul_build(b["elem"], ptr(src), ptr(offs), ptr(n_points), C.c_double(missing), C.c_uint64(n_points.size),
                                     ptr(bitmap), ptr(bm_offs), ptr(counts))
    assert outside == 0
    want = np.concatenate([want_bitmap, np.full(5, 0x5A, np.uint8)])
    want[:b["bm0"]] = 0x5A
    assert np.array_equal(bitmap, want) and np.array_equal(counts, n_values)


def run_pack(emul, b, n_values=None):
    src, offs, bitmap, bm_offs, n_points, nv, work_offs, rooms = lay_out(b, n_values=n_values)
    n = n_points.size
    work = np.full(int(work_offs[-1]), 0x5A, np.uint8)
    fields = np.zeros(n, gc.RECORD_DTYPE)
    bases = np.zeros(sum((int(p) + bc.T - 1) // bc.T for p in n_points), np.uint64)
    D = np.array(b["D"], np.int32)
    params = np.zeros(n, gc.RECORD_DTYPE)
    outside = emul.gribbm_emul_pack((C.c_uint32 * 4)(*b["tmpl"]), b["elem"], ptr(src), ptr(offs), ptr(n_points), ptr(nv), ptr(work_offs),
                                    ptr(D), 0, ptr(params), C.c_uint64(n), ptr(bitmap), ptr(bm_offs), ptr(work), ptr(fields), ptr(bases))
    return outside, fields, work, work_offs, rooms, bases


def expected_work(b, model, work_offs, rooms, skip=(), fill=0x5A):
    nbits = b["tmpl"][0]
    want = np.full(int(work_offs[-1]), fill, np.uint8)
    known = np.ones(want.size, bool)
    for i, ((R, E, st, x), o, r) in enumerate(zip(model, work_offs, rooms)):
        o = int(o)
        if i in skip:
            known[o:o + r] = False
        else:
            want[o:o + r] = gc.x_bytes(x, nbits, r // gc.container(nbits))
    return want, known


def check_records(b, fields, model, skip=()):
    for i, (R, E, st, x) in enumerate(model):
        if i in skip:
            continue
        f = fields[i]
        assert int(f["status"]) == st and int(f["D"]) == b["D"][i], (b["name"], i, f, st)
        assert f["R"].tobytes() == np.float32(R).tobytes() and int(f["E"]) == E, (b["name"], i, f, R, E)


@pytest.mark.parametrize("name", NAMES)
def test_pack_is_the_model_of_the_present_points(emul, name):
    b = batch(name)
    model = gc.model_of(b)
    assert not any(m[2] & gc.BAD for m in model)
    outside, fields, work, work_offs, rooms, bases = run_pack(emul, b)
    assert outside == 0
    assert np.array_equal(bases, np.concatenate([bc.tile_bases(m) for m in b["masks"]]))
    check_records(b, fields, model)
    want, known = expected_work(b, model, work_offs, rooms)
    bad = np.flatnonzero(work != want)
    assert bad.size == 0, (name, int(bad[0]))


def run_unpack(emul, b, model, n_values=None):
    src, offs, bitmap, bm_offs, n_points, nv, work_offs, rooms = lay_out(b, n_values=n_values)
    work, _ = expected_work(b, model, work_offs, rooms, skip=() if n_values is None else {WRONG}, fill=0xFF)
    n = n_points.size
    params = np.zeros(n, gc.RECORD_DTYPE)
    for i, (R, E, st, x) in enumerate(model):
        params[i] = (R, E, b["D"][i], 0)
    dst = np.full(src.size, 0xA5, np.uint8)
    status = np.full(n, 77, np.uint32)
    bases = np.zeros(sum((int(p) + bc.T - 1) // bc.T for p in n_points), np.uint64)
    outside = emul.gribbm_emul_unpack((C.c_uint32 * 4)(*b["tmpl"]), b["elem"], ptr(work), ptr(work_offs), ptr(n_points), ptr(nv),
                                      ptr(params), ptr(offs), C.c_uint64(n), ptr(bitmap), ptr(bm_offs), C.c_double(b["missing"]), ptr(dst),
                                      ptr(status), ptr(bases))
    return outside, dst, status, offs, src.size, bases


def expected_dst(b, model, offs, size, skip=()):
    want = np.full(size, 0xA5, np.uint8)
    known = np.ones(size, bool)
    for i, o in enumerate(offs):
        o = int(o)
        if i in skip:
            known[o:o + b["grids"][i].nbytes] = False
        else:
            want[o:o + b["grids"][i].nbytes] = bc.expanded(b, i, model, b["missing"]).view(np.uint8)
    return want, known


@pytest.mark.parametrize("name", NAMES)
def test_unpack_is_the_model_scattered(emul, name):
    b = batch(name)
    model = gc.model_of(b)
    outside, dst, status, offs, size, bases = run_unpack(emul, b, model)
    assert outside == 0 and not status.any()
    assert np.array_equal(bases, np.concatenate([bc.tile_bases(m) for m in b["masks"]]))
    want, _ = expected_dst(b, model, offs, size)
    bad = np.flatnonzero(dst != want)
    assert bad.size == 0, (name, int(bad[0]))


# the field whose count is wrong: 65T + 3 points at density 0.5 (two rounds of the scan, neighbours on either side)
WRONG = 16


@pytest.mark.parametrize("name", NAMES[:2])
@pytest.mark.parametrize("delta", [1, -1])
def test_a_mismatching_count_stays_inside(emul, name, delta):
    """a host count one more or one less than the bitmap's ones: bit 3 for that field, no index outside its room, its
    bitmap or its grid, every other field exact"""
    b = batch(name)
    model = gc.model_of(b)
    counts = [int(m.sum()) for m in b["masks"]]
    assert 1 < counts[WRONG] < b["masks"][WRONG].size
    n_values = list(counts)
    n_values[WRONG] += delta
    outside, fields, work, work_offs, rooms, bases = run_pack(emul, b, n_values)
    assert outside == 0
    assert [int(s) & bc.MISMATCH for s in fields["status"]] == [bc.MISMATCH if i == WRONG else 0 for i in range(len(counts))]
    check_records(b, fields, model, skip={WRONG})
    want, known = expected_work(b, model, work_offs, rooms, skip={WRONG})
    assert not ((work != want) & known).any()
    outside, dst, status, offs, size, bases = run_unpack(emul, b, model, n_values)
    assert outside == 0
    assert [int(s) for s in status] == [bc.MISMATCH if i == WRONG else 0 for i in range(len(counts))]
    want, known = expected_dst(b, model, offs, size, skip={WRONG})
    assert not ((dst != want) & known).any()
