"""Host arithmetic of the complex-packing calls (include/aec_gpu_grib.h: aec_gpu_grib_complex_plan) against a Python
restatement: the plan is aec_gpu_grib_plan's with workspace_bytes grown by the descriptors, the group tables and the tile
aggregates; tile_values, value_tiles and group_tiles; the new symbols are exported; and what the calls answer without a
device: an empty batch is AEC_OK, every refusal the header lists is AEC_CONF_ERROR before anything touches a device.  No GPU
needed."""
import ctypes as C

import numpy as np
import pytest

import grib_cases as gc
import grib_complex_cases as cc
from libaec_amd import gribgpu

TMPL = (16, gc.PP, 32, 128)
SYMBOLS = ["aec_gpu_grib_complex_plan", "aec_gpu_grib_complex_expand_async", "aec_gpu_grib_complex_unpack_async",
           "aec_gpu_grib_complex_to_ccsds_async"]
FAKE = C.c_void_p(1 << 20)          # a pointer that is not null and 16-byte aligned; a refused call never follows it
GOOD = dict(ref_bits=8, n_groups=10, width_ref=0, width_bits=4, length_ref=1, length_inc=1, last_length=10, length_bits=8, order=2,
            extra_octets=2, missing=0)
HEAD = 3 * 2 + 10 + 5 + 10          # the extra descriptors and the three tables of GOOD


def up256(v):
    return (v + 255) // 256 * 256


def test_the_new_symbols_are_exported():
    lib = gribgpu._lib()
    assert all(hasattr(lib, s) for s in SYMBOLS)
    assert C.sizeof(gribgpu.ComplexField) == 44 and gribgpu.CX_DTYPE.itemsize == 24


@pytest.mark.parametrize("name", [c["name"] for c in cc.cases()])
@pytest.mark.parametrize("elem", [gc.F32, gc.F64])
def test_plan_is_the_restatement(name, elem):
    c = cc.case(name)
    nbits = c["tmpl"][0]
    nv, descs = cc.n_values(c), cc.descs(c)
    got, plain = gribgpu.complex_plan(*c["tmpl"], elem, nv, descs), gribgpu.plan(*c["tmpl"], elem, nv)
    assert got is not None and plain is not None
    for key in ("coder", "work_bytes", "out_bound", "rsi_entries"):
        assert got[key] == plain[key], key
    assert np.array_equal(got["work_offsets"], plain["work_offsets"]) and np.array_equal(got["work_offsets"], cc.work_offsets(c)[:-1])
    n = len(nv)
    vt = sum((r + gc.WAVE_ROOM - 1) // gc.WAVE_ROOM for r in cc.rooms(c))
    gt = sum((d["n_groups"] + cc.GROUP_TILE - 1) // cc.GROUP_TILE for d in descs)
    groups = sum(d["n_groups"] for d in descs)
    assert (got["tile_values"], got["value_tiles"], got["group_tiles"]) == (cc.tile(nbits), vt, gt)
    # descriptors of 136 bytes, per-field records of 40, (values, bits) per group tile, 8 + 8 + 4 + 4 bytes a group, 16 + 8 + 8 a
    # value tile
    grown = (up256((n + 1) * 136) + up256(n * 40) + up256(gt * 16) + 2 * up256(groups * 8) + 2 * up256(groups * 4) + up256(vt * 16) +
             2 * up256(vt * 8))
    assert got["workspace_bytes"] == plain["workspace_bytes"] + grown


def test_plan_of_nothing():
    got = gribgpu.complex_plan(*TMPL, gc.F32, [], [])
    assert got is not None and got["work_bytes"] == 0 and got["value_tiles"] == 0 and got["group_tiles"] == 0


def changed(**kw):
    return dict(GOOD, **kw)


REFUSED = [("missing", changed(missing=1)), ("missing 2", changed(missing=2)), ("order", changed(order=3)),
           ("extra_octets", changed(extra_octets=9)), ("ref_bits", changed(ref_bits=33)), ("width_bits", changed(width_bits=33)),
           ("length_bits", changed(length_bits=33)), ("no group", changed(n_groups=0)), ("more groups than values", changed(n_groups=101))]
TAKEN = [changed(extra_octets=8), changed(ref_bits=32, width_bits=32, length_bits=32), changed(ref_bits=0, width_bits=0, length_bits=0),
         changed(n_groups=100), changed(order=0, extra_octets=99), changed(width_ref=1 << 31, length_ref=(1 << 32) - 1, length_inc=255)]


def test_plan_refuses_what_the_header_lists():
    plan = lambda t, nv, ds, elem=gc.F32: gribgpu.complex_plan(*t, elem, nv, ds)
    assert plan(TMPL, [100, 50], [GOOD, GOOD]) is not None
    for why, d in REFUSED:
        assert plan(TMPL, [100, 50, 100], [GOOD, GOOD, d]) is None, why
    for d in TAKEN:
        assert plan(TMPL, [100, 100], [GOOD, d]) is not None, d
    # whatever aec_gpu_grib_plan refuses for the template and n_values
    assert plan(TMPL, [100, 0], [GOOD, changed(n_groups=1)]) is None
    assert plan((0, gc.PP, 32, 128), [100], [GOOD]) is None and plan((33, gc.PP, 32, 128), [100], [GOOD]) is None
    assert plan((16, gc.PP | gc.SIGNED, 32, 128), [100], [GOOD]) is None and plan((16, gc.PP, 7, 128), [100], [GOOD]) is None
    assert plan(TMPL, [100], [GOOD], elem=3) is None
    assert plan(TMPL, [1 << 32] * 5, [GOOD] * 5) is None                           # more than 2^25 wavefronts
    # the totals of the group tables: 2^25 tiles of 64 groups, 2^31 - 1 groups
    many = changed(n_groups=(1 << 31) - 64)
    assert plan((8, gc.PP, 32, 128), [1 << 31], [many]) is not None
    assert plan((8, gc.PP, 32, 128), [1 << 31, 100], [many, changed(n_groups=65)]) is None


def _calls(t, n, n_values, descs, ptr=FAKE, ctx=FAKE, complex_bytes=1 << 20, offsets=None, each=None, elem=gc.F32, work=None, which=range(3)):
    """the three calls with pointers nothing follows: what they answer before they touch anything"""
    lib = gribgpu._lib()
    tm = gribgpu.Template(*t)
    nv = np.array(n_values, np.uint64)
    offs = np.zeros(max(1, n), np.uint64) if offsets is None else np.array(offsets, np.uint64)
    ea = np.full(max(1, n), 4096, np.uint64) if each is None else np.array(each, np.uint64)
    zero = np.zeros(max(1, n), np.uint64)
    rec = gribgpu.records(R=0.0, E=0, D=0, n=max(1, n))
    h = lambda a: C.c_void_p(a.ctypes.data)
    fields = gribgpu.complex_fields(descs)
    work = ptr if work is None else work
    calls = [lambda: lib.aec_gpu_grib_complex_expand_async(ctx, C.byref(tm), fields, h(nv), n, ptr, complex_bytes, h(offs), h(ea), work, ptr, None),
             lambda: lib.aec_gpu_grib_complex_unpack_async(ctx, C.byref(tm), elem, fields, ptr, complex_bytes, h(offs), h(ea), h(nv), h(rec), h(zero), n,
                                                  work, ptr, ptr, None),
             lambda: lib.aec_gpu_grib_complex_to_ccsds_async(ctx, C.byref(tm), fields, ptr, complex_bytes, h(offs), h(ea), h(nv), n, work, ptr, 1 << 20,
                                                    ptr, None, ptr, ptr, None)]
    return [calls[k]() for k in which]


def test_no_fields_is_ok_and_enqueues_nothing():
    assert _calls(TMPL, 0, [1], [GOOD], ptr=None, ctx=None) == [0] * 3


def test_calls_refuse_before_they_touch_a_device():
    assert _calls((0, gc.PP, 32, 128), 0, [1], [GOOD]) == [-1] * 3                   # (the template is checked first, even for no fields)
    assert _calls(TMPL, 1, [100], [GOOD], elem=3, which=[1]) == [-1]                # an elem that is neither, where a call takes one
    assert _calls(TMPL, 1, [100], [GOOD], ptr=None, ctx=None) == [-1] * 3           # no context, no pointers
    assert _calls(TMPL, 1, [100], [GOOD], work=C.c_void_p((1 << 20) + 8)) == [-1] * 3   # a work buffer off its 16 bytes
    for why, d in REFUSED:
        assert _calls(TMPL, 3, [100, 50, 100], [GOOD, GOOD, d]) == [-1] * 3, why
    assert _calls(TMPL, 2, [100, 0], [GOOD, changed(n_groups=1)]) == [-1] * 3


def test_streams_that_do_not_fit_are_refused():
    """Every argument but the one under test is one the calls take, so AEC_CONF_ERROR is that argument's
    (tests/test_gpu_grib_complex.py runs the same calls, taken, on a device)."""
    nv, ds = [100, 50], [GOOD, GOOD]
    refused = lambda **kw: _calls(TMPL, 2, nv, ds, **kw)
    assert refused(each=[HEAD - 1, 500]) == [-1] * 3                               # shorter than the tables and the extra descriptors
    assert refused(each=[500, HEAD - 1]) == [-1] * 3
    assert refused(each=[1 << 35, 500], complex_bytes=1 << 36) == [-1] * 3         # a stream a launch cannot count
    assert refused(complex_bytes=699, offsets=[3, 200], each=[197, 500]) == [-1] * 3   # the last stream ends one byte behind the buffer
    assert refused(complex_bytes=700, offsets=[3, 1 << 63], each=[197, 500]) == [-1] * 3
    assert refused(complex_bytes=700, offsets=[(1 << 64) - 100, 200], each=[197, 500]) == [-1] * 3   # offset + bytes wraps
