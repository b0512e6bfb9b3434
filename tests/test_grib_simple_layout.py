"""Host arithmetic of the simple-packing calls (include/aec_gpu_grib.h: aec_gpu_grib_simple_plan) against a Python
restatement: the plan is aec_gpu_grib_plan's, simple_bytes the sum of ceil(n * nbits / 8), simple_offsets its running sum;
it refuses what aec_gpu_grib_plan refuses; block size 12 is taken; the new symbols are exported; and what the calls answer
without a device: an empty batch is AEC_OK, a refused one AEC_CONF_ERROR before anything touches a device.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import grib_cases as gc
import grib_simple_cases as sc
from libaec_amd import gribgpu

TMPL = (16, gc.PP, 32, 128)
SYMBOLS = ["aec_gpu_grib_simple_plan", "aec_gpu_grib_bits_pack_async", "aec_gpu_grib_bits_unpack_async", "aec_gpu_grib_simple_pack_async",
           "aec_gpu_grib_simple_unpack_async", "aec_gpu_grib_simple_to_ccsds_async", "aec_gpu_grib_ccsds_to_simple_async"]
FAKE = C.c_void_p(1 << 20)          # a pointer that is not null and 16-byte aligned; a refused call never follows it


def test_the_new_symbols_are_exported():
    lib = gribgpu._lib()
    assert all(hasattr(lib, s) for s in SYMBOLS)


@pytest.mark.parametrize("name", [c["name"] for c in sc.cases()])
@pytest.mark.parametrize("elem", [gc.F32, gc.F64])
def test_plan_is_the_restatement(name, elem):
    c = sc.case(name)
    nbits = c["tmpl"][0]
    nv = sc.n_values(c)
    got, plain = gribgpu.simple_plan(*c["tmpl"], elem, nv), gribgpu.plan(*c["tmpl"], elem, nv)
    assert got is not None and plain is not None, "the batch is refused (block size 12 among it)"
    for key in ("coder", "work_bytes", "out_bound", "rsi_entries", "workspace_bytes"):
        assert got[key] == plain[key], key
    assert np.array_equal(got["work_offsets"], plain["work_offsets"]) and np.array_equal(got["work_offsets"], sc.work_offsets(c)[:-1])
    sizes = [(n * nbits + 7) // 8 for n in nv]
    assert got["simple_bytes"] == sum(sizes)
    assert [int(o) for o in got["simple_offsets"]] == [sum(sizes[:i]) for i in range(len(sizes))]
    if not c["rev"]:
        assert [int(o) - c["first"] for o in sc.placement(c)[0]] == [int(o) for o in got["simple_offsets"]]


def test_block_size_12_is_taken():
    assert sc.ODD_BS == 12
    for nbits in (7, 12, 25):
        s = sc.span(nbits)
        assert gribgpu.plan(nbits, gc.PP, 12, 128, gc.F32, [s, 2 * s]) is not None


def test_plan_of_nothing():
    got = gribgpu.simple_plan(*TMPL, gc.F32, [])
    assert got is not None and got["simple_bytes"] == 0 and got["work_bytes"] == 0 and got["simple_offsets"].size == 0


def test_plan_refuses_what_the_grib_plan_refuses():
    both = lambda t, elem, nv: (gribgpu.simple_plan(*t, elem, nv) is None, gribgpu.plan(*t, elem, nv) is None)
    assert both(TMPL, gc.F32, [100, 0, 5]) == (True, True)                        # a field without a value
    assert both(TMPL, gc.F32, [100, 1, 5]) == (False, False)
    assert both((0, gc.PP, 32, 128), gc.F32, [100]) == (True, True)               # nbits 0 and above 32
    assert both((33, gc.PP, 32, 128), gc.F32, [100]) == (True, True)
    assert both((32, gc.PP, 32, 128), gc.F32, [100]) == (False, False)
    assert both((1, 0, 8, 128), gc.F32, [100]) == (False, False)
    assert both((16, gc.PP | gc.SIGNED, 32, 128), gc.F32, [100]) == (True, True)
    assert both((16, gc.PP, 7, 128), gc.F32, [100]) == (True, True)               # an odd block size
    assert both(TMPL, 2, [100]) == (True, True) and both(TMPL, 16, [100]) == (True, True)
    assert both(TMPL, gc.F32, [1 << 32] * 5) == (True, True)                      # more than 2^25 wavefronts
    assert both(TMPL, gc.F64, [1 << 32]) == (True, True) and both(TMPL, gc.F64, [(1 << 32) - 1]) == (False, False)


def _call_all(t, elem, n, n_values, ptr=None, ctx=None, simple_bytes=0, offsets=None, each=None, which=range(6)):
    """the six calls with no context and null device pointers (or the FAKE ones): what they answer before they touch anything"""
    lib = gribgpu._lib()
    tm = gribgpu.Template(*t)
    nv = np.array(n_values, np.uint64)
    offs = np.zeros(max(1, n), np.uint64) if offsets is None else np.array(offsets, np.uint64)
    zero = np.zeros(max(1, n), np.uint64)
    Dh = np.zeros(max(1, n), np.int32)
    rec = gribgpu.records(R=0.0, E=0, D=0, n=max(1, n))
    h = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    eh = None if each is None else np.array(each, np.uint64)
    calls = [lambda: lib.aec_gpu_grib_bits_pack_async(ctx, C.byref(tm), h(nv), n, ptr, ptr, h(offs), None),
             lambda: lib.aec_gpu_grib_bits_unpack_async(ctx, C.byref(tm), h(nv), n, ptr, simple_bytes, h(offs), h(eh), ptr, None),
             lambda: lib.aec_gpu_grib_simple_pack_async(ctx, C.byref(tm), elem, ptr, h(zero), h(nv), h(Dh), 0, None, n, ptr, ptr, ptr, h(offs), None),
             lambda: lib.aec_gpu_grib_simple_unpack_async(ctx, C.byref(tm), elem, ptr, simple_bytes, h(offs), h(eh), h(nv), h(rec), h(zero),
                                                          n, ptr, ptr, None),
             lambda: lib.aec_gpu_grib_simple_to_ccsds_async(ctx, C.byref(tm), ptr, simple_bytes, h(offs), h(eh), h(nv), n, ptr, ptr, 1 << 20,
                                                            ptr, None, ptr, None),
             lambda: lib.aec_gpu_grib_ccsds_to_simple_async(ctx, C.byref(tm), ptr, 1 << 20, None, None, h(nv), n, ptr, 1, ptr, ptr, ptr, ptr,
                                                            h(offs), None)]
    return [calls[k]() for k in which]


READS = [1, 3, 4]           # the calls of _call_all that read streams: bits_unpack, simple_unpack, simple_to_ccsds


def test_no_fields_is_ok_and_enqueues_nothing():
    assert _call_all(TMPL, gc.F32, 0, [1]) == [0] * 6


def test_calls_refuse_before_they_touch_a_device():
    assert _call_all((0, gc.PP, 32, 128), gc.F32, 0, [1]) == [-1] * 6              # (the template is checked first, even for no fields)
    assert _call_all((33, gc.PP, 32, 128), gc.F32, 0, [1]) == [-1] * 6
    got = _call_all(TMPL, 3, 0, [1])                                               # an elem that is neither, where a call takes one
    assert [got[2], got[3]] == [-1, -1]
    assert _call_all(TMPL, gc.F32, 1, [100]) == [-1] * 6                           # no context, no pointers
    assert _call_all(TMPL, gc.F32, 1, [0], FAKE, FAKE, 1 << 20) == [-1] * 6        # a field without a value
    assert gribgpu.plan(*TMPL, gc.F32, [1 << 32] * 5) is None                      # more than 2^25 wavefronts
    assert _call_all(TMPL, gc.F32, 5, [1 << 32] * 5, FAKE, FAKE, 1 << 40) == [-1] * 6


def test_streams_that_do_not_fit_are_refused():
    """16 bits, fields of 100 and 7 values: S = 200 and 14 bytes.  Every argument but the one under test is one the calls
    take, so AEC_CONF_ERROR is that argument's (tests/test_gpu_grib_simple.py runs the same calls, taken, on a device)."""
    nv, offs = [100, 7], [3, 203]
    refused = lambda **kw: _call_all(TMPL, gc.F32, 2, nv, FAKE, FAKE, which=READS, **kw)
    assert refused(simple_bytes=216, offsets=offs) == [-1] * 3                     # the last stream ends one byte behind the buffer
    assert refused(simple_bytes=217, offsets=offs, each=[199, 14]) == [-1] * 3     # section 7 is one byte too short
    assert refused(simple_bytes=217, offsets=offs, each=[200, 13]) == [-1] * 3
    assert refused(simple_bytes=217, offsets=[3, 1 << 63]) == [-1] * 3             # an offset beyond everything
    assert refused(simple_bytes=217, offsets=[(1 << 64) - 100, 203]) == [-1] * 3   # offset + S wraps
