"""Host arithmetic of the bitmap calls (include/aec_gpu_grib.h: aec_gpu_grib_bitmap_plan) against a Python restatement:
rooms, offsets, out_bound and rsi_entries are aec_gpu_grib_plan's for n_values, tiles is the sum of ceil(n_points / T),
the workspace grows by the tile tables; every refusal at its threshold; and what the calls answer without a device: an
empty batch is AEC_OK, a refused one AEC_CONF_ERROR before anything touches a device.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import grib_bitmap_cases as bc
import grib_cases as gc
from libaec_amd import gribgpu

T = bc.T
TMPL = (16, gc.PP, 32, 128)
TEMPLATES = [(8, gc.PP, 8, 128), (12, gc.PP, 32, 128), (24, 0, 32, 1), (32, gc.PP | gc.PAD_RSI, 64, 7)]


def test_the_constants():
    assert gribgpu.MISMATCH == bc.MISMATCH == 8
    p = gribgpu.bitmap_plan(*TMPL, gc.F32, [100], [50])
    assert p["tile_points"] == T and T % 64 == 0


@pytest.mark.parametrize("tmpl", TEMPLATES, ids=[f"n{t[0]}-bs{t[2]}" for t in TEMPLATES])
@pytest.mark.parametrize("elem", [gc.F32, gc.F64])
def test_plan_is_the_restatement(tmpl, elem):
    n_points = [1, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5, 65 * T + 3]
    n_values = [1, 3, 8, 1, 40, 64, 2, T - 1, 512, 1, T + 9, 33 * T + 1]
    got, plain = gribgpu.bitmap_plan(*tmpl, elem, n_points, n_values), gribgpu.plan(*tmpl, elem, n_values)
    assert got is not None and plain is not None
    for key in ("coder", "work_bytes", "out_bound", "rsi_entries"):
        assert got[key] == plain[key], key
    assert np.array_equal(got["work_offsets"], plain["work_offsets"])
    tiles = sum((p + T - 1) // T for p in n_points)
    assert got["tiles"] == tiles == 9 + 2 + 3 + 66            # nine grids of one tile, T + 1, 2T + 5, 65T + 3
    n = len(n_points)
    grown = got["workspace_bytes"] - plain["workspace_bytes"]
    # per tile: its field (4 bytes), its count (4) and its base (8); per field: two descriptors and the extremes
    assert tiles * 16 <= grown <= tiles * 16 + (n + 1) * (24 + 80) + n * 16 + 6 * 256 + 16


def test_plan_of_nothing():
    got = gribgpu.bitmap_plan(*TMPL, gc.F32, [], [])
    assert got is not None and got["tiles"] == 0 and got["work_bytes"] == 0 and got["work_offsets"].size == 0


def test_plan_refuses_at_the_thresholds():
    plan = lambda elem, p, v: gribgpu.bitmap_plan(*TMPL, elem, p, v)
    assert plan(gc.F32, [100, 5, 7], [100, 0, 5]) is None                          # a field without a present point
    assert plan(gc.F32, [100, 5, 7], [100, 1, 5]) is not None
    assert plan(gc.F32, [100, 5], [100, 6]) is None                                # more present points than points
    assert plan(gc.F32, [100, 5], [100, 5]) is not None
    assert plan(gc.F32, [(1 << 33) - 1], [10]) is not None                         # a grid of 2^35 bytes
    assert plan(gc.F32, [1 << 33], [10]) is None
    assert plan(gc.F64, [(1 << 32) - 1], [10]) is not None
    assert plan(gc.F64, [1 << 32], [10]) is None
    per = (1 << 33) - T                                                            # 2^23 - 1 tiles a grid
    assert (per + T - 1) // T == (1 << 23) - 1
    assert plan(gc.F32, [per] * 4 + [4 * T], [10] * 5) is not None                 # exactly 2^25 tiles
    assert plan(gc.F32, [per] * 4 + [4 * T + 1], [10] * 5) is None
    assert plan(2, [100], [50]) is None and plan(16, [100], [50]) is None          # an elem that is neither
    # everything aec_gpu_grib_plan refuses
    assert gribgpu.bitmap_plan(0, gc.PP, 32, 128, gc.F32, [100], [50]) is None
    assert gribgpu.bitmap_plan(16, gc.PP | gc.SIGNED, 32, 128, gc.F32, [100], [50]) is None
    assert gribgpu.bitmap_plan(16, gc.PP, 7, 128, gc.F32, [100], [50]) is None
    big = [1 << 32] * 5                                                            # more than 2^25 wavefronts of 1 KiB of room
    assert gribgpu.plan(*TMPL, gc.F32, big) is None and plan(gc.F32, [1 << 32] * 5, big) is None


def _call_all(t, elem, n, n_points, n_values, D=0):
    """the six calls with null device pointers and no context: what they answer before they touch anything"""
    lib = gribgpu._lib()
    tm = gribgpu.Template(*t)
    nv, npts = np.array(n_values, np.uint64), np.array(n_points, np.uint64)
    offs = np.zeros(max(1, n), np.uint64)
    Dh = np.full(max(1, n), D, np.int32)
    rec = gribgpu.records(R=0.0, E=0, D=D, n=max(1, n))
    h = lambda a: C.c_void_p(a.ctypes.data)
    return [lib.aec_gpu_grib_bitmap_async(None, elem, None, h(offs), h(npts), 9999.0, n, None, h(offs), None, None),
            lib.aec_gpu_grib_pack_bitmap_async(None, C.byref(tm), elem, None, h(offs), h(nv), h(Dh), 0, None, n, None, None, 0, None, None,
                                               None, None, None, h(offs), h(npts), None),
            lib.aec_gpu_grib_unpack_bitmap_async(None, C.byref(tm), elem, None, 0, None, None, h(nv), h(rec), h(offs), n, None, 0, None,
                                                 None, None, None, None, h(offs), h(npts), 9999.0, None, None),
            lib.aec_gpu_grib_quantise_bitmap_async(None, C.byref(tm), elem, None, h(offs), h(nv), h(Dh), 0, None, n, None, None, None,
                                                   h(offs), h(npts), None),
            lib.aec_gpu_grib_dequantise_bitmap_async(None, C.byref(tm), elem, None, h(nv), h(rec), h(offs), n, None, None, h(offs),
                                                     h(npts), 9999.0, None, None)]


def test_no_fields_is_ok_and_enqueues_nothing():
    assert _call_all(TMPL, gc.F32, 0, [1], [1]) == [0] * 5


def test_calls_refuse_before_they_touch_a_device():
    assert _call_all((0, gc.PP, 32, 128), gc.F32, 0, [1], [1])[1:] == [-1] * 4       # (the template is checked first, even for no fields)
    assert _call_all(TMPL, 3, 0, [1], [1]) == [-1] * 5
    assert _call_all(TMPL, gc.F32, 1, [100], [50]) == [-1] * 5                       # no context, no pointers
    assert _call_all(TMPL, gc.F32, 1, [100], [0]) == [-1] * 5
    assert _call_all(TMPL, gc.F32, 1, [100], [101]) == [-1] * 5
