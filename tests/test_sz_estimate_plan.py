"""aec_gpu_sz_estimate_plan (include/aec_gpu_sz.h; host arithmetic in libaec.so.0, no device): the sizes evaluated, the
passes, the pieces and the refusals, against a restatement in Python over py_layout.  The two entry points are bound here
directly: a library without them fails these tests."""
import ctypes as C

import numpy as np
import pytest

import helpers
from sz_device_cases import MSB, NN, RAW
from test_sz_layout import py_layout


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from libaec_amd import api, szgpu
    lib = api.library()
    lib.aec_gpu_sz_estimate_plan.restype = C.c_int
    lib.aec_gpu_sz_estimate_plan.argtypes = [C.POINTER(szgpu.SZ_com_t), C.c_void_p, C.c_void_p, C.c_uint64,
                                             C.POINTER(szgpu.SzEstimatePlan)]
    lib.aec_gpu_sz_estimate_async.restype = C.c_int
    lib.aec_gpu_sz_estimate_async.argtypes = [C.c_void_p, C.POINTER(szgpu.SZ_com_t)] + [C.c_void_p] * 4 + [C.c_uint64] + \
        [C.c_void_p] * 3
    return lib


def plan(lib, opts, bpp, pps_all, sizes, pps=None, ppb=0):
    from libaec_amd import szgpu
    sz = szgpu.SZ_com_t(opts, bpp, ppb, pps_all)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    vec = (C.c_uint * 4)(*pps) if pps is not None else None
    out = szgpu.SzEstimatePlan()
    if not lib.aec_gpu_sz_estimate_plan(C.byref(sz), vec, C.c_void_p(sizes.ctypes.data), sizes.size, C.byref(out)):
        return None
    return dict(evaluated=out.evaluated, passes=out.passes, pieces=out.pieces, workspace_bytes=out.workspace_bytes)


def restated(opts, bpp, pps, sizes):
    lines_of = {}
    for i in range(4):
        if pps[i]:
            Ls = [py_layout(opts, bpp, 8 << i, pps[i], s) for s in sizes]
            if any(L is None for L in Ls):
                return None
            lines_of.setdefault(pps[i], sum(L["lines"] for L in Ls))
    if not lines_of:
        return None
    return dict(evaluated=sum(1 << i for i in range(4) if pps[i]), passes=len(lines_of),
                pieces=sum(lines * -(-line // 64) for line, lines in lines_of.items()))


SIZES = [4096, 8, 100001, 64, 12345]


@pytest.mark.parametrize("opts,bpp", [(NN | RAW, 8), (RAW, 12), (NN | MSB | RAW, 16), (NN | RAW, 24), (NN | RAW, 32), (MSB | RAW, 64)])
def test_evaluated_passes_and_pieces(lib, opts, bpp):
    for pps in ([5] * 4, [63] * 4, [64] * 4, [65] * 4, [100, 100, 128, 0], [0, 0, 0, 1100], [32768] * 4, [7, 9, 11, 13],
                [0, 130, 0, 130], [262144, 0, 0, 0][::-1]):
        want = restated(opts, bpp, pps, SIZES)
        got = plan(lib, opts, bpp, 1, SIZES, pps)
        assert want is not None and got is not None, pps
        assert {k: got[k] for k in want} == want, pps
        # the records of the largest pass, the sums and the descriptors: more than the records, less than twice the chunks
        assert got["workspace_bytes"] > 0
    assert plan(lib, opts, bpp, 1, [], [64] * 4) == dict(evaluated=15, passes=1, pieces=0, workspace_bytes=0)


def test_null_scan_lines_take_the_sz_com_ts_for_all_four(lib):
    for ppb in (0, 8, 7, 1000):                                    # pixels_per_block is ignored
        got = plan(lib, NN | RAW, 16, 100, SIZES, None, ppb)
        assert got == plan(lib, NN | RAW, 16, 1, SIZES, [100] * 4) and got["evaluated"] == 15 and got["passes"] == 1
    assert plan(lib, NN | RAW, 16, 0, SIZES, None) is None
    assert plan(lib, NN | RAW, 16, -5, SIZES, None) is None


def test_the_workspace_holds_the_records_of_one_pass(lib):
    """16-bit records at line * rsi + block for every size of a pass, passes reusing the room: 64 chunks of 1 MiB of
    16-bit pixels under 1024 pixels per line are 32768 lines of 128 + 64 + 32 + 16 blocks"""
    sizes = [1 << 20] * 64
    one = plan(lib, NN | RAW, 16, 1024, sizes, None)
    records = 32768 * (128 + 64 + 32 + 16) * 2
    assert one["pieces"] == 32768 * 16 and records < one["workspace_bytes"] < records * 5 // 4 + (1 << 16)
    two = plan(lib, NN | RAW, 16, 1, sizes, [1024, 1024, 1000, 1000])
    assert two["passes"] == 2 and two["workspace_bytes"] < one["workspace_bytes"] + (1 << 16)


@pytest.mark.parametrize("opts,bpp,pps,sizes", [
    (NN, 8, [0, 0, 0, 0], [64]),                 # no size asked
    (NN, 8, [32769, 0, 0, 0], [64]),             # 4097 blocks of 8 per line
    (NN, 8, [64, 64, 64, 262145], [64]),         # ... of 64
    (NN, 16, [100] * 4, [200, 1, 200]),          # a chunk without a whole pixel
    (NN, 64, [24] * 4, [800, 7]),
    (NN, 33, [64] * 4, [64]),                    # bits per pixel the layout rejects
    (NN, 0, [64] * 4, [64]),
    (NN, 8, [1024] * 4, [1 << 35]),              # a chunk no launch can count
    (NN, 8, [0, 0, 0, 5], [1 << 30] * 40),       # more than 2^25 wavefronts: 5 pixels a line make a piece a line
])
def test_refusals(lib, opts, bpp, pps, sizes):
    assert plan(lib, opts, bpp, 1, sizes, pps) is None


def test_a_size_that_is_not_asked_is_not_checked(lib):
    assert plan(lib, NN, 8, 1, [64], [0, 32769, 0, 0])["evaluated"] == 2          # 2049 blocks of 16
    assert plan(lib, NN, 8, 1, [64], [32768, 32769, 0, 0])["passes"] == 2


def test_null_arguments(lib):
    from libaec_amd import szgpu
    sz = szgpu.SZ_com_t(NN, 8, 8, 64)
    sizes = np.array([64, 128], dtype=np.uint64)
    out = szgpu.SzEstimatePlan()
    assert lib.aec_gpu_sz_estimate_plan(None, None, C.c_void_p(sizes.ctypes.data), 2, C.byref(out)) == 0
    assert lib.aec_gpu_sz_estimate_plan(C.byref(sz), None, None, 2, C.byref(out)) == 0
    assert lib.aec_gpu_sz_estimate_plan(C.byref(sz), None, C.c_void_p(sizes.ctypes.data), 2, None) == 0
    assert lib.aec_gpu_sz_estimate_plan(C.byref(sz), None, C.c_void_p(sizes.ctypes.data), 2, C.byref(out)) == 1
    assert lib.aec_gpu_sz_estimate_plan(C.byref(sz), None, None, 0, C.byref(out)) == 1 and out.pieces == 0


def test_the_async_call_refuses_before_it_touches_the_device(lib):
    """NULL arguments come back from the host checks: no context, no device needed"""
    from libaec_amd import szgpu
    sz = szgpu.SZ_com_t(NN, 8, 8, 64)
    assert lib.aec_gpu_sz_estimate_async(None, C.byref(sz), None, None, None, None, 0, None, None, None) == helpers.AEC_CONF_ERROR


def test_the_python_mirror_gives_the_same(lib):
    from libaec_amd import szgpu
    assert szgpu.estimate_plan(NN | RAW, 16, 1, SIZES, [100, 100, 128, 0]) == plan(lib, NN | RAW, 16, 1, SIZES, [100, 100, 128, 0])
    assert szgpu.estimate_plan(NN | RAW, 16, 100, SIZES) == plan(lib, NN | RAW, 16, 100, SIZES)
    assert szgpu.estimate_plan(NN | RAW, 16, 1, SIZES, [0] * 4) is None
