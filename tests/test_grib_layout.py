"""Host arithmetic of the GRIB layer (include/aec_gpu_grib.h: aec_gpu_grib_layout, aec_gpu_grib_plan) against a Python
restatement, every refusal the header lists, and what the calls answer without a device: an empty batch is AEC_OK, a
refused one AEC_CONF_ERROR before anything touches a device.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import grib_cases as gc
from libaec_amd import gpu, gribgpu

TEMPLATES = [(nbits, options, bs, rsi)
             for nbits in (1, 2, 4, 8, 9, 12, 16, 17, 24, 25, 32)
             for options, bs, rsi in ((gc.PP, 32, 128), (0, 8, 1), (gc.PP | gc.MSB | gc.THREE_BYTE, 16, 4096), (gc.PP | gc.PAD_RSI, 64, 7))]


def py_plan(tmpl, n_values):
    nbits, options, bs, rsi = tmpl
    rooms = [gc.room(n, bs, nbits) for n in n_values]
    flags = gc.coder_flags(options)
    enc = gpu.encode_chunks_plan(nbits, bs, rsi, flags, np.array(rooms, np.uint64))
    offs = np.concatenate([[0], np.cumsum([gc.up16(r) for r in rooms])]).astype(np.uint64)
    return dict(coder=(nbits, bs, rsi, flags), work_bytes=int(offs[-1]), out_bound=enc["out_bound"], rsi_entries=enc["rsi_entries"],
                work_offsets=offs[:-1])


@pytest.mark.parametrize("tmpl", TEMPLATES, ids=[f"n{t[0]}-o{t[1]}-bs{t[2]}-rsi{t[3]}" for t in TEMPLATES])
def test_layout_and_plan_are_the_restatement(tmpl):
    nbits, options, bs, rsi = tmpl
    L = gribgpu.layout(*tmpl, D=3)
    assert L is not None
    assert (L.coder.bits_per_sample, L.coder.block_size, L.coder.rsi, L.coder.flags) == (nbits, bs, rsi, gc.coder_flags(options))
    assert L.container == gc.container(nbits) and L.container != 3
    n_values = [1, bs - 1, bs, bs + 1, bs * rsi - 1, bs * rsi, bs * rsi + 1, 9001]
    for elem in (gc.F32, gc.F64):
        got, want = gribgpu.plan(*tmpl, elem, n_values), py_plan(tmpl, n_values)
        assert got is not None
        for key in ("coder", "work_bytes", "out_bound", "rsi_entries"):
            assert got[key] == want[key], key
        assert np.array_equal(got["work_offsets"], want["work_offsets"])
        rooms = np.array([gc.room(n, bs, nbits) for n in n_values], np.uint64)
        flags = gc.coder_flags(options)
        coder = max(gpu.encode_chunks_plan(nbits, bs, rsi, flags, rooms)["workspace_bytes"],
                    gpu.decode_chunks_plan(nbits, bs, rsi, flags & ~gc.NOT_ENFORCE, rooms)["workspace_bytes"])
        waves = sum((n * elem + gc.SPAN - 1) // gc.SPAN for n in n_values) + sum((int(r) + gc.WAVE_ROOM - 1) // gc.WAVE_ROOM for r in rooms)
        assert coder < got["workspace_bytes"] <= coder + 3 * 256 + (len(n_values) + 1) * 80 + (waves + 1) * 4 + len(n_values) * 16


def test_msb_and_three_byte_change_nothing():
    for nbits in (9, 24):
        a, b = gribgpu.layout(nbits, gc.PP, 32, 128), gribgpu.layout(nbits, gc.PP | gc.MSB | gc.THREE_BYTE, 32, 128)
        assert bytes(a) == bytes(b) and a.container == gc.container(nbits)


REFUSED = [
    ("signed", (16, gc.PP | gc.SIGNED, 32, 128), 0),
    ("nbits 0", (0, gc.PP, 32, 128), 0),
    ("nbits 33", (33, gc.PP, 32, 128), 0),
    ("D 23", (16, gc.PP, 32, 128), 23),
    ("D -23", (16, gc.PP, 32, 128), -23),
    ("odd block", (16, gc.PP, 7, 128), 0),
    ("block 0", (16, gc.PP, 0, 128), 0),
    ("block 66", (16, gc.PP, 66, 128), 0),
    ("rsi 0", (16, gc.PP, 32, 0), 0),
    ("rsi 4097", (16, gc.PP, 32, 4097), 0),
    ("restricted 5 bits", (5, gc.PP | gc.RESTRICTED, 32, 128), 0),
]


@pytest.mark.parametrize("what,tmpl,D", REFUSED, ids=[r[0] for r in REFUSED])
def test_layout_refuses(what, tmpl, D):
    assert gribgpu.layout(*tmpl, D=D) is None
    p = gpu.Params(tmpl[0], tmpl[2], tmpl[3], gc.coder_flags(tmpl[1]))
    if what not in ("signed", "nbits 0", "D 23", "D -23"):
        assert gpu._lib().aec_gpu_check_params(C.byref(p), 1) != 0          # (what the coder refuses)
    if not what.startswith("D"):
        assert gribgpu.plan(*tmpl, gc.F32, [100]) is None


def test_layout_takes_the_edges():
    assert gribgpu.layout(16, gc.PP, 32, 128, D=22) is not None and gribgpu.layout(16, gc.PP, 32, 128, D=-22) is not None
    assert gribgpu.layout(4, gc.PP | gc.RESTRICTED, 32, 128) is not None
    assert gribgpu.layout(32, 0, 64, 4096) is not None and gribgpu.layout(1, 0, 2, 1) is not None


def test_the_templates_of_the_edge_cases_are_taken():
    """every template of grib_cases.edge_batches() and dequantise_cases(), RSI padding and the restricted code set among
    them: the layout passes the flags through and the plan takes the batch"""
    cases = [(b["name"], b["tmpl"], b["elem"], [f.size for f in b["fields"]]) for b in gc.edge_batches()]
    cases += [(c["name"], c["tmpl"], c["elem"], [x.size for x in c["X"]]) for c in gc.dequantise_cases()]
    seen = set()
    for name, tmpl, elem, n_values in cases:
        L = gribgpu.layout(*tmpl)
        assert L is not None, name
        assert L.coder.flags == gc.coder_flags(tmpl[1]), name
        assert gribgpu.plan(*tmpl, elem, n_values) is not None, name
        seen.add(tmpl[1] & (gc.PP | gc.RESTRICTED | gc.PAD_RSI))
    assert {gc.PP | gc.PAD_RSI, gc.PP | gc.RESTRICTED, gc.RESTRICTED | gc.PAD_RSI} <= seen


def test_plan_refuses():
    t = (16, gc.PP, 32, 128)
    assert gribgpu.plan(*t, 2, [100]) is None and gribgpu.plan(*t, 16, [100]) is None         # an elem that is neither
    assert gribgpu.plan(*t, gc.F32, [100, 0, 5]) is None                                      # a field without a value
    assert gribgpu.plan(*t, gc.F64, [1 << 32]) is None                                        # 2^35 bytes of values
    assert gribgpu.plan(*t, gc.F32, [(1 << 33) - 1]) is not None
    assert gribgpu.plan(*t, gc.F32, [1 << 33]) is None
    big = [(1 << 32)] * 5                                                                     # more than 2^25 wavefronts of 1 KiB of room
    assert gribgpu.plan(*t, gc.F32, big[:4]) is not None and gribgpu.plan(*t, gc.F32, big) is None


def test_plan_of_nothing():
    got = gribgpu.plan(16, gc.PP, 32, 128, gc.F32, [])
    assert got is not None and got["work_bytes"] == 0 and got["rsi_entries"] == 0 and got["work_offsets"].size == 0


def _call_all(t, elem, n, n_values, D):
    """the four calls with null device pointers and no context: what they answer before they touch anything"""
    lib = gribgpu._lib()
    tm = gribgpu.Template(*t)
    nv = np.array(n_values, np.uint64)
    offs = np.zeros(max(1, n), np.uint64)
    Dh = np.array(D, np.int32)
    rec = gribgpu.records(R=0.0, E=0, D=D, n=max(1, n))
    h = lambda a: C.c_void_p(a.ctypes.data)
    return [lib.aec_gpu_grib_pack_async(None, C.byref(tm), elem, None, h(offs), h(nv), h(Dh), 0, None, n, None, None, 0, None, None,
                                        None, None, None),
            lib.aec_gpu_grib_unpack_async(None, C.byref(tm), elem, None, 0, None, None, h(nv), h(rec), h(offs), n, None, 0, None, None,
                                          None, None, None),
            lib.aec_gpu_grib_quantise_async(None, C.byref(tm), elem, None, h(offs), h(nv), h(Dh), 0, None, n, None, None, None),
            lib.aec_gpu_grib_dequantise_async(None, C.byref(tm), elem, None, h(nv), h(rec), h(offs), n, None, None)]


def test_no_fields_is_ok_and_enqueues_nothing():
    assert _call_all((16, gc.PP, 32, 128), gc.F32, 0, [1], [0]) == [0, 0, 0, 0]


def test_calls_refuse_before_they_touch_a_device():
    for what, tmpl, D in REFUSED:
        if not what.startswith("D"):
            assert _call_all(tmpl, gc.F32, 0, [1], [0]) == [-1] * 4, what          # (even an empty batch: the template is checked first)
    assert _call_all((16, gc.PP, 32, 128), 3, 1, [100], [0]) == [-1] * 4
    assert _call_all((16, gc.PP, 32, 128), gc.F32, 1, [100], [0]) == [-1] * 4        # no context, no pointers
