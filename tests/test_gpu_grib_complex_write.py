"""Writing GRIB2 complex packing on the device (include/aec_gpu_grib.h, COMPLEX PACKING, the writer's rule;
libaec_amd/gribgpu.py): complex_write over the case list of tests/grib_complex_write_cases.py against the rule (stated twice
there and pinned to itself, to a fixture derived by hand and to the reader's models by tests/test_grib_complex_write_emul.py);
the writer's output through complex_expand back to the rooms it came from; pack -> ccsds_to_complex -> complex_to_ccsds against
aec_gpu_grib_pack_async in the same process and the reference-made streams of tests/golden/grib_vectors.npz; simple_to_complex
and complex_pack against complex_write; the composition with quantise_bitmap; a damaged CCSDS stream between clean ones; the
refusals.  Every comparison is byte-exact, every buffer a call writes lies between guard bytes and is compared whole."""
import numpy as np
import pytest

import grib_bitmap_cases as bc
import grib_cases as gc
import grib_complex_cases as cc
import grib_complex_write_cases as wc
import grib_simple_cases as sc
from helpers import AEC_DATA_ERROR, oracle_decode
from test_gpu_grib import AEC_CONF_ERROR, AEC_OK, check_records_and_work, given_params, pack, put, whole_is
from test_gpu_grib_complex import clean_given
from test_gpu_sz_device import guarded, guards_intact

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in wc.cases()]
BATCHES = [b["name"] for b in gc.batches()]
REC = wc.CXW_DTYPE.itemsize


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import api, gpu, gribgpu
    return torch, api, gpu, gribgpu


@pytest.fixture(scope="module")
def golden():
    return {b["name"]: b for b in gc.golden_batches()}


def codec_of(mods, tmpl):
    nbits, options, bs, rsi = tmpl
    return mods[3].GribCodec(nbits, bs, rsi, options)


def device_work(torch, c):
    host = wc.work_of(c)
    whole, d_work = guarded(torch, host.size)
    put(torch, d_work, [(0, host)])
    return whole, d_work


def write_case(mods, codec, c, skew, d_work):
    """one complex_write over guarded buffers: (whole, d_complex, offsets, size, the records); streams, records and the
    untouched bytes are checked against the model"""
    torch = mods[0]
    n = len(c["fields"])
    offs, size = wc.placement(c)
    whole, d_complex = guarded(torch, size, skew)
    assert d_complex.data_ptr() % 4 == skew
    cxw_whole, d_cxw = guarded(torch, n * REC)
    rc = codec.complex_write_async(c["order"], c["G"], wc.n_values(c), d_work, d_complex, size, offs, d_cxw)
    torch.cuda.synchronize()
    assert rc == AEC_OK and guards_intact(torch, cxw_whole, n * REC), "written outside d_cxw"
    whole_is(whole, skew, [(int(o), np.frombuffer(s, np.uint8)) for o, (s, d) in zip(offs, wc.model(c))], [], f"d_complex from {skew}")
    got = d_cxw.cpu().numpy().view(wc.CXW_DTYPE)
    for rec, (s, d) in zip(got, wc.model(c)):
        assert rec.tobytes() == wc.record_of(s, d).tobytes(), (c["name"], d, rec)
    return whole, d_complex, offs, size, got


@pytest.mark.parametrize("name", NAMES)
def test_complex_write(mods, name):
    """streams, records and the untouched bytes from S_i to B_i are the model's, from two addresses of d_complex modulo 4; d_work is
    unchanged (the samples that pad its last blocks are poison)"""
    torch = mods[0]
    c = wc.case(name)
    codec = codec_of(mods, c["tmpl"])
    work_whole, d_work = device_work(torch, c)
    before = work_whole.clone()
    for skew in (0, 3):
        write_case(mods, codec, c, skew, d_work)
        assert torch.equal(before, work_whole), "d_work was written"
    codec.close()


@pytest.mark.parametrize("name", NAMES)
def test_write_then_expand_is_identity(mods, name):
    """the device's records and streams go into complex_expand_async with complex_bytes_each = B_i: the rooms come back byte for
    byte, padding included; x_min / x_max are exact and the status is 0"""
    torch, api, gpu, gribgpu = mods
    c = wc.case(name)
    nbits = c["tmpl"][0]
    codec = codec_of(mods, c["tmpl"])
    n = len(c["fields"])
    work_whole, d_work = device_work(torch, c)
    whole, d_complex, offs, size, recs = write_case(mods, codec, c, 1, d_work)
    fields, sizes = gribgpu.complex_fields_of(recs)
    assert [int(s) for s in sizes] == [len(s) for s, d in wc.model(c)]
    back_whole, d_back = guarded(torch, int(wc.work_offsets(c)[-1]))
    cx_whole, d_cx = guarded(torch, n * 24)
    rc = codec.complex_expand_async(fields, wc.n_values(c), d_complex, size, offs, wc.bounds(c), d_back, d_cx)
    torch.cuda.synchronize()
    assert rc == AEC_OK and guards_intact(torch, cx_whole, n * 24)
    whole_is(back_whole, 0, [(int(o), gc.x_bytes(f, nbits, r // gc.container(nbits))) for f, o, r in zip(c["fields"], wc.work_offsets(c), wc.rooms(c))],
             [], "the rooms")
    for rec, f in zip(d_cx.cpu().numpy().view(cc.CX_DTYPE), c["fields"]):
        assert (int(rec["x_min"]), int(rec["x_max"]), int(rec["status"]), int(rec["pad"])) == (int(f.min()), int(f.max()), 0, 0)
    codec.close()


# ---- 5.42 streams to 5.2 / 5.3 streams and back ---------------------------------------------------------------------------------
def write_shape(nbits):
    return min(2, 32 - nbits), 32


def model_of_x(b, xs):
    o, G = write_shape(b["tmpl"][0])
    return [wc.model_numpy(x, b["tmpl"][0], o, G) for x in xs]


def layout(b, n_values, gap=0, first=1):
    o, G = write_shape(b["tmpl"][0])
    B = [wc.bound(v, b["tmpl"][0], o, G) for v in n_values]
    offs = first + np.concatenate([[0], np.cumsum([v + gap for v in B])])
    return B, offs[:-1].astype(np.uint64), int(offs[-1])


def ccsds_to_complex(mods, codec, b, d_in, in_bytes, in_offs, in_sizes, d_table, damaged=()):
    """one call into guarded buffers; every field but the damaged ones is exact and clean, those stay inside their B_i bytes"""
    torch, api, gpu, gribgpu = mods
    n_values = [f.size for f in b["fields"]]
    n = len(n_values)
    o, G = write_shape(b["tmpl"][0])
    plan = codec.complex_write_plan(n_values, o, G)
    B, offs, size = layout(b, n_values)
    model = model_of_x(b, [m[3] for m in b["model"]])
    whole, d_complex = guarded(torch, size, 3)
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    cxw_whole, d_cxw = guarded(torch, n * REC)
    d_results = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
    have = d_table is not None
    if not have:
        d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
    rc = codec.ccsds_to_complex_async(o, G, d_in, in_bytes, in_offs, in_sizes, n_values, d_table, have, d_work, d_results, d_result, d_complex,
                                      size, offs, d_cxw)
    torch.cuda.synchronize()
    assert rc == AEC_OK and guards_intact(torch, work_whole, plan["work_bytes"]) and guards_intact(torch, cxw_whole, n * REC)
    results = d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)
    assert [int(r["status"]) != 0 for r in results] == [i in damaged for i in range(n)]
    whole_is(whole, 3, [(int(o_), np.frombuffer(s, np.uint8)) for i, (o_, (s, d)) in enumerate(zip(offs, model)) if i not in damaged],
             [(int(offs[i]), B[i]) for i in damaged], "d_complex")
    recs = d_cxw.cpu().numpy().view(wc.CXW_DTYPE)
    for i, (rec, (s, d)) in enumerate(zip(recs, model)):
        if i in damaged:
            assert int(rec["bytes"]) <= B[i]
        else:
            assert rec.tobytes() == wc.record_of(s, d).tobytes()
    return d_complex, offs, size, recs


@pytest.mark.parametrize("name", BATCHES + [n + "_golden" for n in BATCHES])
def test_ccsds_to_complex_and_back(mods, golden, name):
    """pack -> ccsds_to_complex (with the pack's table, and bare from its chunk records) -> complex_to_ccsds: d_out, d_chunks,
    the RSI table and d_result are pack_async's, byte for byte; the streams are the reference's where the fixture holds them"""
    torch, api, gpu, gribgpu = mods
    b = clean_given(golden[name[:-len("_golden")]] if name.endswith("_golden") else next(g for g in gc.batches() if g["name"] == name))
    codec = codec_of(mods, b["tmpl"])
    plain = pack(mods, codec, b)
    assert plain["rc"] == AEC_OK
    check_records_and_work(b, plain)
    n_values, plan, cap = plain["n_values"], plain["plan"], plain["cap"]
    n = len(n_values)
    in_offs = [int(base) // 8 for base, bits in plain["rec"]]
    in_sizes = [(int(bits) + 7) // 8 for base, bits in plain["rec"]]
    ccsds_to_complex(mods, codec, b, plain["d_out"], cap, in_offs, in_sizes, None)
    d_complex, offs, size, recs = ccsds_to_complex(mods, codec, b, plain["d_out"], cap, None, None, plain["d_table"].clone())
    fields, sizes = gribgpu.complex_fields_of(recs)
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    out_whole, d_out = guarded(torch, cap)
    cx_whole, d_cx = guarded(torch, n * 24)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
    rc = codec.complex_to_ccsds_async(fields, d_complex, size, offs, sizes, n_values, d_work, d_out, cap, d_rec, d_table, d_res, d_cx)
    torch.cuda.synchronize()
    assert rc == AEC_OK
    assert torch.equal(work_whole, plain["work_whole"]), "d_work (whole buffer, gaps and guards)"
    rec = d_rec.cpu().numpy().view(np.uint64).reshape(n, 2)
    assert np.array_equal(rec, plain["rec"]), "d_chunks"
    assert d_res.cpu().numpy().tobytes() == plain["res"].tobytes(), "d_result"
    assert torch.equal(d_table, plain["d_table"]), "the RSI table"
    assert guards_intact(torch, out_whole, cap) and guards_intact(torch, cx_whole, n * 24)
    nbytes = (int(plain["res"]["total_bits"]) + 7) // 8
    assert torch.equal(d_out[:nbytes], plain["d_out"][:nbytes]), "the streams"
    assert not d_cx.cpu().numpy().view(cc.CX_DTYPE)["status"].any()
    if b.get("streams") is not None:
        out = d_out.cpu().numpy()
        for i, (base, bits) in enumerate(rec):
            if b["model"][i][3].tobytes() == b["X"][i].astype(np.uint32).tobytes():
                assert out[int(base) // 8:int(base) // 8 + (int(bits) + 7) // 8].tobytes() == b["streams"][i], f"stream {i} is not the fixture's"
    codec.close()


def test_a_damaged_ccsds_stream_stays_in_its_range(mods):
    """32 bytes cleared inside a stream in the middle of a batch, chosen on the CPU so that the oracle's decoder says
    AEC_DATA_ERROR for it: its record is not clean, its range of B_i bytes holds whatever was written, its neighbours are exact
    and nothing else is written"""
    torch, api, gpu, gribgpu = mods
    b = clean_given(next(g for g in gc.batches() if g["name"] == "mix12_f4"))
    nbits, options, bs, rsi = b["tmpl"]
    codec = codec_of(mods, b["tmpl"])
    got = pack(mods, codec, b)
    in_offs = [int(base) // 8 for base, bits in got["rec"]]
    in_sizes = [(int(bits) + 7) // 8 for base, bits in got["rec"]]
    k = 5
    assert b["fields"][k].size == 4096 and in_sizes[k] > 128
    host = got["d_out"].cpu().numpy()
    enc = host[in_offs[k]:in_offs[k] + in_sizes[k]].tobytes()
    rng = np.random.default_rng(5)
    for trial in range(400):
        at = int(rng.integers(8, in_sizes[k] - 40))
        bad = bytearray(enc)
        bad[at:at + 32] = bytes(32)
        rc, _, _ = oracle_decode(bytes(bad), nbits, bs, rsi, gc.coder_flags(options, False), gc.room(4096, bs, nbits))
        if rc == AEC_DATA_ERROR:
            break
    else:
        raise AssertionError("no damage found that the oracle's decoder calls a data error")
    host[in_offs[k]:in_offs[k] + in_sizes[k]] = np.frombuffer(bytes(bad), np.uint8)
    d_in = torch.from_numpy(host).cuda()
    ccsds_to_complex(mods, codec, b, d_in, got["cap"], None, None, got["d_table"].clone(), damaged={k})
    codec.close()


# ---- from 5.0 streams and from floats --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_simple_to_complex(mods, name):
    """over the same X, equal to complex_write's output: streams, offsets and records"""
    torch, api, gpu, gribgpu = mods
    c = wc.case(name)
    nbits = c["tmpl"][0]
    codec = codec_of(mods, c["tmpl"])
    streams = [sc.stream_numpy(f, nbits) for f in c["fields"]]
    soffs = 3 + np.concatenate([[0], np.cumsum([s.size for s in streams])])
    d_simple = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8)] + streams)).cuda()
    d_complex, offs, recs = codec.simple_to_complex(d_simple, soffs[:-1], wc.n_values(c), c["order"], c["G"])
    work_whole, d_work = device_work(torch, c)
    d_want, offs_want, recs_want = codec.complex_write(d_work, wc.n_values(c), c["order"], c["G"])
    assert np.array_equal(offs, offs_want) and recs.tobytes() == recs_want.tobytes()
    got, want = d_complex.cpu().numpy(), d_want.cpu().numpy()
    for o, r, (s, d) in zip(offs, recs, wc.model(c)):
        assert int(r["bytes"]) == len(s)
        assert got[int(o):int(o) + len(s)].tobytes() == s == want[int(o):int(o) + len(s)].tobytes()
    codec.close()


@pytest.mark.parametrize("name", ["mix12_f4", "mix16_f8", "shapes_f4", "given_f4", "nonfinite_f4", "nonfinite_f8"])
def test_complex_pack(mods, name):
    """equals quantise + complex_write, and d_work and d_fields are the quantiser's; the neighbours of a BAD field are exact, its
    own range holds whatever was written"""
    torch, api, gpu, gribgpu = mods
    b = next(g for g in gc.batches() if g["name"] == name)
    b = dict(b, model=gc.model_of(b))
    nbits = b["tmpl"][0]
    codec = codec_of(mods, b["tmpl"])
    alone = pack(mods, codec, b, encode=False)
    check_records_and_work(b, alone)
    n_values = alone["n_values"]
    n = len(n_values)
    o, G = write_shape(nbits)
    B, offs, size = layout(b, n_values, gap=2, first=2)
    bad = {i for i, m in enumerate(b["model"]) if m[3] is None}
    assert bool(bad) == name.startswith("nonfinite")
    src_offs, extent = gc.edge_placement(b)
    src_whole, d_src = guarded(torch, extent)
    put(torch, d_src, [(o_, f.view(np.uint8)) for o_, f in zip(src_offs, b["fields"])])
    work_whole, d_work = guarded(torch, alone["plan"]["work_bytes"])
    fields_whole, d_fields = guarded(torch, n * 16)
    whole, d_complex = guarded(torch, size, 2)
    cxw_whole, d_cxw = guarded(torch, n * REC)
    rc = codec.complex_pack_async(o, G, b["elem"], d_src, src_offs, n_values, b["D"], given_params(b), d_work, d_fields, d_complex, size, offs, d_cxw)
    torch.cuda.synchronize()
    assert rc == AEC_OK and guards_intact(torch, cxw_whole, n * REC) and guards_intact(torch, fields_whole, n * 16)
    fields = d_fields.cpu().numpy().view(gc.RECORD_DTYPE)
    clean = [i for i in range(n) if i not in bad]
    assert fields[clean].tobytes() == alone["fields"][clean].tobytes() and all(int(fields[i]["status"]) & gc.BAD for i in bad)
    check_records_and_work(b, dict(alone, fields=fields, work_whole=work_whole))
    model = [None if m[3] is None else wc.model_numpy(m[3], nbits, o, G) for m in b["model"]]
    whole_is(whole, 2, [(int(o_), np.frombuffer(m[0], np.uint8)) for o_, m in zip(offs, model) if m is not None],
             [(int(offs[i]), B[i]) for i in bad], "d_complex")
    recs = d_cxw.cpu().numpy().view(wc.CXW_DTYPE)
    for i, (rec, m) in enumerate(zip(recs, model)):
        assert int(rec["bytes"]) <= B[i] if m is None else rec.tobytes() == wc.record_of(*m).tobytes()
    # ... and the writer alone over the quantiser's rooms gives the same streams
    again_whole, d_again = guarded(torch, size, 2)
    assert codec.complex_write_async(o, G, n_values, alone["d_work"], d_again, size, offs, d_cxw) == AEC_OK
    torch.cuda.synchronize()
    a, g = d_again.cpu().numpy(), d_complex.cpu().numpy()
    for i in clean:
        assert a[int(offs[i]):int(offs[i]) + B[i]].tobytes() == g[int(offs[i]):int(offs[i]) + B[i]].tobytes()
    codec.close()


# ---- with a section 6 bitmap: the two-call composition --------------------------------------------------------------------------------
def test_the_composition_with_quantise_bitmap(mods):
    """quantise_bitmap of whole grids, then complex_write: the streams of the present points' X"""
    torch, api, gpu, gribgpu = mods
    b = next(g for g in bc.batches() if g["name"] == "bm12_bs32_f8")
    model = gc.model_of(b)
    nbits = b["tmpl"][0]
    codec = codec_of(mods, b["tmpl"])
    n_points = [g.size for g in b["grids"]]
    n_values = [f.size for f in b["fields"]]
    n = len(n_values)
    o, G = 2, 16
    host_bm, bm_offs = bc.bitmaps(b)
    d_bm = torch.from_numpy(host_bm).cuda()
    d_grids = torch.from_numpy(np.concatenate(b["grids"])).cuda()
    starts = np.concatenate([[0], np.cumsum(n_points)])[:-1].astype(np.uint64) * np.uint64(b["elem"])
    assert codec.bitmap_plan(n_points, n_values, b["elem"]) is not None
    plan = codec.complex_write_plan(n_values, o, G, b["elem"])
    d_work = torch.zeros(plan["work_bytes"] + 16, dtype=torch.uint8, device="cuda")
    d_fields = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    assert codec.quantise_bitmap_async(b["elem"], d_grids, starts, n_values, b["D"], None, d_work, d_fields, d_bm, bm_offs, n_points) == AEC_OK
    d_complex, offs, recs = codec.complex_write(d_work, n_values, o, G)
    assert not (d_fields.cpu().numpy().view(gc.RECORD_DTYPE)["status"] & (gc.BAD | 8)).any()
    got = d_complex.cpu().numpy()
    for m, o_, rec in zip(model, offs, recs):
        s, d = wc.model_numpy(m[3], nbits, o, G)
        assert rec.tobytes() == wc.record_of(s, d).tobytes() and got[int(o_):int(o_) + len(s)].tobytes() == s
    codec.close()


# ---- what is refused, and a batch of nothing ----------------------------------------------------------------------------------------
def test_no_fields_and_refusals_write_nothing(mods):
    torch, api, gpu, gribgpu = mods
    c = wc.case("rev_n16_g16")
    nbits = c["tmpl"][0]
    codec = codec_of(mods, c["tmpl"])
    n_values, o, G = wc.n_values(c), c["order"], c["G"]
    n = len(n_values)
    plan = codec.complex_write_plan(n_values, o, G)
    offs, size = wc.placement(c)
    B = wc.bounds(c)
    work_whole, d_work = device_work(torch, c)
    whole, d_complex = guarded(torch, size, 1)
    cxw_whole, d_cxw = guarded(torch, n * REC)
    fields_whole, d_fields = guarded(torch, n * 16)
    # sources the composed calls take: floats, 5.42 streams with their table, 5.0 streams
    d_src = torch.zeros(sum(n_values), dtype=torch.float32, device="cuda")
    src_offs = np.concatenate([[0], np.cumsum(n_values)])[:-1] * 4
    d_out, spans, _, d_table = codec.pack(torch.arange(sum(n_values), dtype=torch.float32, device="cuda") % 97, src_offs // 4, n_values, 0,
                                          want_offsets=True)
    d_simple, simple_offs = codec.bits_pack(d_work, n_values)
    d_results = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
    every = (whole, work_whole, cxw_whole, fields_whole, d_table, d_results, d_result)
    before = [t.clone() for t in every]

    def calls(nv=n_values, o=o, G=G, cap=size, co=offs, work=d_work, cxw=d_cxw):
        k = len(nv)
        return [codec.complex_write_async(o, G, nv, work, d_complex, cap, co, cxw),
                codec.complex_pack_async(o, G, gc.F32, d_src, src_offs[:k], nv, [0] * k, None, work, d_fields, d_complex, cap, co, cxw),
                codec.ccsds_to_complex_async(o, G, d_out, d_out.numel(), None, None, nv, d_table, 1, work, d_results, d_result, d_complex, cap, co, cxw),
                codec.simple_to_complex_async(o, G, d_simple, d_simple.numel(), simple_offs[:k], None, nv, work, d_complex, cap, co, cxw)]

    assert calls(nv=[], co=[]) == [AEC_OK] * 4
    assert calls(o=3) == [AEC_CONF_ERROR] * 4 and calls(G=48) == [AEC_CONF_ERROR] * 4 and calls(G=8) == [AEC_CONF_ERROR] * 4
    assert int(offs[0]) == max(int(v) for v in offs)                               # (reversed: the first field lies last)
    assert calls(cap=int(offs[0]) + B[0] - 1) == [AEC_CONF_ERROR] * 4              # ... and its range leaves the buffer by a byte
    over = offs.copy()
    over[2] = offs[3] + np.uint64(B[3] - 1)
    assert calls(co=over) == [AEC_CONF_ERROR] * 4                                  # two ranges overlap by a byte
    assert calls(nv=n_values[:2] + [0] + n_values[3:]) == [AEC_CONF_ERROR] * 4     # a field without a value
    assert calls(work=d_work[8:]) == [AEC_CONF_ERROR] * 4                          # a work buffer off its 16 bytes
    assert calls(cxw=d_cxw[4:]) == [AEC_CONF_ERROR] * 4                            # records off their 8 bytes
    wide = codec_of(mods, (31, gc.PP, 16, 128))
    assert wide.complex_write_async(2, G, n_values, d_work, d_complex, 1 << 20, offs, d_cxw) == AEC_CONF_ERROR      # nbits + order > 32
    wide.close()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, every)), "a refused call, or one without fields, wrote"
    # ... and the same arguments, none of them changed, are taken: the writer alone first, whose output is the model's
    assert codec.complex_write_async(o, G, n_values, d_work, d_complex, size, offs, d_cxw) == AEC_OK
    torch.cuda.synchronize()
    whole_is(whole, 1, [(int(o_), np.frombuffer(s, np.uint8)) for o_, (s, d) in zip(offs, wc.model(c))], [], "d_complex")
    assert torch.equal(before[1], work_whole)
    assert calls() == [AEC_OK] * 4
    torch.cuda.synchronize()
    assert guards_intact(torch, whole, size, 1) and guards_intact(torch, cxw_whole, n * REC) and guards_intact(torch, work_whole, int(wc.work_offsets(c)[-1]))
    codec.close()
