"""GRIB2 complex packing on the device (include/aec_gpu_grib.h, COMPLEX PACKING; libaec_amd/gribgpu.py): complex_expand over the
case list of tests/grib_complex_cases.py against the definition (stated twice there and pinned to itself and to a fixture
derived by hand by tests/test_grib_complex_emul.py); complex_unpack against the NumPy model of the dequantiser over the same
X; complex_to_ccsds against aec_gpu_grib_pack_async in the same process and the reference-made streams of
tests/golden/grib_vectors.npz; complex_to_simple against stream_numpy; the composition with dequantise_bitmap; damaged streams
between clean ones; the refusals.  Every comparison is byte-exact, every buffer a call writes lies between guard bytes and is
compared whole."""
import numpy as np
import pytest

import grib_bitmap_cases as bc
import grib_cases as gc
import grib_complex_cases as cc
import grib_simple_cases as sc
from test_gpu_grib import AEC_CONF_ERROR, AEC_OK, check_records_and_work, pack, put, whole_is
from test_gpu_sz_device import guarded, guards_intact

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in cc.cases()]
BATCHES = [b["name"] for b in gc.batches()]


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


def device_streams(torch, c, skew):
    """the buffer of the case between guard bytes; it ends with its last stream"""
    buf, offs, each = cc.buffer_of(c)
    whole, d_complex = guarded(torch, buf.size, skew)
    put(torch, d_complex, [(0, buf)])
    return whole, d_complex, offs, each, buf.size


def check_records(torch, c, cx_whole, d_cx):
    n = len(c["fields"])
    assert guards_intact(torch, cx_whole, n * 24), "written outside d_cx"
    got = d_cx.cpu().numpy().view(cc.CX_DTYPE)
    for f, want, rec in zip(c["fields"], cc.records(c), got):
        if f["damaged"]:
            assert int(rec["status"]) & cc.MALFORMED, f["damaged"]
        else:
            assert (int(rec["x_min"]), int(rec["x_max"]), int(rec["status"])) == want and int(rec["pad"]) == 0


@pytest.mark.parametrize("name", NAMES)
def test_complex_expand(mods, name):
    """rooms and records are the model's, padding included, from two addresses of the buffer modulo 4; a damaged field is
    MALFORMED, its room holds anything, its neighbours are exact; nothing else is written and the streams stay"""
    torch = mods[0]
    c = cc.case(name)
    codec = codec_of(mods, c["tmpl"])
    n = len(c["fields"])
    exact, loose = cc.room_regions(c)
    for skew in (0, 3):
        whole, d_complex, offs, each, size = device_streams(torch, c, skew)
        before = whole.clone()
        work_whole, d_work = guarded(torch, int(cc.work_offsets(c)[-1]))
        cx_whole, d_cx = guarded(torch, n * 24)
        rc = codec.complex_expand_async(cc.descs(c), cc.n_values(c), d_complex, size, offs, each, d_work, d_cx)
        torch.cuda.synchronize()
        assert rc == AEC_OK and torch.equal(before, whole)
        whole_is(work_whole, 0, exact, loose, f"d_work from {skew}")
        check_records(torch, c, cx_whole, d_cx)
    codec.close()


def params_of(c):
    n = len(c["fields"])
    return [(np.float32(1.5 + i), (-3, 0, 2)[i % 3], (0, 3, -2)[i % 3]) for i in range(n)]


@pytest.mark.parametrize("name", NAMES)
def test_complex_unpack(mods, name):
    """the floats are grib_cases.dequantise of the stored X, bit for bit, as float32 and as float64"""
    torch, api, gpu, gribgpu = mods
    c = cc.case(name)
    nbits = c["tmpl"][0]
    codec = codec_of(mods, c["tmpl"])
    n_values = cc.n_values(c)
    n = len(n_values)
    par = params_of(c)
    rec = gribgpu.records(R=[p[0] for p in par], E=[p[1] for p in par], D=[p[2] for p in par])
    whole, d_complex, offs, each, size = device_streams(torch, c, 1)
    before = whole.clone()
    for dtype in (np.float32, np.float64):
        elem = np.dtype(dtype).itemsize
        plan = codec.complex_plan(n_values, cc.descs(c), elem)
        dst_offs, extent = gc.placement(dict(fields=[np.zeros(v, dtype) for v in n_values], elem=elem), 5)
        dst_whole, d_dst = guarded(torch, extent)
        work_whole, d_work = guarded(torch, plan["work_bytes"])
        cx_whole, d_cx = guarded(torch, n * 24)
        rc = codec.complex_unpack_async(elem, cc.descs(c), d_complex, size, offs, each, n_values, rec, dst_offs, d_work, d_dst, d_cx)
        torch.cuda.synchronize()
        assert rc == AEC_OK and torch.equal(before, whole) and guards_intact(torch, work_whole, plan["work_bytes"])
        check_records(torch, c, cx_whole, d_cx)
        whole_is(dst_whole, 0, [(o, gc.dequantise(cc.stored_x(f, nbits), R, E, D, dtype).view(np.uint8))
                                for o, f, (R, E, D) in zip(dst_offs, c["fields"], par) if not f["damaged"]],
                 [(o, f["n"] * elem) for o, f in zip(dst_offs, c["fields"]) if f["damaged"]], f"d_dst as {np.dtype(dtype)}")
    codec.close()


# ---- 5.2 / 5.3 streams to 5.42 streams --------------------------------------------------------------------------------------------
def clean_given(b):
    """the clean fields of a batch under have_params with the model's R and E: what a transcode and a pack both see"""
    model = gc.model_of(b)
    clean = [i for i, m in enumerate(model) if m[3] is not None]
    sub = dict(b, fields=[b["fields"][i] for i in clean], D=[b["D"][i] for i in clean], given=[(float(model[i][0]), model[i][1]) for i in clean])
    for key in ("X", "streams"):
        if b.get(key) is not None:
            sub[key] = [b[key][i] for i in clean]
    sub["model"] = gc.model_of(sub)
    assert all(m[3] is not None for m in sub["model"])
    return sub


def complex_of(xs, seed):
    """the X of a batch written as complex streams by the test writer: orders 0, 1 and 2 in turn, groups of 1 to 40 values;
    (descriptors, buffer, offsets, sizes)"""
    rng = np.random.default_rng(seed)
    descs, streams = [], []
    for i, x in enumerate(xs):
        s, d = cc.write([int(v) for v in x], cc.grouping(rng, x.size), order=i % 3, extra=5, seed=seed + i)
        assert [int(v) for v in cc.decode_numpy(s, d, x.size)] == [int(v) for v in x]
        descs.append(d)
        streams.append(np.frombuffer(s, np.uint8))
    sizes = [s.size for s in streams]
    offs = 1 + np.concatenate([[0], np.cumsum(sizes)])[:-1]
    buf = np.full(1 + sum(sizes), cc.FILL, np.uint8)
    for o, s in zip(offs, streams):
        buf[int(o):int(o) + s.size] = s
    return descs, buf, offs.astype(np.uint64), sizes


@pytest.mark.parametrize("name", BATCHES + [n + "_golden" for n in BATCHES])
def test_complex_to_ccsds_is_pack(mods, golden, name):
    """d_out, d_chunks, the RSI table, d_result and d_work are pack_async's for the same batch; the streams are the
    reference's where the fixture holds them"""
    torch, api, gpu, gribgpu = mods
    b = clean_given(golden[name[:-len("_golden")]] if name.endswith("_golden") else next(g for g in gc.batches() if g["name"] == name))
    codec = codec_of(mods, b["tmpl"])
    plain = pack(mods, codec, b)
    assert plain["rc"] == AEC_OK
    check_records_and_work(b, plain)
    n_values = plain["n_values"]
    n, plan, cap = len(n_values), plain["plan"], plain["cap"]
    descs, buf, offs, sizes = complex_of([m[3] for m in b["model"]], len(name))
    whole, d_complex = guarded(torch, buf.size, 1)
    put(torch, d_complex, [(0, buf)])
    before = whole.clone()
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    out_whole, d_out = guarded(torch, cap)
    cx_whole, d_cx = guarded(torch, n * 24)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
    rc = codec.complex_to_ccsds_async(descs, d_complex, buf.size, offs, sizes, n_values, d_work, d_out, cap, d_rec, d_table, d_res, d_cx)
    torch.cuda.synchronize()
    assert rc == AEC_OK and torch.equal(before, whole)
    assert torch.equal(work_whole, plain["work_whole"]), "d_work (whole buffer, gaps and guards)"
    rec = d_rec.cpu().numpy().view(np.uint64).reshape(n, 2)
    assert np.array_equal(rec, plain["rec"]), "d_chunks"
    assert d_res.cpu().numpy().tobytes() == plain["res"].tobytes(), "d_result"
    assert torch.equal(d_table, plain["d_table"]), "the RSI table"
    assert guards_intact(torch, out_whole, cap) and guards_intact(torch, cx_whole, n * 24)
    nbytes = (int(plain["res"]["total_bits"]) + 7) // 8
    assert torch.equal(d_out[:nbytes], plain["d_out"][:nbytes]), "the streams"
    cx = d_cx.cpu().numpy().view(cc.CX_DTYPE)
    for r, m in zip(cx, b["model"]):
        assert (int(r["x_min"]), int(r["x_max"]), int(r["status"])) == (int(m[3].min()), int(m[3].max()), 0)
    if b.get("streams") is not None:
        out = d_out.cpu().numpy()
        for i, (base, bits) in enumerate(rec):
            if b["model"][i][3].tobytes() == b["X"][i].astype(np.uint32).tobytes():
                assert out[int(base) // 8:int(base) // 8 + (int(bits) + 7) // 8].tobytes() == b["streams"][i], f"stream {i} is not the fixture's"
    codec.close()


@pytest.mark.parametrize("name", NAMES)
def test_complex_to_simple(mods, name):
    """the 5.0 streams of the stored X, back to back"""
    torch = mods[0]
    c = cc.case(name)
    nbits = c["tmpl"][0]
    codec = codec_of(mods, c["tmpl"])
    buf, offs, each = cc.buffer_of(c)
    d_simple, simple_offs, cx = codec.complex_to_simple(torch.from_numpy(buf).cuda(), offs, each, cc.descs(c), cc.n_values(c))
    got = d_simple.cpu().numpy()
    at = 0
    for f, o, r in zip(c["fields"], simple_offs, cx):
        assert int(o) == at
        size = sc.stream_bytes(f["n"], nbits)
        if f["damaged"]:
            assert int(r["status"]) & cc.MALFORMED
        else:
            assert np.array_equal(got[at:at + size], sc.stream_numpy(cc.stored_x(f, nbits), nbits)), (name, f["n"])
        at += size
    assert got.size == at
    codec.close()


# ---- with a section 6 bitmap: the two-call composition --------------------------------------------------------------------------------
def test_the_composition_with_dequantise_bitmap(mods):
    """complex_expand of the present points' X, then dequantise_bitmap: the model's values scattered, the missing value elsewhere"""
    torch, api, gpu, gribgpu = mods
    b = next(g for g in bc.batches() if g["name"] == "bm12_bs32_f8")
    model = gc.model_of(b)
    codec = codec_of(mods, b["tmpl"])
    n_points = [g.size for g in b["grids"]]
    n_values = [f.size for f in b["fields"]]
    n = len(n_values)
    descs, buf, offs, sizes = complex_of([m[3] for m in model], 6)
    host_bm, bm_offs = bc.bitmaps(b)
    d_bm = torch.from_numpy(host_bm).cuda()
    d_work, plan, cx = codec.complex_expand(torch.from_numpy(buf).cuda(), offs, sizes, descs, n_values)
    assert not cx["status"].any()
    assert codec.bitmap_plan(n_points, n_values, b["elem"]) is not None
    elem = b["elem"]
    dst_offs = np.concatenate([[0], np.cumsum(n_points)])[:-1].astype(np.uint64) * np.uint64(elem)
    dst_whole, d_dst = guarded(torch, sum(n_points) * elem)
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    params = gribgpu.records(R=[m[0] for m in model], E=[m[1] for m in model], D=b["D"])
    rc = codec.dequantise_bitmap_async(elem, d_work, n_values, params, dst_offs, d_dst, d_bm, bm_offs, n_points, b["missing"], d_status)
    torch.cuda.synchronize()
    assert rc == AEC_OK and not d_status.cpu().numpy().any()
    grids = np.concatenate([bc.expanded(b, i, model, b["missing"]) for i in range(n)])
    whole_is(dst_whole, 0, [(0, grids.view(np.uint8))], [], "d_dst")
    codec.close()


# ---- what is refused, and a batch of nothing ----------------------------------------------------------------------------------------
def test_no_fields_and_refusals_write_nothing(mods):
    torch, api, gpu, gribgpu = mods
    c = cc.case("rev_n16")
    codec = codec_of(mods, c["tmpl"])
    n_values, descs = cc.n_values(c), cc.descs(c)
    n = len(n_values)
    plan = codec.complex_plan(n_values, descs)
    whole, d_complex, offs, each, size = device_streams(torch, c, 1)
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    out_whole, d_out = guarded(torch, plan["out_bound"])
    dst_whole, d_dst = guarded(torch, sum(n_values) * 4)
    cx_whole, d_cx = guarded(torch, n * 24)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    d_table = torch.zeros(plan["rsi_entries"], dtype=torch.int64, device="cuda")
    every = (whole, work_whole, out_whole, dst_whole, cx_whole, d_rec, d_res, d_table)
    before = [t.clone() for t in every]
    params = gribgpu.records(R=0.0, E=0, D=0, n=n)
    dst_offs = np.concatenate([[0], np.cumsum(n_values)])[:-1] * 4
    cap = plan["out_bound"]

    def calls(nv=n_values, ds=descs, cb=size, co=offs, ce=each, work=d_work):
        k = len(nv)
        return [codec.complex_expand_async(ds, nv, d_complex, cb, co, ce, work, d_cx),
                codec.complex_unpack_async(gc.F32, ds, d_complex, cb, co, ce, nv, params[:k], dst_offs[:k], work, d_dst, d_cx),
                codec.complex_to_ccsds_async(ds, d_complex, cb, co, ce, nv, work, d_out, cap, d_rec, d_table, d_res, d_cx)]

    def one(**kw):
        return descs[:2] + [dict(descs[2], **kw)] + descs[3:]

    assert calls(nv=[], ds=[], co=[], ce=[]) == [AEC_OK] * 3
    for kw in (dict(missing=1), dict(order=3), dict(extra_octets=9), dict(ref_bits=33), dict(width_bits=33), dict(length_bits=33),
               dict(n_groups=0), dict(n_groups=n_values[2] + 1)):
        assert calls(ds=one(**kw)) == [AEC_CONF_ERROR] * 3, kw
    short = [int(e) for e in each]
    short[3] = cc.head_bytes(descs[3]) - 1
    assert calls(ce=short) == [AEC_CONF_ERROR] * 3                                 # shorter than the tables and the extra descriptors
    assert int(offs[0]) == max(int(o) for o in offs)                               # (reversed: the first field lies last)
    assert calls(cb=int(offs[0]) + int(each[0]) - 1) == [AEC_CONF_ERROR] * 3       # ... and its stream leaves the buffer by a byte
    assert calls(nv=n_values[:2] + [0] + n_values[3:]) == [AEC_CONF_ERROR] * 3     # a field without a value
    assert calls(work=d_work[8:]) == [AEC_CONF_ERROR] * 3                          # a work buffer off its 16 bytes
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, every)), "a refused call, or one without fields, wrote"
    # ... and the same arguments, none of them changed, are taken
    assert calls() == [AEC_OK] * 3
    torch.cuda.synchronize()
    exact, loose = cc.room_regions(c)
    whole_is(work_whole, 0, exact, loose, "d_work")
    codec.close()
