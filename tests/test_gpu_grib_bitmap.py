"""GRIB2 section 6 bitmaps on the device (include/aec_gpu_grib.h, the *_bitmap_* calls; libaec_amd/gribgpu.py) over the case
list of tests/grib_bitmap_cases.py.  The reference of a pack is aec_gpu_grib_pack_async itself, in the same process, on the
fields compacted by NumPy -- everything the two calls leave is compared whole -- and the NumPy model of grib_cases; of an
unpack, grib_cases.dequantise scattered by NumPy with the bits of the missing value elsewhere; of a bitmap, numpy.packbits.
Every buffer a call writes lies between guard bytes and is compared whole.  The indices a mismatching count produces are
checked on the CPU first (tests/test_grib_bitmap_emul.py)."""
import numpy as np
import pytest

import grib_bitmap_cases as bc
import grib_cases as gc
from test_gpu_grib import AEC_OK, check_records_and_work, host_params, pack, put, streams_of, whole_is, work_regions
from test_gpu_sz_device import guarded, guards_intact

pytestmark = pytest.mark.gpu

NAMES = [b["name"] for b in bc.batches()]
WRONG = 16              # the field whose count is wrong in test_a_mismatching_count: 65T + 3 points, half of them present


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import api, gpu, gribgpu
    return torch, api, gpu, gribgpu


def batch(name):
    b = next(b for b in bc.batches() if b["name"] == name)
    return dict(b, model=gc.model_of(b))


def codec_of(mods, b):
    nbits, options, bs, rsi = b["tmpl"]
    return mods[3].GribCodec(nbits, bs, rsi, options)


def device_bitmaps(torch, b):
    """the bitmaps of the batch between guard bytes: (whole, middle, offsets)"""
    host, offs = bc.bitmaps(b)
    whole, d_bm = guarded(torch, host.size)
    put(torch, d_bm, [(0, host)])
    return whole, d_bm, offs


def pack_bitmap(mods, codec, b, n_values=None, out_cap=None, encode=True, grids=None):
    """one pack_bitmap (or quantise_bitmap) call over guarded buffers; returns what it left, shaped as test_gpu_grib.pack's"""
    torch, api, gpu, gribgpu = mods
    grids = b["grids"] if grids is None else grids
    n = len(grids)
    n_points = [g.size for g in grids]
    n_values = [int(m.sum()) for m in b["masks"]] if n_values is None else n_values
    plan = codec.bitmap_plan(n_points, n_values, b["elem"])
    assert plan is not None
    offs, extent = bc.grid_placement(b)
    src_whole, d_src = guarded(torch, extent)
    assert [(d_src.data_ptr() + o) % 16 for o in offs] == [0 if how == "aligned" else b["elem"] for how in b["bases"]]
    put(torch, d_src, [(o, g.view(np.uint8)) for o, g in zip(offs, grids)])
    src_want = src_whole.clone()
    bm_whole, d_bm, bm_offs = device_bitmaps(torch, b)
    bm_want = bm_whole.clone()
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    fields_whole, d_fields = guarded(torch, n * 16)
    got = dict(plan=plan, work_whole=work_whole, d_work=d_work, n_values=n_values)
    if encode:
        cap = plan["out_bound"] if out_cap is None else out_cap
        out_whole, d_out = guarded(torch, cap)
        d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
        d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
        d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
        rc = codec.pack_bitmap_async(b["elem"], d_src, offs, n_values, b["D"], None, d_work, d_out, cap, d_rec, d_table, d_fields, d_res,
                                     d_bm, bm_offs, n_points)
        torch.cuda.synchronize()
        assert guards_intact(torch, out_whole, cap), "written outside d_out"
        got.update(d_out=d_out, d_table=d_table, rec=d_rec.cpu().numpy().view(np.uint64).reshape(n, 2),
                   res=d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0])
    else:
        rc = codec.quantise_bitmap_async(b["elem"], d_src, offs, n_values, b["D"], None, d_work, d_fields, d_bm, bm_offs, n_points)
        torch.cuda.synchronize()
    assert torch.equal(src_whole, src_want), "the source was written"
    assert torch.equal(bm_whole, bm_want), "the bitmap was written"
    assert guards_intact(torch, fields_whole, n * 16), "written outside d_fields"
    got.update(rc=rc, fields=d_fields.cpu().numpy().view(gc.RECORD_DTYPE))
    return got


def same_as_plain(torch, got, plain):
    """everything a pack_bitmap left is what pack_async left for the compacted fields"""
    assert got["rc"] == AEC_OK and plain["rc"] == AEC_OK
    assert got["fields"].tobytes() == plain["fields"].tobytes(), "d_fields"
    assert torch.equal(got["work_whole"], plain["work_whole"]), "d_work (whole buffer, gaps and guards)"
    assert np.array_equal(got["rec"], plain["rec"]), "d_chunks"
    assert got["res"].tobytes() == plain["res"].tobytes(), "d_result"
    assert torch.equal(got["d_table"], plain["d_table"]), "the RSI table"
    nbytes = (int(got["res"]["total_bits"]) + 7) // 8
    assert torch.equal(got["d_out"][:nbytes], plain["d_out"][:nbytes]), "the streams"


@pytest.mark.parametrize("name", NAMES)
def test_pack_bitmap_is_pack_of_the_compacted_fields(mods, name):
    torch = mods[0]
    b = batch(name)
    codec = codec_of(mods, b)
    got = pack_bitmap(mods, codec, b)
    plain = pack(mods, codec, b)                       # b["fields"] are the grids compacted by NumPy
    assert codec.plan(got["n_values"], b["elem"])["work_bytes"] == got["plan"]["work_bytes"]
    same_as_plain(torch, got, plain)
    check_records_and_work(b, got)                     # ... and the NumPy model's
    assert got["res"]["overflow"] == 0 and not (got["fields"]["status"] & (bc.MISMATCH | gc.BAD)).any()
    codec.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("missing", [9999.0, float("nan")], ids=["9999", "nan"])
def test_bitmap_is_packbits(mods, name, missing):
    torch = mods[0]
    b = batch(name)
    codec = codec_of(mods, b)
    grids = bc.build_grids(b, missing)
    offs, extent = bc.grid_placement(b)
    src_whole, d_src = guarded(torch, extent)
    put(torch, d_src, [(o, g.view(np.uint8)) for o, g in zip(offs, grids)])
    src_want = src_whole.clone()
    host, bm_offs = bc.bitmaps(b)
    bm_whole, d_bm = guarded(torch, host.size)
    n = len(grids)
    counts_whole, d_counts8 = guarded(torch, n * 8)
    rc = codec.bitmap_async(b["elem"], d_src, offs, [g.size for g in grids], missing, d_bm, bm_offs, d_counts8)
    torch.cuda.synchronize()
    assert rc == AEC_OK and torch.equal(src_whole, src_want)
    whole_is(bm_whole, 0, [(b["bm0"], host[b["bm0"]:])], [], "d_bitmap")          # (the bytes in front of the first bitmap too)
    assert guards_intact(torch, counts_whole, n * 8)
    assert [int(c) for c in d_counts8.cpu().numpy().view(np.uint64)] == [int(m.sum()) for m in b["masks"]]
    codec.close()


def unpack_bitmap(mods, codec, b, got, have_table, n_values=None, skip=()):
    """one unpack_bitmap call into guarded buffers from what a pack left (with its table, or bare from its chunk records)"""
    torch, api, gpu, gribgpu = mods
    n = len(b["grids"])
    n_points = [g.size for g in b["grids"]]
    n_values = got["n_values"] if n_values is None else n_values
    plan = codec.bitmap_plan(n_points, n_values, b["elem"])
    offs, extent = bc.grid_placement(b)
    dst_whole, d_dst = guarded(torch, extent)
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    bm_whole, d_bm, bm_offs = device_bitmaps(torch, b)
    bm_want = bm_whole.clone()
    status_whole, d_status = guarded(torch, n * 4)
    d_results = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
    if have_table:
        d_table, in_offs, in_sizes = got["d_table"].clone(), None, None
    else:
        d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
        in_offs, in_sizes = [int(r[0]) // 8 for r in got["rec"]], [(int(r[1]) + 7) // 8 for r in got["rec"]]
    rc = codec.unpack_bitmap_async(b["elem"], got["d_out"], got["d_out"].numel(), in_offs, in_sizes, n_values, host_params(b), offs, d_table,
                                   have_table, d_work, d_dst, d_results, d_result, d_bm, bm_offs, n_points, b["missing"], d_status)
    torch.cuda.synchronize()
    assert rc == AEC_OK
    assert guards_intact(torch, work_whole, plan["work_bytes"]) and torch.equal(bm_whole, bm_want)
    assert guards_intact(torch, status_whole, n * 4)
    regions = [(o, bc.expanded(b, i, b["model"], b["missing"]).view(np.uint8)) for i, o in enumerate(offs) if i not in skip]
    whole_is(dst_whole, 0, regions, [(offs[i], b["grids"][i].nbytes) for i in skip], "d_dst")
    results = d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)
    assert not any(int(results[i]["status"]) for i in range(n) if i not in skip)
    return d_status.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", NAMES)
def test_unpack_bitmap(mods, name):
    b = batch(name)
    codec = codec_of(mods, b)
    got = pack_bitmap(mods, codec, b)
    assert got["rc"] == AEC_OK
    for have_table in (1, 0):
        assert not unpack_bitmap(mods, codec, b, got, have_table).any()
    codec.close()


@pytest.mark.parametrize("name", NAMES[:3])
def test_the_halves_alone(mods, name):
    torch = mods[0]
    b = batch(name)
    codec = codec_of(mods, b)
    got = pack_bitmap(mods, codec, b, encode=False)
    check_records_and_work(b, got)
    n_points = [g.size for g in b["grids"]]
    offs, extent = bc.grid_placement(b)
    dst_whole, d_dst = guarded(torch, extent)
    bm_whole, d_bm, bm_offs = device_bitmaps(torch, b)
    status_whole, d_status = guarded(torch, len(n_points) * 4)
    work_before = got["work_whole"].clone()
    rc = codec.dequantise_bitmap_async(b["elem"], got["d_work"], got["n_values"], host_params(b), offs, d_dst, d_bm, bm_offs, n_points,
                                       b["missing"], d_status)
    torch.cuda.synchronize()
    assert rc == AEC_OK and torch.equal(work_before, got["work_whole"])
    whole_is(dst_whole, 0, [(o, bc.expanded(b, i, b["model"], b["missing"]).view(np.uint8)) for i, o in enumerate(offs)], [], "d_dst")
    assert not d_status.cpu().numpy().view(np.uint32).any() and guards_intact(torch, status_whole, len(n_points) * 4)
    codec.close()


def test_a_bitmap_of_ones_is_todays_pack(mods):
    """the same source through pack_async and, under bitmaps that are all ones, through pack_bitmap_async"""
    torch = mods[0]
    b = batch(NAMES[2])
    rng = np.random.default_rng(11)
    fields = [np.ascontiguousarray(gc._smooth(rng, g.size, b["dtype"]).astype(b["dtype"])) for g in b["grids"]]
    ones = dict(b, fields=fields, grids=fields, masks=[np.ones(f.size, bool) for f in fields])
    ones["model"] = gc.model_of(ones)
    codec = codec_of(mods, ones)
    got, plain = pack_bitmap(mods, codec, ones), pack(mods, codec, ones)
    same_as_plain(torch, got, plain)
    check_records_and_work(ones, got)
    codec.close()


def test_the_mask_is_what_saves_a_field_with_nan_and_inf(mods):
    b = batch(NAMES[1])
    codec = codec_of(mods, b)
    got = pack_bitmap(mods, codec, b)
    assert not (got["fields"]["status"] & gc.BAD).any()
    whole = pack(mods, codec, dict(b, fields=b["grids"]))               # the grids as they are, absent points included
    dirty = [bool(not np.isfinite(g).all()) for g in b["grids"]]
    assert any(dirty) and [bool(s & gc.BAD) for s in whole["fields"]["status"]] == dirty
    codec.close()


def test_a_mismatching_count(mods):
    """a host count one more and one less than the ones of field WRONG's bitmap: bit 3 there and only there, guards intact,
    every other field exact (records, X, stream bytes, values).  Every access is held inside by contract (tests/
    test_grib_bitmap_emul.py has run the same indices with bounds checks), so this provokes nothing; it runs once."""
    b = batch(NAMES[0])
    codec = codec_of(mods, b)
    plain = pack(mods, codec, b)
    want_streams = streams_of(plain)
    counts = [int(m.sum()) for m in b["masks"]]
    for delta in (1, -1):
        n_values = list(counts)
        n_values[WRONG] += delta
        got = pack_bitmap(mods, codec, b, n_values=n_values)
        assert got["rc"] == AEC_OK
        assert [int(s) & bc.MISMATCH for s in got["fields"]["status"]] == [bc.MISMATCH if i == WRONG else 0 for i in range(len(counts))]
        for i, (R, E, st, x) in enumerate(b["model"]):
            if i != WRONG:
                assert got["fields"][i].tobytes() == plain["fields"][i].tobytes(), i
        regions, _ = work_regions(dict(b, model=[m if i != WRONG else (m[0], m[1], m[2], None) for i, m in enumerate(b["model"])],
                                       fields=[np.zeros(v, b["dtype"]) for v in n_values]), got["plan"])
        room = gc.room(n_values[WRONG], b["tmpl"][2], b["tmpl"][0])
        whole_is(got["work_whole"], 0, regions, [(int(got["plan"]["work_offsets"][WRONG]), room)], "d_work")
        streams = streams_of(got)
        assert [s for i, s in enumerate(streams) if i != WRONG] == [s for i, s in enumerate(want_streams) if i != WRONG]
        status = unpack_bitmap(mods, codec, b, got, 1, n_values=n_values, skip={WRONG})
        assert [int(s) for s in status] == [bc.MISMATCH if i == WRONG else 0 for i in range(len(counts))]
    codec.close()


def test_out_cap_too_small(mods):
    """overflow as the chunk encoder defines it: set, total_bits as without a cap, nothing written at or beyond the cap"""
    b = batch(NAMES[4])
    codec = codec_of(mods, b)
    full = pack_bitmap(mods, codec, b)
    cap = (int(full["res"]["total_bits"]) + 7) // 8 // 2 // 16 * 16
    got = pack_bitmap(mods, codec, b, out_cap=cap)
    assert got["rc"] == AEC_OK and got["res"]["overflow"] == 1 and int(got["res"]["total_bits"]) == int(full["res"]["total_bits"])
    check_records_and_work(b, got)
    codec.close()


def test_codec_round_trip(mods):
    """the convenience layer: bitmap once per mask, pack_bitmap, unpack_bitmap with and without the table"""
    torch = mods[0]
    b = batch(NAMES[4])
    codec = codec_of(mods, b)
    n_points = [g.size for g in b["grids"]]
    starts = np.concatenate([[0], np.cumsum(n_points)])[:-1]
    d_values = torch.from_numpy(np.concatenate(bc.build_grids(b, 9999.0))).cuda()
    d_bitmap, bm_offs, counts = codec.bitmap(d_values, starts, n_points, 9999.0)
    assert [int(c) for c in counts] == [int(m.sum()) for m in b["masks"]]
    assert d_bitmap.cpu().numpy().tobytes() == np.concatenate([np.packbits(m) for m in b["masks"]]).tobytes()
    d_out, spans, fields, d_table = codec.pack_bitmap(d_values, starts, n_points, d_bitmap, bm_offs, counts, b["D"], want_offsets=True)
    want = np.concatenate([bc.expanded(b, i, b["model"], 9999.0) for i in range(len(n_points))])
    for table in (d_table, None):
        d_back, results, status = codec.unpack_bitmap(d_out, spans, fields, counts, n_points, d_bitmap, bm_offs, 9999.0, table)
        assert not results["status"].any() and not status.any() and d_back.cpu().numpy().tobytes() == want.tobytes()
    codec.close()
