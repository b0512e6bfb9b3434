"""GRIB2 simple packing on the device (include/aec_gpu_grib.h, SIMPLE PACKING; libaec_amd/gribgpu.py): bits_pack and
bits_unpack over the case list of tests/grib_simple_cases.py against the WMO definition (stated twice there and pinned to
itself by tests/test_grib_simple_emul.py); simple_pack and simple_unpack over grib_cases.batches() against the NumPy model
of the quantiser; the transcodes against aec_gpu_grib_pack_async in the same process and the reference-made streams of
tests/golden/grib_vectors.npz; a damaged CCSDS stream between clean ones; the compositions with the bitmap calls; the
refusals.  Every comparison is byte-exact, every buffer a call writes lies between guard bytes and is compared whole."""
import numpy as np
import pytest

import grib_bitmap_cases as bc
import grib_cases as gc
import grib_simple_cases as sc
from helpers import AEC_DATA_ERROR, oracle_decode
from test_gpu_grib import AEC_CONF_ERROR, AEC_OK, check_records_and_work, given_params, host_params, pack, put, whole_is
from test_gpu_sz_device import guarded, guards_intact

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in sc.cases()]
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


def stream_regions(c):
    offs, size = sc.placement(c)
    return [(int(o), s) for o, s in zip(offs, sc.streams(c))], offs, size


def device_work(torch, c, garbage=None):
    host = sc.work_of(c, garbage=garbage)
    whole, d_work = guarded(torch, host.size)
    put(torch, d_work, [(0, host)])
    return whole, d_work


def room_regions(c):
    nbits = c["tmpl"][0]
    return [(int(o), gc.x_bytes(x, nbits, r // gc.container(nbits))) for x, o, r in zip(c["X"], sc.work_offsets(c), sc.rooms(c))]


@pytest.mark.parametrize("name", NAMES)
def test_bits_pack(mods, name):
    """the streams are the model's at every address of the buffer modulo 4, and nothing else is written"""
    torch = mods[0]
    c = sc.case(name)
    codec = codec_of(mods, c["tmpl"])
    regions, offs, size = stream_regions(c)
    work_whole, d_work = device_work(torch, c)
    before = work_whole.clone()
    for skew in range(4):
        whole, d_simple = guarded(torch, size, skew)
        assert d_simple.data_ptr() % 4 == skew
        rc = codec.bits_pack_async(sc.n_values(c), d_work, d_simple, offs)
        torch.cuda.synchronize()
        assert rc == AEC_OK and torch.equal(before, work_whole)
        whole_is(whole, skew, regions, [], f"d_simple at {skew}")
    codec.close()


@pytest.mark.parametrize("name", sc.GARBAGE)
def test_bits_pack_takes_x_modulo_two_to_the_nbits(mods, name):
    torch = mods[0]
    c = sc.case(name)
    codec = codec_of(mods, c["tmpl"])
    regions, offs, size = stream_regions(c)
    work_whole, d_work = device_work(torch, c, garbage=7)
    whole, d_simple = guarded(torch, size, 1)
    rc = codec.bits_pack_async(sc.n_values(c), d_work, d_simple, offs)
    torch.cuda.synchronize()
    assert rc == AEC_OK
    whole_is(whole, 1, regions, [], "d_simple")
    codec.close()


def device_streams(torch, c, skew):
    """the buffer of the case between guard bytes; it ends with its last stream"""
    regions, offs, size = stream_regions(c)
    whole, d_simple = guarded(torch, size, skew)
    put(torch, d_simple, regions)
    return whole, d_simple, offs, size


@pytest.mark.parametrize("name", NAMES)
def test_bits_unpack(mods, name):
    """the rooms are the model's, padding included, from every address of the buffer modulo 4; the bytes between rooms and
    the streams stay"""
    torch = mods[0]
    c = sc.case(name)
    codec = codec_of(mods, c["tmpl"])
    for skew in range(4):
        whole, d_simple, offs, size = device_streams(torch, c, skew)
        before = whole.clone()
        work_whole, d_work = guarded(torch, int(sc.work_offsets(c)[-1]))
        rc = codec.bits_unpack_async(sc.n_values(c), d_simple, size, offs, None, d_work)
        torch.cuda.synchronize()
        assert rc == AEC_OK and torch.equal(before, whole)
        whole_is(work_whole, 0, room_regions(c), [], f"d_work from {skew}")
    codec.close()


@pytest.mark.parametrize("name", NAMES)
def test_bits_unpack_of_bits_pack_is_the_rooms(mods, name):
    torch = mods[0]
    c = sc.case(name)
    codec = codec_of(mods, c["tmpl"])
    work_whole, d_work = device_work(torch, c)
    _, offs, size = stream_regions(c)
    whole, d_simple = guarded(torch, size, 3)
    back_whole, d_back = guarded(torch, d_work.numel())
    assert codec.bits_pack_async(sc.n_values(c), d_work, d_simple, offs) == AEC_OK
    assert codec.bits_unpack_async(sc.n_values(c), d_simple, size, offs, None, d_back) == AEC_OK
    torch.cuda.synchronize()
    whole_is(back_whole, 0, room_regions(c), [], "d_work")
    rooms = torch.zeros(d_work.numel(), dtype=torch.bool, device="cuda")
    for o, r in room_regions(c):
        rooms[o:o + r.size] = True
    assert torch.equal(d_back[rooms], d_work[rooms])
    codec.close()


# ---- floats to 5.0 streams and back ---------------------------------------------------------------------------------------------
def batch(name):
    b = next(b for b in gc.batches() if b["name"] == name)
    return dict(b, model=gc.model_of(b))


def model_streams(b):
    """the 5.0 streams of the model's X (None for a bad field), their sizes, and offsets back to back from byte 1"""
    nbits = b["tmpl"][0]
    streams = [None if m[3] is None else sc.stream_numpy(m[3], nbits) for m in b["model"]]
    sizes = [sc.stream_bytes(f.size, nbits) for f in b["fields"]]
    offs = 1 + np.concatenate([[0], np.cumsum(sizes)])[:-1]
    return streams, sizes, offs.astype(np.uint64), 1 + sum(sizes)


@pytest.mark.parametrize("name", BATCHES)
def test_simple_pack(mods, name):
    """d_fields and d_work are pack_model's, as quantise_async leaves them; the streams are the model's bits of the model's X"""
    torch, api, gpu, gribgpu = mods
    b = batch(name)
    codec = codec_of(mods, b["tmpl"])
    n = len(b["fields"])
    n_values = [f.size for f in b["fields"]]
    plan = codec.simple_plan(n_values, b["elem"])
    src_offs, extent = gc.placement(b)
    src_whole, d_src = guarded(torch, extent)
    put(torch, d_src, [(o, f.view(np.uint8)) for o, f in zip(src_offs, b["fields"])])
    src_want = src_whole.clone()
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    fields_whole, d_fields = guarded(torch, n * 16)
    streams, sizes, offs, size = model_streams(b)
    assert plan["simple_bytes"] == sum(sizes)
    whole, d_simple = guarded(torch, size + 2, 2)
    rc = codec.simple_pack_async(b["elem"], d_src, src_offs, n_values, b["D"], given_params(b), d_work, d_fields, d_simple, offs)
    torch.cuda.synchronize()
    assert torch.equal(src_whole, src_want) and guards_intact(torch, fields_whole, n * 16)
    check_records_and_work(b, dict(rc=rc, fields=d_fields.cpu().numpy().view(gc.RECORD_DTYPE), plan=plan, work_whole=work_whole))
    whole_is(whole, 2, [(int(o), s) for o, s in zip(offs, streams) if s is not None],
             [(int(o), ln) for o, s, ln in zip(offs, streams, sizes) if s is None], "d_simple")
    codec.close()


@pytest.mark.parametrize("name", BATCHES)
def test_simple_unpack(mods, name):
    """the floats are grib_cases.dequantise of the model's X, bit for bit, as float32 and as float64"""
    torch, api, gpu, gribgpu = mods
    b = batch(name)
    codec = codec_of(mods, b["tmpl"])
    clean = [i for i, m in enumerate(b["model"]) if m[3] is not None]
    sub = dict(b, fields=[b["fields"][i] for i in clean], model=[b["model"][i] for i in clean], D=[b["D"][i] for i in clean])
    streams, sizes, offs, size = model_streams(sub)
    n_values = [f.size for f in sub["fields"]]
    whole, d_simple = guarded(torch, size, 1)
    put(torch, d_simple, [(int(o), s) for o, s in zip(offs, streams)])
    before = whole.clone()
    for dtype in (np.float32, np.float64):
        elem = np.dtype(dtype).itemsize
        plan = codec.simple_plan(n_values, elem)
        dst_offs, extent = gc.placement(dict(sub, elem=elem), 5)
        dst_whole, d_dst = guarded(torch, extent)
        work_whole, d_work = guarded(torch, plan["work_bytes"])
        rc = codec.simple_unpack_async(elem, d_simple, size, offs, sizes, n_values, host_params(sub), dst_offs, d_work, d_dst)
        torch.cuda.synchronize()
        assert rc == AEC_OK and torch.equal(before, whole) and guards_intact(torch, work_whole, plan["work_bytes"])
        whole_is(dst_whole, 0, [(o, gc.dequantise(x, R, E, D, dtype).view(np.uint8))
                                for o, (R, E, st, x), D in zip(dst_offs, sub["model"], sub["D"])], [], f"d_dst as {np.dtype(dtype)}")
    codec.close()


# ---- 5.0 streams to 5.42 streams and back ---------------------------------------------------------------------------------------
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


def transcode_source(golden, name):
    if name.endswith("_golden"):
        return clean_given(golden[name[:-len("_golden")]])
    return clean_given(next(b for b in gc.batches() if b["name"] == name))


@pytest.mark.parametrize("name", BATCHES + [n + "_golden" for n in BATCHES])
def test_simple_to_ccsds_is_pack(mods, golden, name):
    """d_out, d_chunks, the RSI table, d_result and d_work are pack_async's for the same batch; the streams are the
    reference's where the fixture holds them"""
    torch, api, gpu, gribgpu = mods
    b = transcode_source(golden, name)
    codec = codec_of(mods, b["tmpl"])
    plain = pack(mods, codec, b)
    assert plain["rc"] == AEC_OK
    check_records_and_work(b, plain)
    n_values = plain["n_values"]
    n, plan, cap = len(n_values), plain["plan"], plain["cap"]
    streams, sizes, offs, size = model_streams(b)
    whole, d_simple = guarded(torch, size, 1)
    put(torch, d_simple, [(int(o), s) for o, s in zip(offs, streams)])
    before = whole.clone()
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    out_whole, d_out = guarded(torch, cap)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
    rc = codec.simple_to_ccsds_async(d_simple, size, offs, sizes, n_values, d_work, d_out, cap, d_rec, d_table, d_res)
    torch.cuda.synchronize()
    assert rc == AEC_OK and torch.equal(before, whole)
    assert torch.equal(work_whole, plain["work_whole"]), "d_work (whole buffer, gaps and guards)"
    rec = d_rec.cpu().numpy().view(np.uint64).reshape(n, 2)
    assert np.array_equal(rec, plain["rec"]), "d_chunks"
    assert d_res.cpu().numpy().tobytes() == plain["res"].tobytes(), "d_result"
    assert torch.equal(d_table, plain["d_table"]), "the RSI table"
    assert guards_intact(torch, out_whole, cap)
    nbytes = (int(plain["res"]["total_bits"]) + 7) // 8
    assert torch.equal(d_out[:nbytes], plain["d_out"][:nbytes]), "the streams"
    if b.get("streams") is not None:
        out = d_out.cpu().numpy()
        for i, (base, bits) in enumerate(rec):
            if b["model"][i][3].tobytes() == b["X"][i].astype(np.uint32).tobytes():
                assert out[int(base) // 8:int(base) // 8 + (int(bits) + 7) // 8].tobytes() == b["streams"][i], f"stream {i} is not the fixture's"
    codec.close()


def ccsds_to_simple(mods, codec, b, d_in, in_bytes, in_offs, in_sizes, d_table, damaged=()):
    """one call into guarded buffers; every field but the damaged ones is exact and clean, those have their S_i bytes"""
    torch, api, gpu, gribgpu = mods
    n_values = [f.size for f in b["fields"]]
    n = len(n_values)
    plan = codec.simple_plan(n_values)
    streams, sizes, offs, size = model_streams(b)
    whole, d_simple = guarded(torch, size, 3)
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    d_results = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
    have = d_table is not None
    if not have:
        d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
    rc = codec.ccsds_to_simple_async(d_in, in_bytes, in_offs, in_sizes, n_values, d_table, have, d_work, d_results, d_result, d_simple, offs)
    torch.cuda.synchronize()
    assert rc == AEC_OK and guards_intact(torch, work_whole, plan["work_bytes"])
    results = d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)
    assert [int(r["status"]) != 0 for r in results] == [i in damaged for i in range(n)]
    whole_is(whole, 3, [(int(o), s) for i, (o, s) in enumerate(zip(offs, streams)) if i not in damaged],
             [(int(offs[i]), sizes[i]) for i in damaged], "d_simple")


@pytest.mark.parametrize("name", BATCHES)
def test_ccsds_to_simple(mods, name):
    """the 5.0 streams of the model's X from what a pack left: with its table, and bare from its chunk records"""
    torch, api, gpu, gribgpu = mods
    b = clean_given(next(g for g in gc.batches() if g["name"] == name))
    codec = codec_of(mods, b["tmpl"])
    got = pack(mods, codec, b)
    assert got["rc"] == AEC_OK
    ccsds_to_simple(mods, codec, b, got["d_out"], got["cap"], None, None, got["d_table"].clone())
    in_offs = [int(base) // 8 for base, bits in got["rec"]]
    in_sizes = [(int(bits) + 7) // 8 for base, bits in got["rec"]]
    ccsds_to_simple(mods, codec, b, got["d_out"], got["cap"], in_offs, in_sizes, None)
    codec.close()


def test_a_damaged_ccsds_stream_stays_in_its_bytes(mods):
    """32 bytes cleared inside a stream in the middle of a batch, chosen on the CPU so that the oracle's decoder says
    AEC_DATA_ERROR for it: its record is not clean, its S_i bytes hold anything, its neighbours are exact and nothing else is
    written"""
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
    ccsds_to_simple(mods, codec, b, d_in, got["cap"], None, None, got["d_table"].clone(), damaged={k})
    codec.close()


# ---- with section 6 bitmaps: the two-call compositions ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bm8_bs8_f4", "bm12_bs32_f8"])
def test_the_bitmap_compositions(mods, name):
    """simple_pack_bitmap of the grids is simple_pack of the compacted fields; simple_unpack_bitmap of those streams is the
    model's values scattered, the missing value elsewhere"""
    torch, api, gpu, gribgpu = mods
    b = next(g for g in bc.batches() if g["name"] == name)
    model = gc.model_of(b)
    codec = codec_of(mods, b["tmpl"])
    n_points = [g.size for g in b["grids"]]
    n_values = [f.size for f in b["fields"]]
    d_grids = torch.from_numpy(np.concatenate(b["grids"])).cuda()
    d_fields = torch.from_numpy(np.concatenate(b["fields"])).cuda()
    starts = lambda sizes: np.concatenate([[0], np.cumsum(sizes)])[:-1]
    host_bm, bm_offs = bc.bitmaps(b)
    d_bm = torch.from_numpy(host_bm).cuda()
    d_simple, offs, fields = codec.simple_pack_bitmap(d_grids, starts(n_points), n_points, d_bm, bm_offs, n_values, b["D"])
    d_plain, offs_plain, fields_plain = codec.simple_pack(d_fields, starts(n_values), n_values, b["D"])
    assert np.array_equal(offs, offs_plain) and fields.tobytes() == fields_plain.tobytes() and torch.equal(d_simple, d_plain)
    want = np.concatenate([sc.stream_numpy(m[3], b["tmpl"][0]) for m in model])
    assert np.array_equal(d_simple.cpu().numpy(), want)
    torch_dtype = torch.float32 if b["elem"] == 4 else torch.float64
    d_back, status = codec.simple_unpack_bitmap(d_simple, offs, fields, n_values, n_points, d_bm, bm_offs, b["missing"], dtype=torch_dtype)
    assert not status.any()
    grids = np.concatenate([bc.expanded(b, i, model, b["missing"]) for i in range(len(n_points))])
    assert d_back.cpu().numpy().tobytes() == grids.tobytes()
    d_flat = codec.simple_unpack(d_simple, offs, fields, n_values, dtype=torch_dtype)
    assert d_flat.cpu().numpy().tobytes() == np.concatenate([gc.dequantise(x, R, E, D, b["dtype"])
                                                             for (R, E, st, x), D in zip(model, b["D"])]).tobytes()
    codec.close()


# ---- what is refused, and a batch of nothing ----------------------------------------------------------------------------------------
def test_no_fields_and_refusals_write_nothing(mods):
    torch, api, gpu, gribgpu = mods
    c = sc.case("n12_rev")
    codec = codec_of(mods, c["tmpl"])
    n_values = sc.n_values(c)
    n = len(n_values)
    nbits = c["tmpl"][0]
    plan = codec.simple_plan(n_values)
    whole, d_simple, offs, size = device_streams(torch, c, 1)
    sizes = [sc.stream_bytes(v, nbits) for v in n_values]
    work_whole, d_work = device_work(torch, c)
    out_whole, d_out = guarded(torch, plan["out_bound"])
    dst_whole, d_dst = guarded(torch, sum(n_values) * 4)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    d_results = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
    d_table = torch.zeros(plan["rsi_entries"], dtype=torch.int64, device="cuda")
    d_fields = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    every = (whole, work_whole, out_whole, dst_whole, d_rec, d_res, d_results, d_result, d_table, d_fields)
    before = [t.clone() for t in every]
    params = gribgpu.records(R=0.0, E=0, D=0, n=n)
    dst_offs = np.concatenate([[0], np.cumsum(n_values)])[:-1] * 4
    cap = plan["out_bound"]

    def reads(nv=n_values, sb=size, so=offs, each=None):
        return [codec.bits_unpack_async(nv, d_simple, sb, so, each, d_work),
                codec.simple_unpack_async(gc.F32, d_simple, sb, so, each, nv, params[:len(nv)], dst_offs[:len(nv)], d_work, d_dst),
                codec.simple_to_ccsds_async(d_simple, sb, so, each, nv, d_work, d_out, cap, d_rec, d_table, d_res)]

    def writes(nv=n_values, so=offs, work=d_work):
        return [codec.bits_pack_async(nv, work, d_simple, so),
                codec.simple_pack_async(gc.F32, d_dst, dst_offs[:len(nv)], nv, [0] * len(nv), None, work, d_fields, d_simple, so),
                codec.ccsds_to_simple_async(d_out, cap, None, None, nv, d_table, 1, work, d_results, d_result, d_simple, so)]

    assert reads(nv=[], so=[]) == [AEC_OK] * 3 and writes(nv=[], so=[]) == [AEC_OK] * 3
    short = list(sizes)
    short[3] -= 1
    assert reads(each=short) == [AEC_CONF_ERROR] * 3                               # section 7 of one message is a byte too short
    assert int(offs[0]) == max(int(o) for o in offs)                               # (reversed: the first field lies last)
    assert reads(sb=int(offs[0]) + sizes[0] - 1) == [AEC_CONF_ERROR] * 3           # ... and its stream leaves the buffer by a byte
    none = n_values[:2] + [0] + n_values[3:]
    assert reads(nv=none) == [AEC_CONF_ERROR] * 3 and writes(nv=none) == [AEC_CONF_ERROR] * 3
    assert writes(work=d_work[8:]) == [AEC_CONF_ERROR] * 3                         # a work buffer off its 16 bytes
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, every)), "a refused call, or one without fields, wrote"
    # ... and exactly S_i bytes per message are taken
    assert codec.bits_unpack_async(n_values, d_simple, size, offs, sizes, d_work) == AEC_OK
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, every)), "the rooms of the streams are not the rooms they came from"
    codec.close()
