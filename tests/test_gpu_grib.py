"""GRIB2 CCSDS packing on the device (include/aec_gpu_grib.h; libaec_amd/gribgpu.py) over the case list of
tests/grib_cases.py: the records, the X in the work buffer, the streams, the chunk records and the RSI table of a pack;
what an unpack writes with the pack's table and from foreign streams; the two halves alone; the refusals; an output that
is too small; a NaN and an Inf in a batch.  References: the NumPy model bit for bit, the streams the reference made of the
model's X (tests/golden/grib_vectors.npz), the library's own aec_buffer_encode, and the reference itself when oracle/_ref
travelled.  Every buffer a call writes lies between guard bytes and is compared whole.

The same checks run over grib_cases.edge_batches() (R, E, D and X at their thresholds, the positions of the extremes in
k_grib_minmax on either alignment, the coder flags) and dequantise_cases() (Y under parameters no pack produced); there
the streams are aec_buffer_encode's of the model's X, and the model is pinned to exact rationals by tests/test_grib_emul.py."""
import numpy as np
import pytest

import grib_cases as gc
from helpers import have_ref, ref_encode
from test_gpu_sz_device import GUARD, guarded, guards_intact

pytestmark = pytest.mark.gpu

AEC_OK, AEC_CONF_ERROR = 0, -1
BATCHES = [b["name"] for b in gc.batches()]
EDGES = [b["name"] for b in gc.edge_batches()]
DEQS = [c["name"] for c in gc.dequantise_cases()]


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import api, gpu, gribgpu
    return torch, api, gpu, gribgpu


@pytest.fixture(scope="module")
def golden():
    return {b["name"]: dict(b, model=gc.model_of(b)) for b in gc.golden_batches()}


def whole_is(whole, skew, regions, unspecified, what):
    """the guarded tensor holds `regions` [(offset in its middle, bytes)] and its pattern everywhere else; `unspecified`
    [(offset, length)] may hold anything"""
    want = (np.arange(whole.numel()) % 251).astype(np.uint8)
    got = whole.cpu().numpy()
    for o, b in regions:
        want[GUARD + skew + o:GUARD + skew + o + b.size] = b
    for o, ln in unspecified:
        want[GUARD + skew + o:GUARD + skew + o + ln] = got[GUARD + skew + o:GUARD + skew + o + ln]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {int(bad[0]) - GUARD - skew} of the middle"


def put(torch, d_mid, pieces):
    """host bytes into the middle of a guarded tensor"""
    host = d_mid.cpu().numpy()
    for o, b in pieces:
        host[o:o + b.size] = b
    d_mid.copy_(torch.from_numpy(host).cuda())


def host_params(b):
    rec = np.zeros(len(b["fields"]), gc.RECORD_DTYPE)
    for i, (R, E, st, x) in enumerate(b["model"]):
        rec[i] = (R, E, b["D"][i], 0)
    return rec


def given_params(b):
    if b["given"] is None:
        return None
    rec = np.zeros(len(b["fields"]), gc.RECORD_DTYPE)
    for i, (R, E) in enumerate(b["given"]):
        rec[i] = (R, E, b["D"][i], 0)
    return rec


def rooms_of(b, plan):
    nbits, _, bs, _ = b["tmpl"]
    return [gc.room(f.size, bs, nbits) for f in b["fields"]]


def work_regions(b, plan):
    """(regions, unspecified) of the work buffer after a pack: the model's X in every clean field's room"""
    nbits = b["tmpl"][0]
    regions, unspecified = [], []
    for (R, E, st, x), o, r in zip(b["model"], plan["work_offsets"], rooms_of(b, plan)):
        if x is None:
            unspecified.append((int(o), r))
        else:
            regions.append((int(o), gc.x_bytes(x, nbits, r // gc.container(nbits))))
    return regions, unspecified


def pack(mods, codec, b, out_cap=None, encode=True):
    """one pack (or quantise) call over guarded buffers; returns what it left"""
    torch, api, gpu, gribgpu = mods
    n = len(b["fields"])
    n_values = [f.size for f in b["fields"]]
    plan = codec.plan(n_values, b["elem"])
    assert plan is not None
    offs, extent = gc.edge_placement(b)
    src_whole, d_src = guarded(torch, extent)
    if b.get("bases") is not None:             # fields that say where they lie: on a multiple of 16 bytes, or one element behind one
        assert [(d_src.data_ptr() + o) % 16 for o in offs] == [0 if how == "aligned" else b["elem"] for how in b["bases"]]
    put(torch, d_src, [(o, f.view(np.uint8)) for o, f in zip(offs, b["fields"])])
    src_want = src_whole.clone()
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    fields_whole, d_fields = guarded(torch, n * 16)
    got = dict(plan=plan, offs=offs, work_whole=work_whole, d_work=d_work, n_values=n_values)
    if encode:
        cap = plan["out_bound"] if out_cap is None else out_cap
        out_whole, d_out = guarded(torch, cap)
        d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
        d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
        d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
        rc = codec.pack_async(b["elem"], d_src, offs, n_values, b["D"], given_params(b), d_work, d_out, cap, d_rec, d_table,
                              d_fields, d_res)
        torch.cuda.synchronize()
        assert guards_intact(torch, out_whole, cap), "written outside d_out"
        got.update(d_out=d_out, out_whole=out_whole, cap=cap, d_table=d_table, rec=d_rec.cpu().numpy().view(np.uint64).reshape(n, 2),
                   res=d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0])
    else:
        rc = codec.quantise_async(b["elem"], d_src, offs, n_values, b["D"], given_params(b), d_work, d_fields)
        torch.cuda.synchronize()
    assert torch.equal(src_whole, src_want), "the source was written"
    assert guards_intact(torch, fields_whole, n * 16), "written outside d_fields"
    got.update(rc=rc, fields=d_fields.cpu().numpy().view(gc.RECORD_DTYPE))
    return got


def check_records_and_work(b, got):
    assert got["rc"] == AEC_OK
    for i, (R, E, st, x) in enumerate(b["model"]):
        f = got["fields"][i]
        assert int(f["status"]) == st and int(f["D"]) == b["D"][i], (b["name"], i, f, st)
        if not st & gc.BAD:
            assert f["R"].tobytes() == np.float32(R).tobytes() and int(f["E"]) == E, (b["name"], i, f, R, E)
    regions, unspecified = work_regions(b, got["plan"])
    whole_is(got["work_whole"], 0, regions, unspecified, "d_work")


def streams_of(got):
    out = got["d_out"].cpu().numpy()
    return [out[int(base) // 8:int(base) // 8 + (int(bits) + 7) // 8].tobytes() for base, bits in got["rec"]]


def check_pack(mods, b):
    """a pack of the batch: records and work buffer are the model's, every stream is b["streams"][i] (where the batch
    brings streams), aec_buffer_encode of the model's X and the reference's; the chunk records and the RSI table are those
    of the chunk coder on the work buffer"""
    torch, api, gpu, gribgpu = mods
    name = b["name"]
    nbits, options, bs, rsi = b["tmpl"]
    codec = gribgpu.GribCodec(nbits, bs, rsi, options)
    got = pack(mods, codec, b)
    check_records_and_work(b, got)
    assert got["res"]["overflow"] == 0
    streams = streams_of(got)
    at = 0
    flags = gc.coder_flags(options, False)
    for i, (s, x) in enumerate(zip(streams, b["X"])):
        assert int(got["rec"][i][0]) == at * 8, f"stream {i} does not lie behind stream {i - 1}"
        at += len(s)
        if x is None:
            continue
        if b.get("streams") is not None:
            want = b["streams"][i]
            assert s == want, f"{name}: stream {i} is not the fixture's ({len(s)} vs {len(want)} bytes)"
        data = gc.x_bytes(x, nbits, x.size)
        assert api.aec_buffer_encode(data, nbits, bs, rsi, flags) == (0, s), f"{name}: stream {i} is not aec_buffer_encode's"
        if have_ref():
            assert ref_encode(data, nbits, bs, rsi, flags) == (0, s), f"{name}: stream {i} is not the reference's"
    assert (int(got["res"]["total_bits"]) + 7) // 8 == at
    coder = gpu.Codec(*got["plan"]["coder"])
    d_out, rec, d_tab, res = coder.encode_chunks(got["d_work"].clone(), got["plan"]["work_offsets"], rooms_of(b, got["plan"]),
                                                 want_offsets=True)
    assert np.array_equal(rec.view(np.uint64), got["rec"]) and int(res["total_bits"]) == int(got["res"]["total_bits"])
    assert torch.equal(d_tab, got["d_table"])
    assert torch.equal(d_out[:at], got["d_out"][:at])
    codec.close()


@pytest.mark.parametrize("name", BATCHES)
def test_pack(mods, golden, name):
    check_pack(mods, golden[name])


def unpack(mods, codec, b, d_in, in_offs, in_sizes, d_table, fields_idx, seed):
    """one unpack call into guarded buffers; the fields fields_idx of b, placed by another shuffle"""
    torch, api, gpu, gribgpu = mods
    sub = dict(b, fields=[b["fields"][i] for i in fields_idx])
    n_values = [f.size for f in sub["fields"]]
    plan = codec.plan(n_values, b["elem"])
    offs, extent = gc.placement(sub, seed)
    dst_whole, d_dst = guarded(torch, extent)
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    n = len(n_values)
    d_results = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
    have = d_table is not None
    if not have:
        d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
    rc = codec.unpack_async(b["elem"], d_in, d_in.numel(), in_offs, in_sizes, n_values, host_params(b)[fields_idx], offs, d_table, have,
                            d_work, d_dst, d_results, d_result)
    torch.cuda.synchronize()
    assert rc == AEC_OK
    assert guards_intact(torch, work_whole, plan["work_bytes"]), "written outside d_work"
    results = d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)
    regions, unspecified = [], []
    for k, i in enumerate(fields_idx):
        R, E, st, x = b["model"][i]
        if x is None:
            unspecified.append((offs[k], b["fields"][i].nbytes))
        else:
            assert int(results[k]["status"]) == 0, (b["name"], i)
            regions.append((offs[k], gc.dequantise(x, R, E, b["D"][i], b["dtype"]).view(np.uint8)))
    whole_is(dst_whole, 0, regions, unspecified, "d_dst")


def check_unpack(mods, b, streams):
    """the round trip with the pack's table, and `streams` (one per field, None for a bad one) back to back from an odd
    byte, bare"""
    torch, api, gpu, gribgpu = mods
    nbits, options, bs, rsi = b["tmpl"]
    codec = gribgpu.GribCodec(nbits, bs, rsi, options)
    got = pack(mods, codec, b)
    assert got["rc"] == AEC_OK
    unpack(mods, codec, b, got["d_out"], None, None, got["d_table"].clone(), list(range(len(b["fields"]))), 1)
    unpack_bare(mods, codec, b, streams)
    codec.close()


def unpack_bare(mods, codec, b, streams):
    torch = mods[0]
    clean = [i for i, m in enumerate(b["model"]) if m[3] is not None]
    in_offs, at = [], 1
    for i in clean:
        in_offs.append(at)
        at += len(streams[i])
    in_whole, d_in = guarded(torch, at + 3)
    put(torch, d_in, [(o, np.frombuffer(streams[i], np.uint8)) for o, i in zip(in_offs, clean)])
    unpack(mods, codec, b, d_in, in_offs, [len(streams[i]) for i in clean], None, clean, 2)


@pytest.mark.parametrize("name", BATCHES)
def test_unpack(mods, golden, name):
    """the round trip with the pack's table, and foreign streams (the reference's, back to back from an odd byte) bare"""
    check_unpack(mods, golden[name], golden[name]["streams"])


def dequantise_alone(mods, codec, b, d_work, work_whole):
    """dequantise_async of the X in d_work under the parameters of b["model"]: the work buffer stays, the whole
    destination is the model's"""
    torch = mods[0]
    n_values = [f.size for f in b["fields"]]
    offs, extent = gc.placement(b, 3)
    dst_whole, d_dst = guarded(torch, extent)
    work_before = work_whole.clone()
    rc = codec.dequantise_async(b["elem"], d_work, n_values, host_params(b), offs, d_dst)
    torch.cuda.synchronize()
    assert rc == AEC_OK and torch.equal(work_before, work_whole)
    regions = [(o, gc.dequantise(x, R, E, D, b["dtype"]).view(np.uint8)) for o, (R, E, st, x), D in zip(offs, b["model"], b["D"])
               if x is not None]
    unspecified = [(o, f.nbytes) for o, f, (R, E, st, x) in zip(offs, b["fields"], b["model"]) if x is None]
    whole_is(dst_whole, 0, regions, unspecified, "d_dst")


def check_halves(mods, b):
    torch, api, gpu, gribgpu = mods
    nbits, options, bs, rsi = b["tmpl"]
    codec = gribgpu.GribCodec(nbits, bs, rsi, options)
    got = pack(mods, codec, b, encode=False)
    check_records_and_work(b, got)
    dequantise_alone(mods, codec, b, got["d_work"], got["work_whole"])
    codec.close()


@pytest.mark.parametrize("name", ["mix12_f4", "mix16_f8", "n32_f8", "shapes_f4", "witness_f8", "given_f4", "nonfinite_f8"])
def test_quantise_and_dequantise_alone(mods, golden, name):
    check_halves(mods, golden[name])


@pytest.mark.parametrize("name", [b["name"] for b in gc.extra_batches()])
def test_status_of_the_extra_batches(mods, name):
    """given parameters with a NaN in a field (bad, and nothing else); E held at 127 (X held to M, status bit 2): the
    records and the X of a pack are the model's"""
    torch, api, gpu, gribgpu = mods
    b = next(g for g in gc.extra_batches() if g["name"] == name)
    b = dict(b, model=gc.model_of(b))
    nbits, options, bs, rsi = b["tmpl"]
    codec = gribgpu.GribCodec(nbits, bs, rsi, options)
    for encode in (True, False):
        check_records_and_work(b, pack(mods, codec, b, encode=encode))
    codec.close()


def edge_of(name):
    """a batch of grib_cases.edge_batches() with what the checks above look at: the model and its X"""
    b = next(g for g in gc.edge_batches() if g["name"] == name)
    model = gc.model_of(b)
    return dict(b, model=model, X=[m[3] for m in model])


def own_streams(mods, tmpl, X):
    """the streams of a foreign producer: aec_buffer_encode of every X (None stays None), and the reference's the same
    where it was built.  Under AEC_PAD_RSI the encoder pads nothing (include/libaec.h: ignored, as by the reference) while
    a decoder under it expects every RSI on a byte, so such a stream is made RSI by RSI and laid back to back, as
    tests/bsmall_cases.py makes them"""
    api = mods[1]
    nbits, options, bs, rsi = tmpl
    flags = gc.coder_flags(options, False) & ~gc.PAD_RSI
    piece = bs * rsi * gc.container(nbits) if options & gc.PAD_RSI else 1 << 62
    out = []
    for x in X:
        if x is None:
            out.append(None)
            continue
        data = gc.x_bytes(x, nbits, x.size)
        s = b""
        for at in range(0, data.size, piece):
            rc, part = api.aec_buffer_encode(data[at:at + piece], nbits, bs, rsi, flags)
            assert rc == 0
            if have_ref():
                assert ref_encode(data[at:at + piece], nbits, bs, rsi, flags) == (0, part)
            s += part
        out.append(s)
    return out


@pytest.mark.parametrize("name", EDGES)
def test_pack_of_the_edge_batches(mods, name):
    """records, X and streams at the thresholds of R, E, D and X (the given records where the batch brings them)"""
    check_pack(mods, edge_of(name))


@pytest.mark.parametrize("name", EDGES)
def test_quantise_and_dequantise_alone_on_the_edge_batches(mods, name):
    check_halves(mods, edge_of(name))


@pytest.mark.parametrize("name", EDGES)
def test_unpack_of_the_edge_batches(mods, name):
    b = edge_of(name)
    check_unpack(mods, b, own_streams(mods, b["tmpl"], b["X"]))


@pytest.mark.parametrize("name", DEQS)
def test_dequantise_cases(mods, name):
    """Y under parameters no pack produced (ties to even, Inf, subnormal results, an exact +0.0, E and D at the limits of
    what the calls accept): dequantise_async on a work buffer that holds the X, and unpack_async, bare, on the streams
    aec_buffer_encode makes of them"""
    torch, api, gpu, gribgpu = mods
    c = next(g for g in gc.dequantise_cases() if g["name"] == name)
    b = gc.deq_as_batch(c)
    nbits, options, bs, rsi = b["tmpl"]
    codec = gribgpu.GribCodec(nbits, bs, rsi, options)
    plan = codec.plan([x.size for x in c["X"]], b["elem"])
    assert plan is not None
    work_whole, d_work = guarded(torch, plan["work_bytes"])
    regions, _ = work_regions(b, plan)
    put(torch, d_work, regions)
    dequantise_alone(mods, codec, b, d_work, work_whole)
    unpack_bare(mods, codec, b, own_streams(mods, b["tmpl"], c["X"]))
    codec.close()


def test_refusals_enqueue_nothing(mods, golden):
    torch, api, gpu, gribgpu = mods
    b = golden["shapes_f4"]
    nbits, options, bs, rsi = b["tmpl"]
    codec = gribgpu.GribCodec(nbits, bs, rsi, options)
    n = len(b["fields"])
    n_values = [f.size for f in b["fields"]]
    plan = codec.plan(n_values, b["elem"])
    offs, extent = gc.placement(b)
    src_whole, d_src = guarded(torch, extent)
    work_whole, d_work = guarded(torch, plan["work_bytes"] + 16)
    out_whole, d_out = guarded(torch, plan["out_bound"])
    fields_whole, d_fields = guarded(torch, n * 16)
    dst_whole, d_dst = guarded(torch, extent)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    d_results = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
    d_table = torch.zeros(plan["rsi_entries"], dtype=torch.int64, device="cuda")
    before = [t.clone() for t in (src_whole, work_whole, out_whole, fields_whole, dst_whole, d_rec, d_res, d_results, d_result, d_table)]
    cap = plan["out_bound"]
    params = host_params(b)
    D = list(b["D"])

    def packs(elem=b["elem"], src=d_src, o=offs, nv=n_values, Dd=D, prm=None, work=d_work, out=d_out, oc=cap):
        return [codec.pack_async(elem, src, o, nv, Dd, prm, work, out, oc, d_rec, d_table, d_fields, d_res),
                codec.quantise_async(elem, src, o, nv, Dd, prm, work, d_fields)]

    def unpacks(elem=b["elem"], o=offs, nv=n_values, prm=params, work=d_work):
        return [codec.unpack_async(elem, d_out, cap, None, None, nv, prm, o, d_table, 1, work, d_dst, d_results, d_result),
                codec.dequantise_async(elem, work, nv, prm, o, d_dst)]

    bad_D = D[:3] + [23] + D[4:]
    odd = [offs[0] + 2] + offs[1:]
    none = n_values[:2] + [0] + n_values[3:]
    far = params.copy()
    far["E"][1] = 1023
    bad_params = params.copy()
    bad_params["D"][2] = -23
    assert packs(elem=2) == [AEC_CONF_ERROR] * 2 and unpacks(elem=16) == [AEC_CONF_ERROR] * 2
    assert packs(Dd=bad_D) == [AEC_CONF_ERROR] * 2 and unpacks(prm=bad_params) == [AEC_CONF_ERROR] * 2
    assert packs(o=odd) == [AEC_CONF_ERROR] * 2 and unpacks(o=odd) == [AEC_CONF_ERROR] * 2
    assert packs(nv=none) == [AEC_CONF_ERROR] * 2 and unpacks(nv=none) == [AEC_CONF_ERROR] * 2
    assert packs(work=d_work[8:]) == [AEC_CONF_ERROR] * 2 and unpacks(work=d_work[8:]) == [AEC_CONF_ERROR] * 2
    assert packs(prm=far) == [AEC_CONF_ERROR] * 2 and unpacks(prm=far) == [AEC_CONF_ERROR] * 2
    low = params.copy()
    low["E"][1] = -1023
    assert packs(prm=low) == [AEC_CONF_ERROR] * 2 and unpacks(prm=low) == [AEC_CONF_ERROR] * 2
    for out, oc in ((d_out[8:], cap - 16), (d_out, cap - 8), (d_out, 0)):         # (the encoder's own conditions on its output)
        assert codec.pack_async(b["elem"], d_src, offs, n_values, D, None, d_work, out, oc, d_rec, d_table, d_fields, d_res) == AEC_CONF_ERROR
    signed = gribgpu.GribCodec(nbits, bs, rsi, options)
    signed.t.options |= gc.SIGNED
    assert signed.pack_async(b["elem"], d_src, offs, n_values, D, None, d_work, d_out, cap, d_rec, d_table, d_fields, d_res) == AEC_CONF_ERROR
    torch.cuda.synchronize()
    after = (src_whole, work_whole, out_whole, fields_whole, dst_whole, d_rec, d_res, d_results, d_result, d_table)
    assert all(torch.equal(x, y) for x, y in zip(before, after)), "a refused call wrote"
    assert codec.pack_async(b["elem"], d_src, [], [], [], None, d_work, d_out, cap, d_rec, d_table, d_fields, d_res) == AEC_OK
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, after)), "a call without fields wrote"
    signed.close()
    # the limits themselves are taken: a given E of exactly +-1022 and a D of exactly +-22, and what comes out is the model's
    ends = dict(b, D=[22, -22, 22, -22] + D[4:], given=[(float(R), [1022, -1022, -1022, 1022][i] if i < 4 else E)
                                                         for i, (R, E, st, x) in enumerate(b["model"])])
    ends["model"] = gc.model_of(ends)
    assert [m[1] for m in ends["model"][:4]] == [1022, -1022, -1022, 1022] and not any(m[2] & gc.BAD for m in ends["model"])
    for encode in (True, False):
        got = pack(mods, codec, ends, encode=encode)
        check_records_and_work(ends, got)
    dequantise_alone(mods, codec, ends, got["d_work"], got["work_whole"])
    unpack_bare(mods, codec, ends, own_streams(mods, ends["tmpl"], [m[3] for m in ends["model"]]))
    codec.close()


def test_out_cap_too_small(mods, golden):
    """overflow is set and nothing is written at or beyond the cap (the guards behind it say so)"""
    torch, api, gpu, gribgpu = mods
    b = golden["mix12_f4"]
    nbits, options, bs, rsi = b["tmpl"]
    codec = gribgpu.GribCodec(nbits, bs, rsi, options)
    full = pack(mods, codec, b)
    need = (int(full["res"]["total_bits"]) + 7) // 8
    cap = need // 2 // 16 * 16
    got = pack(mods, codec, b, out_cap=cap)
    assert got["rc"] == AEC_OK and got["res"]["overflow"] == 1 and int(got["res"]["total_bits"]) == int(full["res"]["total_bits"])
    check_records_and_work(b, got)
    codec.close()


def test_codec_round_trip(mods, golden):
    """the convenience layer: pack, unpack with and without the table, quantise and dequantise on tensors"""
    torch, api, gpu, gribgpu = mods
    b = golden["mix16_f8"]
    nbits, options, bs, rsi = b["tmpl"]
    codec = gribgpu.GribCodec(nbits, bs, rsi, options)
    n_values = [f.size for f in b["fields"]]
    starts = np.concatenate([[0], np.cumsum(n_values)])[:-1]
    d_values = torch.from_numpy(np.concatenate(b["fields"])).cuda()
    d_out, spans, fields, d_table = codec.pack(d_values, starts, n_values, b["D"], want_offsets=True)
    want = np.concatenate([gc.dequantise(x, R, E, D, b["dtype"]) for (R, E, st, x), D in zip(b["model"], b["D"])])
    for i, (s, ln) in enumerate(spans):
        assert d_out[s:s + ln].cpu().numpy().tobytes() == b["streams"][i]
    for table in (d_table, None):
        d_back, results = codec.unpack(d_out, spans, fields, n_values, table, dtype=torch.float64)
        assert np.all(results["status"] == 0) and d_back.cpu().numpy().tobytes() == want.tobytes()
    d_work, plan, fields2 = codec.quantise(d_values, starts, n_values, b["D"])
    assert fields2.tobytes() == fields.tobytes()
    assert codec.dequantise(d_work, n_values, fields, dtype=torch.float64).cpu().numpy().tobytes() == want.tobytes()
    codec.close()
