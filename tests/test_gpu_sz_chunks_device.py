"""SZIP chunks of any size in one call (include/aec_gpu_sz.h: aec_gpu_sz_compress_chunks_async /
aec_gpu_sz_decompress_chunks_async; libaec_amd/szgpu.py): against streams the reference's shim made
(tests/golden/sz_chunks_vectors.npz), against the host path (szip.compress per chunk, which tests/test_gpu_szip.py pins to
the reference and which is compared with the reference shim itself when oracle/_ref travelled), and against the NumPy
restatement of sz_abi.cpp for what the work buffer holds.  Every buffer a call writes lies between guard bytes and is
compared whole: the rooms hold what they must, everything between and around them is as it was."""
import ctypes as C

import numpy as np
import pytest

from helpers import REF_SO, have_ref
from sz_chunks_cases import eligible, golden_batches, small_batch, synthetic_batch, unit_of
from sz_device_cases import NN, RAW, chunk_data, sweep_cases
from test_gpu_sz_device import GUARD, guarded, guards_intact
from test_sz_layout import SYNTHETIC, np_marshal, py_layout

pytestmark = pytest.mark.gpu

AEC_OK, AEC_CONF_ERROR = 0, -1


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import gpu, szgpu, szip
    szip.library()
    return torch, gpu, szgpu, szip


@pytest.fixture(scope="module")
def fixture_streams():
    return {name: (params, sizes, chunks, streams) for name, params, sizes, chunks, streams in golden_batches()}


def host_streams(szip, chunks, opts, bpp, ppb, pps):
    """the host path's stream of every chunk; when oracle/_ref travelled, compared with the reference shim's -- of the
    chunk's whole pixels: handed a trailing fraction of a pixel, the reference codes bytes it never wrote (with byte
    planes) or a pixel that starts in the middle of one (tests/golden/make_golden_sz_chunks.py)"""
    out = []
    ref = szip.bind(C.CDLL(REF_SO)) if have_ref() else None
    for c in chunks:
        rc, enc = szip.compress(c, c.size * 2 + 4096, opts, bpp, ppb, pps)
        assert rc == szip.SZ_OK
        if ref is not None:
            whole = c[:c.size - c.size % unit_of(bpp)]
            assert szip.compress(whole, c.size * 2 + 4096, opts, bpp, ppb, pps, lib=ref) == (rc, enc)
        out.append(enc)
    return out


def up16(v):
    return (v + 15) // 16 * 16


def place(sizes, order, gap):
    """offsets of the chunks when they lie in `order`, gap(k) bytes behind the k-th of them; (offsets, extent)"""
    offs, at = [0] * len(sizes), 0
    for k, i in enumerate(order):
        offs[i] = at
        at += sizes[i] + gap(k)
    return offs, at


def assert_whole(whole, skew, regions, what):
    """the guarded tensor holds `regions` [(offset in its middle, bytes)] and its pattern everywhere else"""
    want = (np.arange(whole.numel()) % 251).astype(np.uint8)
    for o, b in regions:
        want[GUARD + skew + o:GUARD + skew + o + b.size] = b
    got = whole.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {int(bad[0]) - GUARD - skew} of the middle"


def zero_tail(chunk, params):
    out = chunk.copy()
    out[chunk.size - chunk.size % unit_of(params[1]):] = 0
    return out


def compress(mods, codec, params, chunks, src_offs, src_skew, with_work=True, out_cap=None):
    """one compress call over guarded buffers; returns what it left"""
    torch, gpu, szgpu, szip = mods
    sizes = [c.size for c in chunks]
    n = len(sizes)
    plan = codec.chunks_plan(sizes)
    assert plan is not None
    extent = max(o + s for o, s in zip(src_offs, sizes))
    src_whole, d_src = guarded(torch, extent, src_skew)
    host = d_src.cpu().numpy()
    for o, c in zip(src_offs, chunks):
        host[o:o + c.size] = c
    d_src.copy_(torch.from_numpy(host).cuda())
    src_want = src_whole.clone()
    work_whole, d_work = guarded(torch, plan["work_bytes"]) if with_work else (None, None)
    cap = plan["out_bound"] if out_cap is None else out_cap
    out_whole, d_out = guarded(torch, cap)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
    rc = codec.compress_chunks_async(d_src, src_offs, sizes, d_work, d_out, cap, d_rec, d_table, d_res)
    torch.cuda.synchronize()
    assert torch.equal(src_whole, src_want), "the source was written"
    assert guards_intact(torch, out_whole, cap), "written outside d_out"
    return dict(rc=rc, plan=plan, d_out=d_out, out_whole=out_whole, work_whole=work_whole, d_table=d_table, sizes=sizes,
                rec=d_rec.cpu().numpy().view(np.uint64).reshape(n, 2), res=d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0])


def streams_of(got):
    out = got["d_out"].cpu().numpy()
    return [out[int(b) // 8:int(b) // 8 + (int(bits) + 7) // 8].tobytes() for b, bits in got["rec"]]


def check_compressed(mods, got, params, chunks, want_streams, check_table=False):
    torch, gpu, szgpu, szip = mods
    assert got["rc"] == AEC_OK and got["res"]["overflow"] == 0
    streams = streams_of(got)
    at = 0
    for i, (s, w) in enumerate(zip(streams, want_streams)):
        assert int(got["rec"][i][0]) == at * 8, f"stream {i} does not lie behind stream {i - 1}"
        assert s == w, f"stream {i} of {len(streams)}: {len(s)} vs {len(w)} bytes"
        at += len(s)
    assert (int(got["res"]["total_bits"]) + 7) // 8 == at
    if got["work_whole"] is not None:
        rooms = [(int(o), np_marshal(c, *params)) for o, c in zip(got["plan"]["work_offsets"], chunks)]
        assert_whole(got["work_whole"], 0, rooms, "d_work")
    if check_table:
        table = got["d_table"].cpu().numpy()
        L0 = py_layout(*params, 64)
        coder = gpu.Codec(L0["bps"], L0["bs"], L0["rsi"], L0["flags"])
        entry = 0
        for i, c in enumerate(chunks):
            lines = py_layout(*params, c.size)["lines"]
            d_in = torch.from_numpy(np_marshal(c, *params)).cuda()
            _, _, _, _, d_off = coder.encode(d_in)
            alone = d_off.cpu().numpy().astype(np.int64)
            assert alone.size == lines + 1
            assert np.array_equal(table[entry:entry + lines + 1] - int(got["rec"][i][0]), alone), f"table of chunk {i}"
            entry += lines + 1
        assert entry == got["plan"]["rsi_entries"]


def decompress(mods, codec, params, chunks, got, dst_offs, dst_skew, have_table, with_work=True, streams=None):
    """one decompress call into guarded buffers; the compress call's output is its input, with that call's table or bare"""
    torch, gpu, szgpu, szip = mods
    sizes = [c.size for c in chunks]
    n = len(sizes)
    plan = got["plan"]
    extent = max(o + s for o, s in zip(dst_offs, sizes))
    dst_whole, d_dst = guarded(torch, extent, dst_skew)
    work_whole, d_work = guarded(torch, plan["work_bytes"]) if with_work else (None, None)
    d_results = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
    d_in = got["d_out"]
    if have_table:
        d_table, in_offs, in_sizes = got["d_table"].clone(), None, None
    else:
        d_table = torch.full((plan["rsi_entries"],), -1, dtype=torch.int64, device="cuda")
        in_offs = [int(b) // 8 for b, _ in got["rec"]]
        in_sizes = [(int(bits) + 7) // 8 for _, bits in got["rec"]]
    rc = codec.decompress_chunks_async(d_in, d_in.numel(), in_offs, in_sizes, dst_offs, sizes, d_table, have_table, d_work, d_dst,
                                       d_results, d_result)
    torch.cuda.synchronize()
    if work_whole is not None:
        assert guards_intact(torch, work_whole, plan["work_bytes"]), "written outside d_work"
    return dict(rc=rc, dst_whole=dst_whole, results=d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE),
                result=d_result.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0])


def check_restored(back, params, chunks, dst_offs, dst_skew, what):
    assert back["rc"] == AEC_OK, what
    lines = [py_layout(*params, c.size)["lines"] for c in chunks]
    assert np.all(back["results"]["status"] == 0) and [int(v) for v in back["results"]["n_rsi"]] == lines, what
    assert_whole(back["dst_whole"], dst_skew, [(o, zero_tail(c, params)) for o, c in zip(dst_offs, chunks)], what)


def round_trip(mods, params, chunks, want_streams, src_offs, src_skew, check_table=False, direct=False, seed=0):
    """compress (streams, work buffer, table), then decompress with the table to chunks in another shuffled order and
    bare to chunks back to back from an address 11 off a 16-byte boundary (or, direct: to aligned places, no work buffer)"""
    torch, gpu, szgpu, szip = mods
    sizes = [c.size for c in chunks]
    codec = szgpu.SzCodec(*params)
    got = compress(mods, codec, params, chunks, src_offs, src_skew, with_work=not direct)
    assert got["plan"]["direct"] == int(direct)
    check_compressed(mods, got, params, chunks, want_streams, check_table)
    order = list(np.random.default_rng(seed + 1).permutation(len(sizes)))
    if direct:
        offs, _ = place(sizes, order, lambda k: -sizes[order[k]] % 16 + 16 * (k % 2))
        for have_table in (1, 0):
            back = decompress(mods, codec, params, chunks, got, offs, 0, have_table, with_work=False)
            check_restored(back, params, chunks, offs, 0, f"direct, table {have_table}")
    else:
        offs, _ = place(sizes, order, lambda k: 3 + 13 * (k % 3))
        back = decompress(mods, codec, params, chunks, got, offs, 0, 1)
        check_restored(back, params, chunks, offs, 0, "with the table")
        offs, _ = place(sizes, list(range(len(sizes))), lambda k: 0)
        back = decompress(mods, codec, params, chunks, got, offs, 11, 0)
        check_restored(back, params, chunks, offs, 11, "bare")
    codec.close()


# ---- 1. synthetic unequal batches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SYNTHETIC)), ids=lambda k: f"{SYNTHETIC[k][1]}bpp")
def test_synthetic_unequal_batches(mods, fixture_streams, k):
    torch, gpu, szgpu, szip = mods
    case = SYNTHETIC[k]
    params, sizes, chunks, streams = fixture_streams[f"synthetic-{case[1]}"]
    again_sizes, again = synthetic_batch(case)
    assert sizes == again_sizes and all(np.array_equal(a, b) for a, b in zip(chunks, again))
    assert host_streams(szip, chunks, *params) == streams
    order = list(np.random.default_rng(k).permutation(len(sizes)))
    for skew in (0, 5):
        # (the eligible chunk of a set with byte planes at a 16-byte aligned address when skew is 0)
        offs, _ = place(sizes, order, lambda j: -sizes[order[j]] % 16 if skew == 0 else 3 + 7 * j)
        round_trip(mods, params, chunks, streams, offs, skew, check_table=skew == 0, seed=k)


# ---- 2. beyond the uniform limit ----------------------------------------------------------------------------------------------
def test_chunks_beyond_the_uniform_batch(mods, fixture_streams):
    torch, gpu, szgpu, szip = mods
    params, sizes, chunks, streams = fixture_streams["beyond-127"]
    assert params == (NN | RAW, 8, 2, 127) and sizes == [300 << 10, 10 << 10, 300 << 10]
    assert szgpu.batch_ok(*params, 300 << 10, 2) == 0
    L = py_layout(*params, 300 << 10)
    assert (L["lines"], L["rsi"]) == (2419, 64)
    assert host_streams(szip, chunks, *params) == streams
    offs, _ = place(sizes, [2, 0, 1], lambda k: 5)
    round_trip(mods, params, chunks, streams, offs, 3)


def test_chunks_beyond_the_uniform_batch_coded_where_they_lie(mods, fixture_streams):
    torch, gpu, szgpu, szip = mods
    params, sizes, chunks, streams = fixture_streams["beyond-128"]
    assert params == (NN | RAW, 8, 2, 128) and szgpu.batch_ok(*params, 300 << 10, 2) == 0
    assert host_streams(szip, chunks, *params) == streams
    offs, _ = place(sizes, [1, 2, 0], lambda k: 16 * k)
    round_trip(mods, params, chunks, streams, offs, 0, direct=True)


# ---- 3. many small chunks -----------------------------------------------------------------------------------------------------
def test_many_small_chunks(mods, fixture_streams):
    torch, gpu, szgpu, szip = mods
    params, sizes, chunks, streams = fixture_streams["small-300"]
    assert len(sizes) == 300 and min(sizes) >= 2 and max(sizes) <= 4000 and sizes == small_batch()[1]
    some = list(range(0, 300, 15))
    assert host_streams(szip, [chunks[i] for i in some], *params) == [streams[i] for i in some]
    offs, _ = place(sizes, list(range(300)), lambda k: 0)
    round_trip(mods, params, chunks, streams, offs, 1)


# ---- 4. mixed paths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpp", [32, 64])
def test_mixed_paths(mods, fixture_streams, bpp):
    torch, gpu, szgpu, szip = mods
    params, sizes, chunks, streams = fixture_streams[f"mixed-{bpp}"]
    case = params + (0,)
    assert [eligible(case, s) for s in sizes] == [True, False, True, True]
    assert sizes[1] // unit_of(bpp) % 2 == 1
    assert host_streams(szip, chunks, *params) == streams
    offs, at = [0], up16(sizes[0])
    offs.append(at)                                  # chunk 1: anywhere
    at = up16(at + sizes[1]) + 4
    offs.append(at)                                  # chunk 2: eligible, 4 off a 16-byte boundary
    offs.append(up16(at + sizes[2]))                 # chunk 3: eligible and aligned
    assert [o % 16 for o in offs] == [0, 0, 4, 0]
    round_trip(mods, params, chunks, streams, offs, 0, check_table=True, seed=bpp)


# ---- 5. sweep -----------------------------------------------------------------------------------------------------------------
def test_random_sweep_against_the_host_path(mods):
    torch, gpu, szgpu, szip = mods
    refused = 0
    for case in sweep_cases():
        params = (case["opts"], case["bpp"], case["ppb"], case["pps"])
        rng = np.random.default_rng(500 + case["seed"])
        u = unit_of(case["bpp"])
        sizes = [int(v) * u for v in rng.integers(1, 65536 // u + 1, size=int(rng.integers(1, 13)))]
        if szgpu.layout(*params, 64) is None:
            assert szgpu.chunks_plan(*params, sizes) is None
            refused += 1
            continue
        chunks = [chunk_data(dict(case, n=1, chunk_bytes=s, seed=case["seed"] + 100 * j))[0] for j, s in enumerate(sizes)]
        want = host_streams(szip, chunks, *params)
        codec = szgpu.SzCodec(*params)
        order = list(rng.permutation(len(sizes)))
        offs, _ = place(sizes, order, lambda k: int(case["seed"] + 5 * k) % 23)
        got = compress(mods, codec, params, chunks, offs, case["seed"] % 3 * 4)
        check_compressed(mods, got, params, chunks, want)
        dst, _ = place(sizes, list(range(len(sizes))), lambda k: k % 2)
        have_table = case["seed"] % 2
        back = decompress(mods, codec, params, chunks, got, dst, case["seed"] % 16, have_table)
        check_restored(back, params, chunks, dst, case["seed"] % 16, f"case {case['seed']}, table {have_table}")
        codec.close()
    assert refused * 4 <= 30


# ---- 6. errors and refusals -----------------------------------------------------------------------------------------------------
def smooth(size, seed):
    rng = np.random.default_rng(seed)
    return (128 + np.cumsum(rng.integers(-2, 3, size=size)) % 64).astype(np.uint8)


def test_a_damaged_stream_spoils_its_own_chunk_only(mods):
    """8 chunks, 8 / 8 / 1024 NN; the head of stream 5 overwritten with a second-extension code beyond the table, the
    error only the decoder sees that tests/test_gpu_szip.py::test_batch_of_small_chunks_reports_errors_per_chunk uses"""
    torch, gpu, szgpu, szip = mods
    from test_gpu_szip import _bits_to_bytes
    params = (NN | RAW, 8, 8, 1024)
    sizes = [8192, 3000, 1024, 20000, 5, 8192, 4096, 1]
    chunks = [smooth(s, 60 + i) for i, s in enumerate(sizes)]
    codec = szgpu.SzCodec(*params)
    offs, _ = place(sizes, list(range(8)), lambda k: 0)
    got = compress(mods, codec, params, chunks, offs, 0)
    check_compressed(mods, got, params, chunks, host_streams(szip, chunks, *params))
    bad = _bits_to_bytes("000" + "1" + "10000000" + "0" * 95 + "1" + "1" * 3 + "1" * 64)
    at = int(got["rec"][5][0]) // 8
    assert len(bad) < (int(got["rec"][5][1]) + 7) // 8
    got["d_out"][at:at + len(bad)] = torch.frombuffer(bytearray(bad), dtype=torch.uint8).cuda()
    back = decompress(mods, codec, params, chunks, got, offs, 7, 0)
    assert back["rc"] == AEC_OK and back["results"][5]["status"] != 0
    good = [i for i in range(8) if i != 5]
    assert all(back["results"][i]["status"] == 0 for i in good)
    whole = back["dst_whole"].cpu().numpy()
    for i in good:
        assert np.array_equal(whole[GUARD + 7 + offs[i]:GUARD + 7 + offs[i] + sizes[i]], chunks[i]), i
    assert guards_intact(torch, back["dst_whole"], offs[-1] + sizes[-1], 7)         # (the chunks lie back to back)
    codec.close()


def test_an_output_16_bytes_short_overflows_and_stays_inside(mods):
    torch, gpu, szgpu, szip = mods
    params = (NN | RAW, 16, 16, 100)
    sizes = [2000, 6, 1234, 4000]
    chunks = [smooth(s, 70 + i) for i, s in enumerate(sizes)]
    codec = szgpu.SzCodec(*params)
    offs, _ = place(sizes, [3, 1, 0, 2], lambda k: 1)
    total = sum(len(s) for s in host_streams(szip, chunks, *params))
    fits = compress(mods, codec, params, chunks, offs, 0, out_cap=up16(total))
    assert fits["rc"] == AEC_OK and fits["res"]["overflow"] == 0 and int(fits["res"]["total_bits"] + 7) // 8 == total
    short = compress(mods, codec, params, chunks, offs, 0, out_cap=up16(total) - 16)    # (compress checks the guards)
    assert short["rc"] == AEC_OK and short["res"]["overflow"] == 1
    codec.close()


def test_refusals_and_what_the_context_holds(mods):
    torch, gpu, szgpu, szip = mods
    params = (NN | RAW, 8, 8, 1024)
    sizes = [4096, 1024, 8192]
    chunks = [smooth(s, 80 + i) for i, s in enumerate(sizes)]
    offs, _ = place(sizes, [0, 1, 2], lambda k: 0)
    # every chunk is the coder's input: coded where it lies when aligned, through d_work when not
    there = szgpu.SzCodec(*params)
    assert there.held_bytes() == 0
    got = compress(mods, there, params, chunks, offs, 0, with_work=False)
    want = host_streams(szip, chunks, *params)
    check_compressed(mods, got, params, chunks, want)
    coder_holds = there.held_bytes()
    moved = szgpu.SzCodec(*params)
    got = compress(mods, moved, params, chunks, offs, 8)
    check_compressed(mods, got, params, chunks, want)
    assert moved.held_bytes() >= coder_holds + 256 + 256                     # (the descriptors and the wavefront table)
    assert got["plan"]["workspace_bytes"] >= 512
    moved.trim(0)
    assert moved.held_bytes() == 0
    got = compress(mods, moved, params, chunks, offs, 8)                     # (and it comes back)
    check_compressed(mods, got, params, chunks, want)

    def call(codec, sizes, d_work, src_skew=8, n=None):
        whole, d_src = guarded(torch, sum(sizes) + 16, src_skew)
        d_out = torch.zeros(65536, dtype=torch.uint8, device="cuda")
        d_rec = torch.zeros(16, dtype=torch.int64, device="cuda")
        d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
        o = [int(v) for v in np.cumsum([0] + sizes[:-1])]
        if n == 0:
            o, sizes = [], []
        rc = codec.compress_chunks_async(d_src, o, sizes, d_work, d_out, d_out.numel(), d_rec, None, d_res)
        d_table = torch.zeros(64, dtype=torch.int64, device="cuda")
        d_results = torch.zeros(16 * 40, dtype=torch.uint8, device="cuda")
        d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
        rd = codec.decompress_chunks_async(d_out, d_out.numel(), None, None, o, sizes, d_table, 1, d_work, d_src, d_results, d_result)
        torch.cuda.synchronize()
        assert not d_rec.any() and not d_out.any() and not d_res.any() and not d_results.any() and guards_intact(
            torch, whole, sum(sizes) + 16, src_skew) or n == 0
        return rc, rd

    d_work = torch.zeros(32768 + 16, dtype=torch.uint8, device="cuda")
    assert call(moved, [], d_work, n=0) == (AEC_OK, AEC_OK)
    assert call(moved, [4096, 1000], None) == (AEC_CONF_ERROR, AEC_CONF_ERROR)          # a work buffer is needed
    assert call(moved, [4096, 1024], None) == (AEC_CONF_ERROR, AEC_CONF_ERROR)          # ... for unaligned chunks too
    assert call(moved, [4096, 1000], d_work[1:]) == (AEC_CONF_ERROR, AEC_CONF_ERROR)    # and an aligned one
    wide = szgpu.SzCodec(NN | RAW, 16, 16, 100)
    assert call(wide, [200, 1], d_work) == (AEC_CONF_ERROR, AEC_CONF_ERROR)             # a chunk without a whole pixel
    wide.sz.pixels_per_block = 15
    assert call(wide, [200, 100], d_work) == (AEC_CONF_ERROR, AEC_CONF_ERROR)           # an SZ_com_t the layout rejects
    assert call(wide, [], d_work, n=0) == (AEC_CONF_ERROR, AEC_CONF_ERROR)
    assert moved.held_bytes() > 0 and wide.held_bytes() == 0
    for c in (there, moved, wide):
        c.close()
