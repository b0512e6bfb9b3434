"""aec_gpu_sz_estimate_async (include/aec_gpu_sz.h; libaec_amd/szgpu.py): the length of SZ_BufftoBuffCompress's stream of
every chunk under pixels per block 8, 16, 32 and 64 in one pass, next to what a caller did before it -- one
aec_gpu_sz_compress_chunks_async per candidate on the same device buffers: d_chunk_bits[c * 4 + i] must be the bits that
call writes into d_chunks[c], total_bytes and best what they are defined to be, and the bytes the lengths of the streams
the reference's shim made (tests/golden/sz_estimate.json).  The cases are those of tests/test_sz_estimate_emul.py."""
import ctypes as C

import numpy as np
import pytest

import sz_estimate_cases as sc
from test_gpu_sz_device import GUARD, guarded, guards_intact

pytestmark = pytest.mark.gpu

AEC_OK, AEC_CONF_ERROR = 0, -1
NOT_ASKED = (1 << 64) - 1


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import api, gpu, szgpu
    lib = api.library()
    # bound here, not through the package: a library without the call fails these tests
    lib.aec_gpu_sz_estimate_plan.restype = C.c_int
    lib.aec_gpu_sz_estimate_plan.argtypes = [C.POINTER(szgpu.SZ_com_t), C.c_void_p, C.c_void_p, C.c_uint64,
                                             C.POINTER(szgpu.SzEstimatePlan)]
    lib.aec_gpu_sz_estimate_async.restype = C.c_int
    lib.aec_gpu_sz_estimate_async.argtypes = [C.c_void_p, C.POINTER(szgpu.SZ_com_t)] + [C.c_void_p] * 4 + [C.c_uint64] + \
        [C.c_void_p] * 3
    return torch, gpu, szgpu, lib


def codec_for(szgpu, opts, bpp, pps):
    i = sc.asked(pps)[0]
    return szgpu.SzCodec(opts, bpp, 8 << i, pps[i])


def upload(torch, buf, skew):
    whole, d_src = guarded(torch, buf.size, skew)
    d_src.copy_(torch.from_numpy(buf).cuda())
    return whole, d_src


def estimate(mods, codec, pps, d_src, offs, sizes, want_bits=True):
    """one call into guarded buffers -> (rc, bits per chunk and size, the record)"""
    torch, gpu, szgpu, lib = mods
    n = len(sizes)
    bits_whole, d_bits = guarded(torch, max(1, n) * 32)
    est_whole, d_est = guarded(torch, 40)
    offs, sizes = np.ascontiguousarray(offs, dtype=np.uint64), np.ascontiguousarray(sizes, dtype=np.uint64)
    vec = (C.c_uint * 4)(*pps) if pps is not None else None
    rc = lib.aec_gpu_sz_estimate_async(codec.ctx, C.byref(codec.sz), vec, C.c_void_p(d_src.data_ptr()), C.c_void_p(offs.ctypes.data),
                                       C.c_void_p(sizes.ctypes.data), n, C.c_void_p(d_bits.data_ptr()) if want_bits else None,
                                       C.c_void_p(d_est.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert guards_intact(torch, bits_whole, max(1, n) * 32), "written outside d_chunk_bits"
    assert guards_intact(torch, est_whole, 40), "written outside d_estimate"
    bits = d_bits.cpu().numpy().view(np.uint64).reshape(-1, 4)[:n]
    return rc, [[int(v) for v in row] for row in bits], d_est.cpu().numpy().view(szgpu.SZ_ESTIMATE_DTYPE)[0], (d_bits, d_est)


def compress_bits(mods, codec, i, line, d_src, offs, sizes):
    """what a caller does today for candidate i: the bits of every chunk's stream"""
    torch, gpu, szgpu, lib = mods
    codec.sz.pixels_per_block, codec.sz.pixels_per_scanline = 8 << i, line
    plan = codec.chunks_plan(sizes)
    assert plan is not None
    n = len(sizes)
    d_work = torch.empty(plan["work_bytes"] + 16, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(plan["out_bound"], dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(n * 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
    rc = codec.compress_chunks_async(d_src, offs, sizes, d_work, d_out, d_out.numel(), d_rec, None, d_res)
    torch.cuda.synchronize()
    assert rc == AEC_OK and d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["overflow"] == 0
    return [int(v) for v in d_rec.cpu().numpy().view(np.uint64).reshape(n, 2)[:, 1]]


def check_record(rec, bits, pps):
    for i in range(4):
        if pps[i]:
            assert int(rec["total_bytes"][i]) == sum(max(1, (row[i] + 7) // 8) for row in bits), i
        else:
            assert int(rec["total_bytes"][i]) == NOT_ASKED and all(row[i] == NOT_ASKED for row in bits), i
    totals = [int(v) for v in rec["total_bytes"]]
    assert int(rec["best"]) == min(sc.asked(pps), key=lambda i: (totals[i], i)) and int(rec["pad"]) == 0


def check_case(mods, name, opts, bpp, pps, chunks, golden=None):
    torch, gpu, szgpu, lib = mods
    codec = codec_for(szgpu, opts, bpp, pps)
    buf, offs, sizes = sc.place(chunks, "aligned")
    _, d_src = upload(torch, buf, 0)
    rc, bits, rec, _ = estimate(mods, codec, pps, d_src, offs, sizes)
    assert rc == AEC_OK, name
    for i in sc.asked(pps):
        want = compress_bits(mods, codec, i, pps[i], d_src, offs, sizes)
        assert [row[i] for row in bits] == want, (name, i)
    check_record(rec, bits, pps)
    if golden is not None:
        for c, row in enumerate(bits):
            assert [max(1, (b + 7) // 8) if pps[i] else None for i, b in enumerate(row)] == golden[c], (name, c)
    # the chunks at unaligned offsets, in another order: the same answers
    buf, offs, sizes = sc.place(chunks, "shuffled", 5)
    _, d_src = upload(torch, buf, 5)
    rc, again, rec2, _ = estimate(mods, codec, pps, d_src, offs, sizes)
    assert rc == AEC_OK and again == bits and rec2.tobytes() == rec.tobytes(), name
    codec.close()
    return bits


GROUPS = sorted(set(c[0].split("-")[0] for c in sc.all_cases()), key=lambda g: (not g.isdigit(), int(g) if g.isdigit() else 0, g))


@pytest.mark.parametrize("group", GROUPS)
def test_estimate_next_to_one_compress_per_candidate(mods, group):
    golden = sc.golden()
    seen = 0
    for name, opts, bpp, pps, chunks in sc.all_cases():
        if name.split("-")[0] == group:
            check_case(mods, name, opts, bpp, pps, chunks, golden[name])
            seen += 1
    assert seen


@pytest.mark.parametrize("bpp,path", [(32, "4-byte planes"), (16, "straight")])
def test_one_eligible_chunk_between_two_odd_ones(mods, bpp, path):
    """the middle chunk on a 16-byte boundary, its neighbours off one: a fast path and the byte-wise map in one call"""
    torch, gpu, szgpu, lib = mods
    rng = np.random.default_rng(3)
    opts, pps = sc.NN | sc.RAW, [64] * 4
    chunks = [sc.pixels(rng, "walk", 2 * 64, bpp, opts) for _ in range(3)]
    n = chunks[0].size
    mid = 16 * (-(-(3 + n) // 16))
    offs, sizes = [3, mid, mid + n + 5], [n] * 3
    buf = np.full(mid + 2 * n + 5 + 16, 0x3C, dtype=np.uint8)
    for o, c in zip(offs, chunks):
        buf[o:o + n] = c
    _, d_src = upload(torch, buf, 0)
    codec = codec_for(szgpu, opts, bpp, pps)
    rc, bits, rec, _ = estimate(mods, codec, pps, d_src, offs, sizes)
    assert rc == AEC_OK
    for i in range(4):
        assert [row[i] for row in bits] == compress_bits(mods, codec, i, 64, d_src, offs, sizes), (path, i)
    check_record(rec, bits, pps)
    codec.close()


def test_one_chunk_of_2_mib_of_float32(mods):
    """512 Ki pixels, 1024 a line: 32768 pieces of the plane path, several workgroups of every kernel"""
    torch, gpu, szgpu, lib = mods
    rng = np.random.default_rng(32)
    chunk = np.cumsum(rng.standard_normal(512 << 10)).astype("<f4").view(np.uint8)
    opts, pps = sc.NN | sc.RAW, [1024, 1024, 1024, 0]
    codec = codec_for(szgpu, opts, 32, pps)
    _, d_src = upload(torch, chunk, 0)
    rc, bits, rec, _ = estimate(mods, codec, pps, d_src, [0], [chunk.size])
    assert rc == AEC_OK
    for i in range(3):
        assert bits[0][i] == compress_bits(mods, codec, i, 1024, d_src, [0], [chunk.size])[0], i
    check_record(rec, bits, pps)
    # without d_chunk_bits: the same record
    rc, _, again, _ = estimate(mods, codec, pps, d_src, [0], [chunk.size], want_bits=False)
    assert rc == AEC_OK and again.tobytes() == rec.tobytes()
    codec.close()


def test_what_the_context_holds(mods):
    torch, gpu, szgpu, lib = mods
    _, opts, bpp, pps, chunks = [c for c in sc.all_cases() if c[0] == "small-300"][0]
    buf, offs, sizes = sc.place(chunks, "aligned")
    _, d_src = upload(torch, buf, 0)
    codec = codec_for(szgpu, opts, bpp, pps)
    plan = szgpu.SzEstimatePlan()
    assert lib.aec_gpu_sz_estimate_plan(C.byref(codec.sz), (C.c_uint * 4)(*pps), C.c_void_p(sizes.ctypes.data), len(sizes), C.byref(plan)) == 1
    assert codec.held_bytes() == 0
    rc, bits, rec, _ = estimate(mods, codec, pps, d_src, offs, sizes)
    assert rc == AEC_OK and 0 < codec.held_bytes() <= plan.workspace_bytes
    held = codec.held_bytes()
    rc, again, _, _ = estimate(mods, codec, pps, d_src, offs, sizes)             # (a second call: nothing grows)
    assert rc == AEC_OK and again == bits and codec.held_bytes() == held
    codec.trim(0)
    assert codec.held_bytes() == 0
    rc, again, rec2, _ = estimate(mods, codec, pps, d_src, offs, sizes)          # (and it comes back)
    assert rc == AEC_OK and again == bits and rec2.tobytes() == rec.tobytes()
    # the mirror in szgpu.py gives the same
    total, best, chunk_bits = codec.estimate(d_src, offs, sizes, pps)
    assert total == [int(v) for v in rec["total_bytes"]] and best == int(rec["best"]) and chunk_bits.tolist() == bits
    codec.close()


def test_an_empty_batch_and_refusals(mods):
    torch, gpu, szgpu, lib = mods
    codec = szgpu.SzCodec(sc.NN | sc.RAW, 16, 16, 100)
    d_src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rc, bits, rec, _ = estimate(mods, codec, [0, 100, 0, 100], d_src, [], [])
    assert rc == AEC_OK and bits == []
    assert [int(v) for v in rec["total_bytes"]] == [NOT_ASKED, 0, NOT_ASKED, 0] and (int(rec["best"]), int(rec["pad"])) == (1, 0)
    rc, _, rec, _ = estimate(mods, codec, None, d_src, [], [])                   # NULL scan lines: the SZ_com_t's for all four
    assert rc == AEC_OK and [int(v) for v in rec["total_bytes"]] == [0] * 4 and int(rec["best"]) == 0
    for pps, sizes in (([0] * 4, [200]), ([32769, 100, 100, 100], [200]), ([100] * 4, [200, 1, 200])):
        offs = [int(v) for v in np.cumsum([0] + sizes[:-1])]
        rc, _, _, (d_bits, d_est) = estimate(mods, codec, pps, d_src, offs, sizes)
        want = (torch.arange(GUARD, GUARD + 128, device="cuda") % 251).to(torch.uint8)      # (what guarded() fills in)
        assert rc == AEC_CONF_ERROR and torch.equal(d_bits, want[:d_bits.numel()]) and torch.equal(d_est, want[:40]), pps
    assert codec.held_bytes() == 0
    codec.close()
