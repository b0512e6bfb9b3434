#!/usr/bin/env python3
"""SZIP chunks of any size in one call (run on the GPU box): aec_gpu_sz_compress_chunks_async /
aec_gpu_sz_decompress_chunks_async beside, in the same run,
(a) the equal-chunk calls (aec_gpu_sz_compress_batch_async / aec_gpu_sz_decompress_batch_async) on the four shapes of
    tests/bench_sz_device.py, 64 chunks of 1 MiB -- the yardstick: the equal-chunk path of the same build;
(b) what a caller had to do before for 1024 float32 chunks of 4 .. 128 KiB and for 16 chunks of 8 MiB: one
    aec_gpu_sz_marshal_async per group of equal chunks, offset arrays, aec_gpu_encode_chunks_async; and one
    aec_gpu_sz_decompress_batch_async per group of equal chunks (the chunks of a group lie back to back for it).
Decompression is timed with the compress call's table and bare.  A device-to-device copy of the same bytes is printed
beside.  Device times are HIP events around 10 enqueues, best of 5 rounds."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_sz_device import CHUNK, N, NN, RAW, SHAPES, data_for, device_ms  # noqa: E402


def up16(v):
    return (v + 15) // 16 * 16


def line(what, ms, nbytes, note=""):
    print(f"  {what:<58}: {ms:8.3f} ms  {nbytes / 1e6 / ms:8.1f} GB/s  {note}")


class Chunks:
    """the new calls over chunks of `sizes` lying back to back in d_src"""

    def __init__(self, torch, gpu, codec, d_src, sizes):
        self.torch, self.gpu, self.codec, self.d_src = torch, gpu, codec, d_src
        self.sizes = np.asarray(sizes, dtype=np.uint64)
        self.offs = np.concatenate([[0], np.cumsum(self.sizes)[:-1]]).astype(np.uint64)
        n = self.sizes.size
        self.plan = plan = codec.chunks_plan(self.sizes)
        dev = dict(device="cuda")
        self.d_work = None if plan["direct"] else torch.empty(plan["work_bytes"], dtype=torch.uint8, **dev)
        self.d_out = torch.empty(plan["out_bound"], dtype=torch.uint8, **dev)
        self.d_rec = torch.zeros(n * 2, dtype=torch.int64, **dev)
        self.d_res = torch.zeros(24, dtype=torch.uint8, **dev)
        self.d_table = torch.zeros(plan["rsi_entries"], dtype=torch.int64, **dev)
        self.d_bare = torch.zeros(plan["rsi_entries"], dtype=torch.int64, **dev)
        self.d_dst = torch.empty(d_src.numel(), dtype=torch.uint8, **dev)
        self.d_results = torch.zeros(n * 40, dtype=torch.uint8, **dev)
        self.d_result = torch.zeros(40, dtype=torch.uint8, **dev)

    def compress(self):
        assert self.codec.compress_chunks_async(self.d_src, self.offs, self.sizes, self.d_work, self.d_out, self.d_out.numel(),
                                                self.d_rec, self.d_table, self.d_res) == 0

    def streams(self):
        rec = self.d_rec.cpu().numpy().view(np.uint64).reshape(-1, 2)
        self.in_offs = (rec[:, 0] // 8).astype(np.uint64)
        self.in_sizes = ((rec[:, 1] + 7) // 8).astype(np.uint64)
        out = self.d_out.cpu().numpy()
        return [out[int(o):int(o + k)] for o, k in zip(self.in_offs, self.in_sizes)]

    def decompress(self, have_table):
        assert self.codec.decompress_chunks_async(self.d_out, self.d_out.numel(), self.in_offs, self.in_sizes, self.offs,
                                                  self.sizes, self.d_table if have_table else self.d_bare, have_table,
                                                  self.d_work, self.d_dst, self.d_results, self.d_result) == 0

    def check(self):
        self.torch.cuda.synchronize()
        assert self.torch.equal(self.d_dst, self.d_src)
        assert not self.d_results.cpu().numpy().view(self.gpu.DEC_RESULT_DTYPE)["status"].any()
        self.d_dst.zero_()


def aligned_blob(torch, streams):
    offs = [0]
    for s in streams:
        offs.append(offs[-1] + up16(s.size))
    blob = np.zeros(offs[-1] + 16, dtype=np.uint8)
    for s, o in zip(streams, offs):
        blob[o:o + s.size] = s
    return torch.from_numpy(blob).cuda(), offs


def equal_shapes(torch, gpu, szgpu):
    print(f"(a) {N} equal chunks of {CHUNK >> 10} KiB: the equal-chunk calls and the chunk calls")
    for name, opts, bpp, ppb, pps in SHAPES:
        data = data_for(bpp)
        codec = szgpu.SzCodec(opts, bpp, ppb, pps)
        L = codec.layout(CHUNK)
        print(f" {name}")
        d_src = torch.from_numpy(data.copy()).cuda()
        total = N * CHUNK
        d_copy = torch.empty(total, dtype=torch.uint8, device="cuda")
        line("device copy", device_ms(torch, lambda: d_copy.copy_(d_src)), total)
        new = Chunks(torch, gpu, codec, d_src, [CHUNK] * N)
        t_new = device_ms(torch, new.compress)
        streams = new.streams()
        if codec.batch_ok(CHUNK, N):
            d_work = None if L.passthrough else torch.empty(N * L.coder_bytes, dtype=torch.uint8, device="cuda")
            d_out = torch.empty(codec.encode_bound(CHUNK) * N, dtype=torch.uint8, device="cuda")
            d_rec = torch.zeros(N * 2, dtype=torch.int64, device="cuda")
            d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
            t_old = device_ms(torch, lambda: codec.compress_batch_async(d_src, CHUNK, N, d_work, d_out, d_rec, d_res))
            rec = d_rec.cpu().numpy().reshape(N, 2)
            assert [int(n) for _, n in rec] == [int(n) for _, n in new.d_rec.cpu().numpy().reshape(N, 2)]
            line("aec_gpu_sz_compress_batch_async", t_old, total)
            line("aec_gpu_sz_compress_chunks_async (with the table)", t_new, total, f"({t_new / t_old:.2f} x)")
        else:
            line("aec_gpu_sz_compress_chunks_async (with the table)", t_new, total, "(the equal-chunk call refuses the batch)")
        d_in, offs = aligned_blob(torch, streams)
        d_offs = torch.tensor(offs, dtype=torch.int64, device="cuda")
        d_rsi = torch.zeros(N * L.lines, dtype=torch.int64, device="cuda")
        d_work = torch.empty(N * L.coder_bytes, dtype=torch.uint8, device="cuda")
        d_results = torch.zeros(N * 40, dtype=torch.uint8, device="cuda")
        d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")
        t_old = device_ms(torch, lambda: codec.decompress_batch_async(d_in, d_in.numel(), d_offs, N, CHUNK, d_rsi, d_work, new.d_dst,
                                                                      d_results, d_result))
        new.check()
        line("aec_gpu_sz_decompress_batch_async (index pass)", t_old, total)
        for have_table, what in ((1, "with the table"), (0, "bare: index pass")):
            t = device_ms(torch, lambda: new.decompress(have_table))
            new.check()
            line(f"aec_gpu_sz_decompress_chunks_async ({what})", t, total, f"({t / t_old:.2f} x)")
        codec.close()


def recipe(torch, gpu, szgpu, name, sizes, opts, bpp, ppb, pps):
    """chunks of `sizes` (sorted: the chunks of a size lie back to back, as the calls for equal chunks need them)"""
    sizes = sorted(int(s) for s in sizes)
    total = sum(sizes)
    rng = np.random.default_rng(len(sizes))
    data = np.cumsum(rng.standard_normal(total // 4)).astype("<f4").view(np.uint8)
    print(f" {name}: {len(sizes)} chunks, {total >> 20} MiB, {len(set(sizes))} sizes")
    d_src = torch.from_numpy(data.copy()).cuda()
    d_copy = torch.empty(total, dtype=torch.uint8, device="cuda")
    line("device copy", device_ms(torch, lambda: d_copy.copy_(d_src)), total)
    codec = szgpu.SzCodec(opts, bpp, ppb, pps)
    new = Chunks(torch, gpu, codec, d_src, sizes)
    # the recipe: groups of equal chunks, each with its layout, its place in the source and in the work buffer
    groups, at, work_at = [], 0, 0
    for s in sorted(set(sizes)):
        k = sizes.count(s)
        L = codec.layout(s)
        assert L.coder_bytes % 16 == 0
        groups.append(dict(size=s, n=k, src=at, work=work_at, L=L))
        at += k * s
        work_at += k * L.coder_bytes
    coder = gpu.Codec(*new.plan["coder"])
    d_work = torch.empty(work_at, dtype=torch.uint8, device="cuda")
    w_sizes = np.concatenate([[g["L"].coder_bytes] * g["n"] for g in groups]).astype(np.uint64)
    w_offs = np.concatenate([[0], np.cumsum(w_sizes)[:-1]]).astype(np.uint64)
    d_out = torch.empty(new.plan["out_bound"], dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(len(sizes) * 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")

    def marshal():
        for g in groups:
            if not g["L"].passthrough:
                assert codec.marshal_async(d_src[g["src"]:], g["size"], g["n"], d_work[g["work"]:]) == 0

    def old_compress():
        marshal()
        coder.encode_chunks_async(d_work, w_offs, w_sizes, d_out, d_out.numel(), d_rec, None, d_res)

    t_m = device_ms(torch, marshal)
    t_old = device_ms(torch, old_compress)
    t_new = device_ms(torch, new.compress)
    assert torch.equal(d_rec, new.d_rec), "the recipe's streams differ in length"
    streams = new.streams()
    line(f"{len(groups)} x aec_gpu_sz_marshal_async alone", t_m, total)
    line("... + aec_gpu_encode_chunks_async (the recipe)", t_old, total)
    line("aec_gpu_sz_compress_chunks_async (with the table)", t_new, total, f"({t_new / t_old:.2f} x)")
    # reading: one equal-chunk call per group
    d_in, offs = aligned_blob(torch, streams)
    c = 0
    for g in groups:
        g["d_offs"] = torch.tensor(offs[c:c + g["n"] + 1], dtype=torch.int64, device="cuda")
        g["d_rsi"] = torch.zeros(g["n"] * g["L"].lines, dtype=torch.int64, device="cuda")
        g["d_results"] = torch.zeros(g["n"] * 40, dtype=torch.uint8, device="cuda")
        c += g["n"]
    d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")

    def old_decompress():
        for g in groups:
            assert codec.decompress_batch_async(d_in, d_in.numel(), g["d_offs"], g["n"], g["size"], g["d_rsi"], d_work[g["work"]:],
                                                new.d_dst[g["src"]:], g["d_results"], d_result) == 0

    t_old = device_ms(torch, old_decompress)
    new.check()
    line(f"{len(groups)} x aec_gpu_sz_decompress_batch_async (index pass)", t_old, total)
    for have_table, what in ((1, "with the table"), (0, "bare: index pass")):
        t = device_ms(torch, lambda: new.decompress(have_table))
        new.check()
        line(f"aec_gpu_sz_decompress_chunks_async ({what})", t, total, f"({t / t_old:.2f} x)")
    codec.close()


def main():
    import torch
    from libaec_amd import gpu, szgpu
    equal_shapes(torch, gpu, szgpu)
    print("(b) what a caller had to do before, and the one call")
    rng = np.random.default_rng(1024)
    recipe(torch, gpu, szgpu, "float32, 32 / 16 / 1024, 4 .. 128 KiB", 4096 * rng.integers(1, 33, size=1024), NN | RAW, 32, 16, 1024)
    recipe(torch, gpu, szgpu, "float32, 32 / 16 / 1024, 8 MiB", [8 << 20] * 16, NN | RAW, 32, 16, 1024)


if __name__ == "__main__":
    main()
