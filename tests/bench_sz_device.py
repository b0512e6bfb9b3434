#!/usr/bin/env python3
"""SZIP chunks that stay on the device (run on the GPU box): 64 chunks of 1 MiB in four shapes through
(a) aec_gpu_sz_marshal_async / aec_gpu_sz_unmarshal_async alone, next to a device-to-device copy of the same byte count
    in the same run (what a pure data-movement kernel has to be compared with),
(b) aec_gpu_sz_compress_batch_async / aec_gpu_sz_decompress_batch_async, device buffers in and out, next to
    SZ_BatchCompress / SZ_BatchDecompress on host buffers for the same chunks (tests/bench_sz_chunks.py's calls).
Device times are HIP events around 10 enqueues, best of 5 rounds; host-buffer times are wall clock of the call, best of 6."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, CHUNK = 64, 1 << 20
MSB, NN, RAW = 16, 32, 128
SHAPES = [("8 bpp / 8 / 1024 (passthrough)", NN | RAW, 8, 8, 1024),
          ("32 bpp / 16 / 1024 (planes)", NN | RAW, 32, 16, 1024),
          ("64 bpp / 8 / 1024 (planes)", NN | RAW, 64, 8, 1024),
          ("16 bpp / 16 / 1000 (padded lines)", NN | RAW, 16, 16, 1000)]


def data_for(bpp):
    from test_gpu_parity import gen
    if bpp == 8:
        return gen(2, N * CHUNK)
    if bpp == 16:
        return gen(0, N * CHUNK)
    rng = np.random.default_rng(bpp)
    x = np.cumsum(rng.standard_normal(N * CHUNK * 8 // bpp))
    return x.astype("<f4" if bpp == 32 else "<f8").view(np.uint8)


def device_ms(torch, fn, calls=10, rounds=5):
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b) / calls
        best = t if best is None or t < best else best
    return best


def main():
    import torch
    from libaec_amd import gpu, szgpu, szip
    for name, opts, bpp, ppb, pps in SHAPES:
        data = data_for(bpp)
        chunks = [data[i * CHUNK:(i + 1) * CHUNK] for i in range(N)]
        codec = szgpu.SzCodec(opts, bpp, ppb, pps)
        L = codec.layout(CHUNK)
        one_call = bool(codec.batch_ok(CHUNK, N))
        gb = N * CHUNK / 1e9
        print(f"{name}: {N} x {CHUNK >> 10} KiB, coder input {L.coder_bytes} bytes per chunk")
        d_src = torch.from_numpy(data.copy()).cuda()
        d_work = torch.empty(N * L.coder_bytes, dtype=torch.uint8, device="cuda")
        d_dst = torch.empty(N * CHUNK, dtype=torch.uint8, device="cuda")
        d_copy = torch.empty(N * L.coder_bytes, dtype=torch.uint8, device="cuda")
        # (a) data movement alone
        t_copy = device_ms(torch, lambda: d_copy[:N * CHUNK].copy_(d_src))
        t_m = device_ms(torch, lambda: codec.marshal_async(d_src, CHUNK, N, d_work))
        t_u = device_ms(torch, lambda: codec.unmarshal_async(d_work, CHUNK, N, d_dst))
        torch.cuda.synchronize()
        assert torch.equal(d_dst, d_src)
        print(f"  device copy of {N * CHUNK >> 20} MiB             : {t_copy:8.3f} ms  {gb / t_copy * 1e3:8.1f} GB/s")
        print(f"  marshal                           : {t_m:8.3f} ms  {gb / t_m * 1e3:8.1f} GB/s  ({t_m / t_copy:.2f} x the copy)")
        print(f"  un-marshal                        : {t_u:8.3f} ms  {gb / t_u * 1e3:8.1f} GB/s  ({t_u / t_copy:.2f} x the copy)")
        # (b) the one-call forms
        slot = codec.encode_bound(CHUNK)
        d_out = torch.empty(slot * N, dtype=torch.uint8, device="cuda")
        d_rec = torch.zeros(N * 2, dtype=torch.int64, device="cuda")
        d_res = torch.zeros(24 * N, dtype=torch.uint8, device="cuda")
        work = None if L.passthrough else d_work

        def comp():
            if one_call:
                assert codec.compress_batch_async(d_src, CHUNK, N, work, d_out, d_rec, d_res) == 0
            else:       # (aec_gpu_sz_batch_ok says no: marshal, then the encoder chunk by chunk)
                assert codec.marshal_async(d_src, CHUNK, N, d_work) == 0
                assert codec.encode_chunks_async(d_work, L.coder_bytes, N, d_out, slot, d_res) == 0
        t_c = device_ms(torch, comp)
        out = d_out.cpu().numpy()
        if one_call:
            rec = d_rec.cpu().numpy().reshape(N, 2)
            streams = [out[int(b) // 8:int(b) // 8 + (int(n) + 7) // 8] for b, n in rec]
        else:
            res = d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)
            streams = [out[i * slot:i * slot + (int(res[i]["total_bits"]) + 7) // 8] for i in range(N)]
        offs = [0]
        for s in streams:
            offs.append(offs[-1] + (s.size + 15) // 16 * 16)
        blob = np.zeros(offs[-1] + 16, dtype=np.uint8)
        for s, o in zip(streams, offs):
            blob[o:o + s.size] = s
        d_in = torch.from_numpy(blob).cuda()
        d_offs = torch.tensor(offs, dtype=torch.int64, device="cuda")
        d_rsi = torch.zeros(N * L.lines, dtype=torch.int64, device="cuda")
        d_results = torch.zeros(N * 40, dtype=torch.uint8, device="cuda")
        d_result = torch.zeros(40, dtype=torch.uint8, device="cuda")

        def decomp():
            assert codec.decompress_batch_async(d_in, blob.size, d_offs, N, CHUNK, d_rsi, d_work, d_dst, d_results, d_result) == 0
        t_d = device_ms(torch, decomp)
        assert torch.equal(d_dst, d_src) and not d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)["status"].any()
        ratio = N * CHUNK / sum(s.size for s in streams)
        how = "aec_gpu_sz_compress_batch_async  " if one_call else "marshal + encode chunk by chunk  "
        print(f"  {how} : {t_c:8.3f} ms  {gb / t_c * 1e3:8.1f} GB/s  (ratio {ratio:.2f})")
        print(f"  aec_gpu_sz_decompress_batch_async : {t_d:8.3f} ms  {gb / t_d * 1e3:8.1f} GB/s")
        # the host-buffer batch calls on the same chunks
        best_c = best_d = None
        for _ in range(6):
            t0 = time.perf_counter()
            rc, enc, st = szip.compress_batch(chunks, [CHUNK * 2] * N, opts, bpp, ppb, pps)
            t = time.perf_counter() - t0
            assert rc == 0
            best_c = t if best_c is None or t < best_c else best_c
        assert all(e == s.tobytes() for e, s in zip(enc, streams))
        for _ in range(6):
            t0 = time.perf_counter()
            rc, dec, st = szip.decompress_batch(enc, [CHUNK] * N, opts, bpp, ppb, pps)
            t = time.perf_counter() - t0
            assert rc == 0
            best_d = t if best_d is None or t < best_d else best_d
        print(f"  SZ_BatchCompress   (host buffers, incl. the wrapper's copies) : {best_c * 1e3:8.2f} ms  {gb / best_c:7.2f} GB/s")
        print(f"  SZ_BatchDecompress (host buffers, incl. the wrapper's copies) : {best_d * 1e3:8.2f} ms  {gb / best_d:7.2f} GB/s")
        codec.close()


if __name__ == "__main__":
    main()
