#!/usr/bin/env python3
"""Batches of chunks on the device (run on the GPU box): aec_gpu_encode_chunks_async, one launch set for any batch, beside
aec_gpu_encode_batch_async, the same chunks one after the other, on the same inputs in the same process, alternating; on
the rows aec_gpu_encode_uniform_batch_async takes, that call as well.  Device buffers in and out; times are HIP events
around 10 enqueues, best of 5 rounds, the calls taking turns round by round.  The last row is the 1024-chunk batch through
aec_buffer_encode_batch on host buffers (wall clock, best of 6), whose trace names the path it took."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PP = 8
C2, C5 = (16, 16, 128, PP), (8, 8, 128, PP)
KIB, MIB = 1 << 10, 1 << 20


def rows():
    rng = np.random.default_rng(7)
    return [("64 x 1 MiB equal (config 5)", C5, [MIB] * 64),
            ("1024 unequal chunks of 4 to 128 KiB (config 5)", C5, rng.integers(4 * KIB, 128 * KIB + 1, size=1024).tolist()),
            ("256 unequal chunks of 4 KiB to 1 MiB (config 5)", C5, rng.integers(4 * KIB, MIB + 1, size=256).tolist()),
            ("16 x 8 MiB (config 5: 16384 segments per chunk)", C5, [8 * MIB] * 16),
            ("64 x 1 000 000 bytes (config 2: no whole RSIs)", C2, [1000000] * 64)]


def alternating_ms(torch, fns, calls=10, rounds=5):
    """best time per call of every function; a round times each of them once, one after the other"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    best = [None] * len(fns)
    for _ in range(rounds):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            t = a.elapsed_time(b) / calls
            best[j] = t if best[j] is None or t < best[j] else best[j]
    return best


def main():
    import torch
    from test_gpu_parity import gen
    from fuzz_batch_gpu import batch
    from libaec_amd import api, gpu
    lib = gpu._lib()
    u64 = C.c_uint64
    loop_call = lib.aec_gpu_encode_batch_async
    loop_call.restype = C.c_int
    loop_call.argtypes = [C.c_void_p, C.POINTER(gpu.Params), C.c_void_p, C.POINTER(u64), u64, C.c_void_p, C.c_size_t, C.c_void_p,
                          C.c_void_p]
    host_row = None
    for name, prm, sizes in rows():
        n = len(sizes)
        sizes_a = np.array(sizes, dtype=np.uint64)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum((sizes_a + 15) // 16 * 16)
        data = gen(2 if prm[0] == 8 else 0, int(offsets[n]) + 64)
        d_in = torch.from_numpy(data).cuda()
        codec = gpu.Codec(*prm)
        plan = codec.encode_chunks_plan(sizes_a)
        total = int(sizes_a.sum())
        d_out = torch.empty(plan["out_bound"], dtype=torch.uint8, device="cuda")
        d_rec = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
        d_res = torch.zeros(24, dtype=torch.uint8, device="cuda")
        starts = np.ascontiguousarray(offsets[:n])

        def chunks_call():
            codec.encode_chunks_async(d_in, starts, sizes_a, d_out, plan["out_bound"], d_rec, None, d_res)

        # chunk by chunk: slots for the largest chunk; chunk i = [offsets[i], offsets[i] + sizes[i]) as a pair of its own
        slot = (codec.encode_bound(int(sizes_a.max())) + 15) // 16 * 16
        d_slots = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
        d_results = torch.zeros(24 * n, dtype=torch.uint8, device="cuda")
        pairs = [(u64 * 2)(int(offsets[i]), int(offsets[i]) + int(sizes_a[i])) for i in range(n)]
        st = codec._stream(None)

        def loop_fn():
            for i in range(n):
                rc = loop_call(codec.ctx, C.byref(codec.p), d_in.data_ptr(), pairs[i], 1, d_slots.data_ptr() + i * slot, slot,
                               d_results.data_ptr() + 24 * i, st)
                assert rc == 0

        fns, labels = [chunks_call, loop_fn], ["one launch set (chunks)", "chunk by chunk"]
        equal = len(set(sizes)) == 1
        if equal and lib.aec_gpu_uniform_batch_ok(C.byref(codec.p), sizes[0], n):
            d_uin = torch.from_numpy(np.ascontiguousarray(data[:total])).cuda()
            cap = (codec.encode_bound(sizes[0]) + 15) // 16 * 16 * n
            d_uout = torch.empty(cap, dtype=torch.uint8, device="cuda")

            def uniform_fn():
                rc = lib.aec_gpu_encode_uniform_batch_async(codec.ctx, C.byref(codec.p), d_uin.data_ptr(), sizes[0], n,
                                                            d_uout.data_ptr(), cap, d_rec.data_ptr(), d_res.data_ptr(), st)
                assert rc == 0
            fns.append(uniform_fn)
            labels.append("one launch set (uniform)")
        # the two ways give the same streams
        chunks_call()
        rec = d_rec.cpu().numpy().reshape(n, 2).copy()
        loop_fn()
        res = d_results.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)
        out, slots = d_out.cpu().numpy(), d_slots.cpu().numpy()
        for i in range(n):
            nbytes = (int(rec[i][1]) + 7) // 8
            assert int(res[i]["total_bits"]) == int(rec[i][1])
            assert np.array_equal(out[int(rec[i][0]) // 8:int(rec[i][0]) // 8 + nbytes], slots[i * slot:i * slot + nbytes]), (name, i)
        best = alternating_ms(torch, fns)
        print(f"{name}: {n} chunks, {total / MIB:.1f} MiB, {plan['waves']} waves")
        for label, t in zip(labels, best):
            print(f"  {label:28s}: {t:9.3f} ms  {total / 1e6 / t:8.1f} GB/s")
        print(f"  chunk by chunk / chunks      : {best[1] / best[0]:9.1f} x")
        if n == 1024:
            host_row = (name, prm, [np.ascontiguousarray(data[int(offsets[i]):int(offsets[i]) + sizes[i]]) for i in range(n)], total)
        codec.close()
        del d_in, d_out, d_slots
    name, prm, chunks, total = host_row
    caps = [c.size + c.size // 2 + 256 for c in chunks]
    alib = api.library()
    best = None
    for _ in range(6):
        t0 = time.perf_counter()
        rc, got, st = batch(alib, "aec_buffer_encode_batch", prm, chunks, caps)
        t = (time.perf_counter() - t0) * 1e3
        assert rc == 0
        best = t if best is None or t < best else best
    print(f"{name} through aec_buffer_encode_batch on host buffers: {best:9.3f} ms  {total / 1e6 / best:8.1f} GB/s (wall clock)")


if __name__ == "__main__":
    main()
