#!/usr/bin/env python3
"""Batches of unequal chunks decoded on the device (run on the GPU box): aec_gpu_decode_chunks_async beside the calls that
served such a batch before it, on the same streams in the same process, the calls taking turns round by round:
  with the table   one call, one decode launch            against  aec_gpu_decode_async chunk by chunk (the loop is
                                                                   issued from Python: its time is largely the host's)
  bare streams     one walker launch + one decode launch  against  aec_gpu_decode_batch_async with every chunk padded
                                                                   to the largest (streams moved to 16-byte offsets)
The streams and the table come from aec_gpu_encode_chunks_async; every way's output is compared with the data that was
encoded before anything is timed.  Times are HIP events around 5 enqueues, 7 rounds: best, median and worst per call."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PP = 8
C2, C5 = (16, 16, 128, PP), (8, 8, 128, PP)
KIB, MIB = 1 << 10, 1 << 20


def rows():
    rng = np.random.default_rng(7)
    out = []
    for cname, prm in (("config 5", C5), ("config 2", C2)):
        out += [(f"1024 unequal chunks of 4 to 128 KiB ({cname})", prm, (rng.integers(4 * KIB, 128 * KIB + 1, size=1024) // 2 * 2).tolist()),
                (f"64 x 1 MiB equal ({cname})", prm, [MIB] * 64),
                (f"4000 unequal chunks of 16 bytes to 4 KiB ({cname})", prm, (rng.integers(16, 4 * KIB, size=4000) // 2 * 2).tolist()),
                (f"16 unequal chunks of 4 to 128 KiB ({cname})", prm, (rng.integers(4 * KIB, 128 * KIB + 1, size=16) // 2 * 2).tolist())]
    return out


def alternating_ms(torch, fns, calls=5, rounds=7):
    """(best, median, worst) time per call of every function; a round times each of them once, one after the other"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[j].append(a.elapsed_time(b) / calls)
    return [(min(t), float(np.median(t)), max(t)) for t in times]


def main():
    import torch
    from test_gpu_parity import gen
    from libaec_amd import gpu
    lib = gpu._lib()
    u64, vp = C.c_uint64, C.c_void_p
    lib.aec_gpu_decode_batch_async.restype = C.c_int
    lib.aec_gpu_decode_batch_async.argtypes = [vp, C.POINTER(gpu.Params), vp, C.c_size_t, vp, u64, u64, vp, vp, vp, vp, vp]
    missed = []
    for name, prm, sizes in rows():
        n = len(sizes)
        nb = 2 if prm[0] > 8 else 1
        blk, rsi_b = prm[1] * nb, prm[1] * nb * prm[2]
        sizes_a = np.array(sizes, dtype=np.uint64)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum((sizes_a + 15) // 16 * 16)
        data = gen(2 if prm[0] == 8 else 0, int(offsets[n]) + 64)
        d_in = torch.from_numpy(data).cuda()
        codec = gpu.Codec(*prm)
        starts = np.ascontiguousarray(offsets[:n])
        d_enc, rec, d_tab, res = codec.encode_chunks(d_in, starts, sizes_a, want_offsets=True)
        assert not int(res["overflow"])
        enc_bytes = int(res["total_bits"]) // 8
        total = int(sizes_a.sum())
        blocks = (sizes_a // nb + prm[1] - 1) // prm[1]
        rsis = (blocks + prm[2] - 1) // prm[2]
        entry0 = np.zeros(n, dtype=np.uint64)
        entry0[1:] = np.cumsum(rsis[:-1] + 1)
        plan = codec.decode_chunks_plan(sizes_a)
        out_off = np.zeros(n, dtype=np.uint64)
        out_off[1:] = np.cumsum((blocks[:-1] * blk + 15) // 16 * 16)
        st = codec._stream(None)
        want = [data[int(offsets[i]):int(offsets[i]) + sizes[i]] for i in range(n)]

        def same(d_out, at):
            out = d_out.cpu().numpy()
            return all(np.array_equal(out[int(at[i]):int(at[i]) + sizes[i]], want[i]) for i in range(n))

        # ---- with the table
        d_out = torch.zeros(plan["out_bytes"] + 16, dtype=torch.uint8, device="cuda")
        d_rec = torch.zeros(40 * n, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")

        def table_call():
            assert codec.decode_chunks_async(d_enc, enc_bytes, None, None, out_off, sizes_a, d_tab, 1, d_out, d_rec, d_res) == 0

        d_out_loop = torch.zeros(plan["out_bytes"] + 16, dtype=torch.uint8, device="cuda")
        d_res_loop = torch.zeros(40 * n, dtype=torch.uint8, device="cuda")
        loop_args = [(d_tab.data_ptr() + 8 * int(entry0[i]), int(rsis[i]), int(blocks[i]), d_out_loop.data_ptr() + int(out_off[i]),
                      d_res_loop.data_ptr() + 40 * i) for i in range(n)]

        def loop_fn():
            for tab, r, b, out, rs in loop_args:
                assert lib.aec_gpu_decode_async(codec.ctx, C.byref(codec.p), d_enc.data_ptr(), enc_bytes, tab, r, b, out, rs, st) == 0

        # ---- bare streams
        in_off = np.ascontiguousarray(rec[:, 0] // 8).astype(np.uint64)
        in_len = np.maximum((rec[:, 1] + 7) // 8, 1).astype(np.uint64)
        d_tab_bare = torch.zeros(plan["rsi_entries"], dtype=torch.int64, device="cuda")
        d_out_bare = torch.zeros(plan["out_bytes"] + 16, dtype=torch.uint8, device="cuda")

        def bare_call():
            assert codec.decode_chunks_async(d_enc, enc_bytes, in_off, in_len, out_off, sizes_a, d_tab_bare, 0, d_out_bare, d_rec, d_res) == 0

        # (the batch call wants streams at multiples of 16 and pads every chunk to the RSIs of the largest)
        enc = d_enc.cpu().numpy()
        choff = np.zeros(n + 1, dtype=np.int64)
        choff[1:] = np.cumsum((in_len.astype(np.int64) + 15) // 16 * 16 + 16)
        blob = np.zeros(int(choff[n]) + 16, dtype=np.uint8)
        for i in range(n):
            blob[choff[i]:choff[i] + int(in_len[i])] = enc[int(in_off[i]):int(in_off[i] + in_len[i])]
        rpc = int(rsis.max())
        d_blob, d_choff = torch.from_numpy(blob).cuda(), torch.from_numpy(choff).cuda()
        d_tab_old = torch.zeros(n * rpc, dtype=torch.int64, device="cuda")
        d_out_old = torch.zeros(n * rpc * rsi_b + 16, dtype=torch.uint8, device="cuda")
        d_rec_old = torch.zeros(40 * n, dtype=torch.uint8, device="cuda")
        codec_old = gpu.Codec(*prm)

        def batch_fn():
            assert lib.aec_gpu_decode_batch_async(codec_old.ctx, C.byref(codec_old.p), d_blob.data_ptr(), int(choff[n]), d_choff.data_ptr(),
                                                  n, rpc, d_tab_old.data_ptr(), d_out_old.data_ptr(), d_rec_old.data_ptr(),
                                                  d_res.data_ptr(), st) == 0

        for fn in (table_call, loop_fn, bare_call, batch_fn):
            fn()
        torch.cuda.synchronize()
        assert same(d_out, out_off) and same(d_out_loop, out_off) and same(d_out_bare, out_off), name
        assert same(d_out_old, np.arange(n, dtype=np.uint64) * np.uint64(rpc * rsi_b)), name
        t = alternating_ms(torch, [table_call, loop_fn, bare_call, batch_fn])
        print(f"{name}: {n} chunks, {total / MIB:.1f} MiB decoded, {enc_bytes / MIB:.1f} MiB coded, {plan['items']} items")
        labels = ["with the table: one launch (chunks)", "with the table: chunk by chunk", "bare: walk + one launch (chunks)",
                  "bare: padded to the largest (batch)"]
        mem = [plan["out_bytes"], plan["out_bytes"], plan["out_bytes"], n * rpc * rsi_b]
        for label, (lo, med, hi), m in zip(labels, t, mem):
            print(f"  {label:38s}: best {lo:9.3f}  median {med:9.3f}  worst {hi:9.3f} ms  {total / 1e6 / lo:8.1f} GB/s  output {m / MIB:8.1f} MiB")
        print(f"  chunk by chunk / one launch            : {t[1][0] / t[0][0]:9.1f} x        padded batch / chunks (bare): {t[3][0] / t[2][0]:6.2f} x")
        # the expectation: with 16 chunks or more the one launch is not slower than the loop beyond the spread of the loop's repeats
        if n >= 16 and t[0][1] > t[1][1] + (t[1][2] - t[1][0]):
            missed.append(name)
            print("  MISSED: the one launch is slower than the loop beyond the spread of the loop's repeats")
        codec.close()
        codec_old.close()
        del d_in, d_enc, d_out, d_out_loop, d_out_bare, d_out_old, d_blob
    print("rows that miss the expectation: " + (", ".join(missed) if missed else "none"))


if __name__ == "__main__":
    main()
