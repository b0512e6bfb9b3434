#!/usr/bin/env python3
"""aec_gpu_sz_estimate_async with pixels per block 8, 16 and 32 asked beside what a caller had to do before: one
aec_gpu_sz_compress_chunks_async per candidate on the same device buffers (run on the GPU box).  Shapes, those of
tests/bench_sz_chunks_device.py: 64 float32 chunks of 1 MiB (NN, 1024 pixels per line), 1024 float32 chunks of 4 .. 128 KiB,
64 chunks of 1 MiB of 16-bit pixels (1000 pixels per line).  Device times are HIP events around 10 enqueues, 5 rounds: the
best round, and the spread (slowest - best) beside it; a device-to-device copy of the same bytes is printed beside.

  bench_sz_estimate.py --json before.jsonl              with AEC_AMD_LIB=<a build from before the call>: the compress leg alone
  bench_sz_estimate.py --against before.jsonl           the shipped build: both legs, and the ratio to the recorded leg
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_estimate import line, rounds_ms  # noqa: E402
from bench_sz_device import CHUNK, N, NN, RAW, data_for  # noqa: E402

ASKED = (0, 1, 2)                   # pixels per block 8, 16, 32


def shapes():
    rng = np.random.default_rng(1024)
    small = sorted(int(s) for s in 4096 * rng.integers(1, 33, size=1024))
    walk = np.cumsum(np.random.default_rng(len(small)).standard_normal(sum(small) // 4)).astype("<f4").view(np.uint8)
    yield "64 x 1 MiB float32, 1024 a line", NN | RAW, 32, 1024, [CHUNK] * N, data_for(32)
    yield "1024 x 4..128 KiB float32, 1024 a line", NN | RAW, 32, 1024, small, walk
    yield "64 x 1 MiB 16-bit, 1000 a line", NN | RAW, 16, 1000, [CHUNK] * N, data_for(16)


def main():
    import torch
    from libaec_amd import gpu, szgpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", help="append one JSON line per shape here")
    ap.add_argument("--against", help="JSON lines of an earlier run (the compress leg of another build) to compare with")
    args = ap.parse_args()
    before = {}
    if args.against:
        for ln in open(args.against):
            r = json.loads(ln)
            before[r["shape"]] = r
    have = hasattr(gpu._lib(), "aec_gpu_sz_estimate_async")
    print(f"library: {gpu._lib()._name}; estimate call: {'yes' if have else 'no (compress leg only)'}")
    for name, opts, bpp, pps, sizes, data in shapes():
        total = sum(sizes)
        sizes = np.asarray(sizes, dtype=np.uint64)
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
        d_src = torch.from_numpy(data[:total].copy()).cuda()
        d_copy = torch.empty_like(d_src)
        legs = []
        for i in ASKED:
            codec = szgpu.SzCodec(opts, bpp, 8 << i, pps)
            plan = codec.chunks_plan(sizes)
            legs.append(dict(codec=codec, d_work=torch.empty(plan["work_bytes"] + 16, dtype=torch.uint8, device="cuda"),
                             d_out=torch.empty(plan["out_bound"], dtype=torch.uint8, device="cuda"),
                             d_rec=torch.zeros(sizes.size * 2, dtype=torch.int64, device="cuda"),
                             d_res=torch.zeros(24, dtype=torch.uint8, device="cuda")))

        def compresses():
            for g in legs:
                assert g["codec"].compress_chunks_async(d_src, offs, sizes, g["d_work"], g["d_out"], g["d_out"].numel(), g["d_rec"],
                                                        None, g["d_res"]) == 0

        print(f" {name}, {total >> 20} MiB")
        t_copy = rounds_ms(torch, lambda: d_copy.copy_(d_src))
        line("device copy", t_copy, total)
        t_old = rounds_ms(torch, compresses)
        line("3 x aec_gpu_sz_compress_chunks_async (8, 16, 32)", t_old, total)
        bits = [[int(v) for v in g["d_rec"].cpu().numpy().view(np.uint64).reshape(-1, 2)[:, 1]] for g in legs]
        nbytes = [sum(max(1, (b + 7) // 8) for b in row) for row in bits]
        rec = {"shape": name, "copy_ms": t_copy, "compress_ms": t_old, "total_bytes": nbytes}
        if have:
            codec = legs[0]["codec"]
            vec = [pps, pps, pps, 0]
            d_bits = torch.zeros(sizes.size * 4, dtype=torch.int64, device="cuda")
            d_est = torch.zeros(40, dtype=torch.uint8, device="cuda")
            t_est = rounds_ms(torch, lambda: codec.estimate_async(d_src, offs, sizes, d_bits, d_est, vec))
            e = d_est.cpu().numpy().view(szgpu.SZ_ESTIMATE_DTYPE)[0]
            got = d_bits.cpu().numpy().view(np.uint64).reshape(-1, 4)
            assert all([int(v) for v in got[:, i]] == bits[i] for i in ASKED), "the estimate differs from the compress calls"
            assert [int(v) for v in e["total_bytes"][:3]] == nbytes
            line("aec_gpu_sz_estimate_async (8, 16, 32)", t_est, total, f"({min(t_old) / min(t_est):.2f} x the compress calls of this build)")
            rec["estimate_ms"] = t_est
            rec["best"] = int(e["best"])
            if name in before:
                b = before[name]
                assert b["total_bytes"] == nbytes, "the recorded compress leg saw other data"
                spread = max(max(b["compress_ms"]) - min(b["compress_ms"]), max(t_est) - min(t_est))
                gain = min(b["compress_ms"]) - min(t_est)
                print(f"  against the recorded compress leg {min(b['compress_ms']):.3f} ms (+{max(b['compress_ms']) - min(b['compress_ms']):.3f}): "
                      f"{min(b['compress_ms']) / min(t_est):.2f} x faster, {gain:.3f} ms against a spread of {spread:.3f} ms "
                      f"-> {'faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'}", flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps(rec) + "\n")
        for g in legs:
            g["codec"].close()
        del d_src, d_copy, legs


if __name__ == "__main__":
    main()
