#!/usr/bin/env python3
"""aec_gpu_estimate_async of all four block sizes beside what a caller had to do before: four
aec_gpu_encode_plan_async calls, block sizes 8, 16, 32 and 64, on the same device buffer (run on the GPU box).
Shapes: 256 MiB of bench.py's config 2 (16-bit, rsi 128), config 5 (8-bit, rsi 128) and config 3 (32-bit, rsi 4096) data.
Device times are HIP events around 10 enqueues, 5 rounds: the best round, and the spread (slowest - best) beside it; a
device-to-device copy of the same bytes is printed beside.

  bench_estimate.py --json plans.jsonl                 with AEC_AMD_LIB=<a build from before the call>: the plan leg alone
  bench_estimate.py --against plans.jsonl              the shipped build: both legs, and the ratio to the recorded plan leg
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

SHAPES = [("c2 16-bit rsi 128", "c2"), ("c5 8-bit rsi 128", "c5"), ("c3 32-bit rsi 4096", "c3")]


def rounds_ms(torch, fn, calls=10, rounds=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def line(what, ms, nbytes, note=""):
    print(f"  {what:<50}: {min(ms):8.3f} ms (+{max(ms) - min(ms):.3f})  {nbytes / 1e6 / min(ms):8.1f} GB/s  {note}", flush=True)


def main():
    import ctypes as C

    import torch
    from libaec_amd import gpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--json", help="append one JSON line per shape here")
    ap.add_argument("--against", help="JSON lines of an earlier run (the plan leg of another build) to compare with")
    args = ap.parse_args()
    before = {}
    if args.against:
        for ln in open(args.against):
            r = json.loads(ln)
            before[r["shape"]] = r
    nbytes = args.mib << 20
    have = hasattr(gpu._lib(), "aec_gpu_estimate_async")
    print(f"library: {gpu._lib()._name}; estimate call: {'yes' if have else 'no (plan leg only)'}")
    for name, cfg in SHAPES:
        _, kind, bps, _, rsi, flags = bench.CONFIGS[cfg]
        data = bench.generate(kind, nbytes, 0, 16)
        d_in = torch.from_numpy(data).cuda()
        d_copy = torch.empty_like(d_in)
        codec = gpu.Codec(bps, 16, rsi, flags)
        d_plan = torch.zeros(4 * 24, dtype=torch.uint8, device="cuda").view(4, 24)
        prm = [gpu.Params(bps, 8 << i, rsi, flags) for i in range(4)]
        st = codec._stream(None)

        def plans():
            for i in range(4):
                rc = codec.lib.aec_gpu_encode_plan_async(codec.ctx, C.byref(prm[i]), d_in.data_ptr(), nbytes, d_plan[i].data_ptr(), st)
                assert rc == 0

        print(f" {name}, {args.mib} MiB")
        t_copy = rounds_ms(torch, lambda: d_copy.copy_(d_in))
        line("device copy", t_copy, nbytes)
        t_plan = rounds_ms(torch, plans)
        line("4 x aec_gpu_encode_plan_async (8, 16, 32, 64)", t_plan, nbytes)
        bits = [int(v) for v in d_plan.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)["total_bits"].reshape(-1)]
        rec = {"shape": name, "mib": args.mib, "copy_ms": t_copy, "plan_ms": t_plan, "total_bits": bits}
        if have:
            d_est = torch.zeros(40, dtype=torch.uint8, device="cuda")
            t_est = rounds_ms(torch, lambda: codec.estimate_async(d_in, nbytes, None, d_est))
            e = d_est.cpu().numpy().view(gpu.ESTIMATE_DTYPE)[0]
            assert [int(v) for v in e["total_bits"]] == bits, "the estimate differs from the plan calls"
            line("aec_gpu_estimate_async (all four)", t_est, nbytes, f"({min(t_plan) / min(t_est):.2f} x the plans of this build)")
            rec["estimate_ms"] = t_est
            rec["best"] = int(e["best"])
            if name in before:
                b = before[name]
                assert b["total_bits"] == bits, "the recorded plan leg saw other data"
                spread = max(max(b["plan_ms"]) - min(b["plan_ms"]), max(t_est) - min(t_est))
                gain = min(b["plan_ms"]) - min(t_est)
                print(f"  against the recorded plan leg {min(b['plan_ms']):.3f} ms (+{max(b['plan_ms']) - min(b['plan_ms']):.3f}): "
                      f"{min(b['plan_ms']) / min(t_est):.2f} x faster, {gain:.3f} ms against a spread of {spread:.3f} ms "
                      f"-> {'faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'}", flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps(rec) + "\n")
        codec.close()
        del d_in, d_copy


if __name__ == "__main__":
    main()
