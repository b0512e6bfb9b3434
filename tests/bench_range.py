#!/usr/bin/env python3
"""Random access through the libaec ABI (aec_decode_range with the encoder's RSI offsets) against the bare one-shot
decode, for BASELINE configurations 2, 3 and 5 at 1 GiB; one JSON line per configuration:
  bare_decode_gbs      aec_buffer_decode of the bare stream (index pass included), GB/s of decoded output
  range_all_gbs        aec_decode_range(0, everything) with the encoder's offsets, GB/s of decoded output
  sample_ms_median     median latency of 1000 single-sample ranges at random positions
  range4k_ms_median    the same for 4 KiB ranges
  bare64k_ms_median    aec_buffer_decode with avail_out = 65536 (the first 64 KiB of output; the input: the stream
                       bytes of the RSIs those lie in) -- the yardstick of the single-sample latency

    python tests/bench_range.py [--size-mib 1024] [--configs c2,c3,c5] [--reps 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c2": (0, 16, 16, 128, 8), "c3": (1, 32, 32, 4096, 8 | 4 | 1), "c5": (2, 8, 8, 128, 8)}


def gen(kind, nbytes):
    lib = C.CDLL(os.path.join(ROOT, "libaec_amd", "lib", "libaec_datagen.so"))
    a = np.empty(nbytes, dtype=np.uint8)
    lib.aec_gen_fill_parallel(C.c_uint(kind), C.c_uint64(0), C.c_void_p(a.ctypes.data),
                              C.c_size_t(nbytes // {0: 2, 1: 4, 2: 1}[kind]), C.c_uint(8))
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=int, default=1024)
    ap.add_argument("--configs", default="c2,c3,c5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ranges", type=int, default=1000)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available()
    from libaec_amd import api
    lib = api.library()
    for name in args.configs.split(","):
        kind, bps, bs, rsi, flags = CONFIGS[name]
        data = gen(kind, args.size_mib << 20)
        rc, enc, offs = api.encode_with_offsets(data, bps, bs, rsi, flags)
        assert rc == api.AEC_OK
        ea = np.frombuffer(enc, dtype=np.uint8)
        out = np.empty(data.size, dtype=np.uint8)
        out[::4096] = 0                                           # (pages touched before timing)

        def bare(n_out, src=ea):
            s = api.AecStream()
            s.next_in, s.avail_in = src.ctypes.data, src.size
            s.next_out, s.avail_out = out.ctypes.data, n_out
            s.bits_per_sample, s.block_size, s.rsi, s.flags = bps, bs, rsi, flags
            t = time.perf_counter()
            rc = lib.aec_buffer_decode(C.byref(s))
            return rc, time.perf_counter() - t

        bare_t = []
        for _ in range(args.reps + 1):
            rc, t = bare(data.size)
            assert rc == api.AEC_OK
            bare_t.append(t)
        assert np.array_equal(out, data)
        dec = api.Decoder(bps, bs, rsi, flags)
        offp = offs.ctypes.data_as(C.POINTER(C.c_size_t))

        def rng_call(pos, size, dst):
            s = dec.s
            s.next_in, s.avail_in = ea.ctypes.data, ea.size
            s.next_out, s.avail_out = dst, size
            t = time.perf_counter()
            rc = lib.aec_decode_range(C.byref(s), offp, offs.size, pos, size)
            return rc, time.perf_counter() - t

        out[:] = 0
        all_t = []
        for _ in range(args.reps + 1):
            rc, t = rng_call(0, data.size, out.ctypes.data)
            assert rc == api.AEC_OK
            all_t.append(t)
        assert np.array_equal(out, data)
        r = np.random.default_rng(1)
        nb = api.bytes_per_sample(bps, flags)
        small = np.empty(4096, dtype=np.uint8)
        lat = {}
        for label, size in (("sample", nb), ("range4k", 4096)):
            ts = []
            for i in range(args.ranges + 10):
                pos = int(r.integers(0, data.size - size)) // nb * nb
                rc, t = rng_call(pos, size, small.ctypes.data)
                assert rc == api.AEC_OK and small[:size].tobytes() == data[pos:pos + size].tobytes()
                if i >= 10:
                    ts.append(t)
            lat[label] = float(np.median(ts)) * 1e3
        dec.end()
        # the one-shot decode of 64 KiB of output: avail_out = 65536, the input the stream of the RSIs that holds them
        rsi_bytes = rsi * bs * nb
        n64 = (65536 + rsi_bytes - 1) // rsi_bytes
        end = int(offs[n64]) // 8 + 1 if n64 < offs.size else ea.size
        piece = ea[:end].copy()
        t64 = []
        for _ in range(50):
            rc, t = bare(65536, piece)
            assert rc == api.AEC_OK and np.array_equal(out[:65536], data[:65536])
            t64.append(t)
        print(json.dumps({
            "config": name, "size_mib": args.size_mib, "ratio": round(data.size / len(enc), 3),
            "bare_decode_gbs": round(data.size / min(bare_t[1:]) / 1e9, 2),
            "range_all_gbs": round(data.size / min(all_t[1:]) / 1e9, 2),
            "sample_ms_median": round(lat["sample"], 4), "range4k_ms_median": round(lat["range4k"], 4),
            "bare64k_ms_median": round(float(np.median(t64[5:])) * 1e3, 4),
        }), flush=True)


if __name__ == "__main__":
    main()
