#!/usr/bin/env python3
"""GRIB2 simple packing on the device (run on the GPU box): the bit layer between the X rooms and template 7.0 streams,
alone and inside the calls that compose it, beside, in the same run,
(a) the floor: a device-to-device copy of the bytes a bits call moves -- the rooms read and the streams written by
    bits_pack, the reverse by bits_unpack;
(b) the coder alone over the same rooms -- aec_gpu_encode_chunks_async beside simple_to_ccsds, aec_gpu_decode_chunks_async
    beside ccsds_to_simple -- so that the bit layer's share of a transcode is visible;
(c) the only device route that exists without this layer: the library's quantiser / dequantiser and a chain of torch integer
    ops (shifts and ors over the same X, lcm(nbits, 8) bits at a time) beside simple_pack / simple_unpack.  For the unequal
    fields the chain is a Python loop over the fields: its time is printed, but the comparison to go by is the grids.
Shapes, as tests/bench_grib_device.py: 64 float32 fields of 1 038 240 values (a 0.25 degree global grid) at 12, 16 and 24
bits; 1024 float32 fields of 10^4 to 10^5 values at 16 bits.  Times are HIP events around 10 enqueues, the median (and the
best) of 5 rounds after a warm-up call."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grib_cases as gc  # noqa: E402
from bench_grib_device import device_ms  # noqa: E402


def line(what, t, nbytes, note=""):
    print(f"  {what:<66}: median {t[1]:8.3f} ms (best {t[0]:8.3f})  {nbytes / 1e6 / t[1]:8.1f} GB/s moved  {note}")


def shape(torch, gpu, gribgpu, name, n_values, nbits, calls):
    n_values = [int(v) for v in n_values]
    n, total = len(n_values), sum(n_values)
    cont = gc.container(nbits)
    print(f" {name}: {n} fields, {total * 4 >> 20} MiB of float32, {nbits} bits")
    torch.manual_seed(n)
    i = torch.arange(total, device="cuda", dtype=torch.float32)
    d_src = 280.0 + 25.0 * torch.sin(i / 37.0) + 0.4 * torch.randn(total, device="cuda")
    del i
    starts = np.concatenate([[0], np.cumsum(n_values)]).astype(np.uint64)
    offs = starts[:-1] * np.uint64(4)
    D = np.zeros(n, np.int32)
    codec = gribgpu.GribCodec(nbits, 32, 128)
    plan = codec.simple_plan(n_values, gc.F32)
    s_offs, s_bytes = plan["simple_offsets"], plan["simple_bytes"]
    sizes = np.array([(v * nbits + 7) // 8 for v in n_values], np.uint64)
    rooms = np.array([gc.room(v, 32, nbits) for v in n_values], np.uint64)
    w_offs = plan["work_offsets"]
    room_bytes = int(rooms.sum())
    dev = dict(device="cuda")
    d_work = torch.zeros(plan["work_bytes"], dtype=torch.uint8, **dev)
    d_work2 = torch.zeros(plan["work_bytes"], dtype=torch.uint8, **dev)
    d_simple = torch.zeros(s_bytes + 1, dtype=torch.uint8, **dev)[1:]           # (streams at an odd address, as in a message)
    d_simple2 = torch.zeros(s_bytes, dtype=torch.uint8, **dev)
    d_out = torch.empty(plan["out_bound"], dtype=torch.uint8, **dev)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, **dev)
    d_res = torch.zeros(24, dtype=torch.uint8, **dev)
    d_table = torch.zeros(plan["rsi_entries"], dtype=torch.int64, **dev)
    d_fields = torch.zeros(n * 16, dtype=torch.uint8, **dev)
    d_dst = torch.empty_like(d_src)
    d_results = torch.zeros(n * 40, dtype=torch.uint8, **dev)
    d_result = torch.zeros(40, dtype=torch.uint8, **dev)

    # (a) the bit layer beside a copy of the bytes it moves
    moved = room_bytes + s_bytes
    d_a = torch.empty(moved // 2, dtype=torch.uint8, **dev)
    d_b = torch.empty_like(d_a)
    t_copy = device_ms(torch, lambda: d_b.copy_(d_a), calls)
    line("device copy of as many bytes (rooms + streams)", t_copy, moved)
    assert codec.quantise_async(gc.F32, d_src, offs, n_values, D, None, d_work, d_fields) == 0
    torch.cuda.synchronize()
    fields = d_fields.cpu().numpy().view(gc.RECORD_DTYPE).copy()
    assert not fields["status"].any()
    t_bp = device_ms(torch, lambda: codec.bits_pack_async(n_values, d_work, d_simple, s_offs), calls)
    line("bits_pack (aec_gpu_grib_bits_pack_async)", t_bp, moved, f"({t_bp[1] / t_copy[1]:.2f} x the copy)")
    t_bu = device_ms(torch, lambda: codec.bits_unpack_async(n_values, d_simple, s_bytes, s_offs, sizes, d_work2), calls)
    line("bits_unpack (aec_gpu_grib_bits_unpack_async)", t_bu, moved, f"({t_bu[1] / t_copy[1]:.2f} x the copy)")
    torch.cuda.synchronize()
    equal = len(set(n_values)) == 1
    first = plan["work_bytes"] if equal and int(rooms[0]) % 16 == 0 else int(rooms[0])
    assert torch.equal(d_work2[:first], d_work[:first]), "bits_unpack(bits_pack(rooms)) differs from the rooms"

    # (b) the transcodes beside the coder alone over the same rooms
    coder = gpu.Codec(*plan["coder"])
    t_enc = device_ms(torch, lambda: coder.encode_chunks_async(d_work, w_offs, rooms, d_out, d_out.numel(), d_rec, d_table, d_res), calls)
    line("aec_gpu_encode_chunks_async alone over the rooms", t_enc, room_bytes)
    t_sc = device_ms(torch, lambda: codec.simple_to_ccsds_async(d_simple, s_bytes, s_offs, sizes, n_values, d_work2, d_out, d_out.numel(), d_rec,
                                                                d_table, d_res), calls)
    line("simple_to_ccsds (bits_unpack + the encoder)", t_sc, moved, f"({t_sc[1] / t_enc[1]:.2f} x the encoder alone)")
    torch.cuda.synchronize()
    assert d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["overflow"] == 0
    rec = d_rec.cpu().numpy().view(np.uint64).reshape(n, 2)
    in_offs, in_sizes = (rec[:, 0] // 8).astype(np.uint64), ((rec[:, 1] + 7) // 8).astype(np.uint64)
    print(f"  (CCSDS streams {int(in_sizes.sum()) / s_bytes:.3f} of the simple streams)")
    t_dec = device_ms(torch, lambda: coder.decode_chunks_async(d_out, d_out.numel(), in_offs, in_sizes, w_offs, rooms, d_table, 1, d_work2,
                                                               d_results, d_result), calls)
    line("aec_gpu_decode_chunks_async alone into the rooms (with the table)", t_dec, room_bytes)
    t_cs = device_ms(torch, lambda: codec.ccsds_to_simple_async(d_out, d_out.numel(), in_offs, in_sizes, n_values, d_table, 1, d_work2, d_results,
                                                                d_result, d_simple2, s_offs), calls)
    line("ccsds_to_simple (the decoder + bits_pack)", t_cs, moved, f"({t_cs[1] / t_dec[1]:.2f} x the decoder alone)")
    torch.cuda.synchronize()
    assert torch.equal(d_simple2, d_simple), "the transcode there and back differs"

    # (c) floats to streams and back beside the quantiser and a chain of torch integer ops
    int_t = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[cont]
    group = math.lcm(nbits, 8) // nbits                  # values whose bits end on a byte
    nb = group * nbits // 8
    mask = (1 << (8 * cont)) - 1
    assert all(v % group == 0 for v in n_values)
    d_chain = torch.zeros(s_bytes, dtype=torch.uint8, **dev)

    def bits_of(x):                                     # x: int64, a multiple of `group` values -> their bytes
        x = x.view(-1, group)
        acc = x[:, 0]
        for k in range(1, group):
            acc = (acc << nbits) | x[:, k]
        return torch.stack([(acc >> (8 * (nb - 1 - j))) & 255 for j in range(nb)], 1).to(torch.uint8).view(-1)

    def values_of(b):                                   # the reverse
        b = b.view(-1, nb).to(torch.int64)
        acc = b[:, 0]
        for j in range(1, nb):
            acc = (acc << 8) | b[:, j]
        return torch.stack([(acc >> (nbits * (group - 1 - k))) & ((1 << nbits) - 1) for k in range(group)], 1).view(-1)

    def chain_pack():
        assert codec.quantise_async(gc.F32, d_src, offs, n_values, D, None, d_work, d_fields) == 0
        w = d_work.view(int_t)
        if equal:
            x = w.view(n, -1)[:, :n_values[0]].to(torch.int64) & mask
            d_chain.view(n, -1).copy_(bits_of(x.reshape(-1)).view(n, -1))
        else:
            for k in range(n):
                o = int(w_offs[k]) // cont
                d_chain[int(s_offs[k]):int(s_offs[k]) + int(sizes[k])] = bits_of(w[o:o + n_values[k]].to(torch.int64) & mask)

    def chain_unpack():
        w = d_work2.view(int_t)
        if equal:
            x = values_of(d_chain.view(n, -1)).view(n, -1).to(int_t)
            room = int(rooms[0]) // cont
            wv = w.view(n, -1)
            wv[:, :n_values[0]] = x
            wv[:, n_values[0]:room] = x[:, -1:]
        else:
            for k in range(n):
                x = values_of(d_chain[int(s_offs[k]):int(s_offs[k]) + int(sizes[k])]).to(int_t)
                o = int(w_offs[k]) // cont
                w[o:o + n_values[k]] = x
                w[o + n_values[k]:o + int(rooms[k]) // cont] = x[-1]
        assert codec.dequantise_async(gc.F32, d_work2, n_values, fields, offs, d_dst) == 0

    few = calls if equal else max(1, calls // 5)
    t_cp = device_ms(torch, chain_pack, few, 3)
    torch.cuda.synchronize()
    assert torch.equal(d_chain, d_simple), "the chain's streams differ"
    line("quantise_async + torch shifts and ors (the route without this layer)", t_cp, total * 4 + s_bytes)
    t_sp = device_ms(torch, lambda: codec.simple_pack_async(gc.F32, d_src, offs, n_values, D, None, d_work, d_fields, d_simple, s_offs), calls)
    line("simple_pack (aec_gpu_grib_simple_pack_async)", t_sp, total * 4 + s_bytes, f"({t_sp[1] / t_cp[1]:.3f} x the chain)")
    t_cu = device_ms(torch, chain_unpack, few, 3)
    torch.cuda.synchronize()
    want = d_dst.clone()
    d_dst.zero_()
    line("torch shifts and ors + dequantise_async", t_cu, total * 4 + s_bytes)
    t_su = device_ms(torch, lambda: codec.simple_unpack_async(gc.F32, d_simple, s_bytes, s_offs, sizes, n_values, fields, offs, d_work2, d_dst),
                     calls)
    torch.cuda.synchronize()
    assert torch.equal(d_dst, want), "simple_unpack differs from the chain"
    line("simple_unpack (aec_gpu_grib_simple_unpack_async)", t_su, total * 4 + s_bytes, f"({t_su[1] / t_cu[1]:.3f} x the chain)")
    codec.close()


def main():
    import torch
    from libaec_amd import gpu, gribgpu
    print(torch.cuda.get_device_name(0))
    grid = 1038240
    for nbits in (12, 16, 24):
        shape(torch, gpu, gribgpu, f"0.25 degree grids, {nbits} bits", [grid] * 64, nbits, 10)
    rng = np.random.default_rng(1024)
    shape(torch, gpu, gribgpu, "unequal fields of 10^4 .. 10^5 values", rng.integers(10 ** 4, 10 ** 5 + 1, size=1024), 16, 10)


if __name__ == "__main__":
    main()
