#!/usr/bin/env python3
"""Writing GRIB2 complex packing on the device (run on the GPU box): the writer of templates 5.2 / 5.3 alone (complex_write),
behind the quantiser (complex_pack) and behind the chunk decoder (ccsds_to_complex), beside, in the same run,
(a) the floor: a device-to-device copy of the bytes complex_write moves -- the rooms read and the streams written;
(b) the nearest existing paths over the same X: bits_pack and simple_pack (template 5.0), and complex_expand of the streams
    just written, which must give the quantiser's rooms back byte for byte.
Shapes: 64 float32 fields of 1 038 240 values (a 0.25 degree global grid); 1024 fields of 10^4 to 10^5 values.  16 bits, order
2, groups of 32.  The X are those the library's quantiser gives for a smooth field with noise.
It also prints the written sizes for orders 0 / 1 / 2 x G 16 / 32 / 64 beside the 5.0 size and the 5.42 streams of the same
fields.  Times are HIP events around 10 enqueues, the median (and the best) of 5 rounds after a warm-up call.
--write-only runs complex_write alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python
tests/bench_grib_complex_write.py --write-only gives the kernels' shares)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grib_cases as gc  # noqa: E402
from bench_grib_device import device_ms  # noqa: E402

NBITS, BS, ORDER, G = 16, 32, 2, 32


def line(what, t, nbytes, note=""):
    print(f"  {what:<66}: median {t[1]:8.3f} ms (best {t[0]:8.3f})  {nbytes / 1e6 / t[1]:8.1f} GB/s moved  {note}")


def shape(torch, gpu, gribgpu, name, n_values, calls, write_only):
    n_values = [int(v) for v in n_values]
    n, total = len(n_values), sum(n_values)
    print(f" {name}: {n} fields, {total} values, {NBITS} bits, order {ORDER}, groups of {G}")
    torch.manual_seed(n)
    i = torch.arange(total, device="cuda", dtype=torch.float32)
    d_src = 280.0 + 25.0 * torch.sin(i / 37.0) + 0.4 * torch.randn(total, device="cuda")
    del i
    src_offs = np.concatenate([[0], np.cumsum(n_values)]).astype(np.uint64)[:-1] * np.uint64(4)
    D = np.zeros(n, np.int32)
    codec = gribgpu.GribCodec(NBITS, BS, 128)
    plan = codec.complex_write_plan(n_values, ORDER, G, gc.F32)
    splan = codec.simple_plan(n_values, gc.F32)
    assert plan is not None and plan["work_bytes"] == splan["work_bytes"]
    dev = dict(device="cuda")
    d_work = torch.zeros(plan["work_bytes"], dtype=torch.uint8, **dev)
    d_fields = torch.zeros(n * 16, dtype=torch.uint8, **dev)
    assert codec.quantise_async(gc.F32, d_src, src_offs, n_values, D, None, d_work, d_fields) == 0
    torch.cuda.synchronize()
    cap, c_offs = plan["complex_bound"], plan["complex_offsets"]
    d_complex = torch.zeros(cap, dtype=torch.uint8, **dev)
    d_cxw = torch.zeros(n * gribgpu.CXW_DTYPE.itemsize, dtype=torch.uint8, **dev)
    rooms = np.array([gc.room(v, BS, NBITS) for v in n_values], np.uint64)
    room_bytes = int(rooms.sum())

    t_w = device_ms(torch, lambda: codec.complex_write_async(ORDER, G, n_values, d_work, d_complex, cap, c_offs, d_cxw), calls)
    torch.cuda.synchronize()
    recs = d_cxw.cpu().numpy().view(gribgpu.CXW_DTYPE)
    written = int(recs["bytes"].sum())
    moved = room_bytes + written
    print(f"  (streams {written / (2 * total):.3f} of the 16-bit values, {written / cap:.3f} of the bound; {int(recs['n_groups'].sum())} groups; "
          f"{plan['value_tiles']} value tiles, {plan['group_tiles']} table tiles, {plan['out_tiles']} output tiles)")
    if write_only:
        line("complex_write (aec_gpu_grib_complex_write_async)", t_w, moved)
        codec.close()
        return
    d_a = torch.empty(moved // 2, dtype=torch.uint8, **dev)
    d_b = torch.empty_like(d_a)
    t_copy = device_ms(torch, lambda: d_b.copy_(d_a), calls)
    line("device copy of as many bytes (rooms + streams)", t_copy, moved)
    line("complex_write (aec_gpu_grib_complex_write_async)", t_w, moved, f"({t_w[1] / t_copy[1]:.2f} x the copy)")

    # the streams just written, read back: the quantiser's rooms byte for byte
    fields, sizes = gribgpu.complex_fields_of(recs)
    fields = gribgpu.complex_fields(fields)
    d_work2 = torch.zeros(plan["work_bytes"], dtype=torch.uint8, **dev)
    d_cx = torch.zeros(n * 24, dtype=torch.uint8, **dev)
    t_ex = device_ms(torch, lambda: codec.complex_expand_async(fields, n_values, d_complex, cap, c_offs, sizes, d_work2, d_cx), calls)
    torch.cuda.synchronize()
    assert torch.equal(d_work2, d_work), "complex_expand of the written streams differs from the quantiser's rooms"
    assert not d_cx.cpu().numpy().view(gribgpu.CX_DTYPE)["status"].any()
    line("complex_expand of the streams just written", t_ex, moved, f"({t_w[1] / t_ex[1]:.2f}: the writer against the reader)")

    # the same X as template 5.0
    s_offs, s_bytes = splan["simple_offsets"], splan["simple_bytes"]
    d_simple = torch.zeros(s_bytes + 1, dtype=torch.uint8, **dev)[1:]
    t_bp = device_ms(torch, lambda: codec.bits_pack_async(n_values, d_work, d_simple, s_offs), calls)
    line("bits_pack over the same X", t_bp, room_bytes + s_bytes, f"(complex_write is {t_w[1] / t_bp[1]:.2f} x)")
    t_q = device_ms(torch, lambda: codec.quantise_async(gc.F32, d_src, src_offs, n_values, D, None, d_work2, d_fields), calls)
    line("quantise alone", t_q, 4 * total + room_bytes)
    t_sp = device_ms(torch, lambda: codec.simple_pack_async(gc.F32, d_src, src_offs, n_values, D, None, d_work2, d_fields, d_simple, s_offs), calls)
    line("simple_pack (quantise + bits_pack)", t_sp, 4 * total + s_bytes)
    d_complex2 = torch.zeros(cap, dtype=torch.uint8, **dev)
    t_cp = device_ms(torch, lambda: codec.complex_pack_async(ORDER, G, gc.F32, d_src, src_offs, n_values, D, None, d_work2, d_fields, d_complex2, cap,
                                                             c_offs, d_cxw), calls)
    line("complex_pack (quantise + complex_write)", t_cp, 4 * total + written, f"({t_cp[1] / t_sp[1]:.2f} x simple_pack)")
    torch.cuda.synchronize()
    assert torch.equal(d_complex2, d_complex), "complex_pack differs from quantise + complex_write"

    # from template 5.42: the pack's streams and table
    d_out = torch.empty(plan["out_bound"], dtype=torch.uint8, **dev)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, **dev)
    d_res = torch.zeros(24, dtype=torch.uint8, **dev)
    d_table = torch.zeros(max(1, plan["rsi_entries"]), dtype=torch.int64, **dev)
    assert codec.pack_async(gc.F32, d_src, src_offs, n_values, D, None, d_work2, d_out, d_out.numel(), d_rec, d_table, d_fields, d_res) == 0
    torch.cuda.synchronize()
    ccsds = (int(d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["total_bits"]) + 7) // 8
    d_results = torch.zeros(n * 40, dtype=torch.uint8, **dev)
    d_result = torch.zeros(40, dtype=torch.uint8, **dev)
    d_complex2.zero_()
    t_cc = device_ms(torch, lambda: codec.ccsds_to_complex_async(ORDER, G, d_out, d_out.numel(), None, None, n_values, d_table, 1, d_work2, d_results,
                                                                 d_result, d_complex2, cap, c_offs, d_cxw), calls)
    line("ccsds_to_complex (the decoder with its table + complex_write)", t_cc, ccsds + written)
    torch.cuda.synchronize()
    assert torch.equal(d_complex2, d_complex), "ccsds_to_complex differs from complex_write"

    # written sizes
    print(f"  sizes: template 5.0 {s_bytes} bytes (1.000), template 5.42 {ccsds} bytes ({ccsds / s_bytes:.3f})")
    for o in (0, 1, 2):
        row = []
        for g in (16, 32, 64):
            p = codec.complex_write_plan(n_values, o, g, gc.F32)
            d_c = torch.zeros(p["complex_bound"], dtype=torch.uint8, **dev)
            assert codec.complex_write_async(o, g, n_values, d_work, d_c, p["complex_bound"], p["complex_offsets"], d_cxw) == 0
            torch.cuda.synchronize()
            size = int(d_cxw.cpu().numpy().view(gribgpu.CXW_DTYPE)["bytes"].sum())
            row.append(f"G {g}: {size} ({size / s_bytes:.3f})")
            del d_c
        print(f"    order {o}:  " + "   ".join(row))
    codec.close()


def main():
    import torch
    from libaec_amd import gpu, gribgpu
    write_only = "--write-only" in sys.argv[1:]
    print(torch.cuda.get_device_name(0))
    shape(torch, gpu, gribgpu, "0.25 degree grids", [1038240] * 64, 10, write_only)
    rng = np.random.default_rng(1024)
    shape(torch, gpu, gribgpu, "unequal fields of 10^4 .. 10^5 values", list(rng.integers(10 ** 4, 10 ** 5 + 1, size=1024)), 10, write_only)


if __name__ == "__main__":
    main()
