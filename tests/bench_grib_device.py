#!/usr/bin/env python3
"""GRIB2 CCSDS packing on the device (run on the GPU box): aec_gpu_grib_pack_async / aec_gpu_grib_unpack_async and their
halves alone, beside, in the same run,
(a) the yardstick: the same work done as a caller does it today on this library -- torch float64 ops for the minimum and
    maximum (with the host round trip for R and E), the quantisation and the cast, then Codec.encode_chunks_async; and
    Codec.decode_chunks_async, then torch ops back to floats;
(b) the floor: a device-to-device copy, whose rate prices the bytes the new kernels move -- 4 read by the min/max, 4 read
    and a container written by the quantiser (8 + c per value), a container read and 4 written by the dequantiser.
For the unequal fields the chain is a Python loop over the fields (a caller with a segmented reduction would do better):
its time is printed, but the comparison to go by is the grids.
Shapes: 64 float32 fields of 1 038 240 values (a 0.25 degree global grid) at 16, 12 and 24 bits; 1024 float32 fields of 10^4
to 10^5 values at 16 bits.  Times are HIP events around 10 enqueues (the torch chain synchronises inside: the events see its
stalls), best and median of 5 rounds after a warm-up call."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grib_cases as gc  # noqa: E402


def device_ms(torch, fn, calls=10, rounds=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    return min(ts), float(np.median(ts))


def line(what, t, nbytes, note=""):
    print(f"  {what:<62}: {t[0]:8.3f} ms (median {t[1]:8.3f})  {nbytes / 1e6 / t[0]:8.1f} GB/s of floats  {note}")


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
    d_copy = torch.empty_like(d_src)
    t_copy = device_ms(torch, lambda: d_copy.copy_(d_src), calls)
    rate = 8.0 * total / t_copy[0]                  # bytes moved per ms: 4 read and 4 written per value
    line("device copy of the floats", t_copy, total * 4, f"({rate / 1e6:.0f} GB/s moved)")

    codec = gribgpu.GribCodec(nbits, 32, 128)
    plan = codec.plan(n_values, gc.F32)
    dev = dict(device="cuda")
    d_work = torch.empty(plan["work_bytes"], dtype=torch.uint8, **dev)
    d_out = torch.empty(plan["out_bound"], dtype=torch.uint8, **dev)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, **dev)
    d_res = torch.zeros(24, dtype=torch.uint8, **dev)
    d_table = torch.zeros(plan["rsi_entries"], dtype=torch.int64, **dev)
    d_bare = torch.zeros(plan["rsi_entries"], dtype=torch.int64, **dev)
    d_fields = torch.zeros(n * 16, dtype=torch.uint8, **dev)
    d_dst = torch.empty_like(d_src)
    d_results = torch.zeros(n * 40, dtype=torch.uint8, **dev)
    d_result = torch.zeros(40, dtype=torch.uint8, **dev)

    def quantise():
        assert codec.quantise_async(gc.F32, d_src, offs, n_values, D, None, d_work, d_fields) == 0

    def pack():
        assert codec.pack_async(gc.F32, d_src, offs, n_values, D, None, d_work, d_out, d_out.numel(), d_rec, d_table, d_fields, d_res) == 0

    t_q = device_ms(torch, quantise, calls)
    floor_q = (8 + cont) * total / rate
    line("min/max + parameters + quantise (aec_gpu_grib_quantise_async)", t_q, total * 4, f"({t_q[0] / floor_q:.2f} x the copy floor of {floor_q:.3f} ms)")
    t_pack = device_ms(torch, pack, calls)
    fields = d_fields.cpu().numpy().view(gc.RECORD_DTYPE).copy()
    assert not fields["status"].any() and d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["overflow"] == 0
    rec = d_rec.cpu().numpy().view(np.uint64).reshape(n, 2)
    in_offs, in_sizes = (rec[:, 0] // 8).astype(np.uint64), ((rec[:, 1] + 7) // 8).astype(np.uint64)
    stream_bytes = int(in_sizes.sum())

    # (a) the caller's chain of today: torch float64 ops and the chunk coder
    coder = gpu.Codec(*plan["coder"])
    rooms = np.array([gc.room(v, 32, nbits) for v in n_values], np.uint64)
    w_offs = plan["work_offsets"]
    int_t = torch.int16 if cont == 2 else torch.int32
    d_work2 = torch.zeros(plan["work_bytes"], dtype=torch.uint8, **dev)
    equal = len(set(n_values)) == 1
    M = float(2 ** nbits - 1)

    def host_params(lo, hi):
        out = []
        for a, b in zip(lo.tolist(), hi.tolist()):
            R = gc.float_below(a)
            m, e = math.frexp(b - float(R))
            out.append((float(R), e - nbits + (1 if math.ldexp(m, nbits) > M else 0)))
        return out

    def chain_quantise():
        y = d_src.double()
        if equal:
            y2 = y.view(n, n_values[0])
            prm = host_params(y2.amin(1).cpu(), y2.amax(1).cpu())           # the host round trip
            R = torch.tensor([p[0] for p in prm], dtype=torch.float64, **dev)[:, None]
            s = torch.tensor([2.0 ** -p[1] for p in prm], dtype=torch.float64, **dev)[:, None]
            x = torch.trunc((y2 - R) * s + 0.5).to(torch.int32).to(int_t)
            room = int(rooms[0]) // cont
            w = d_work2.view(int_t).view(n, -1)                             # (equal rooms, each a multiple of 16 bytes here)
            w[:, :n_values[0]] = x
            w[:, n_values[0]:room] = x[:, -1:]
        else:
            ends = torch.stack([torch.stack((y[a:b].min(), y[a:b].max())) for a, b in zip(starts[:-1].tolist(), starts[1:].tolist())]).cpu()
            prm = host_params(ends[:, 0], ends[:, 1])
            for k, (a, b) in enumerate(zip(starts[:-1].tolist(), starts[1:].tolist())):
                x = torch.trunc((y[a:b] - prm[k][0]) * 2.0 ** -prm[k][1] + 0.5).to(torch.int32).to(int_t)
                o = int(w_offs[k]) // cont
                w = d_work2.view(int_t)
                w[o:o + b - a] = x
                w[o + b - a:o + int(rooms[k]) // cont] = x[-1]

    def chain_pack():
        chain_quantise()
        coder.encode_chunks_async(d_work2, w_offs, rooms, d_out, d_out.numel(), d_rec, d_table, d_res)

    few = max(1, calls // 5) if not equal else calls
    t_cq = device_ms(torch, chain_quantise, few, 3)
    torch.cuda.synchronize()
    pack()
    torch.cuda.synchronize()
    first = int(rooms[0]) if not equal else plan["work_bytes"]              # (unequal rooms: the gaps between them are nobody's)
    assert torch.equal(d_work2[:first], d_work[:first]), "the chain's X differ"
    t_cp = device_ms(torch, chain_pack, few, 3)
    line("torch float64 chain: min/max, host parameters, quantise, cast", t_cq, total * 4)
    line("... + Codec.encode_chunks_async (the caller's pack of today)", t_cp, total * 4)
    line("aec_gpu_grib_pack_async (with the table)", t_pack, total * 4, f"({t_pack[0] / t_cp[0]:.3f} x the chain; streams {stream_bytes / (total * 4):.3f} of the floats)")

    # reading
    params = fields.copy()
    pack()
    torch.cuda.synchronize()

    def dequantise():
        assert codec.dequantise_async(gc.F32, d_work, n_values, params, offs, d_dst) == 0

    def unpack(have):
        assert codec.unpack_async(gc.F32, d_out, d_out.numel(), in_offs, in_sizes, n_values, params, offs, d_table if have else d_bare, have,
                                  d_work, d_dst, d_results, d_result) == 0

    t_d = device_ms(torch, dequantise, calls)
    floor_d = (4 + cont) * total / rate
    line("dequantise (aec_gpu_grib_dequantise_async)", t_d, total * 4, f"({t_d[0] / floor_d:.2f} x the copy floor of {floor_d:.3f} ms)")
    d_R = torch.tensor(np.repeat(params["R"].astype(np.float64), n_values), **dev) if not equal else \
        torch.tensor(params["R"].astype(np.float64), **dev)[:, None]
    d_S = torch.tensor(np.repeat(2.0 ** params["E"].astype(np.float64), n_values), **dev) if not equal else \
        torch.tensor(2.0 ** params["E"].astype(np.float64), **dev)[:, None]
    mask = 0xFFFF if cont == 2 else 0xFFFFFFFF
    d_work3 = torch.empty(plan["work_bytes"], dtype=torch.uint8, **dev)

    def chain_unpack():
        coder.decode_chunks_async(d_out, d_out.numel(), in_offs, in_sizes, w_offs, rooms, d_table, 1, d_work3, d_results, d_result)
        w = d_work3.view(int_t)
        if equal:
            x = (w.view(n, -1)[:, :n_values[0]].to(torch.int64) & mask).double()
            d_dst.view(n, -1).copy_((x * d_S + d_R).float())
        else:
            for k, (a, b) in enumerate(zip(starts[:-1].tolist(), starts[1:].tolist())):
                o = int(w_offs[k]) // cont
                x = (w[o:o + b - a].to(torch.int64) & mask).double()
                d_dst[a:b] = (x * float(2.0 ** params["E"][k]) + float(params["R"][k])).float()

    t_cu = device_ms(torch, chain_unpack, few, 3)
    torch.cuda.synchronize()
    want = d_dst.clone()
    d_dst.zero_()
    line("Codec.decode_chunks_async + torch float64 ops (the caller's unpack of today)", t_cu, total * 4)
    for have, what in ((1, "with the table"), (0, "bare: index pass")):
        t = device_ms(torch, lambda: unpack(have), calls)
        torch.cuda.synchronize()
        assert torch.equal(d_dst, want), "unpack differs from the chain"
        assert not d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)["status"].any()
        d_dst.zero_()
        line(f"aec_gpu_grib_unpack_async ({what})", t, total * 4, f"({t[0] / t_cu[0]:.3f} x the chain)")
    codec.close()


def main():
    import torch
    from libaec_amd import gpu, gribgpu
    print(torch.cuda.get_device_name(0))
    grid = 1038240
    for nbits in (16, 12, 24):
        shape(torch, gpu, gribgpu, f"0.25 degree grids, {nbits} bits", [grid] * 64, nbits, 10)
    rng = np.random.default_rng(1024)
    shape(torch, gpu, gribgpu, "unequal fields of 10^4 .. 10^5 values", rng.integers(10 ** 4, 10 ** 5 + 1, size=1024), 16, 10)


if __name__ == "__main__":
    main()
