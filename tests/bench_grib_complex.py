#!/usr/bin/env python3
"""GRIB2 complex packing on the device (run on the GPU box): the reader of templates 5.2 / 5.3 alone and inside the transcode
to template 5.42, beside, in the same run,
(a) the floor: a device-to-device copy of the bytes complex_expand moves -- the streams read and the rooms written;
(b) the nearest existing path: simple_to_ccsds over the same X (template 5.0 streams of the same fields), beside
    complex_to_ccsds, and the coder alone over the rooms.
Shapes: 64 fields of 1 038 240 values (a 0.25 degree global grid) at order 2 with groups of 8 to 64 values; 1024 fields of
10^4 to 10^5 values.  16 bits.  The X are those the library's quantiser gives for a smooth field with noise; the streams are
written on the host by a vectorised writer (second differences, minsd their minimum, a reference and a width per group) and
checked here: the rooms complex_expand leaves must be the quantiser's, byte for byte.  The grids cycle through 4 distinct
fields and the small fields through 32 distinct sizes, to keep the host's writing short.
Times are HIP events around 10 enqueues, the median (and the best) of 5 rounds after a warm-up call.
--expand-only runs complex_expand alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python
tests/bench_grib_complex.py --expand-only gives the kernels' shares)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grib_cases as gc  # noqa: E402
from bench_grib_device import device_ms  # noqa: E402

NBITS, BS, EXTRA = 16, 32, 4


def line(what, t, nbytes, note=""):
    print(f"  {what:<66}: median {t[1]:8.3f} ms (best {t[0]:8.3f})  {nbytes / 1e6 / t[1]:8.1f} GB/s moved  {note}")


def _table(values, bits):
    """NG integers of `bits` bits, padded to a byte, as bytes"""
    if bits == 0:
        return np.zeros(0, np.uint8)
    v = values.astype(np.uint64)
    planes = ((v[:, None] >> np.arange(bits - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(planes.reshape(-1))


def _sm(v, octets):
    return np.frombuffer((((1 if v < 0 else 0) << (8 * octets - 1)) | abs(int(v))).to_bytes(octets, "big"), np.uint8)


def write(x, rng):
    """(stream as uint8, descriptor) of the uint32 values x at order 2, groups of 8 to 64 values"""
    x = x.astype(np.int64)
    n = x.size
    assert n >= 9
    dd = np.zeros(n, np.int64)
    dd[2:] = x[2:] - 2 * x[1:-1] + x[:-2]
    minsd = int(dd[2:].min())
    s = dd - minsd
    s[:2] = 0
    lengths = rng.integers(8, 65, n // 8 + 1)
    ends = np.cumsum(lengths)
    ng = int(np.searchsorted(ends, n)) + 1
    lengths = lengths[:ng].copy()
    lengths[-1] = n - (int(ends[ng - 2]) if ng > 1 else 0)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    refs = np.minimum.reduceat(s, starts)
    top = np.maximum.reduceat(s, starts) - refs
    widths = np.where(top > 0, np.floor(np.log2(np.maximum(top, 1))).astype(np.int64) + 1, 0)
    assert int(widths.max()) <= 32 and int(refs.max()) < 1 << 32
    w = np.repeat(widths, lengths)
    p = (s - np.repeat(refs, lengths)).astype(np.uint64)
    k = np.arange(int(widths.max()), dtype=np.int64)
    keep = k < w[:, None]
    shift = np.where(keep, w[:, None] - 1 - k, 0).astype(np.uint64)
    data = np.packbits((((p[:, None] >> shift) & np.uint64(1)).astype(np.uint8))[keep])
    ref_bits, width_bits = int(refs.max()).bit_length(), int(widths.max()).bit_length()
    stored = lengths - 8
    length_bits = int(stored[:-1].max()).bit_length() if ng > 1 else 0
    desc = dict(ref_bits=ref_bits, n_groups=ng, width_ref=0, width_bits=width_bits, length_ref=8, length_inc=1, last_length=int(lengths[-1]),
                length_bits=length_bits, order=2, extra_octets=EXTRA, missing=0)
    stored[-1] = 0
    stream = np.concatenate([_sm(x[0], EXTRA), _sm(x[1], EXTRA), _sm(minsd, EXTRA), _table(refs, ref_bits), _table(widths, width_bits),
                             _table(stored, length_bits), data])
    return stream, desc


def shape(torch, gpu, gribgpu, name, n_values, distinct, calls, expand_only):
    n_values = [int(v) for v in n_values]
    n, total = len(n_values), sum(n_values)
    print(f" {name}: {n} fields, {total} values, {NBITS} bits, order 2, groups of 8 to 64 values")
    torch.manual_seed(n)
    i = torch.arange(total, device="cuda", dtype=torch.float32)
    d_src = 280.0 + 25.0 * torch.sin(i / 37.0) + 0.4 * torch.randn(total, device="cuda")
    del i
    starts = np.concatenate([[0], np.cumsum(n_values)]).astype(np.uint64)
    # the fields repeat with period `distinct`: field i holds the values of field i % distinct
    for i in range(distinct, n):
        assert n_values[i] == n_values[i % distinct]
        d_src[int(starts[i]):int(starts[i + 1])] = d_src[int(starts[i % distinct]):int(starts[i % distinct + 1])]
    codec = gribgpu.GribCodec(NBITS, BS, 128)
    plan = codec.simple_plan(n_values, gc.F32)
    dev = dict(device="cuda")
    d_work = torch.zeros(plan["work_bytes"], dtype=torch.uint8, **dev)
    d_fields = torch.zeros(n * 16, dtype=torch.uint8, **dev)
    assert codec.quantise_async(gc.F32, d_src, starts[:-1] * np.uint64(4), n_values, np.zeros(n, np.int32), None, d_work, d_fields) == 0
    torch.cuda.synchronize()
    w_offs = plan["work_offsets"]
    rng = np.random.default_rng(n)
    made = []
    for i in range(distinct):
        x = d_work[int(w_offs[i]):int(w_offs[i]) + 2 * n_values[i]].cpu().numpy().view("<u2")
        made.append(write(x, rng))
    descs = [made[i % distinct][1] for i in range(n)]
    sizes = np.array([made[i % distinct][0].size for i in range(n)], np.uint64)
    offs = (np.uint64(1) + np.concatenate([[0], np.cumsum(sizes)])[:-1]).astype(np.uint64)      # (an odd address, as in a message)
    cbytes = 1 + int(sizes.sum())
    host = np.zeros(cbytes, np.uint8)
    for i in range(n):
        host[int(offs[i]):int(offs[i]) + int(sizes[i])] = made[i % distinct][0]
    d_complex = torch.from_numpy(host).cuda()
    groups = sum(d["n_groups"] for d in descs)
    rooms = np.array([gc.room(v, BS, NBITS) for v in n_values], np.uint64)
    room_bytes = int(rooms.sum())
    print(f"  (streams {cbytes / (2 * total):.3f} of the 16-bit values, {groups} groups, {total / groups:.1f} values a group)")
    cplan = codec.complex_plan(n_values, descs)
    assert cplan is not None and cplan["work_bytes"] == plan["work_bytes"]
    d_work2 = torch.zeros(plan["work_bytes"], dtype=torch.uint8, **dev)
    d_cx = torch.zeros(n * 24, dtype=torch.uint8, **dev)
    fields = gribgpu.complex_fields(descs)

    t_ex = device_ms(torch, lambda: codec.complex_expand_async(fields, n_values, d_complex, cbytes, offs, sizes, d_work2, d_cx), calls)
    torch.cuda.synchronize()
    assert torch.equal(d_work2, d_work), "complex_expand differs from the quantiser's rooms"
    assert not d_cx.cpu().numpy().view(gribgpu.CX_DTYPE)["status"].any()
    moved = cbytes + room_bytes
    if expand_only:
        line("complex_expand (aec_gpu_grib_complex_expand_async)", t_ex, moved)
        codec.close()
        return
    d_a = torch.empty(moved // 2, dtype=torch.uint8, **dev)
    d_b = torch.empty_like(d_a)
    t_copy = device_ms(torch, lambda: d_b.copy_(d_a), calls)
    line("device copy of as many bytes (streams + rooms)", t_copy, moved)
    line("complex_expand (aec_gpu_grib_complex_expand_async)", t_ex, moved, f"({t_ex[1] / t_copy[1]:.2f} x the copy)")

    d_out = torch.empty(plan["out_bound"], dtype=torch.uint8, **dev)
    d_out2 = torch.empty(plan["out_bound"], dtype=torch.uint8, **dev)
    d_rec = torch.zeros(n * 2, dtype=torch.int64, **dev)
    d_res = torch.zeros(24, dtype=torch.uint8, **dev)
    d_table = torch.zeros(plan["rsi_entries"], dtype=torch.int64, **dev)
    coder = gpu.Codec(*plan["coder"])
    t_enc = device_ms(torch, lambda: coder.encode_chunks_async(d_work, w_offs, rooms, d_out, d_out.numel(), d_rec, d_table, d_res), calls)
    line("aec_gpu_encode_chunks_async alone over the rooms", t_enc, room_bytes)
    s_offs, s_bytes = plan["simple_offsets"], plan["simple_bytes"]
    s_sizes = np.array([(v * NBITS + 7) // 8 for v in n_values], np.uint64)
    d_simple = torch.zeros(s_bytes + 1, dtype=torch.uint8, **dev)[1:]
    assert codec.bits_pack_async(n_values, d_work, d_simple, s_offs) == 0
    t_sc = device_ms(torch, lambda: codec.simple_to_ccsds_async(d_simple, s_bytes, s_offs, s_sizes, n_values, d_work2, d_out, d_out.numel(), d_rec,
                                                                d_table, d_res), calls)
    line("simple_to_ccsds (bits_unpack + the encoder)", t_sc, s_bytes + room_bytes, f"({t_sc[1] / t_enc[1]:.2f} x the encoder alone)")
    torch.cuda.synchronize()
    nbytes = (int(d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["total_bits"]) + 7) // 8
    t_cc = device_ms(torch, lambda: codec.complex_to_ccsds_async(fields, d_complex, cbytes, offs, sizes, n_values, d_work2, d_out2, d_out2.numel(),
                                                                 d_rec, d_table, d_res, d_cx), calls)
    line("complex_to_ccsds (complex_expand + the encoder)", t_cc, moved, f"({t_cc[1] / t_sc[1]:.2f} x simple_to_ccsds, "
         f"{t_cc[1] / t_enc[1]:.2f} x the encoder alone)")
    torch.cuda.synchronize()
    assert torch.equal(d_out2[:nbytes], d_out[:nbytes]), "the two transcodes differ"
    print(f"  (CCSDS streams {nbytes / cbytes:.3f} of the complex streams)")
    codec.close()


def main():
    import torch
    from libaec_amd import gpu, gribgpu
    expand_only = "--expand-only" in sys.argv[1:]
    print(torch.cuda.get_device_name(0))
    shape(torch, gpu, gribgpu, "0.25 degree grids", [1038240] * 64, 4, 10, expand_only)
    rng = np.random.default_rng(1024)
    shape(torch, gpu, gribgpu, "unequal fields of 10^4 .. 10^5 values", list(rng.integers(10 ** 4, 10 ** 5 + 1, size=32)) * 32, 32, 10, expand_only)


if __name__ == "__main__":
    main()
