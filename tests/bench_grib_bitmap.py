#!/usr/bin/env python3
"""GRIB2 packing of fields with section 6 bitmaps on the device (run on the GPU box): aec_gpu_grib_pack_bitmap_async /
aec_gpu_grib_unpack_bitmap_async beside, in the same run and alternating round by round,
(a) the yardstick: what a caller does today -- pack: a torch boolean-mask compaction per field into one buffer, then
    aec_gpu_grib_pack_async; unpack: aec_gpu_grib_unpack_async, then a torch masked scatter per field into grids filled
    with the missing value.  Printed beside it: the same with the mask's indices found ONCE (index_select / index_copy_),
    which a caller with a static mask can do and which spares torch's per-call nonzero and its host round trip;
(b) the floor: a device-to-device copy, whose rate prices the bytes moved -- pack 4 + 4 + c per present point (read by
    the min/max, read by the quantiser, a container written) plus N / 8 of bitmap twice; unpack c per present point
    plus 4 N written.  The coder's own traffic is on both sides of every comparison and in no floor.
Shape: 64 float32 fields of 1 038 240 points (a 0.25 degree global grid) at 16 bits; masks: patches with about 30 % missing
(a land-sea shape), random bits with 50 % missing (the worst case for rank-addressed stores).  Times are HIP events around
10 enqueues, best and median of 5 rounds after a warm-up call."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grib_cases as gc  # noqa: E402

MISSING = 9999.0


def alternate(torch, fns, calls=10, rounds=5):
    """[(best, median) ms per call] of every fn, the fns taking turns within every round"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) / calls)
    return [(min(t), float(np.median(t))) for t in ts]


def line(what, t, note=""):
    print(f"  {what:<72}: {t[0]:8.3f} ms (median {t[1]:8.3f})  {note}", flush=True)


def mask_of(kind, n, rng):
    if kind == "random":
        return rng.random(n) < 0.5
    m = np.zeros(n, bool)
    at, sea = 0, True
    while at < n:
        run = int(rng.integers(200, 6000 if sea else 2600))
        m[at:at + run] = sea
        at, sea = at + run, not sea
    return m


def shape(torch, gpu, gribgpu, kind, n_fields=64, grid=1038240, nbits=16):
    rng = np.random.default_rng(30 if kind == "patches" else 50)
    mask = mask_of(kind, grid, rng)
    present = int(mask.sum())
    cont = gc.container(nbits)
    print(f" {kind}: {n_fields} float32 fields of {grid} points, {present} present ({100.0 * (grid - present) / grid:.1f} % missing), {nbits} bits",
          flush=True)
    dev = dict(device="cuda")
    torch.manual_seed(n_fields)
    total = n_fields * grid
    i = torch.arange(total, dtype=torch.float32, **dev)
    d_src = 280.0 + 25.0 * torch.sin(i / 37.0) + 0.4 * torch.randn(total, **dev)
    del i
    d_mask = torch.from_numpy(mask).cuda()
    d_src.view(n_fields, grid)[:, ~d_mask] = MISSING
    d_idx = d_mask.nonzero().flatten()
    d_copy = torch.empty_like(d_src)
    t_copy = alternate(torch, [lambda: d_copy.copy_(d_src)])[0]
    rate = 8.0 * total / t_copy[0]                       # bytes moved per ms
    line("device copy of the grids", t_copy, f"({rate / 1e6:.0f} GB/s moved)")
    del d_copy

    codec = gribgpu.GribCodec(nbits, 32, 128)
    n_points, n_values = [grid] * n_fields, [present] * n_fields
    offs = np.arange(n_fields, dtype=np.uint64) * np.uint64(grid * 4)
    c_offs = np.arange(n_fields, dtype=np.uint64) * np.uint64(present * 4)
    D = np.zeros(n_fields, np.int32)
    # the bitmaps, once per mask: every field brings its own copy, as every message does
    d_bitmap, bm_offs, counts = codec.bitmap(d_src, np.arange(n_fields) * grid, n_points, MISSING)
    assert [int(c) for c in counts] == n_values
    assert d_bitmap[:(grid + 7) // 8].cpu().numpy().tobytes() == np.packbits(mask).tobytes()
    d_counts = torch.zeros(n_fields, dtype=torch.int64, **dev)

    def build():
        assert codec.bitmap_async(gc.F32, d_src, offs, n_points, MISSING, d_bitmap, bm_offs, d_counts) == 0

    plan = codec.bitmap_plan(n_points, n_values, gc.F32)
    bufs = lambda: dict(work=torch.zeros(plan["work_bytes"], dtype=torch.uint8, **dev), out=torch.empty(plan["out_bound"], dtype=torch.uint8, **dev),
                        rec=torch.zeros(n_fields * 2, dtype=torch.int64, **dev), res=torch.zeros(24, dtype=torch.uint8, **dev),
                        table=torch.zeros(plan["rsi_entries"], dtype=torch.int64, **dev), fields=torch.zeros(n_fields * 16, dtype=torch.uint8, **dev))
    A, B = bufs(), bufs()
    d_compact = torch.empty(n_fields * present, dtype=torch.float32, **dev)
    src2, compact2 = d_src.view(n_fields, grid), d_compact.view(n_fields, present)

    def pack_new():
        assert codec.pack_bitmap_async(gc.F32, d_src, offs, n_values, D, None, A["work"], A["out"], A["out"].numel(), A["rec"], A["table"],
                                       A["fields"], A["res"], d_bitmap, bm_offs, n_points) == 0

    def pack_plain():
        assert codec.pack_async(gc.F32, d_compact, c_offs, n_values, D, None, B["work"], B["out"], B["out"].numel(), B["rec"], B["table"],
                                B["fields"], B["res"]) == 0

    def pack_mask():
        for k in range(n_fields):
            compact2[k] = src2[k][d_mask]
        pack_plain()

    def pack_index():
        for k in range(n_fields):
            torch.index_select(src2[k], 0, d_idx, out=compact2[k])
        pack_plain()

    t_build = alternate(torch, [build])[0]
    line("aec_gpu_grib_bitmap_async (once per mask)", t_build, f"({t_build[0] / ((4 * total + total / 8) / rate):.2f} x the copy floor)")
    t_new, t_mask, t_index = alternate(torch, [pack_new, pack_mask, pack_index])
    torch.cuda.synchronize()
    for key in ("work", "rec", "res", "table", "fields"):
        assert torch.equal(A[key], B[key]), f"pack_bitmap differs from the chain in {key}"
    nbytes = (int(A["res"].cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["total_bits"]) + 7) // 8
    assert torch.equal(A["out"][:nbytes], B["out"][:nbytes]), "pack_bitmap's streams differ from the chain's"
    floor = n_fields * ((8 + cont) * present + 2 * (grid / 8)) / rate
    t_plain = alternate(torch, [pack_plain])[0]
    line("aec_gpu_grib_pack_async of compacted fields (the part both chains share)", t_plain)
    line("torch boolean-mask compaction per field + pack_async (the caller today)", t_mask)
    line("torch index_select per field (indices found once) + pack_async", t_index)
    line("aec_gpu_grib_pack_bitmap_async", t_new, f"({t_new[0] / t_mask[0]:.3f} x the caller today, {t_new[0] / t_index[0]:.3f} x index_select; "
         f"the layer in front of the coder {t_new[0] - t_plain[0] + 0:.3f} ms over {t_plain[0]:.3f}, copy floor of its bytes {floor:.3f} ms)")

    # reading
    fields = A["fields"].cpu().numpy().view(gc.RECORD_DTYPE).copy()
    assert not fields["status"].any()
    d_dst_new, d_dst_old = torch.empty_like(d_src), torch.empty_like(d_src)
    d_vals = torch.empty(n_fields * present, dtype=torch.float32, **dev)
    vals2, old2 = d_vals.view(n_fields, present), d_dst_old.view(n_fields, grid)
    d_results = torch.zeros(n_fields * 40, dtype=torch.uint8, **dev)
    d_result = torch.zeros(40, dtype=torch.uint8, **dev)
    d_status = torch.zeros(n_fields, dtype=torch.int32, **dev)
    d_work_u = torch.empty(plan["work_bytes"], dtype=torch.uint8, **dev)

    def unpack_new():
        assert codec.unpack_bitmap_async(gc.F32, A["out"], A["out"].numel(), None, None, n_values, fields, offs, A["table"], 1, d_work_u,
                                         d_dst_new, d_results, d_result, d_bitmap, bm_offs, n_points, MISSING, d_status) == 0

    def unpack_plain():
        assert codec.unpack_async(gc.F32, A["out"], A["out"].numel(), None, None, n_values, fields, c_offs, A["table"], 1, d_work_u, d_vals,
                                  d_results, d_result) == 0

    def unpack_mask():
        unpack_plain()
        d_dst_old.fill_(MISSING)
        for k in range(n_fields):
            old2[k][d_mask] = vals2[k]

    def unpack_index():
        unpack_plain()
        d_dst_old.fill_(MISSING)
        for k in range(n_fields):
            old2[k].index_copy_(0, d_idx, vals2[k])

    t_new, t_mask, t_index = alternate(torch, [unpack_new, unpack_mask, unpack_index])
    torch.cuda.synchronize()
    assert torch.equal(d_dst_new, d_dst_old), "unpack_bitmap differs from the chain"
    assert not d_status.cpu().numpy().any()
    t_plain = alternate(torch, [unpack_plain])[0]
    floor = n_fields * (cont * present + 4 * grid + grid / 8) / rate
    line("aec_gpu_grib_unpack_async into compacted fields (the shared part)", t_plain)
    line("unpack_async + fill + torch masked scatter per field (the caller today)", t_mask)
    line("unpack_async + fill + index_copy_ per field (indices found once)", t_index)
    line("aec_gpu_grib_unpack_bitmap_async (with the table)", t_new, f"({t_new[0] / t_mask[0]:.3f} x the caller today, {t_new[0] / t_index[0]:.3f} x "
         f"index_copy_; copy floor of the expansion's bytes {floor:.3f} ms)")
    codec.close()


def main():
    import torch
    from libaec_amd import gpu, gribgpu
    print(torch.cuda.get_device_name(0))
    for kind in ("patches", "random"):
        shape(torch, gpu, gribgpu, kind)


if __name__ == "__main__":
    main()
