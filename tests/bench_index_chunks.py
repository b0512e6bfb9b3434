#!/usr/bin/env python3
"""Bare batches of unequal chunks decoded on the device (run on the GPU box): aec_gpu_decode_chunks_async(have_table == 0)
of this tree -- the index pass as the plan decides (PLANNED), the every-bit scheme for every stream it can take
(EVERY_BIT), the serial walk alone (SERIAL) -- beside the same call of ANOTHER build of the library (--parent, or the
environment's AEC_AMD_LIB_PARENT: the parent commit's libaec.so.0), on the same streams in the same process, the calls
taking turns round by round.  The batches are those of tests/bench_decode_chunks.py.  Every way's output is compared with
the data that was encoded before anything is timed.  Times are HIP events around 3 enqueues, 7 rounds: best, median and
worst per call.

--sweep: what decides kBsB0 and kBsR (libaec_amd/csrc/aec_bsmall.h) -- the index pass alone (aec_gpu_index_chunks_async),
256 equal chunks of 2^k blocks under SERIAL and EVERY_BIT, and the 1024-chunk batch under EVERY_BIT in 1 .. 32 rounds."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_decode_chunks import C2, C5, KIB, MIB, alternating_ms, rows  # noqa: E402


class Other:
    """another build of the library: a context of its own and the one call that is timed"""

    def __init__(self, path, gpu, prm):
        self.lib = C.CDLL(path)
        vp, u64 = C.c_void_p, C.c_uint64
        self.lib.aec_gpu_create.argtypes = [C.POINTER(vp)]
        self.lib.aec_gpu_destroy.argtypes = [vp]
        self.lib.aec_gpu_decode_chunks_async.restype = C.c_int
        self.lib.aec_gpu_decode_chunks_async.argtypes = [vp, C.POINTER(gpu.Params), vp, C.c_size_t, vp, vp, vp, vp, u64, vp, C.c_int, vp,
                                                         vp, vp, vp]
        self.p = gpu.Params(*prm)
        self.ctx = vp()
        assert self.lib.aec_gpu_create(C.byref(self.ctx)) == 0

    def decode_bare(self, d_in, in_bytes, in_off, in_len, out_off, sizes, d_tab, d_out, d_rec, d_res, st):
        host = lambda a: C.c_void_p(a.ctypes.data)
        return self.lib.aec_gpu_decode_chunks_async(self.ctx, C.byref(self.p), d_in.data_ptr(), in_bytes, host(in_off), host(in_len),
                                                    host(out_off), host(sizes), int(sizes.size), d_tab.data_ptr(), 0, d_out.data_ptr(),
                                                    d_rec.data_ptr(), d_res.data_ptr(), st)

    def close(self):
        self.lib.aec_gpu_destroy(self.ctx)


def encoded(torch, gpu, prm, sizes):
    """the batch encoded on the device: (codec, data, d_enc, enc_bytes, in_off, in_len, offsets of the chunks in data)"""
    from test_gpu_parity import gen
    n = len(sizes)
    sizes_a = np.array(sizes, dtype=np.uint64)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum((sizes_a + 15) // 16 * 16)
    data = gen(2 if prm[0] == 8 else 0, int(offsets[n]) + 64)
    codec = gpu.Codec(*prm)
    d_enc, rec, _, res = codec.encode_chunks(torch.from_numpy(data).cuda(), np.ascontiguousarray(offsets[:n]), sizes_a)
    assert not int(res["overflow"])
    in_off = np.ascontiguousarray(rec[:, 0] // 8).astype(np.uint64)
    in_len = np.maximum((rec[:, 1] + 7) // 8, 1).astype(np.uint64)
    return codec, data, d_enc, int(res["total_bits"]) // 8, in_off, in_len, offsets


def fmt(t):
    return f"best {t[0]:9.3f}  median {t[1]:9.3f}  worst {t[2]:9.3f} ms"


def bench_rows(torch, gpu, parent):
    missed = []
    for name, prm, sizes in rows():
        n = len(sizes)
        nb = 2 if prm[0] > 8 else 1
        blk = prm[1] * nb
        sizes_a = np.array(sizes, dtype=np.uint64)
        codec, data, d_enc, enc_bytes, in_off, in_len, offsets = encoded(torch, gpu, prm, sizes)
        blocks = (sizes_a // nb + prm[1] - 1) // prm[1]
        plan = codec.decode_chunks_plan(sizes_a)
        out_off = np.zeros(n, dtype=np.uint64)
        out_off[1:] = np.cumsum((blocks[:-1] * blk + 15) // 16 * 16)
        st = codec._stream(None)
        want = [data[int(offsets[i]):int(offsets[i]) + sizes[i]] for i in range(n)]

        def same(d_out):
            out = d_out.cpu().numpy()
            return all(np.array_equal(out[int(out_off[i]):int(out_off[i]) + sizes[i]], want[i]) for i in range(n))

        ways, fns, outs, codecs = [], [], [], []
        for label, how in (("planned", gpu.CHUNKS_INDEX_PLANNED), ("every bit", gpu.CHUNKS_INDEX_EVERY_BIT), ("serial walk", gpu.CHUNKS_INDEX_SERIAL)):
            cd = gpu.Codec(*prm)
            cd.set_chunks_index(how)
            bufs = (torch.zeros(plan["rsi_entries"], dtype=torch.int64, device="cuda"), torch.zeros(plan["out_bytes"] + 16, dtype=torch.uint8, device="cuda"),
                    torch.zeros(40 * n, dtype=torch.uint8, device="cuda"), torch.zeros(40, dtype=torch.uint8, device="cuda"))

            def call(cd=cd, bufs=bufs):
                assert cd.decode_chunks_async(d_enc, enc_bytes, in_off, in_len, out_off, sizes_a, bufs[0], 0, bufs[1], bufs[2], bufs[3]) == 0

            ip = cd.index_chunks_plan(in_len, sizes_a)
            ways.append(f"this tree, {label} ({ip['taken']} streams in {ip['rounds']} rounds, {ip['workspace_bytes'] / MIB:.1f} MiB)")
            fns.append(call)
            outs.append(bufs[1])
            codecs.append(cd)
        other = None
        if parent:
            other = Other(parent, gpu, prm)
            bufs = (torch.zeros(plan["rsi_entries"], dtype=torch.int64, device="cuda"), torch.zeros(plan["out_bytes"] + 16, dtype=torch.uint8, device="cuda"),
                    torch.zeros(40 * n, dtype=torch.uint8, device="cuda"), torch.zeros(40, dtype=torch.uint8, device="cuda"))

            def parent_call(bufs=bufs):
                assert other.decode_bare(d_enc, enc_bytes, in_off, in_len, out_off, sizes_a, bufs[0], bufs[1], bufs[2], bufs[3], st) == 0

            ways.append("the parent's library")
            fns.append(parent_call)
            outs.append(bufs[1])
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        assert all(same(o) for o in outs), name
        t = alternating_ms(torch, fns, calls=3)
        print(f"{name}: {n} chunks, {int(sizes_a.sum()) / MIB:.1f} MiB decoded, {enc_bytes / MIB:.1f} MiB coded, longest stream {int(in_len.max()) / KIB:.1f} KiB")
        for w, x in zip(ways, t):
            print(f"  {w:72s}: {fmt(x)}")
        if parent:
            spread = t[-1][2] - t[-1][0]
            slower = t[0][1] > t[-1][1] + spread
            faster = t[0][1] < t[-1][1] - spread
            print(f"  planned / parent (medians): {t[0][1] / t[-1][1]:6.2f} x   the parent's spread {spread:.3f} ms   "
                  + ("SLOWER beyond the spread" if slower else ("faster beyond the spread" if faster else "within the spread")))
            if slower or (int(in_len.max()) >= 10 * KIB and not faster):
                missed.append(name)
            other.close()
        for cd in codecs:
            cd.close()
        codec.close()
    print("rows that miss the expectation: " + (", ".join(missed) if missed else "none"))


def index_ms(torch, gpu, prm, d_enc, enc_bytes, in_off, in_len, sizes_a, settings):
    """the index pass alone under each (how, round_bits) of settings, taking turns: [(best, median, worst)], plans"""
    n = int(sizes_a.size)
    fns, plans, codecs = [], [], []
    entries = gpu.decode_chunks_plan(*prm, sizes_a)["rsi_entries"]
    for how, rb in settings:
        cd = gpu.Codec(*prm)
        cd.set_chunks_index(how, rb)
        bufs = (torch.zeros(entries, dtype=torch.int64, device="cuda"), torch.zeros(40 * n, dtype=torch.uint8, device="cuda"))

        def call(cd=cd, bufs=bufs):
            assert cd.index_chunks_async(d_enc, enc_bytes, in_off, in_len, sizes_a, bufs[0], bufs[1]) == 0

        fns.append(call)
        plans.append(cd.index_chunks_plan(in_len, sizes_a))
        codecs.append((cd, bufs))
    t = alternating_ms(torch, fns, calls=3)
    torch.cuda.synchronize()
    first = codecs[0][1]
    for cd, bufs in codecs[1:]:
        assert torch.equal(bufs[1], first[1]), "records differ between the ways"
    for cd, _ in codecs:
        cd.close()
    return t, plans


def sweep(torch, gpu):
    print("index pass alone, 256 equal chunks of B blocks: serial walk against every bit")
    for cname, prm in (("config 5", C5), ("config 2", C2)):
        nb = 2 if prm[0] > 8 else 1
        for blocks in (32, 64, 128, 256, 512, 1024, 2048, 4096):
            sizes = [blocks * prm[1] * nb] * 256
            codec, _, d_enc, enc_bytes, in_off, in_len, _ = encoded(torch, gpu, prm, sizes)
            t, plans = index_ms(torch, gpu, prm, d_enc, enc_bytes, in_off, in_len, np.array(sizes, dtype=np.uint64),
                                [(gpu.CHUNKS_INDEX_SERIAL, 0), (gpu.CHUNKS_INDEX_EVERY_BIT, 0)])
            print(f"  {cname} B = {blocks:5d} ({int(in_len.mean()):7d} bytes of stream each): serial {fmt(t[0])}   every bit {fmt(t[1])}   "
                  f"every bit / serial {t[1][1] / t[0][1]:5.2f}")
            codec.close()
    print("index pass alone, 1024 unequal chunks of 4 to 128 KiB under EVERY_BIT: rounds")
    for name, prm, sizes in rows():
        if not name.startswith("1024"):
            continue
        codec, _, d_enc, enc_bytes, in_off, in_len, _ = encoded(torch, gpu, prm, sizes)
        total = int(sum((8 * int(s) + 1 + 1023) // 1024 * 1024 for s in in_len))
        settings = [(gpu.CHUNKS_INDEX_SERIAL, 0)] + [(gpu.CHUNKS_INDEX_EVERY_BIT, max(total // k + 1024, 1 << 20)) for k in (1, 2, 4, 8, 16, 32)]
        t, plans = index_ms(torch, gpu, prm, d_enc, enc_bytes, in_off, in_len, np.array(sizes, dtype=np.uint64), settings)
        print(f"  {name}: serial {fmt(t[0])}")
        for x, pl in zip(t[1:], plans[1:]):
            print(f"    {pl['rounds']:3d} rounds, {pl['workspace_bytes'] / MIB:7.1f} MiB: {fmt(x)}")
        codec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.environ.get("AEC_AMD_LIB_PARENT"), help="libaec.so.0 of the parent commit")
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    import torch
    from libaec_amd import gpu
    if args.sweep:
        sweep(torch, gpu)
    else:
        bench_rows(torch, gpu, args.parent)


if __name__ == "__main__":
    main()
