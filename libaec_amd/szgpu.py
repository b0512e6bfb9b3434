"""SZIP chunks that stay on the device (include/aec_gpu_sz.h) for torch tensors living in HBM.

torch is used for device memory and streams only; byte planes, scan-line padding and the coder are kernels launched by
libaec.so.0 through the C entry points declared in aec_gpu_sz.h.  Same parameters as szip.py (the host-buffer SZIP calls).
"""
import ctypes as C

import numpy as np

from . import gpu
from .szip import SZ_com_t

AEC_CONF_ERROR = -1


class Layout(C.Structure):
    """aec_gpu_sz_layout_t"""
    _fields_ = [("coder", gpu.Params), ("word", C.c_uint), ("pixel", C.c_uint), ("fill_repeat", C.c_uint),
                ("passthrough", C.c_uint), ("line", C.c_uint64), ("padded_line", C.c_uint64), ("lines", C.c_uint64),
                ("coder_bytes", C.c_uint64), ("coded_bytes", C.c_uint64)]


class ChunksPlan(C.Structure):
    """aec_gpu_sz_chunks_plan_t"""
    _fields_ = [("coder", gpu.Params), ("work_bytes", C.c_size_t), ("out_bound", C.c_size_t), ("rsi_entries", C.c_uint64),
                ("workspace_bytes", C.c_size_t), ("direct", C.c_uint)]


class SzEstimate(C.Structure):
    """aec_gpu_sz_estimate_t"""
    _fields_ = [("total_bytes", C.c_uint64 * 4), ("best", C.c_uint32), ("pad", C.c_uint32)]


class SzEstimatePlan(C.Structure):
    """struct aec_gpu_sz_estimate_plan"""
    _fields_ = [("evaluated", C.c_uint32), ("passes", C.c_uint32), ("pieces", C.c_uint64), ("workspace_bytes", C.c_size_t)]


BATCH_CHUNK_DTYPE = np.dtype([("base_bits", "<u8"), ("bits", "<u8")])
SZ_ESTIMATE_DTYPE = np.dtype([("total_bytes", "<u8", 4), ("best", "<u4"), ("pad", "<u4")])
SZ_ESTIMATE_SIZES = 4               # pixels per block 8, 16, 32, 64 in this order
NOT_ASKED = (1 << 64) - 1

_bound = False


def _lib():
    global _bound
    lib = gpu._lib()
    if not _bound:
        vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
        ps = C.POINTER(SZ_com_t)
        lib.aec_gpu_sz_layout.restype = C.c_int
        lib.aec_gpu_sz_layout.argtypes = [ps, sz, C.POINTER(Layout)]
        lib.aec_gpu_sz_batch_ok.restype = C.c_int
        lib.aec_gpu_sz_batch_ok.argtypes = [ps, sz, u64]
        lib.aec_gpu_sz_marshal_async.restype = C.c_int
        lib.aec_gpu_sz_marshal_async.argtypes = [ps, vp, sz, u64, vp, vp]
        lib.aec_gpu_sz_unmarshal_async.restype = C.c_int
        lib.aec_gpu_sz_unmarshal_async.argtypes = [ps, vp, sz, u64, vp, vp]
        lib.aec_gpu_sz_compress_batch_async.restype = C.c_int
        lib.aec_gpu_sz_compress_batch_async.argtypes = [vp, ps, vp, sz, u64, vp, vp, sz, vp, vp, vp]
        lib.aec_gpu_sz_decompress_batch_async.restype = C.c_int
        lib.aec_gpu_sz_decompress_batch_async.argtypes = [vp, ps, vp, sz, vp, u64, sz, vp, vp, vp, vp, vp, vp]
        lib.aec_gpu_encode_batch_async.restype = C.c_int
        lib.aec_gpu_encode_batch_async.argtypes = [vp, C.POINTER(gpu.Params), vp, C.POINTER(u64), u64, vp, sz, vp, vp]
        if hasattr(lib, "aec_gpu_sz_chunks_plan"):          # (AEC_AMD_LIB: a build from before the calls)
            lib.aec_gpu_sz_chunks_plan.restype = C.c_int
            lib.aec_gpu_sz_chunks_plan.argtypes = [ps, vp, u64, C.POINTER(ChunksPlan), vp]
            lib.aec_gpu_sz_compress_chunks_async.restype = C.c_int
            lib.aec_gpu_sz_compress_chunks_async.argtypes = [vp, ps, vp, vp, vp, u64, vp, vp, sz, vp, vp, vp, vp]
            lib.aec_gpu_sz_decompress_chunks_async.restype = C.c_int
            lib.aec_gpu_sz_decompress_chunks_async.argtypes = [vp, ps, vp, sz, vp, vp, vp, vp, u64, vp, C.c_int, vp, vp, vp,
                                                               vp, vp]
        if hasattr(lib, "aec_gpu_sz_estimate_plan"):        # (AEC_AMD_LIB: a build from before the call)
            lib.aec_gpu_sz_estimate_plan.restype = C.c_int
            lib.aec_gpu_sz_estimate_plan.argtypes = [ps, vp, vp, u64, C.POINTER(SzEstimatePlan)]
            lib.aec_gpu_sz_estimate_async.restype = C.c_int
            lib.aec_gpu_sz_estimate_async.argtypes = [vp, ps, vp, vp, vp, vp, u64, vp, vp, vp]
        _bound = True
    return lib


def _u64(a):
    """a host array of uint64 for a call (None stays None); the array must outlive the call, so it is returned"""
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint64)


def _host(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def chunks_plan(options_mask, bits_per_pixel, pixels_per_block, pixels_per_scanline, sizes):
    """aec_gpu_sz_chunks_plan (host arithmetic, no device needed) for chunks of `sizes` bytes under one SZ_com_t.  Returns
    the dict {coder, work_bytes, out_bound, rsi_entries, workspace_bytes, direct, work_offsets}, or None where the batch
    would be refused."""
    lib = _lib()
    p = SZ_com_t(options_mask, bits_per_pixel, pixels_per_block, pixels_per_scanline)
    sizes = _u64(sizes)
    offs = np.zeros(max(1, sizes.size), dtype=np.uint64)
    plan = ChunksPlan()
    if not lib.aec_gpu_sz_chunks_plan(C.byref(p), _host(sizes), sizes.size, C.byref(plan), _host(offs)):
        return None
    return dict(coder=(plan.coder.bits_per_sample, plan.coder.block_size, plan.coder.rsi, plan.coder.flags),
                work_bytes=int(plan.work_bytes), out_bound=int(plan.out_bound), rsi_entries=int(plan.rsi_entries),
                workspace_bytes=int(plan.workspace_bytes), direct=int(plan.direct), work_offsets=offs[:sizes.size])


def _pps(pps):
    """the four candidates' pixels per scan line for a call (None stays None: the SZ_com_t's for all four)"""
    if pps is None:
        return None
    if len(pps) != SZ_ESTIMATE_SIZES:
        raise ValueError("pixels per scan line: one value per pixels-per-block 8, 16, 32, 64 (0: not asked)")
    return (C.c_uint * SZ_ESTIMATE_SIZES)(*[int(v) for v in pps])


def estimate_plan(options_mask, bits_per_pixel, pixels_per_scanline, sizes, pps=None):
    """aec_gpu_sz_estimate_plan (host arithmetic, no device needed) for chunks of `sizes` bytes: the dict {evaluated, passes,
    pieces, workspace_bytes}, or None where the call would be refused.  pps: per pixels-per-block 8, 16, 32, 64 the pixels
    per scan line (0: not asked); None: pixels_per_scanline for all four."""
    p = SZ_com_t(options_mask, bits_per_pixel, 0, pixels_per_scanline)
    sizes = _u64(sizes)
    plan = SzEstimatePlan()
    if not _lib().aec_gpu_sz_estimate_plan(C.byref(p), _pps(pps), _host(sizes), sizes.size, C.byref(plan)):
        return None
    return dict(evaluated=int(plan.evaluated), passes=int(plan.passes), pieces=int(plan.pieces),
                workspace_bytes=int(plan.workspace_bytes))


def layout(options_mask, bits_per_pixel, pixels_per_block, pixels_per_scanline, chunk_bytes):
    """aec_gpu_sz_layout (host arithmetic, no device needed): a Layout, or None where the call says AEC_CONF_ERROR"""
    p = SZ_com_t(options_mask, bits_per_pixel, pixels_per_block, pixels_per_scanline)
    out = Layout()
    rc = _lib().aec_gpu_sz_layout(C.byref(p), chunk_bytes, C.byref(out))
    if rc == AEC_CONF_ERROR:
        return None
    if rc != 0:
        raise RuntimeError(f"aec_gpu_sz_layout failed ({rc})")
    return out


def batch_ok(options_mask, bits_per_pixel, pixels_per_block, pixels_per_scanline, chunk_bytes, n_chunks):
    """aec_gpu_sz_batch_ok: 1 when compress_batch / decompress_batch take such a batch in one call"""
    p = SZ_com_t(options_mask, bits_per_pixel, pixels_per_block, pixels_per_scanline)
    return int(_lib().aec_gpu_sz_batch_ok(C.byref(p), chunk_bytes, n_chunks))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class SzCodec:
    """One SZ_com_t and one aec_gpu context (workspace) on the current torch device."""

    def __init__(self, options_mask, bits_per_pixel, pixels_per_block, pixels_per_scanline):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("libaec_amd.szgpu needs a HIP device (no CPU implementation)")
        self.torch = torch
        self.lib = _lib()
        self.sz = SZ_com_t(options_mask, bits_per_pixel, pixels_per_block, pixels_per_scanline)
        if layout(options_mask, bits_per_pixel, pixels_per_block, pixels_per_scanline, 64) is None:
            raise ValueError("invalid SZIP parameters (aec_gpu_sz_layout -> AEC_CONF_ERROR)")
        self.ctx = C.c_void_p()
        torch.zeros(1, device="cuda")          # make sure the HIP context of this device is current
        rc = self.lib.aec_gpu_create(C.byref(self.ctx))
        if rc != 0:
            raise RuntimeError(f"aec_gpu_create failed ({rc})")

    def close(self):
        if self.ctx:
            self.lib.aec_gpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self, stream):
        return C.c_void_p(stream if stream is not None else self.torch.cuda.current_stream().cuda_stream)

    def layout(self, chunk_bytes):
        s = self.sz
        return layout(s.options_mask, s.bits_per_pixel, s.pixels_per_block, s.pixels_per_scanline, chunk_bytes)

    def batch_ok(self, chunk_bytes, n_chunks):
        return int(self.lib.aec_gpu_sz_batch_ok(C.byref(self.sz), chunk_bytes, n_chunks))

    def encode_bound(self, chunk_bytes):
        """bytes (a multiple of 16) that hold the stream of any chunk of this size"""
        L = self.layout(chunk_bytes)
        return int(self.lib.aec_gpu_encode_bound(C.byref(L.coder), L.coder_bytes))

    # ---- enqueue -------------------------------------------------------------------------------
    def marshal_async(self, d_src, chunk_bytes, n_chunks, d_coder_in, stream=None):
        """d_src: uint8 CUDA tensor of n equal chunks back to back; d_coder_in: 16-byte aligned, n * coder_bytes"""
        return self.lib.aec_gpu_sz_marshal_async(C.byref(self.sz), _ptr(d_src), chunk_bytes, n_chunks, _ptr(d_coder_in),
                                                 self._stream(stream))

    def unmarshal_async(self, d_coder_out, chunk_bytes, n_chunks, d_dst, stream=None):
        return self.lib.aec_gpu_sz_unmarshal_async(C.byref(self.sz), _ptr(d_coder_out), chunk_bytes, n_chunks, _ptr(d_dst),
                                                   self._stream(stream))

    def compress_batch_async(self, d_src, chunk_bytes, n_chunks, d_work, d_out, d_chunks, d_result, stream=None):
        """d_work: n * coder_bytes bytes, 16-byte aligned (None when the layout says passthrough); d_chunks: n * 16 bytes
        (BATCH_CHUNK_DTYPE); d_result: 24 bytes (gpu.ENC_RESULT_DTYPE).  Returns the call's return code."""
        return self.lib.aec_gpu_sz_compress_batch_async(self.ctx, C.byref(self.sz), _ptr(d_src), chunk_bytes, n_chunks,
                                                        _ptr(d_work), _ptr(d_out), d_out.numel(), _ptr(d_chunks),
                                                        _ptr(d_result), self._stream(stream))

    def decompress_batch_async(self, d_in, in_bytes, d_chunk_offsets, n_chunks, chunk_bytes, d_rsi_offsets, d_work, d_dst,
                               d_results, d_result, stream=None):
        """d_chunk_offsets: int64 tensor, n + 1 byte offsets (multiples of 16); d_rsi_offsets: int64, n * lines;
        d_results: n * 40 bytes, d_result: 40 bytes (gpu.DEC_RESULT_DTYPE).  Returns the call's return code."""
        return self.lib.aec_gpu_sz_decompress_batch_async(self.ctx, C.byref(self.sz), _ptr(d_in), in_bytes,
                                                          _ptr(d_chunk_offsets), n_chunks, chunk_bytes, _ptr(d_rsi_offsets),
                                                          _ptr(d_work), _ptr(d_dst), _ptr(d_results), _ptr(d_result),
                                                          self._stream(stream))

    def encode_chunks_async(self, d_coder_in, coder_bytes, n_chunks, d_out, slot_bytes, d_results, stream=None):
        """the path for batches batch_ok refuses: aec_gpu_encode_batch_async, chunk by chunk, over marshalled chunks
        (d_results: n * 24 bytes)"""
        L = self.layout(64)
        for i in range(n_chunks):
            offs = (C.c_uint64 * 2)(0, coder_bytes)
            rc = self.lib.aec_gpu_encode_batch_async(
                self.ctx, C.byref(L.coder), C.c_void_p(d_coder_in.data_ptr() + i * coder_bytes), offs, 1,
                C.c_void_p(d_out.data_ptr() + i * slot_bytes), slot_bytes, C.c_void_p(d_results.data_ptr() + i * 24),
                self._stream(stream))
            if rc != 0:
                return rc
        return 0

    # ---- chunks of any size, one call (aec_gpu_sz_*_chunks_async) ---------------------------------
    def chunks_plan(self, sizes):
        s = self.sz
        return chunks_plan(s.options_mask, s.bits_per_pixel, s.pixels_per_block, s.pixels_per_scanline, sizes)

    def compress_chunks_async(self, d_src, src_offsets, sizes, d_work, d_out, out_cap, d_chunks, d_table, d_result, stream=None):
        """src_offsets / sizes: uint64 arrays on the host; d_work: the plan's work_bytes, 16-byte aligned (None when the
        chunks are coded where they lie); d_chunks: n * 16 bytes (BATCH_CHUNK_DTYPE); d_table: int64 tensor of the plan's
        rsi_entries, or None; d_result: 24 bytes.  Returns the call's return code."""
        offs, sizes = _u64(src_offsets), _u64(sizes)
        return self.lib.aec_gpu_sz_compress_chunks_async(self.ctx, C.byref(self.sz), _ptr(d_src), _host(offs), _host(sizes),
                                                         sizes.size, _ptr(d_work), _ptr(d_out), out_cap, _ptr(d_chunks),
                                                         _ptr(d_table), _ptr(d_result), self._stream(stream))

    def decompress_chunks_async(self, d_in, in_bytes, in_offsets, in_sizes, dst_offsets, sizes, d_table, have_table, d_work,
                                d_dst, d_results, d_result, stream=None):
        """in_offsets / in_sizes (None with a table), dst_offsets, sizes: uint64 arrays on the host; d_table: int64 tensor
        of the plan's rsi_entries; d_results: n * 40 bytes, d_result: 40 bytes.  Returns the call's return code."""
        ino, ins, dso, sizes = _u64(in_offsets), _u64(in_sizes), _u64(dst_offsets), _u64(sizes)
        return self.lib.aec_gpu_sz_decompress_chunks_async(self.ctx, C.byref(self.sz), _ptr(d_in), in_bytes, _host(ino),
                                                           _host(ins), _host(dso), _host(sizes), sizes.size, _ptr(d_table),
                                                           int(bool(have_table)), _ptr(d_work), _ptr(d_dst), _ptr(d_results),
                                                           _ptr(d_result), self._stream(stream))

    # ---- which pixels_per_block? (aec_gpu_sz_estimate_async) -------------------------------------
    def estimate_plan(self, sizes, pps=None):
        s = self.sz
        return estimate_plan(s.options_mask, s.bits_per_pixel, s.pixels_per_scanline, sizes, pps)

    def estimate_async(self, d_src, src_offsets, sizes, d_chunk_bits, d_estimate, pps=None, stream=None):
        """src_offsets / sizes: uint64 arrays on the host; d_chunk_bits: int64 tensor of n * 4 entries, or None;
        d_estimate: 40 bytes (SZ_ESTIMATE_DTYPE).  Returns the call's return code."""
        offs, sizes = _u64(src_offsets), _u64(sizes)
        return self.lib.aec_gpu_sz_estimate_async(self.ctx, C.byref(self.sz), _pps(pps), _ptr(d_src), _host(offs), _host(sizes),
                                                  sizes.size, _ptr(d_chunk_bits), _ptr(d_estimate), self._stream(stream))

    def estimate(self, d_src, src_offsets, sizes, pps=None):
        """the length of SZ_BufftoBuffCompress's streams of the chunks under pixels per block 8, 16, 32, 64 ->
        (total_bytes, best, chunk_bits): total_bytes[i] over all chunks (None: not asked), best the index of the smallest,
        chunk_bits an (n, 4) uint64 array of the streams' bits (NOT_ASKED where not asked).  Synchronises."""
        torch = self.torch
        n = len(sizes)
        d_bits = torch.zeros(max(1, n) * SZ_ESTIMATE_SIZES, dtype=torch.int64, device=d_src.device)
        d_est = torch.zeros(SZ_ESTIMATE_DTYPE.itemsize, dtype=torch.uint8, device=d_src.device)
        rc = self.estimate_async(d_src, src_offsets, sizes, d_bits, d_est, pps)
        if rc != 0:
            raise ValueError("not an estimate for one call (aec_gpu_sz_estimate_plan)") if rc == AEC_CONF_ERROR else \
                RuntimeError(f"aec_gpu_sz_estimate_async failed ({rc})")
        est = d_est.cpu().numpy().view(SZ_ESTIMATE_DTYPE)[0]
        total = [None if int(v) == NOT_ASKED else int(v) for v in est["total_bytes"]]
        return total, int(est["best"]), d_bits.cpu().numpy().view(np.uint64)[:n * SZ_ESTIMATE_SIZES].reshape(n, SZ_ESTIMATE_SIZES)

    def held_bytes(self):
        self.lib.aec_gpu_held_bytes.restype = C.c_size_t
        self.lib.aec_gpu_held_bytes.argtypes = [C.c_void_p]
        return int(self.lib.aec_gpu_held_bytes(self.ctx))

    def trim(self, keep_bytes=0):
        self.lib.aec_gpu_trim.restype = None
        self.lib.aec_gpu_trim.argtypes = [C.c_void_p, C.c_size_t]
        self.lib.aec_gpu_trim(self.ctx, keep_bytes)

    def set_chunks_index(self, how=gpu.CHUNKS_INDEX_PLANNED, round_bits=0):
        """aec_gpu_set_chunks_index on this codec's context: how decompress_chunks without a table finds the RSI starts"""
        gpu._lib().aec_gpu_set_chunks_index(self.ctx, int(how), int(round_bits))

    def compress_chunks(self, d_src, src_offsets, sizes, want_table=False):
        """chunks of sizes[i] bytes at d_src[src_offsets[i]:] -> (d_out, records, d_table, d_work): stream i is
        d_out[records[i]["base_bits"] // 8 :][: (records[i]["bits"] + 7) // 8], what SZ_BufftoBuffCompress gives for
        chunk i; d_table the int64 RSI table for decompress_chunks (None unless want_table); buffers come from the plan"""
        torch = self.torch
        plan = self.chunks_plan(sizes)
        if plan is None:
            raise ValueError("not a batch for one call (aec_gpu_sz_chunks_plan)")
        n = len(sizes)
        dev = d_src.device
        d_out = torch.empty(plan["out_bound"], dtype=torch.uint8, device=dev)
        d_work = torch.empty(plan["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_rec = torch.zeros(max(1, n) * 2, dtype=torch.int64, device=dev)
        d_res = torch.zeros(gpu.ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_table = torch.zeros(max(1, plan["rsi_entries"]), dtype=torch.int64, device=dev) if want_table else None
        rc = self.compress_chunks_async(d_src, src_offsets, sizes, d_work, d_out, d_out.numel(), d_rec, d_table, d_res)
        if rc != 0:
            raise RuntimeError(f"aec_gpu_sz_compress_chunks_async failed ({rc})")
        if n and d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["overflow"]:
            raise RuntimeError("encode overflow")
        return d_out, d_rec.cpu().numpy().view(np.uint64).view(BATCH_CHUNK_DTYPE)[:n], d_table, d_work

    def decompress_chunks(self, d_in, in_bytes, sizes, d_table=None, in_offsets=None, in_sizes=None):
        """streams -> (d_dst with the chunks back to back, per-chunk records, overall record).  With d_table (of
        compress_chunks(..., want_table=True), positions relative to d_in) no index pass runs; without it the streams are
        in_sizes[i] bytes at d_in[in_offsets[i]:]."""
        torch = self.torch
        plan = self.chunks_plan(sizes)
        if plan is None:
            raise ValueError("not a batch for one call (aec_gpu_sz_chunks_plan)")
        n = len(sizes)
        dev = d_in.device
        dst_offsets = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)
        d_dst = torch.empty(int(dst_offsets[-1]), dtype=torch.uint8, device=dev)
        d_work = torch.empty(plan["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        have = d_table is not None
        if not have:
            d_table = torch.zeros(max(1, plan["rsi_entries"]), dtype=torch.int64, device=dev)
        d_results = torch.zeros(max(1, n) * gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_result = torch.zeros(gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        rc = self.decompress_chunks_async(d_in, in_bytes, in_offsets, in_sizes, dst_offsets[:n], sizes, d_table, have, d_work,
                                          d_dst, d_results, d_result)
        if rc != 0:
            raise RuntimeError(f"aec_gpu_sz_decompress_chunks_async failed ({rc})")
        return (d_dst, d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[:n],
                d_result.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0])

    # ---- convenience (synchronising) -------------------------------------------------------------
    def compress_batch(self, d_src, chunk_bytes, n_chunks):
        """n equal chunks back to back in d_src -> list of the n streams (bytes), each what SZ_BufftoBuffCompress gives"""
        torch = self.torch
        L = self.layout(chunk_bytes)
        if L is None or not self.batch_ok(chunk_bytes, n_chunks):
            raise ValueError("not a batch for one call (aec_gpu_sz_batch_ok)")
        cap = self.encode_bound(chunk_bytes) * n_chunks
        d_out = torch.empty(cap, dtype=torch.uint8, device=d_src.device)
        d_work = None if L.passthrough else torch.empty(n_chunks * L.coder_bytes + 16, dtype=torch.uint8, device=d_src.device)
        d_rec = torch.zeros(n_chunks * 2, dtype=torch.int64, device=d_src.device)
        d_res = torch.zeros(gpu.ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_src.device)
        rc = self.compress_batch_async(d_src, chunk_bytes, n_chunks, d_work, d_out, d_rec, d_res)
        if rc != 0:
            raise RuntimeError(f"aec_gpu_sz_compress_batch_async failed ({rc})")
        rec = d_rec.cpu().numpy().reshape(n_chunks, 2)
        if d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["overflow"]:
            raise RuntimeError("encode overflow")
        out = d_out.cpu().numpy()
        return [out[int(b) // 8:int(b) // 8 + (int(n) + 7) // 8].tobytes() for b, n in rec]

    def decompress_batch(self, d_in, d_chunk_offsets, n_chunks, chunk_bytes):
        """streams at d_in[d_chunk_offsets[i] : d_chunk_offsets[i + 1]] -> (d_dst of n * chunk_bytes, per-chunk records,
        overall record)"""
        torch = self.torch
        L = self.layout(chunk_bytes)
        d_work = torch.empty(n_chunks * L.coder_bytes + 16, dtype=torch.uint8, device=d_in.device)
        d_dst = torch.empty(n_chunks * chunk_bytes, dtype=torch.uint8, device=d_in.device)
        d_off = torch.zeros(n_chunks * L.lines, dtype=torch.int64, device=d_in.device)
        d_results = torch.zeros(n_chunks * gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_in.device)
        d_result = torch.zeros(gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_in.device)
        rc = self.decompress_batch_async(d_in, d_in.numel(), d_chunk_offsets, n_chunks, chunk_bytes, d_off, d_work, d_dst,
                                         d_results, d_result)
        if rc != 0:
            raise RuntimeError(f"aec_gpu_sz_decompress_batch_async failed ({rc})")
        return (d_dst, d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE),
                d_result.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0])
