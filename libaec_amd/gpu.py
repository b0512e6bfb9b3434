"""Device-resident batch interface (include/aec_gpu.h) for torch tensors living in HBM.

torch is used for device memory and streams only; every codec operation is a kernel launched
by libaec.so.0 on the tensor's device through the C entry points declared in aec_gpu.h.
"""
import ctypes as C

import numpy as np

from .api import library


class Params(C.Structure):
    _fields_ = [("bits_per_sample", C.c_uint), ("block_size", C.c_uint), ("rsi", C.c_uint),
                ("flags", C.c_uint)]


class ChunksPlan(C.Structure):
    _fields_ = [("out_bound", C.c_size_t), ("rsi_entries", C.c_uint64), ("workspace_bytes", C.c_size_t),
                ("waves", C.c_uint64)]


class DChunksPlan(C.Structure):
    _fields_ = [("items", C.c_uint64), ("rsi_entries", C.c_uint64), ("out_bytes", C.c_size_t),
                ("workspace_bytes", C.c_size_t)]


class IChunksPlan(C.Structure):
    _fields_ = [("taken", C.c_uint64), ("rounds", C.c_uint64), ("table_bits", C.c_uint64), ("rsi_entries", C.c_uint64),
                ("workspace_bytes", C.c_size_t)]


CHUNKS_INDEX_PLANNED, CHUNKS_INDEX_SERIAL, CHUNKS_INDEX_EVERY_BIT = 0, 1, 2


class Estimate(C.Structure):
    """aec_gpu_estimate: total_bits per block size 8, 16, 32, 64 (~0: not asked for) and the index of the smallest"""
    _fields_ = [("total_bits", C.c_uint64 * 4), ("best", C.c_uint32), ("pad", C.c_uint32)]


class EstimatePlan(C.Structure):
    _fields_ = [("evaluated", C.c_uint32), ("pad", C.c_uint32), ("workspace_bytes", C.c_size_t)]


ESTIMATE_DTYPE = np.dtype([("total_bits", "<u8", (4,)), ("best", "<u4"), ("pad", "<u4")])
SEG_ENTRY_DTYPE = np.dtype([("bit", "<u8"), ("prev", "<u4"), ("pad", "<u4")])
ENC_RESULT_DTYPE = np.dtype([("total_bits", "<u8"), ("k_out", "<u4"), ("overflow", "<u4"),
                             ("k_lo", "<u4"), ("k_hi", "<u4")])
DEC_RESULT_DTYPE = np.dtype([("n_rsi", "<u8"), ("tail_blocks", "<u8"), ("end_bit", "<u8"),
                             ("status", "<u4"), ("pad", "<u4"), ("bad_rsi", "<u8")])

_bound = False


def _lib():
    global _bound
    lib = library()
    if not _bound:
        vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
        pp = C.POINTER(Params)
        lib.aec_gpu_create.restype = C.c_int
        lib.aec_gpu_create.argtypes = [C.POINTER(vp)]
        lib.aec_gpu_destroy.restype = None
        lib.aec_gpu_destroy.argtypes = [vp]
        lib.aec_gpu_check_params.restype = C.c_int
        lib.aec_gpu_check_params.argtypes = [pp, C.c_int]
        lib.aec_gpu_encode_bound.restype = sz
        lib.aec_gpu_encode_bound.argtypes = [pp, sz]
        lib.aec_gpu_rsi_count.restype = u64
        lib.aec_gpu_rsi_count.argtypes = [pp, sz]
        lib.aec_gpu_block_count.restype = u64
        lib.aec_gpu_block_count.argtypes = [pp, sz]
        lib.aec_gpu_reserve.restype = C.c_int
        lib.aec_gpu_reserve.argtypes = [vp, pp, sz]
        lib.aec_gpu_encode_async.restype = C.c_int
        lib.aec_gpu_encode_async.argtypes = [vp, pp, vp, sz, vp, sz, C.c_uint, C.c_uint, vp, vp, vp]
        lib.aec_gpu_encode_plan_async.restype = C.c_int
        lib.aec_gpu_encode_plan_async.argtypes = [vp, pp, vp, sz, vp, vp]
        lib.aec_gpu_encode_emit_async.restype = C.c_int
        lib.aec_gpu_encode_emit_async.argtypes = [vp, pp, vp, sz, vp, sz, C.c_uint, C.c_uint, vp, vp, vp]
        lib.aec_gpu_encode_emit_planned_async.restype = C.c_int
        lib.aec_gpu_encode_emit_planned_async.argtypes = [vp, pp, vp, sz, vp, sz, vp, C.c_uint, vp, vp, vp]
        lib.aec_gpu_stitch_async.restype = C.c_int
        lib.aec_gpu_stitch_async.argtypes = [vp, sz, vp, C.c_uint, vp, sz, vp, vp]
        lib.aec_gpu_index_resume_async.restype = C.c_int
        lib.aec_gpu_index_resume_async.argtypes = [vp, pp, vp, sz, u64, C.c_uint, u64, vp, u64, vp, vp]
        lib.aec_gpu_decode_indexed_async.restype = C.c_int
        lib.aec_gpu_decode_indexed_async.argtypes = [vp, pp, vp, sz, vp, u64, vp, vp, vp, vp]
        lib.aec_gpu_decode_async.restype = C.c_int
        lib.aec_gpu_decode_async.argtypes = [vp, pp, vp, sz, vp, u64, u64, vp, vp, vp]
        lib.aec_gpu_segment_count.restype = u64
        lib.aec_gpu_segment_count.argtypes = [pp, sz]
        lib.aec_gpu_set_segment_table.restype = None
        lib.aec_gpu_set_segment_table.argtypes = [vp, vp]
        lib.aec_gpu_decode_segments_async.restype = C.c_int
        lib.aec_gpu_decode_segments_async.argtypes = [vp, pp, vp, sz, vp, u64, u64, vp, vp, vp]
        lib.aec_gpu_index_batch_async.restype = C.c_int
        lib.aec_gpu_index_batch_async.argtypes = [vp, pp, vp, sz, vp, u64, u64, vp, vp, vp]
        lib.aec_gpu_uniform_batch_ok.restype = C.c_int
        lib.aec_gpu_uniform_batch_ok.argtypes = [pp, sz, u64]
        lib.aec_gpu_encode_uniform_batch_async.restype = C.c_int
        lib.aec_gpu_encode_uniform_batch_async.argtypes = [vp, pp, vp, sz, u64, vp, sz, vp, vp, vp]
        lib.aec_gpu_encode_chunks_plan.restype = C.c_int
        lib.aec_gpu_encode_chunks_plan.argtypes = [pp, vp, u64, C.POINTER(ChunksPlan)]
        lib.aec_gpu_encode_chunks_async.restype = C.c_int
        lib.aec_gpu_encode_chunks_async.argtypes = [vp, pp, vp, vp, vp, u64, vp, sz, vp, vp, vp, vp]
        if hasattr(lib, "aec_gpu_decode_chunks_plan"):      # (AEC_AMD_LIB: a build from before the call)
            lib.aec_gpu_decode_chunks_plan.restype = C.c_int
            lib.aec_gpu_decode_chunks_plan.argtypes = [pp, vp, u64, C.POINTER(DChunksPlan)]
            lib.aec_gpu_decode_chunks_async.restype = C.c_int
            lib.aec_gpu_decode_chunks_async.argtypes = [vp, pp, vp, sz, vp, vp, vp, vp, u64, vp, C.c_int, vp, vp, vp, vp]
        if hasattr(lib, "aec_gpu_index_chunks_async"):      # (AEC_AMD_LIB: a build from before the call)
            lib.aec_gpu_set_chunks_index.restype = None
            lib.aec_gpu_set_chunks_index.argtypes = [vp, C.c_int, u64]
            lib.aec_gpu_index_chunks_plan.restype = C.c_int
            lib.aec_gpu_index_chunks_plan.argtypes = [pp, C.c_int, u64, vp, vp, u64, C.POINTER(IChunksPlan)]
            lib.aec_gpu_index_chunks_async.restype = C.c_int
            lib.aec_gpu_index_chunks_async.argtypes = [vp, pp, vp, sz, vp, vp, vp, u64, vp, vp, vp, vp]
        if hasattr(lib, "aec_gpu_estimate_async"):          # (AEC_AMD_LIB: a build from before the call)
            lib.aec_gpu_estimate_plan.restype = C.c_int
            lib.aec_gpu_estimate_plan.argtypes = [pp, C.POINTER(C.c_uint), sz, C.POINTER(EstimatePlan)]
            lib.aec_gpu_estimate_async.restype = C.c_int
            lib.aec_gpu_estimate_async.argtypes = [vp, pp, vp, sz, C.POINTER(C.c_uint), vp, vp]
        lib.aec_gpu_index_async.restype = C.c_int
        lib.aec_gpu_index_async.argtypes = [vp, pp, vp, sz, u64, vp, u64, vp, vp]
        lib.aec_gpu_segments_per_rsi.restype = C.c_uint
        lib.aec_gpu_segments_per_rsi.argtypes = [pp]
        lib.aec_gpu_index_segments_async.restype = C.c_int
        lib.aec_gpu_index_segments_async.argtypes = [vp, pp, vp, sz, u64, C.c_uint, u64, vp, vp, u64, vp, vp]
        lib.aec_gpu_index_scheme.restype = C.c_int
        lib.aec_gpu_index_scheme.argtypes = [pp, sz, u64, C.c_uint]
        lib.aec_gpu_index_plan.restype = C.c_int
        lib.aec_gpu_index_plan.argtypes = [pp, sz, u64, C.c_uint, C.c_int, C.c_int, sz, C.POINTER(C.c_int),
                                           C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
        lib.aec_gpu_decode_bare_async.restype = C.c_int
        lib.aec_gpu_decode_bare_async.argtypes = [vp, pp, vp, sz, vp, vp, u64, u64, vp, vp, vp, vp]
        _bound = True
    return lib


def _ptr(t):
    """the address of a tensor's data as a c_void_p; None is the NULL pointer"""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _call(fn, *args):
    """calls an entry point of the library; a return code other than 0 raises"""
    rc = fn(*args)
    if rc != 0:
        raise RuntimeError(f"{fn.__name__} failed ({rc})")


def bytes_per_sample(bits_per_sample, flags):
    """bytes a sample takes in memory: 1, 2, 4, or 3 for 17 to 24 bits with AEC_DATA_3BYTE (flag 2)"""
    if bits_per_sample > 16:
        return 3 if bits_per_sample <= 24 and flags & 2 else 4
    return 2 if bits_per_sample > 8 else 1


def stitch_async(d_gathered, slot, d_plans, world, d_stream, d_total=None, stream=None):
    """aec_gpu_stitch_async: compact the all-gathered slices (world slots of `slot` bytes in d_gathered,
    16 readable bytes behind the last) into one stream at d_stream, on the device."""
    import torch
    lib = _lib()
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    _call(lib.aec_gpu_stitch_async, _ptr(d_gathered), slot, _ptr(d_plans), world, _ptr(d_stream), d_stream.numel(),
          _ptr(d_total), st)


INDEX_SCHEMES = ("serial walk", "phase-locked chains", "window tables", "trunk", "every bit parsed (small streams)",
                 "regions walked from guessed entries (large streams)")


def index_scheme(bits_per_sample, block_size, rsi, flags, in_bytes, rsi_bits=0, start_block=0):
    """aec_gpu_index_scheme: which scheme the index pass of such a stream takes (index into INDEX_SCHEMES)."""
    p = Params(bits_per_sample, block_size, rsi, flags)
    return _lib().aec_gpu_index_scheme(C.byref(p), in_bytes, rsi_bits, start_block)


def index_plan(bits_per_sample, block_size, rsi, flags, in_bytes, rsi_bits=0, start_block=0, want_segments=False,
               piece=False, ws_bytes=0):
    """aec_gpu_index_plan: the chain of schemes the index pass of such a stream enqueues (indices into INDEX_SCHEMES), the
    workspace the pass asks for, what it asks for without the every-bit scheme's tables, what the chain occupies."""
    p = Params(bits_per_sample, block_size, rsi, flags)
    ids = (C.c_int * 6)()
    asked, large, used = C.c_size_t(), C.c_size_t(), C.c_size_t()
    n = _lib().aec_gpu_index_plan(C.byref(p), in_bytes, rsi_bits, start_block, int(want_segments), int(piece), ws_bytes,
                                  ids, C.byref(asked), C.byref(large), C.byref(used))
    if n < 0:
        raise ValueError("invalid stream parameters")
    return list(ids[:n]), asked.value, large.value, used.value


def encode_chunks_plan(bits_per_sample, block_size, rsi, flags, sizes):
    """aec_gpu_encode_chunks_plan: host arithmetic of a batch of chunks of `sizes` bytes.  Returns the dict
    {out_bound, rsi_entries, workspace_bytes, waves}, or None where the batch would be refused."""
    p = Params(bits_per_sample, block_size, rsi, flags)
    a = np.ascontiguousarray(sizes, dtype=np.uint64)
    plan = ChunksPlan()
    if not _lib().aec_gpu_encode_chunks_plan(C.byref(p), C.c_void_p(a.ctypes.data), a.size, C.byref(plan)):
        return None
    return {"out_bound": int(plan.out_bound), "rsi_entries": int(plan.rsi_entries),
            "workspace_bytes": int(plan.workspace_bytes), "waves": int(plan.waves)}


def decode_chunks_plan(bits_per_sample, block_size, rsi, flags, out_sizes):
    """aec_gpu_decode_chunks_plan: host arithmetic of a batch of chunks that decode to `out_sizes` bytes.  Returns the dict
    {items, rsi_entries, out_bytes, workspace_bytes}, or None where the batch would be refused."""
    p = Params(bits_per_sample, block_size, rsi, flags)
    a = np.ascontiguousarray(out_sizes, dtype=np.uint64)
    plan = DChunksPlan()
    if not _lib().aec_gpu_decode_chunks_plan(C.byref(p), C.c_void_p(a.ctypes.data), a.size, C.byref(plan)):
        return None
    return {"items": int(plan.items), "rsi_entries": int(plan.rsi_entries), "out_bytes": int(plan.out_bytes),
            "workspace_bytes": int(plan.workspace_bytes)}


def index_chunks_plan(bits_per_sample, block_size, rsi, flags, in_sizes, out_sizes, how=CHUNKS_INDEX_PLANNED, round_bits=0):
    """aec_gpu_index_chunks_plan: host arithmetic of the index pass of a batch of bare streams of `in_sizes` bytes that
    decode to `out_sizes` bytes, run as `how` (CHUNKS_INDEX_*) with rounds of `round_bits` table entries (0: the default).
    Returns the dict {taken, rounds, table_bits, rsi_entries, workspace_bytes}, or None where the batch would be refused."""
    p = Params(bits_per_sample, block_size, rsi, flags)
    a = np.ascontiguousarray(in_sizes, dtype=np.uint64)
    b = np.ascontiguousarray(out_sizes, dtype=np.uint64)
    if a.size != b.size:
        raise ValueError("in_sizes and out_sizes differ in length")
    plan = IChunksPlan()
    if not _lib().aec_gpu_index_chunks_plan(C.byref(p), int(how), int(round_bits), C.c_void_p(a.ctypes.data),
                                            C.c_void_p(b.ctypes.data), a.size, C.byref(plan)):
        return None
    return {"taken": int(plan.taken), "rounds": int(plan.rounds), "table_bits": int(plan.table_bits),
            "rsi_entries": int(plan.rsi_entries), "workspace_bytes": int(plan.workspace_bytes)}


def _rsi4(rsi):
    """the four RSIs of an estimate as the C array; None stays NULL (the parameter set's rsi for all four sizes)"""
    if rsi is None:
        return None
    if len(rsi) != 4:
        raise ValueError("rsi: one value per block size 8, 16, 32, 64 (0 = not evaluated), or None")
    return (C.c_uint * 4)(*[int(r) for r in rsi])


def estimate_plan(bits_per_sample, flags, rsi, in_bytes, rsi_all=0):
    """aec_gpu_estimate_plan: host arithmetic of an estimate of in_bytes.  rsi: four RSIs in blocks for block sizes 8, 16,
    32, 64 (0 = not evaluated) or None (rsi_all, the parameter set's rsi, for all).  Returns the dict {evaluated, workspace_bytes}, or None where
    the call would be refused."""
    p = Params(bits_per_sample, 0, rsi_all, flags)
    plan = EstimatePlan()
    if not _lib().aec_gpu_estimate_plan(C.byref(p), _rsi4(rsi), in_bytes, C.byref(plan)):
        return None
    return {"evaluated": int(plan.evaluated), "workspace_bytes": int(plan.workspace_bytes)}


class Codec:
    """One aec_gpu context (workspace) on the current torch device."""

    def __init__(self, bits_per_sample, block_size, rsi, flags):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("libaec_amd.gpu needs a HIP device (no CPU implementation)")
        self.torch = torch
        self.lib = _lib()
        self.p = Params(bits_per_sample, block_size, rsi, flags)
        rc = self.lib.aec_gpu_check_params(C.byref(self.p), 1)
        if rc != 0:
            raise ValueError(f"invalid stream parameters (aec_gpu_check_params -> {rc})")
        self.ctx = C.c_void_p()
        torch.cuda.current_device()
        torch.zeros(1, device="cuda")          # make sure the HIP context of this device is current
        _call(self.lib.aec_gpu_create, C.byref(self.ctx))

    def close(self):
        if self.ctx:
            self.lib.aec_gpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- sizes ---------------------------------------------------------------------------------
    def encode_bound(self, in_bytes):
        return int(self.lib.aec_gpu_encode_bound(C.byref(self.p), in_bytes))

    def rsi_count(self, in_bytes):
        return int(self.lib.aec_gpu_rsi_count(C.byref(self.p), in_bytes))

    def block_count(self, in_bytes):
        return int(self.lib.aec_gpu_block_count(C.byref(self.p), in_bytes))

    def segment_count(self, in_bytes):
        return int(self.lib.aec_gpu_segment_count(C.byref(self.p), in_bytes))

    def set_segment_table(self, d_table):
        """d_table: uint8 CUDA tensor of segment_count * 16 bytes (or None): filled by later encodes"""
        self._seg_table = d_table          # keep it alive
        self.lib.aec_gpu_set_segment_table(self.ctx, _ptr(d_table))

    def decode_segments_async(self, d_in, in_bytes, d_table, n_seg, total_blocks, d_out, d_result, stream=None):
        self._enqueue(self.lib.aec_gpu_decode_segments_async, stream, _ptr(d_in), in_bytes, _ptr(d_table), n_seg, total_blocks,
                      _ptr(d_out), _ptr(d_result))

    def reserve(self, in_bytes):
        rc = self.lib.aec_gpu_reserve(self.ctx, C.byref(self.p), in_bytes)
        if rc != 0:
            raise MemoryError(f"aec_gpu_reserve({in_bytes}) failed ({rc})")

    def held_bytes(self):
        """aec_gpu_held_bytes: device memory the context holds between calls"""
        self.lib.aec_gpu_held_bytes.restype = C.c_size_t
        self.lib.aec_gpu_held_bytes.argtypes = [C.c_void_p]
        return int(self.lib.aec_gpu_held_bytes(self.ctx))

    def trim(self, keep_bytes=0):
        """aec_gpu_trim: release every buffer of the context above keep_bytes (synchronises the device)"""
        self.lib.aec_gpu_trim.restype = None
        self.lib.aec_gpu_trim.argtypes = [C.c_void_p, C.c_size_t]
        self.lib.aec_gpu_trim(self.ctx, keep_bytes)

    def _stream(self, stream):
        return C.c_void_p(stream if stream is not None else self.torch.cuda.current_stream().cuda_stream)

    # ---- enqueue -------------------------------------------------------------------------------
    def _enqueue(self, fn, stream, *args):
        """fn(context, parameters, args..., stream): every *_async entry point has this shape"""
        _call(fn, self.ctx, C.byref(self.p), *args, self._stream(stream))

    def encode_async(self, d_in, in_bytes, d_out, d_offsets, d_result, start_bit=0, k_in=0, stream=None):
        """d_in/d_out: uint8 CUDA tensors; d_offsets: int64 tensor with rsi_count+1 entries or None;
        d_result: uint8 tensor of >= 16 bytes."""
        self._enqueue(self.lib.aec_gpu_encode_async, stream, _ptr(d_in), in_bytes, _ptr(d_out), d_out.numel(), start_bit, k_in,
                      _ptr(d_offsets), _ptr(d_result))

    def encode_plan_async(self, d_in, in_bytes, d_result, stream=None):
        """first half of an encode: leaves total_bits and (k_lo, k_hi) in d_result"""
        self._enqueue(self.lib.aec_gpu_encode_plan_async, stream, _ptr(d_in), in_bytes, _ptr(d_result))

    def estimate_async(self, d_in, in_bytes, rsi, d_estimate, stream=None):
        """aec_gpu_estimate_async: the exact total_bits of d_in under block sizes 8, 16, 32 and 64 from one pass, into
        d_estimate (uint8 tensor of 40 bytes: ESTIMATE_DTYPE).  rsi: four RSIs in blocks (0 = not evaluated) or None (this
        codec's rsi for all); the codec's block size plays no part.  Returns the call's return code."""
        return self.lib.aec_gpu_estimate_async(self.ctx, C.byref(self.p), _ptr(d_in), in_bytes, _rsi4(rsi),
                                               _ptr(d_estimate), self._stream(stream))

    def estimate(self, d_in, rsi=None):
        """estimate_async on the whole tensor, synchronising: returns (total_bits[4], best); a size not asked for has
        total_bits None"""
        d_est = self.torch.zeros(ESTIMATE_DTYPE.itemsize, dtype=self.torch.uint8, device=d_in.device)
        rc = self.estimate_async(d_in, d_in.numel(), rsi, d_est)
        if rc != 0:
            raise ValueError(f"aec_gpu_estimate_async failed ({rc})")
        rec = d_est.cpu().numpy().view(ESTIMATE_DTYPE)[0]
        none = (1 << 64) - 1
        return [None if int(t) == none else int(t) for t in rec["total_bits"]], int(rec["best"])

    def encode_emit_async(self, d_in, in_bytes, d_out, d_offsets, d_result, start_bit, k_in, stream=None):
        """second half: writes the stream at bit `start_bit` of d_out[0] with carried k `k_in`"""
        self._enqueue(self.lib.aec_gpu_encode_emit_async, stream, _ptr(d_in), in_bytes, _ptr(d_out), d_out.numel(), start_bit,
                      k_in, _ptr(d_offsets), _ptr(d_result))

    def encode_emit_planned_async(self, d_in, in_bytes, d_out, d_offsets, d_result, d_plans, rank, stream=None):
        """second half without a host round trip: d_plans = the all-gathered 24-byte plan records of
        all shards (uint8 tensor, world * 24 bytes), rank = this shard's index; start bit and carried
        k are computed on the device"""
        self._enqueue(self.lib.aec_gpu_encode_emit_planned_async, stream, _ptr(d_in), in_bytes, _ptr(d_out), d_out.numel(),
                      _ptr(d_plans), rank, _ptr(d_offsets), _ptr(d_result))

    def index_resume_async(self, d_in, in_bytes, start_bit, start_block, rsi_start_bit, d_offsets, max_rsi,
                           d_result, stream=None):
        """d_offsets needs max_rsi + 1 entries (the last receives the start of the trailing partial RSI)"""
        self._enqueue(self.lib.aec_gpu_index_resume_async, stream, _ptr(d_in), in_bytes, start_bit, start_block, rsi_start_bit,
                      _ptr(d_offsets), max_rsi, _ptr(d_result))

    def decode_indexed_async(self, d_in, in_bytes, d_offsets, max_rsi, d_index_result, d_out, d_result, stream=None):
        self._enqueue(self.lib.aec_gpu_decode_indexed_async, stream, _ptr(d_in), in_bytes, _ptr(d_offsets), max_rsi,
                      _ptr(d_index_result), _ptr(d_out), _ptr(d_result))

    def decode_async(self, d_in, in_bytes, d_offsets, n_rsi, total_blocks, d_out, d_result, stream=None):
        self._enqueue(self.lib.aec_gpu_decode_async, stream, _ptr(d_in), in_bytes, _ptr(d_offsets), n_rsi, total_blocks,
                      _ptr(d_out), _ptr(d_result))

    def index_async(self, d_in, in_bytes, start_bit, d_offsets, max_rsi, d_result, stream=None):
        self._enqueue(self.lib.aec_gpu_index_async, stream, _ptr(d_in), in_bytes, start_bit, _ptr(d_offsets), max_rsi,
                      _ptr(d_result))

    def segments_per_rsi(self):
        return int(self.lib.aec_gpu_segments_per_rsi(C.byref(self.p)))

    def index_segments_async(self, d_in, in_bytes, start_bit, d_offsets, d_seg_bits, max_rsi, d_result, stream=None,
                             start_block=0, rsi_start_bit=0):
        """index pass that also leaves the segment starts: d_offsets int64 (max_rsi + 1), d_seg_bits int64
        ((max_rsi + 1) * segments_per_rsi())"""
        self._enqueue(self.lib.aec_gpu_index_segments_async, stream, _ptr(d_in), in_bytes, start_bit, start_block, rsi_start_bit,
                      _ptr(d_offsets), _ptr(d_seg_bits), max_rsi, _ptr(d_result))

    def decode_bare_async(self, d_in, in_bytes, d_offsets, d_seg_bits, max_rsi, total_blocks, d_index_result, d_out,
                          d_result, stream=None):
        """decode behind index_segments_async, a lane per segment where the index pass found the segment starts;
        d_index_result: the index record (counts taken on the device) or None (max_rsi RSIs, total_blocks blocks)"""
        self._enqueue(self.lib.aec_gpu_decode_bare_async, stream, _ptr(d_in), in_bytes, _ptr(d_offsets), _ptr(d_seg_bits), max_rsi,
                      total_blocks, _ptr(d_index_result), _ptr(d_out), _ptr(d_result))

    def index_batch_async(self, d_in, in_bytes, d_chunk_offsets, n_chunks, rsi_per_chunk, d_offsets, d_results,
                          stream=None):
        """d_chunk_offsets: int64 tensor (n_chunks + 1 byte offsets, multiples of 16);
        d_offsets: int64 tensor (n_chunks * rsi_per_chunk); d_results: uint8 tensor (n_chunks * 40)"""
        self._enqueue(self.lib.aec_gpu_index_batch_async, stream, _ptr(d_in), in_bytes, _ptr(d_chunk_offsets), n_chunks,
                      rsi_per_chunk, _ptr(d_offsets), _ptr(d_results))

    def encode_uniform_batch(self, d_in, chunk_bytes, n_chunks):
        """n equal chunks of whole RSIs, back to back in d_in, as one launch set (include/aec_gpu.h:
        aec_gpu_encode_uniform_batch_async).  Returns (d_out, records) with records[i] = (base_bits, bits) of
        stream i inside d_out; synchronises."""
        torch = self.torch
        if not self.lib.aec_gpu_uniform_batch_ok(C.byref(self.p), chunk_bytes, n_chunks):
            raise ValueError("not a uniform batch (whole RSIs, at most 2048 segments per chunk)")
        cap = (self.encode_bound(chunk_bytes) + 15) // 16 * 16 * n_chunks
        d_out = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
        d_rec = torch.zeros(n_chunks * 2, dtype=torch.int64, device=d_in.device)
        d_res = torch.zeros(ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_in.device)
        self._enqueue(self.lib.aec_gpu_encode_uniform_batch_async, None, _ptr(d_in), chunk_bytes, n_chunks, _ptr(d_out), cap,
                      _ptr(d_rec), _ptr(d_res))
        rec = d_rec.cpu().numpy().reshape(n_chunks, 2)
        res = d_res.cpu().numpy().view(ENC_RESULT_DTYPE)[0]
        if res["overflow"]:
            raise RuntimeError("encode overflow")
        return d_out, rec

    def encode_chunks_plan(self, sizes):
        return encode_chunks_plan(self.p.bits_per_sample, self.p.block_size, self.p.rsi, self.p.flags, sizes)

    def encode_chunks_async(self, d_in, offsets, sizes, d_out, out_cap, d_records, d_table, d_result, stream=None):
        """aec_gpu_encode_chunks_async as it is: offsets / sizes are uint64 numpy arrays on the host, d_records an int64
        tensor of 2 n entries, d_table an int64 tensor of the plan's rsi_entries (or None), d_result 24 bytes"""
        self._enqueue(self.lib.aec_gpu_encode_chunks_async, stream, _ptr(d_in), C.c_void_p(offsets.ctypes.data),
                      C.c_void_p(sizes.ctypes.data), int(sizes.size), _ptr(d_out), out_cap, _ptr(d_records), _ptr(d_table),
                      _ptr(d_result))

    def encode_chunks(self, d_in, offsets, sizes, want_offsets=False, out_cap=None, d_out=None):
        """Chunks of sizes[i] bytes at byte offsets[i] (multiples of 16) of d_in, each a stream of its own, as one launch
        set (include/aec_gpu.h: aec_gpu_encode_chunks_async).  Returns (d_out, records, d_table, result): records[i] =
        (base_bits, bits) of stream i inside d_out, d_table the int64 RSI table (plan rsi_entries entries; None unless
        want_offsets), result the ENC_RESULT_DTYPE record (overflow is reported there, not raised).  out_cap / d_out:
        a capacity or a buffer of the caller's instead of the plan's bound.  Synchronises."""
        torch = self.torch
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        siz = np.ascontiguousarray(sizes, dtype=np.uint64)
        if off.size != siz.size:
            raise ValueError("offsets and sizes differ in length")
        plan = self.encode_chunks_plan(siz)
        if plan is None:
            raise ValueError("aec_gpu_encode_chunks_plan refuses this batch")
        n = int(siz.size)
        cap = plan["out_bound"] if out_cap is None else out_cap
        if d_out is None:
            d_out = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
        d_rec = torch.zeros(max(n, 1) * 2, dtype=torch.int64, device=d_in.device)
        d_tab = torch.zeros(max(plan["rsi_entries"], 1), dtype=torch.int64, device=d_in.device) if want_offsets else None
        d_res = torch.zeros(ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_in.device)
        self.encode_chunks_async(d_in, off, siz, d_out, cap, d_rec, d_tab, d_res)
        rec = d_rec.cpu().numpy().reshape(-1, 2)[:n]
        res = d_res.cpu().numpy().view(ENC_RESULT_DTYPE)[0]
        return d_out, rec, d_tab, res

    def decode_chunks_plan(self, out_sizes):
        return decode_chunks_plan(self.p.bits_per_sample, self.p.block_size, self.p.rsi, self.p.flags, out_sizes)

    def decode_chunks_async(self, d_in, in_bytes, in_offsets, in_sizes, out_offsets, out_sizes, d_table, have_table, d_out,
                            d_records, d_result, stream=None):
        """aec_gpu_decode_chunks_async as it is: the four arrays are uint64 numpy arrays on the host (in_offsets / in_sizes
        may be None with a table), d_table an int64 tensor of the plan's rsi_entries, d_records a uint8 tensor of 40 n
        bytes, d_result one of 40 bytes.  Returns the call's return code."""
        def host(a):
            return C.c_void_p(a.ctypes.data) if a is not None else None
        return self.lib.aec_gpu_decode_chunks_async(
            self.ctx, C.byref(self.p), _ptr(d_in), in_bytes, host(in_offsets), host(in_sizes), host(out_offsets),
            host(out_sizes), int(out_sizes.size), _ptr(d_table), int(have_table), _ptr(d_out), _ptr(d_records), _ptr(d_result),
            self._stream(stream))

    def decode_chunks(self, d_in, in_bytes, out_sizes, d_table=None, in_offsets=None, in_sizes=None):
        """Streams that decode to out_sizes[i] bytes, as one decode launch (include/aec_gpu.h:
        aec_gpu_decode_chunks_async) into a packed output allocated here.  With d_table (the int64 RSI table of
        encode_chunks(..., want_offsets=True), positions relative to d_in) no index pass runs; without it the streams are
        in_sizes[i] bytes at byte in_offsets[i] of d_in and are walked first.  Returns (d_out, out_offsets, records,
        result): chunk i's whole blocks at d_out[out_offsets[i]:], records the DEC_RESULT_DTYPE record per chunk, result
        the overall one.  Synchronises."""
        torch = self.torch
        osz = np.ascontiguousarray(out_sizes, dtype=np.uint64)
        plan = self.decode_chunks_plan(osz)
        if plan is None:
            raise ValueError("aec_gpu_decode_chunks_plan refuses this batch")
        n = int(osz.size)
        nb = bytes_per_sample(self.p.bits_per_sample, self.p.flags)
        blk = self.p.block_size * nb
        rooms = [((int(b) // nb + self.p.block_size - 1) // self.p.block_size * blk + 15) // 16 * 16 for b in osz]
        ooff = np.zeros(n, dtype=np.uint64)
        if n:
            ooff[1:] = np.cumsum(rooms[:-1], dtype=np.uint64)
        ioff = np.ascontiguousarray(in_offsets, dtype=np.uint64) if in_offsets is not None else None
        isz = np.ascontiguousarray(in_sizes, dtype=np.uint64) if in_sizes is not None else None
        if d_table is None and (ioff is None or isz is None or ioff.size != n or isz.size != n):
            raise ValueError("bare streams need in_offsets and in_sizes, one entry per chunk")
        have = d_table is not None
        if not have:
            d_table = torch.zeros(max(plan["rsi_entries"], 1), dtype=torch.int64, device=d_in.device)
        d_out = torch.empty(plan["out_bytes"] + 16, dtype=torch.uint8, device=d_in.device)
        d_rec = torch.zeros(max(n, 1) * DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_in.device)
        d_res = torch.zeros(DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_in.device)
        rc = self.decode_chunks_async(d_in, in_bytes, ioff, isz, ooff, osz, d_table, have, d_out, d_rec, d_res)
        if rc != 0:
            raise RuntimeError(f"aec_gpu_decode_chunks_async failed ({rc})")
        rec = d_rec.cpu().numpy().view(DEC_RESULT_DTYPE)[:n]
        res = d_res.cpu().numpy().view(DEC_RESULT_DTYPE)[0]
        return d_out[: plan["out_bytes"]], ooff, rec, res

    def set_chunks_index(self, how=CHUNKS_INDEX_PLANNED, round_bits=0):
        """aec_gpu_set_chunks_index: how the bare chunk index passes of this context run (CHUNKS_INDEX_*), and the budget
        of a round of the every-bit scheme in table entries (0: the default)"""
        self._chunks_index = (int(how), int(round_bits))
        self.lib.aec_gpu_set_chunks_index(self.ctx, int(how), int(round_bits))

    def index_chunks_plan(self, in_sizes, out_sizes, how=None, round_bits=None):
        """index_chunks_plan for this codec's parameters; how / round_bits default to what set_chunks_index was given"""
        cur = getattr(self, "_chunks_index", (CHUNKS_INDEX_PLANNED, 0))
        return index_chunks_plan(self.p.bits_per_sample, self.p.block_size, self.p.rsi, self.p.flags, in_sizes, out_sizes,
                                 cur[0] if how is None else how, cur[1] if round_bits is None else round_bits)

    def index_chunks_async(self, d_in, in_bytes, in_offsets, in_sizes, out_sizes, d_table, d_records, d_how=None, stream=None):
        """aec_gpu_index_chunks_async as it is: the three arrays are uint64 numpy arrays on the host, d_table an int64
        tensor of the plan's rsi_entries, d_records a uint8 tensor of 40 n bytes, d_how an int32 tensor of n entries or
        None.  Returns the call's return code."""
        return self.lib.aec_gpu_index_chunks_async(
            self.ctx, C.byref(self.p), _ptr(d_in), in_bytes, C.c_void_p(in_offsets.ctypes.data),
            C.c_void_p(in_sizes.ctypes.data), C.c_void_p(out_sizes.ctypes.data), int(out_sizes.size), _ptr(d_table),
            _ptr(d_records), _ptr(d_how), self._stream(stream))

    def index_chunks(self, d_in, in_bytes, out_sizes, in_offsets, in_sizes):
        """The index pass of a batch of bare streams (in_sizes[i] bytes at byte in_offsets[i] of d_in, decoding to
        out_sizes[i] bytes).  Returns (d_table, records, how): the int64 RSI table on the device in the layout
        decode_chunks takes as d_table, the DEC_RESULT_DTYPE record per stream, and per stream 1 where the every-bit scheme
        delivered it, 0 where the serial walker did.  Synchronises."""
        torch = self.torch
        osz = np.ascontiguousarray(out_sizes, dtype=np.uint64)
        ioff = np.ascontiguousarray(in_offsets, dtype=np.uint64)
        isz = np.ascontiguousarray(in_sizes, dtype=np.uint64)
        n = int(osz.size)
        if ioff.size != n or isz.size != n:
            raise ValueError("in_offsets, in_sizes and out_sizes differ in length")
        plan = self.index_chunks_plan(isz, osz)
        if plan is None:
            raise ValueError("aec_gpu_index_chunks_plan refuses this batch")
        d_table = torch.zeros(max(plan["rsi_entries"], 1), dtype=torch.int64, device=d_in.device)
        d_rec = torch.zeros(max(n, 1) * DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_in.device)
        d_how = torch.zeros(max(n, 1), dtype=torch.int32, device=d_in.device)
        rc = self.index_chunks_async(d_in, in_bytes, ioff, isz, osz, d_table, d_rec, d_how)
        if rc != 0:
            raise RuntimeError(f"aec_gpu_index_chunks_async failed ({rc})")
        rec = d_rec.cpu().numpy().view(DEC_RESULT_DTYPE)[:n]
        return d_table, rec, d_how.cpu().numpy()[:n]

    # ---- convenience (synchronising) -------------------------------------------------------------
    def encode(self, d_in, start_bit=0, k_in=0):
        """Encode a uint8 CUDA tensor.  Returns (d_out, n_bytes, total_bits, k_out, d_offsets)."""
        torch = self.torch
        n = d_in.numel()
        d_out = torch.empty(self.encode_bound(n), dtype=torch.uint8, device=d_in.device)
        d_off = torch.empty(self.rsi_count(n) + 1, dtype=torch.int64, device=d_in.device)
        d_res = torch.zeros(ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_in.device)
        self.encode_async(d_in, n, d_out, d_off, d_res, start_bit, k_in)
        res = d_res.cpu().numpy().view(ENC_RESULT_DTYPE)[0]
        if res["overflow"]:
            raise RuntimeError("encode overflow")
        bits = int(res["total_bits"])
        nbytes = max(1, (start_bit + bits + 7) // 8) if (start_bit + bits) else 1
        return d_out, nbytes, bits, int(res["k_out"]), d_off

    def decode(self, d_in, in_bytes, d_offsets, n_rsi, total_blocks):
        torch = self.torch
        nb = bytes_per_sample(self.p.bits_per_sample, self.p.flags)
        d_out = torch.empty(total_blocks * self.p.block_size * nb + 16, dtype=torch.uint8, device=d_in.device)
        d_res = torch.zeros(DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_in.device)
        self.decode_async(d_in, in_bytes, d_offsets, n_rsi, total_blocks, d_out, d_res)
        res = d_res.cpu().numpy().view(DEC_RESULT_DTYPE)[0]
        return d_out[: total_blocks * self.p.block_size * nb], int(res["status"])
