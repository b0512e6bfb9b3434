"""GRIB2 CCSDS packing and simple packing that stay on the device (include/aec_gpu_grib.h) for torch tensors living in HBM:
float fields to section-7 streams and back, template 5.0 streams to template 5.42 streams and back, and complex packing
(templates 5.2 / 5.3) read into floats, template 5.42 streams or template 5.0 streams, and written from any of the three.

torch is used for device memory and streams only; the minimum / maximum, the parameters, the quantisation and the coder are
kernels launched by libaec.so.0 through the C entry points declared in aec_gpu_grib.h.
"""
import ctypes as C

import numpy as np

from . import gpu
from .api import AEC_DATA_PREPROCESS

AEC_CONF_ERROR = -1
F32, F64 = 4, 8                       # elem: the element type by its size
BAD, CONSTANT, CLAMPED = 1, 2, 4      # status bits of a field record
MISMATCH = 8                          # ... of the bitmap calls: the bitmap does not hold n_values ones
CX_RANGE, CX_MALFORMED = 1, 2         # status bits of a complex-packing record (CX_DTYPE)


class Template(C.Structure):
    """aec_gpu_grib_template"""
    _fields_ = [("nbits", C.c_uint), ("options", C.c_uint), ("block_size", C.c_uint), ("rsi", C.c_uint)]


class Layout(C.Structure):
    """aec_gpu_grib_layout_t"""
    _fields_ = [("coder", gpu.Params), ("container", C.c_uint)]


class Plan(C.Structure):
    """aec_gpu_grib_plan_t"""
    _fields_ = [("coder", gpu.Params), ("work_bytes", C.c_size_t), ("out_bound", C.c_size_t), ("rsi_entries", C.c_uint64),
                ("workspace_bytes", C.c_size_t)]


class BitmapPlan(C.Structure):
    """aec_gpu_grib_bitmap_plan_t"""
    _fields_ = [("plan", Plan), ("tile_points", C.c_uint64), ("tiles", C.c_uint64)]


class SimplePlan(C.Structure):
    """aec_gpu_grib_simple_plan_t"""
    _fields_ = [("plan", Plan), ("simple_bytes", C.c_size_t)]


class ComplexField(C.Structure):
    """aec_gpu_grib_complex_field: what section 5 of a template 5.2 / 5.3 message says"""
    _fields_ = [(k, C.c_uint32) for k in ("ref_bits", "n_groups", "width_ref", "width_bits", "length_ref", "length_inc", "last_length",
                                          "length_bits", "order", "extra_octets", "missing")]


class ComplexPlan(C.Structure):
    """aec_gpu_grib_complex_plan_t"""
    _fields_ = [("plan", Plan), ("tile_values", C.c_uint64), ("value_tiles", C.c_uint64), ("group_tiles", C.c_uint64)]


class ComplexWrite(C.Structure):
    """aec_gpu_grib_complex_write: what a batch of template 5.2 / 5.3 streams is written under"""
    _fields_ = [("order", C.c_uint32), ("group_length", C.c_uint32)]


class ComplexWritePlan(C.Structure):
    """aec_gpu_grib_complex_write_plan_t"""
    _fields_ = [("plan", Plan), ("complex_bound", C.c_size_t), ("tile_values", C.c_uint64), ("value_tiles", C.c_uint64),
                ("group_tiles", C.c_uint64), ("out_tiles", C.c_uint64)]


COMPLEX_KEYS = [k for k, _ in ComplexField._fields_]
CXW_DTYPE = np.dtype([(k, "<u4") for k in COMPLEX_KEYS] + [("pad", "<u4"), ("bytes", "<u8")])     # aec_gpu_grib_cxw
CX_DTYPE = np.dtype([("x_min", "<i8"), ("x_max", "<i8"), ("status", "<u4"), ("pad", "<u4")])     # aec_gpu_grib_cx
FIELD_DTYPE = np.dtype([("R", "<f4"), ("E", "<i4"), ("D", "<i4"), ("status", "<u4")])      # aec_gpu_grib_field
BATCH_CHUNK_DTYPE = np.dtype([("base_bits", "<u8"), ("bits", "<u8")])

_bound = False


def _lib():
    global _bound
    lib = gpu._lib()
    if not _bound:
        if not hasattr(lib, "aec_gpu_grib_pack_async"):
            raise RuntimeError("this libaec.so.0 has no GRIB layer (aec_gpu_grib_*): rebuild it")
        vp, sz, u64, pt = C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(Template)
        lib.aec_gpu_grib_layout.restype = C.c_int
        lib.aec_gpu_grib_layout.argtypes = [pt, C.c_int, C.POINTER(Layout)]
        lib.aec_gpu_grib_plan.restype = C.c_int
        lib.aec_gpu_grib_plan.argtypes = [pt, C.c_int, vp, u64, C.POINTER(Plan), vp]
        lib.aec_gpu_grib_pack_async.restype = C.c_int
        lib.aec_gpu_grib_pack_async.argtypes = [vp, pt, C.c_int, vp, vp, vp, vp, C.c_int, vp, u64, vp, vp, sz, vp, vp, vp, vp, vp]
        lib.aec_gpu_grib_unpack_async.restype = C.c_int
        lib.aec_gpu_grib_unpack_async.argtypes = [vp, pt, C.c_int, vp, sz, vp, vp, vp, vp, vp, u64, vp, C.c_int, vp, vp, vp, vp, vp]
        lib.aec_gpu_grib_quantise_async.restype = C.c_int
        lib.aec_gpu_grib_quantise_async.argtypes = [vp, pt, C.c_int, vp, vp, vp, vp, C.c_int, vp, u64, vp, vp, vp]
        lib.aec_gpu_grib_dequantise_async.restype = C.c_int
        lib.aec_gpu_grib_dequantise_async.argtypes = [vp, pt, C.c_int, vp, vp, vp, vp, u64, vp, vp]
        if not hasattr(lib, "aec_gpu_grib_pack_bitmap_async"):
            raise RuntimeError("this libaec.so.0 has no bitmap calls (aec_gpu_grib_*_bitmap_*): rebuild it")
        dbl = C.c_double
        lib.aec_gpu_grib_bitmap_plan.restype = C.c_int
        lib.aec_gpu_grib_bitmap_plan.argtypes = [pt, C.c_int, vp, vp, u64, C.POINTER(BitmapPlan), vp]
        lib.aec_gpu_grib_bitmap_async.restype = C.c_int
        lib.aec_gpu_grib_bitmap_async.argtypes = [vp, C.c_int, vp, vp, vp, dbl, u64, vp, vp, vp, vp]
        lib.aec_gpu_grib_pack_bitmap_async.restype = C.c_int
        lib.aec_gpu_grib_pack_bitmap_async.argtypes = lib.aec_gpu_grib_pack_async.argtypes[:-1] + [vp, vp, vp, vp]
        lib.aec_gpu_grib_unpack_bitmap_async.restype = C.c_int
        lib.aec_gpu_grib_unpack_bitmap_async.argtypes = lib.aec_gpu_grib_unpack_async.argtypes[:-1] + [vp, vp, vp, dbl, vp, vp]
        lib.aec_gpu_grib_quantise_bitmap_async.restype = C.c_int
        lib.aec_gpu_grib_quantise_bitmap_async.argtypes = lib.aec_gpu_grib_quantise_async.argtypes[:-1] + [vp, vp, vp, vp]
        lib.aec_gpu_grib_dequantise_bitmap_async.restype = C.c_int
        lib.aec_gpu_grib_dequantise_bitmap_async.argtypes = lib.aec_gpu_grib_dequantise_async.argtypes[:-1] + [vp, vp, vp, dbl, vp, vp]
        if not hasattr(lib, "aec_gpu_grib_bits_pack_async"):
            raise RuntimeError("this libaec.so.0 has no simple packing (aec_gpu_grib_simple_*, aec_gpu_grib_bits_*): rebuild it")
        lib.aec_gpu_grib_simple_plan.restype = C.c_int
        lib.aec_gpu_grib_simple_plan.argtypes = [pt, C.c_int, vp, u64, C.POINTER(SimplePlan), vp, vp]
        lib.aec_gpu_grib_bits_pack_async.restype = C.c_int
        lib.aec_gpu_grib_bits_pack_async.argtypes = [vp, pt, vp, u64, vp, vp, vp, vp]
        lib.aec_gpu_grib_bits_unpack_async.restype = C.c_int
        lib.aec_gpu_grib_bits_unpack_async.argtypes = [vp, pt, vp, u64, vp, sz, vp, vp, vp, vp]
        lib.aec_gpu_grib_simple_pack_async.restype = C.c_int
        lib.aec_gpu_grib_simple_pack_async.argtypes = [vp, pt, C.c_int, vp, vp, vp, vp, C.c_int, vp, u64, vp, vp, vp, vp, vp]
        lib.aec_gpu_grib_simple_unpack_async.restype = C.c_int
        lib.aec_gpu_grib_simple_unpack_async.argtypes = [vp, pt, C.c_int, vp, sz, vp, vp, vp, vp, vp, u64, vp, vp, vp]
        lib.aec_gpu_grib_simple_to_ccsds_async.restype = C.c_int
        lib.aec_gpu_grib_simple_to_ccsds_async.argtypes = [vp, pt, vp, sz, vp, vp, vp, u64, vp, vp, sz, vp, vp, vp, vp]
        lib.aec_gpu_grib_ccsds_to_simple_async.restype = C.c_int
        lib.aec_gpu_grib_ccsds_to_simple_async.argtypes = [vp, pt, vp, sz, vp, vp, vp, u64, vp, C.c_int, vp, vp, vp, vp, vp, vp]
        if not hasattr(lib, "aec_gpu_grib_complex_expand_async"):
            raise RuntimeError("this libaec.so.0 has no complex packing (aec_gpu_grib_complex_*): rebuild it")
        lib.aec_gpu_grib_complex_plan.restype = C.c_int
        lib.aec_gpu_grib_complex_plan.argtypes = [pt, C.c_int, vp, vp, u64, C.POINTER(ComplexPlan), vp]
        lib.aec_gpu_grib_complex_expand_async.restype = C.c_int
        lib.aec_gpu_grib_complex_expand_async.argtypes = [vp, pt, vp, vp, u64, vp, sz, vp, vp, vp, vp, vp]
        lib.aec_gpu_grib_complex_unpack_async.restype = C.c_int
        lib.aec_gpu_grib_complex_unpack_async.argtypes = [vp, pt, C.c_int, vp, vp, sz, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp]
        lib.aec_gpu_grib_complex_to_ccsds_async.restype = C.c_int
        lib.aec_gpu_grib_complex_to_ccsds_async.argtypes = [vp, pt, vp, vp, sz, vp, vp, vp, u64, vp, vp, sz, vp, vp, vp, vp, vp]
        if not hasattr(lib, "aec_gpu_grib_complex_write_async"):
            raise RuntimeError("this libaec.so.0 writes no complex packing (aec_gpu_grib_complex_write_*): rebuild it")
        pw = C.POINTER(ComplexWrite)
        lib.aec_gpu_grib_complex_write_plan.restype = C.c_int
        lib.aec_gpu_grib_complex_write_plan.argtypes = [pt, pw, C.c_int, vp, u64, C.POINTER(ComplexWritePlan), vp, vp]
        lib.aec_gpu_grib_complex_write_async.restype = C.c_int
        lib.aec_gpu_grib_complex_write_async.argtypes = [vp, pt, pw, vp, u64, vp, vp, sz, vp, vp, vp]
        lib.aec_gpu_grib_complex_pack_async.restype = C.c_int
        lib.aec_gpu_grib_complex_pack_async.argtypes = [vp, pt, pw, C.c_int, vp, vp, vp, vp, C.c_int, vp, u64, vp, vp, vp, sz, vp, vp, vp]
        lib.aec_gpu_grib_ccsds_to_complex_async.restype = C.c_int
        lib.aec_gpu_grib_ccsds_to_complex_async.argtypes = [vp, pt, pw, vp, sz, vp, vp, vp, u64, vp, C.c_int, vp, vp, vp, vp, sz, vp, vp, vp]
        lib.aec_gpu_grib_simple_to_complex_async.restype = C.c_int
        lib.aec_gpu_grib_simple_to_complex_async.argtypes = [vp, pt, pw, vp, sz, vp, vp, vp, u64, vp, vp, sz, vp, vp, vp]
        _bound = True
    return lib


def complex_fields(fields):
    """a host array of aec_gpu_grib_complex_field from ComplexField objects, dicts with its members' names, or such an array"""
    if isinstance(fields, C.Array):
        return fields
    arr = (ComplexField * max(1, len(fields)))()
    for i, f in enumerate(fields):
        arr[i] = f if isinstance(f, ComplexField) else ComplexField(**{k: int(v) for k, v in f.items()})
    return arr


def _u64(a):
    """a host array of uint64 for a call (None stays None); the array must outlive the call, so it is returned"""
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint64)


def _host(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def records(R=None, E=None, D=None, n=None):
    """a host array of aec_gpu_grib_field from per-field R, E, D (scalars or sequences)"""
    n = n if n is not None else len(D if D is not None else R)
    rec = np.zeros(n, FIELD_DTYPE)
    for key, v in (("R", R), ("E", E), ("D", D)):
        if v is not None:
            rec[key] = v
    return rec


def layout(nbits, options, block_size, rsi, D=0):
    """aec_gpu_grib_layout (host arithmetic, no device needed): a Layout, or None where the call says AEC_CONF_ERROR"""
    t = Template(nbits, options, block_size, rsi)
    out = Layout()
    rc = _lib().aec_gpu_grib_layout(C.byref(t), D, C.byref(out))
    if rc == AEC_CONF_ERROR:
        return None
    if rc != 0:
        raise RuntimeError(f"aec_gpu_grib_layout failed ({rc})")
    return out


def plan(nbits, options, block_size, rsi, elem, n_values):
    """aec_gpu_grib_plan (host arithmetic, no device needed) for fields of n_values values: the dict {coder, work_bytes,
    out_bound, rsi_entries, workspace_bytes, work_offsets}, or None where the batch would be refused"""
    t = Template(nbits, options, block_size, rsi)
    n_values = _u64(n_values)
    offs = np.zeros(max(1, n_values.size), dtype=np.uint64)
    p = Plan()
    if not _lib().aec_gpu_grib_plan(C.byref(t), elem, _host(n_values), n_values.size, C.byref(p), _host(offs)):
        return None
    return dict(coder=(p.coder.bits_per_sample, p.coder.block_size, p.coder.rsi, p.coder.flags), work_bytes=int(p.work_bytes),
                out_bound=int(p.out_bound), rsi_entries=int(p.rsi_entries), workspace_bytes=int(p.workspace_bytes),
                work_offsets=offs[:n_values.size])


def bitmap_plan(nbits, options, block_size, rsi, elem, n_points, n_values):
    """aec_gpu_grib_bitmap_plan (host arithmetic, no device needed) for grids of n_points points of which n_values are
    present: the dict of plan() plus tile_points and tiles, or None where the batch would be refused"""
    t = Template(nbits, options, block_size, rsi)
    n_points, n_values = _u64(n_points), _u64(n_values)
    if n_points.size != n_values.size:
        raise ValueError("n_points and n_values are per field")
    offs = np.zeros(max(1, n_values.size), dtype=np.uint64)
    bp = BitmapPlan()
    if not _lib().aec_gpu_grib_bitmap_plan(C.byref(t), elem, _host(n_points), _host(n_values), n_values.size, C.byref(bp), _host(offs)):
        return None
    p = bp.plan
    return dict(coder=(p.coder.bits_per_sample, p.coder.block_size, p.coder.rsi, p.coder.flags), work_bytes=int(p.work_bytes),
                out_bound=int(p.out_bound), rsi_entries=int(p.rsi_entries), workspace_bytes=int(p.workspace_bytes),
                work_offsets=offs[:n_values.size], tile_points=int(bp.tile_points), tiles=int(bp.tiles))


def simple_plan(nbits, options, block_size, rsi, elem, n_values):
    """aec_gpu_grib_simple_plan (host arithmetic, no device needed): the dict of plan() plus simple_bytes and simple_offsets
    (the streams back to back), or None where the batch would be refused"""
    t = Template(nbits, options, block_size, rsi)
    n_values = _u64(n_values)
    offs = np.zeros(max(1, n_values.size), dtype=np.uint64)
    soffs = np.zeros(max(1, n_values.size), dtype=np.uint64)
    sp = SimplePlan()
    if not _lib().aec_gpu_grib_simple_plan(C.byref(t), elem, _host(n_values), n_values.size, C.byref(sp), _host(offs), _host(soffs)):
        return None
    p = sp.plan
    return dict(coder=(p.coder.bits_per_sample, p.coder.block_size, p.coder.rsi, p.coder.flags), work_bytes=int(p.work_bytes),
                out_bound=int(p.out_bound), rsi_entries=int(p.rsi_entries), workspace_bytes=int(p.workspace_bytes),
                work_offsets=offs[:n_values.size], simple_bytes=int(sp.simple_bytes), simple_offsets=soffs[:n_values.size])


def complex_plan(nbits, options, block_size, rsi, elem, n_values, fields):
    """aec_gpu_grib_complex_plan (host arithmetic, no device needed): the dict of plan() plus tile_values, value_tiles and
    group_tiles, or None where the batch would be refused"""
    t = Template(nbits, options, block_size, rsi)
    n_values = _u64(n_values)
    if len(fields) != n_values.size:
        raise ValueError("fields and n_values are per field")
    offs = np.zeros(max(1, n_values.size), dtype=np.uint64)
    cp = ComplexPlan()
    if not _lib().aec_gpu_grib_complex_plan(C.byref(t), elem, _host(n_values), complex_fields(fields), n_values.size, C.byref(cp), _host(offs)):
        return None
    p = cp.plan
    return dict(coder=(p.coder.bits_per_sample, p.coder.block_size, p.coder.rsi, p.coder.flags), work_bytes=int(p.work_bytes),
                out_bound=int(p.out_bound), rsi_entries=int(p.rsi_entries), workspace_bytes=int(p.workspace_bytes),
                work_offsets=offs[:n_values.size], tile_values=int(cp.tile_values), value_tiles=int(cp.value_tiles),
                group_tiles=int(cp.group_tiles))


def complex_write_plan(nbits, options, block_size, rsi, elem, n_values, order, group_length):
    """aec_gpu_grib_complex_write_plan (host arithmetic, no device needed): the dict of plan() plus complex_bound (the sum of the
    B_i), complex_offsets (their running sum), tile_values, value_tiles, group_tiles and out_tiles, or None where the batch would
    be refused"""
    t = Template(nbits, options, block_size, rsi)
    w = ComplexWrite(order, group_length)
    n_values = _u64(n_values)
    offs = np.zeros(max(1, n_values.size), dtype=np.uint64)
    coffs = np.zeros(max(1, n_values.size), dtype=np.uint64)
    wp = ComplexWritePlan()
    if not _lib().aec_gpu_grib_complex_write_plan(C.byref(t), C.byref(w), elem, _host(n_values), n_values.size, C.byref(wp), _host(offs),
                                                  _host(coffs)):
        return None
    p = wp.plan
    return dict(coder=(p.coder.bits_per_sample, p.coder.block_size, p.coder.rsi, p.coder.flags), work_bytes=int(p.work_bytes),
                out_bound=int(p.out_bound), rsi_entries=int(p.rsi_entries), workspace_bytes=int(p.workspace_bytes),
                work_offsets=offs[:n_values.size], complex_bound=int(wp.complex_bound), complex_offsets=coffs[:n_values.size],
                tile_values=int(wp.tile_values), value_tiles=int(wp.value_tiles), group_tiles=int(wp.group_tiles),
                out_tiles=int(wp.out_tiles))


def complex_fields_of(cxw):
    """the records of a write (a CXW_DTYPE array) as (what complex_fields() takes, complex_sizes): a writer's output feeds the
    reading calls directly"""
    return [{k: int(r[k]) for k in COMPLEX_KEYS} for r in cxw], np.array([int(r["bytes"]) for r in cxw], np.uint64)


def _elem_of(t):
    import torch
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise ValueError("fields are float32 or float64 tensors")


class GribCodec:
    """One template 5.42 (nbits, compression options, block size, reference sample interval) and one aec_gpu context
    (workspace) on the current torch device.  The simple_* and bits_* methods read and write template 5.0 / 7.0 (simple
    packing) under the same nbits; block size and interval then only size the rooms of the work buffer."""

    def __init__(self, nbits, block_size=32, rsi=128, mask=AEC_DATA_PREPROCESS):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("libaec_amd.gribgpu needs a HIP device (no CPU implementation)")
        self.torch = torch
        self.lib = _lib()
        self.t = Template(nbits, mask, block_size, rsi)
        if layout(nbits, mask, block_size, rsi) is None:
            raise ValueError("invalid template (aec_gpu_grib_layout -> AEC_CONF_ERROR)")
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

    def plan(self, n_values, elem=F32):
        t = self.t
        return plan(t.nbits, t.options, t.block_size, t.rsi, elem, n_values)

    # ---- enqueue -------------------------------------------------------------------------------
    def pack_async(self, elem, d_src, src_offsets, n_values, D, params, d_work, d_out, out_cap, d_chunks, d_table, d_fields,
                   d_result, stream=None):
        """src_offsets (bytes) / n_values: uint64 arrays on the host, D: int32 array on the host, params: a FIELD_DTYPE
        array on the host or None; d_work: the plan's work_bytes, 16-byte aligned; d_chunks: n * 16 bytes
        (BATCH_CHUNK_DTYPE); d_table: int64 tensor of the plan's rsi_entries, or None; d_fields: n * 16 bytes (FIELD_DTYPE);
        d_result: 24 bytes (gpu.ENC_RESULT_DTYPE).  Returns the call's return code."""
        offs, nv = _u64(src_offsets), _u64(n_values)
        Dh = None if D is None else np.ascontiguousarray(D, dtype=np.int32)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_pack_async(self.ctx, C.byref(self.t), elem, _ptr(d_src), _host(offs), _host(nv), _host(Dh),
                                                int(ph is not None), _host(ph), nv.size, _ptr(d_work), _ptr(d_out), out_cap,
                                                _ptr(d_chunks), _ptr(d_table), _ptr(d_fields), _ptr(d_result), self._stream(stream))

    def unpack_async(self, elem, d_in, in_bytes, in_offsets, in_sizes, n_values, params, dst_offsets, d_table, have_table, d_work,
                     d_dst, d_results, d_result, stream=None):
        """in_offsets / in_sizes (None with a table), n_values, dst_offsets (bytes): uint64 arrays on the host; params: a
        FIELD_DTYPE array on the host; d_table: int64 tensor of the plan's rsi_entries; d_results: n * 40 bytes, d_result:
        40 bytes (gpu.DEC_RESULT_DTYPE).  Returns the call's return code."""
        ino, ins, nv, dso = _u64(in_offsets), _u64(in_sizes), _u64(n_values), _u64(dst_offsets)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_unpack_async(self.ctx, C.byref(self.t), elem, _ptr(d_in), in_bytes, _host(ino), _host(ins),
                                                  _host(nv), _host(ph), _host(dso), nv.size, _ptr(d_table), int(bool(have_table)),
                                                  _ptr(d_work), _ptr(d_dst), _ptr(d_results), _ptr(d_result), self._stream(stream))

    def quantise_async(self, elem, d_src, src_offsets, n_values, D, params, d_work, d_fields, stream=None):
        """pack_async without the encoder"""
        offs, nv = _u64(src_offsets), _u64(n_values)
        Dh = None if D is None else np.ascontiguousarray(D, dtype=np.int32)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_quantise_async(self.ctx, C.byref(self.t), elem, _ptr(d_src), _host(offs), _host(nv), _host(Dh),
                                                    int(ph is not None), _host(ph), nv.size, _ptr(d_work), _ptr(d_fields),
                                                    self._stream(stream))

    def dequantise_async(self, elem, d_work, n_values, params, dst_offsets, d_dst, stream=None):
        """unpack_async without the decoder: d_work holds the X in the plan's rooms"""
        nv, dso = _u64(n_values), _u64(dst_offsets)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_dequantise_async(self.ctx, C.byref(self.t), elem, _ptr(d_work), _host(nv), _host(ph),
                                                      _host(dso), nv.size, _ptr(d_dst), self._stream(stream))

    # ---- enqueue, fields with section 6 bitmaps ----------------------------------------------------
    def bitmap_plan(self, n_points, n_values, elem=F32):
        t = self.t
        return bitmap_plan(t.nbits, t.options, t.block_size, t.rsi, elem, n_points, n_values)

    def bitmap_async(self, elem, d_src, src_offsets, n_points, missing, d_bitmap, bitmap_offsets, d_counts, stream=None):
        """section 6 from values: a point is missing iff it == missing (a NaN: iff it is a NaN).  src_offsets / bitmap_offsets
        (bytes), n_points: uint64 arrays on the host; d_bitmap: uint8 tensor; d_counts: int64 tensor, a count per field."""
        offs, npts, bmo = _u64(src_offsets), _u64(n_points), _u64(bitmap_offsets)
        return self.lib.aec_gpu_grib_bitmap_async(self.ctx, elem, _ptr(d_src), _host(offs), _host(npts), float(missing), npts.size,
                                                  _ptr(d_bitmap), _host(bmo), _ptr(d_counts), self._stream(stream))

    def pack_bitmap_async(self, elem, d_src, src_offsets, n_values, D, params, d_work, d_out, out_cap, d_chunks, d_table, d_fields,
                          d_result, d_bitmap, bitmap_offsets, n_points, stream=None):
        """pack_async over whole grids: src_offsets / n_points describe the grids, n_values the present points, d_bitmap /
        bitmap_offsets (bytes, host) the bitmaps"""
        offs, nv, bmo, npts = _u64(src_offsets), _u64(n_values), _u64(bitmap_offsets), _u64(n_points)
        Dh = None if D is None else np.ascontiguousarray(D, dtype=np.int32)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_pack_bitmap_async(self.ctx, C.byref(self.t), elem, _ptr(d_src), _host(offs), _host(nv), _host(Dh),
                                                       int(ph is not None), _host(ph), nv.size, _ptr(d_work), _ptr(d_out), out_cap,
                                                       _ptr(d_chunks), _ptr(d_table), _ptr(d_fields), _ptr(d_result), _ptr(d_bitmap),
                                                       _host(bmo), _host(npts), self._stream(stream))

    def unpack_bitmap_async(self, elem, d_in, in_bytes, in_offsets, in_sizes, n_values, params, dst_offsets, d_table, have_table, d_work,
                            d_dst, d_results, d_result, d_bitmap, bitmap_offsets, n_points, missing, d_status, stream=None):
        """unpack_async into whole grids: n_points elements per field at dst_offsets, absent points get the bits of missing;
        d_status: int32 tensor, 0 or MISMATCH per field"""
        ino, ins, nv, dso = _u64(in_offsets), _u64(in_sizes), _u64(n_values), _u64(dst_offsets)
        bmo, npts = _u64(bitmap_offsets), _u64(n_points)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_unpack_bitmap_async(self.ctx, C.byref(self.t), elem, _ptr(d_in), in_bytes, _host(ino), _host(ins),
                                                         _host(nv), _host(ph), _host(dso), nv.size, _ptr(d_table), int(bool(have_table)),
                                                         _ptr(d_work), _ptr(d_dst), _ptr(d_results), _ptr(d_result), _ptr(d_bitmap),
                                                         _host(bmo), _host(npts), float(missing), _ptr(d_status), self._stream(stream))

    def quantise_bitmap_async(self, elem, d_src, src_offsets, n_values, D, params, d_work, d_fields, d_bitmap, bitmap_offsets, n_points,
                              stream=None):
        """pack_bitmap_async without the encoder"""
        offs, nv, bmo, npts = _u64(src_offsets), _u64(n_values), _u64(bitmap_offsets), _u64(n_points)
        Dh = None if D is None else np.ascontiguousarray(D, dtype=np.int32)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_quantise_bitmap_async(self.ctx, C.byref(self.t), elem, _ptr(d_src), _host(offs), _host(nv), _host(Dh),
                                                           int(ph is not None), _host(ph), nv.size, _ptr(d_work), _ptr(d_fields),
                                                           _ptr(d_bitmap), _host(bmo), _host(npts), self._stream(stream))

    def dequantise_bitmap_async(self, elem, d_work, n_values, params, dst_offsets, d_dst, d_bitmap, bitmap_offsets, n_points, missing,
                                d_status, stream=None):
        """unpack_bitmap_async without the decoder"""
        nv, dso, bmo, npts = _u64(n_values), _u64(dst_offsets), _u64(bitmap_offsets), _u64(n_points)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_dequantise_bitmap_async(self.ctx, C.byref(self.t), elem, _ptr(d_work), _host(nv), _host(ph),
                                                             _host(dso), nv.size, _ptr(d_dst), _ptr(d_bitmap), _host(bmo), _host(npts),
                                                             float(missing), _ptr(d_status), self._stream(stream))

    # ---- enqueue, simple packing (templates 5.0 / 7.0) ------------------------------------------------
    def simple_plan(self, n_values, elem=F32):
        t = self.t
        return simple_plan(t.nbits, t.options, t.block_size, t.rsi, elem, n_values)

    def bits_pack_async(self, n_values, d_work, d_simple, simple_offsets, stream=None):
        """rooms to streams: the X in the plan's rooms of d_work to ceil(n_values[i] * nbits / 8) bytes at d_simple +
        simple_offsets[i] (bytes, a uint64 array on the host, any byte)"""
        nv, so = _u64(n_values), _u64(simple_offsets)
        return self.lib.aec_gpu_grib_bits_pack_async(self.ctx, C.byref(self.t), _host(nv), nv.size, _ptr(d_work), _ptr(d_simple), _host(so),
                                                     self._stream(stream))

    def bits_unpack_async(self, n_values, d_simple, simple_bytes, simple_offsets, simple_sizes, d_work, stream=None):
        """streams to rooms; simple_sizes: section 7's data length per message (uint64 on the host) or None"""
        nv, so, ss = _u64(n_values), _u64(simple_offsets), _u64(simple_sizes)
        return self.lib.aec_gpu_grib_bits_unpack_async(self.ctx, C.byref(self.t), _host(nv), nv.size, _ptr(d_simple), simple_bytes, _host(so),
                                                       _host(ss), _ptr(d_work), self._stream(stream))

    def simple_pack_async(self, elem, d_src, src_offsets, n_values, D, params, d_work, d_fields, d_simple, simple_offsets, stream=None):
        """quantise_async, then bits_pack_async"""
        offs, nv, so = _u64(src_offsets), _u64(n_values), _u64(simple_offsets)
        Dh = None if D is None else np.ascontiguousarray(D, dtype=np.int32)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_simple_pack_async(self.ctx, C.byref(self.t), elem, _ptr(d_src), _host(offs), _host(nv), _host(Dh),
                                                       int(ph is not None), _host(ph), nv.size, _ptr(d_work), _ptr(d_fields), _ptr(d_simple),
                                                       _host(so), self._stream(stream))

    def simple_unpack_async(self, elem, d_simple, simple_bytes, simple_offsets, simple_sizes, n_values, params, dst_offsets, d_work, d_dst,
                            stream=None):
        """bits_unpack_async, then dequantise_async"""
        so, ss, nv, dso = _u64(simple_offsets), _u64(simple_sizes), _u64(n_values), _u64(dst_offsets)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_simple_unpack_async(self.ctx, C.byref(self.t), elem, _ptr(d_simple), simple_bytes, _host(so), _host(ss),
                                                         _host(nv), _host(ph), _host(dso), nv.size, _ptr(d_work), _ptr(d_dst),
                                                         self._stream(stream))

    def simple_to_ccsds_async(self, d_simple, simple_bytes, simple_offsets, simple_sizes, n_values, d_work, d_out, out_cap, d_chunks, d_table,
                              d_result, stream=None):
        """template 5.0 streams to template 5.42 streams: bits_unpack_async, then the chunk encoder; the outputs are pack_async's"""
        so, ss, nv = _u64(simple_offsets), _u64(simple_sizes), _u64(n_values)
        return self.lib.aec_gpu_grib_simple_to_ccsds_async(self.ctx, C.byref(self.t), _ptr(d_simple), simple_bytes, _host(so), _host(ss),
                                                           _host(nv), nv.size, _ptr(d_work), _ptr(d_out), out_cap, _ptr(d_chunks),
                                                           _ptr(d_table), _ptr(d_result), self._stream(stream))

    def ccsds_to_simple_async(self, d_in, in_bytes, in_offsets, in_sizes, n_values, d_table, have_table, d_work, d_results, d_result,
                              d_simple, simple_offsets, stream=None):
        """template 5.42 streams to template 5.0 streams: the chunk decoder (with the pack's table, or bare), then bits_pack_async"""
        ino, ins, nv, so = _u64(in_offsets), _u64(in_sizes), _u64(n_values), _u64(simple_offsets)
        return self.lib.aec_gpu_grib_ccsds_to_simple_async(self.ctx, C.byref(self.t), _ptr(d_in), in_bytes, _host(ino), _host(ins), _host(nv),
                                                           nv.size, _ptr(d_table), int(bool(have_table)), _ptr(d_work), _ptr(d_results),
                                                           _ptr(d_result), _ptr(d_simple), _host(so), self._stream(stream))

    # ---- enqueue, complex packing (templates 5.2 / 5.3), reading ---------------------------------------
    def complex_plan(self, n_values, fields, elem=F32):
        t = self.t
        return complex_plan(t.nbits, t.options, t.block_size, t.rsi, elem, n_values, fields)

    def complex_expand_async(self, fields, n_values, d_complex, complex_bytes, complex_offsets, complex_sizes, d_work, d_cx, stream=None):
        """streams to rooms: fields as complex_fields() takes them; complex_offsets / complex_sizes (section 7's data length per
        message): uint64 arrays on the host; d_cx: n * 24 bytes (CX_DTYPE)"""
        nv, co, cs = _u64(n_values), _u64(complex_offsets), _u64(complex_sizes)
        return self.lib.aec_gpu_grib_complex_expand_async(self.ctx, C.byref(self.t), complex_fields(fields), _host(nv), nv.size, _ptr(d_complex),
                                                          complex_bytes, _host(co), _host(cs), _ptr(d_work), _ptr(d_cx), self._stream(stream))

    def complex_unpack_async(self, elem, fields, d_complex, complex_bytes, complex_offsets, complex_sizes, n_values, params, dst_offsets,
                             d_work, d_dst, d_cx, stream=None):
        """complex_expand_async, then dequantise_async"""
        nv, co, cs, dso = _u64(n_values), _u64(complex_offsets), _u64(complex_sizes), _u64(dst_offsets)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        return self.lib.aec_gpu_grib_complex_unpack_async(self.ctx, C.byref(self.t), elem, complex_fields(fields), _ptr(d_complex), complex_bytes,
                                                          _host(co), _host(cs), _host(nv), _host(ph), _host(dso), nv.size, _ptr(d_work),
                                                          _ptr(d_dst), _ptr(d_cx), self._stream(stream))

    def complex_to_ccsds_async(self, fields, d_complex, complex_bytes, complex_offsets, complex_sizes, n_values, d_work, d_out, out_cap,
                               d_chunks, d_table, d_result, d_cx, stream=None):
        """template 5.2 / 5.3 streams to template 5.42 streams: complex_expand_async, then the chunk encoder; the outputs are
        pack_async's"""
        nv, co, cs = _u64(n_values), _u64(complex_offsets), _u64(complex_sizes)
        return self.lib.aec_gpu_grib_complex_to_ccsds_async(self.ctx, C.byref(self.t), complex_fields(fields), _ptr(d_complex), complex_bytes,
                                                            _host(co), _host(cs), _host(nv), nv.size, _ptr(d_work), _ptr(d_out), out_cap,
                                                            _ptr(d_chunks), _ptr(d_table), _ptr(d_result), _ptr(d_cx), self._stream(stream))

    # ---- enqueue, complex packing (templates 5.2 / 5.3), writing ---------------------------------------
    def complex_write_plan(self, n_values, order, group_length, elem=F32):
        t = self.t
        return complex_write_plan(t.nbits, t.options, t.block_size, t.rsi, elem, n_values, order, group_length)

    def complex_write_async(self, order, group_length, n_values, d_work, d_complex, complex_cap, complex_offsets, d_cxw, stream=None):
        """rooms to streams under the writer's rule: at most B_i bytes at d_complex + complex_offsets[i] (bytes, a uint64 array on
        the host); d_cxw: n * 56 bytes (CXW_DTYPE)"""
        nv, co = _u64(n_values), _u64(complex_offsets)
        w = ComplexWrite(order, group_length)
        return self.lib.aec_gpu_grib_complex_write_async(self.ctx, C.byref(self.t), C.byref(w), _host(nv), nv.size, _ptr(d_work),
                                                         _ptr(d_complex), complex_cap, _host(co), _ptr(d_cxw), self._stream(stream))

    def complex_pack_async(self, order, group_length, elem, d_src, src_offsets, n_values, D, params, d_work, d_fields, d_complex, complex_cap,
                           complex_offsets, d_cxw, stream=None):
        """quantise_async, then complex_write_async"""
        offs, nv, co = _u64(src_offsets), _u64(n_values), _u64(complex_offsets)
        Dh = None if D is None else np.ascontiguousarray(D, dtype=np.int32)
        ph = None if params is None else np.ascontiguousarray(params, dtype=FIELD_DTYPE)
        w = ComplexWrite(order, group_length)
        return self.lib.aec_gpu_grib_complex_pack_async(self.ctx, C.byref(self.t), C.byref(w), elem, _ptr(d_src), _host(offs), _host(nv),
                                                        _host(Dh), int(ph is not None), _host(ph), nv.size, _ptr(d_work), _ptr(d_fields),
                                                        _ptr(d_complex), complex_cap, _host(co), _ptr(d_cxw), self._stream(stream))

    def ccsds_to_complex_async(self, order, group_length, d_in, in_bytes, in_offsets, in_sizes, n_values, d_table, have_table, d_work,
                               d_results, d_result, d_complex, complex_cap, complex_offsets, d_cxw, stream=None):
        """template 5.42 streams to template 5.2 / 5.3 streams: the chunk decoder (with the pack's table, or bare), then
        complex_write_async"""
        ino, ins, nv, co = _u64(in_offsets), _u64(in_sizes), _u64(n_values), _u64(complex_offsets)
        w = ComplexWrite(order, group_length)
        return self.lib.aec_gpu_grib_ccsds_to_complex_async(self.ctx, C.byref(self.t), C.byref(w), _ptr(d_in), in_bytes, _host(ino), _host(ins),
                                                            _host(nv), nv.size, _ptr(d_table), int(bool(have_table)), _ptr(d_work),
                                                            _ptr(d_results), _ptr(d_result), _ptr(d_complex), complex_cap, _host(co),
                                                            _ptr(d_cxw), self._stream(stream))

    def simple_to_complex_async(self, order, group_length, d_simple, simple_bytes, simple_offsets, simple_sizes, n_values, d_work, d_complex,
                                complex_cap, complex_offsets, d_cxw, stream=None):
        """template 5.0 streams to template 5.2 / 5.3 streams: bits_unpack_async, then complex_write_async"""
        so, ss, nv, co = _u64(simple_offsets), _u64(simple_sizes), _u64(n_values), _u64(complex_offsets)
        w = ComplexWrite(order, group_length)
        return self.lib.aec_gpu_grib_simple_to_complex_async(self.ctx, C.byref(self.t), C.byref(w), _ptr(d_simple), simple_bytes, _host(so),
                                                             _host(ss), _host(nv), nv.size, _ptr(d_work), _ptr(d_complex), complex_cap,
                                                             _host(co), _ptr(d_cxw), self._stream(stream))

    # ---- convenience (synchronising) -------------------------------------------------------------
    def _complex_write_plan_or_raise(self, n_values, order, group_length, elem=F32):
        pl = self.complex_write_plan(n_values, order, group_length, elem)
        if pl is None:
            raise ValueError("not a batch for one call (aec_gpu_grib_complex_write_plan)")
        return pl

    def _complex_out(self, pl, n, dev):
        torch = self.torch
        return (torch.empty(max(1, pl["complex_bound"]), dtype=torch.uint8, device=dev),
                torch.zeros(max(1, n) * CXW_DTYPE.itemsize, dtype=torch.uint8, device=dev))

    def complex_write(self, d_work, n_values, order, group_length):
        """X in the plan's rooms of d_work -> (d_complex, complex_offsets, the CXW_DTYPE records): section 7 of field i under template
        5.2 (order 0) or 5.3 is d_complex[complex_offsets[i]:][:records[i]["bytes"]], the record's other members go into section 5
        (complex_fields_of() turns them into what the reading calls take)"""
        pl = self._complex_write_plan_or_raise(n_values, order, group_length)
        n = len(n_values)
        d_complex, d_cxw = self._complex_out(pl, n, d_work.device)
        self._check(self.complex_write_async(order, group_length, n_values, d_work, d_complex, d_complex.numel(), pl["complex_offsets"], d_cxw),
                    "aec_gpu_grib_complex_write_async")
        return d_complex, pl["complex_offsets"], d_cxw.cpu().numpy().view(CXW_DTYPE)[:n]

    def complex_pack(self, d_values, offsets, n_values, D, order, group_length, params=None):
        """fields of n_values[i] elements at ELEMENT offsets[i] of the float tensor d_values -> (d_complex, complex_offsets, the
        CXW_DTYPE records, the FIELD_DTYPE records (R, E, D, status) of section 5)"""
        torch = self.torch
        elem = _elem_of(d_values)
        pl = self._complex_write_plan_or_raise(n_values, order, group_length, elem)
        n, dev = len(n_values), d_values.device
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_fields = torch.zeros(max(1, n) * FIELD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_complex, d_cxw = self._complex_out(pl, n, dev)
        Dh = np.broadcast_to(np.asarray(D, dtype=np.int32), (n,))
        self._check(self.complex_pack_async(order, group_length, elem, d_values, _u64(offsets) * np.uint64(elem), n_values, Dh, params, d_work,
                                            d_fields, d_complex, d_complex.numel(), pl["complex_offsets"], d_cxw),
                    "aec_gpu_grib_complex_pack_async")
        return d_complex, pl["complex_offsets"], d_cxw.cpu().numpy().view(CXW_DTYPE)[:n], d_fields.cpu().numpy().view(FIELD_DTYPE)[:n]

    def ccsds_to_complex(self, d_streams, spans, n_values, order, group_length, d_table=None):
        """template 7.42 streams (spans[i] = (start, bytes) of the uint8 tensor d_streams; with d_table no index pass runs) ->
        (d_complex, complex_offsets, the CXW_DTYPE records, per-field decode records)"""
        torch = self.torch
        pl = self._complex_write_plan_or_raise(n_values, order, group_length)
        n, dev = len(n_values), d_streams.device
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_complex, d_cxw = self._complex_out(pl, n, dev)
        have = d_table is not None
        if not have:
            d_table = torch.zeros(max(1, pl["rsi_entries"]), dtype=torch.int64, device=dev)
        d_results = torch.zeros(max(1, n) * gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_result = torch.zeros(gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        in_offs = None if have else [s for s, _ in spans]
        in_sizes = None if have else [b for _, b in spans]
        self._check(self.ccsds_to_complex_async(order, group_length, d_streams, d_streams.numel(), in_offs, in_sizes, n_values, d_table, have,
                                                d_work, d_results, d_result, d_complex, d_complex.numel(), pl["complex_offsets"], d_cxw),
                    "aec_gpu_grib_ccsds_to_complex_async")
        return (d_complex, pl["complex_offsets"], d_cxw.cpu().numpy().view(CXW_DTYPE)[:n],
                d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[:n])

    def simple_to_complex(self, d_simple, simple_offsets, n_values, order, group_length, simple_sizes=None):
        """template 7.0 streams at simple_offsets (bytes) of the uint8 tensor d_simple -> (d_complex, complex_offsets, the CXW_DTYPE
        records)"""
        torch = self.torch
        pl = self._complex_write_plan_or_raise(n_values, order, group_length)
        n, dev = len(n_values), d_simple.device
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_complex, d_cxw = self._complex_out(pl, n, dev)
        self._check(self.simple_to_complex_async(order, group_length, d_simple, d_simple.numel(), simple_offsets, simple_sizes, n_values, d_work,
                                                 d_complex, d_complex.numel(), pl["complex_offsets"], d_cxw),
                    "aec_gpu_grib_simple_to_complex_async")
        return d_complex, pl["complex_offsets"], d_cxw.cpu().numpy().view(CXW_DTYPE)[:n]

    def _complex_plan_or_raise(self, n_values, fields, elem=F32):
        pl = self.complex_plan(n_values, fields, elem)
        if pl is None:
            raise ValueError("not a batch for one call (aec_gpu_grib_complex_plan)")
        return pl

    def complex_expand(self, d_complex, complex_offsets, complex_sizes, fields, n_values):
        """template 7.2 / 7.3 streams at complex_offsets (bytes) of the uint8 tensor d_complex -> (d_work with the X in the plan's
        rooms, the plan, the CX_DTYPE records: x_min, x_max and status per field)"""
        torch = self.torch
        pl = self._complex_plan_or_raise(n_values, fields)
        n = len(n_values)
        d_work = torch.zeros(pl["work_bytes"] + 16, dtype=torch.uint8, device=d_complex.device)
        d_cx = torch.zeros(max(1, n) * CX_DTYPE.itemsize, dtype=torch.uint8, device=d_complex.device)
        self._check(self.complex_expand_async(fields, n_values, d_complex, d_complex.numel(), complex_offsets, complex_sizes, d_work, d_cx),
                    "aec_gpu_grib_complex_expand_async")
        return d_work, pl, d_cx.cpu().numpy().view(CX_DTYPE)[:n]

    def complex_unpack(self, d_complex, complex_offsets, complex_sizes, fields, params, n_values, dtype=None):
        """template 7.2 / 7.3 streams -> (a float tensor with the fields back to back, the CX_DTYPE records); params the
        FIELD_DTYPE records (R, E, D) of section 5"""
        torch = self.torch
        dtype = dtype or torch.float32
        elem = F32 if dtype == torch.float32 else F64
        pl = self._complex_plan_or_raise(n_values, fields, elem)
        n, dev = len(n_values), d_complex.device
        dst_offsets = np.concatenate([[0], np.cumsum(np.asarray(n_values, dtype=np.uint64))]).astype(np.uint64) * np.uint64(elem)
        d_dst = torch.empty(int(dst_offsets[-1]) // elem, dtype=dtype, device=dev)
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_cx = torch.zeros(max(1, n) * CX_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self._check(self.complex_unpack_async(elem, fields, d_complex, d_complex.numel(), complex_offsets, complex_sizes, n_values, params,
                                              dst_offsets[:n], d_work, d_dst, d_cx), "aec_gpu_grib_complex_unpack_async")
        return d_dst, d_cx.cpu().numpy().view(CX_DTYPE)[:n]

    def complex_to_ccsds(self, d_complex, complex_offsets, complex_sizes, fields, n_values, want_offsets=False):
        """template 7.2 / 7.3 streams -> (d_out, spans, d_table, the CX_DTYPE records): section 7 under template 5.42 of field i is
        d_out[spans[i][0]:][:spans[i][1]].  R, E and D of section 5 stay as they are; nbits becomes this codec's."""
        torch = self.torch
        pl = self._complex_plan_or_raise(n_values, fields)
        n, dev = len(n_values), d_complex.device
        d_out = torch.empty(pl["out_bound"], dtype=torch.uint8, device=dev)
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_rec = torch.zeros(max(1, n) * 2, dtype=torch.int64, device=dev)
        d_res = torch.zeros(gpu.ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_cx = torch.zeros(max(1, n) * CX_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_table = torch.zeros(max(1, pl["rsi_entries"]), dtype=torch.int64, device=dev) if want_offsets else None
        self._check(self.complex_to_ccsds_async(fields, d_complex, d_complex.numel(), complex_offsets, complex_sizes, n_values, d_work, d_out,
                                                d_out.numel(), d_rec, d_table, d_res, d_cx), "aec_gpu_grib_complex_to_ccsds_async")
        if n and d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["overflow"]:
            raise RuntimeError("encode overflow")
        rec = d_rec.cpu().numpy().view(np.uint64).view(BATCH_CHUNK_DTYPE)[:n]
        return d_out, [(int(r["base_bits"]) // 8, (int(r["bits"]) + 7) // 8) for r in rec], d_table, d_cx.cpu().numpy().view(CX_DTYPE)[:n]

    def complex_to_simple(self, d_complex, complex_offsets, complex_sizes, fields, n_values):
        """template 7.2 / 7.3 streams -> (d_simple, simple_offsets, the CX_DTYPE records): complex_expand, then bits_pack"""
        d_work, pl, cx = self.complex_expand(d_complex, complex_offsets, complex_sizes, fields, n_values)
        d_simple, simple_offsets = self.bits_pack(d_work, n_values)
        return d_simple, simple_offsets, cx

    def _simple_plan_or_raise(self, n_values, elem=F32):
        pl = self.simple_plan(n_values, elem)
        if pl is None:
            raise ValueError("not a batch for one call (aec_gpu_grib_simple_plan)")
        return pl

    def bits_pack(self, d_work, n_values):
        """X in the plan's rooms of d_work -> (uint8 tensor with the template 7.0 streams back to back, their byte offsets)"""
        pl = self._simple_plan_or_raise(n_values)
        d_simple = self.torch.empty(max(1, pl["simple_bytes"]), dtype=self.torch.uint8, device=d_work.device)
        self._check(self.bits_pack_async(n_values, d_work, d_simple, pl["simple_offsets"]), "aec_gpu_grib_bits_pack_async")
        return d_simple[:pl["simple_bytes"]], pl["simple_offsets"]

    def bits_unpack(self, d_simple, simple_offsets, n_values, simple_sizes=None):
        """template 7.0 streams at simple_offsets (bytes) of the uint8 tensor d_simple -> (d_work with the X in the plan's rooms,
        the plan)"""
        pl = self._simple_plan_or_raise(n_values)
        d_work = self.torch.zeros(pl["work_bytes"] + 16, dtype=self.torch.uint8, device=d_simple.device)
        self._check(self.bits_unpack_async(n_values, d_simple, d_simple.numel(), simple_offsets, simple_sizes, d_work),
                    "aec_gpu_grib_bits_unpack_async")
        return d_work, pl

    def simple_pack(self, d_values, offsets, n_values, D, params=None):
        """fields of n_values[i] elements at ELEMENT offsets[i] of the float tensor d_values -> (d_simple, simple_offsets, fields):
        section 7 of field i under template 5.0 is d_simple[simple_offsets[i]:][:ceil(n_values[i] * nbits / 8)], fields the
        FIELD_DTYPE records (R, E, D, status) of section 5"""
        torch = self.torch
        elem = _elem_of(d_values)
        pl = self._simple_plan_or_raise(n_values, elem)
        n, dev = len(n_values), d_values.device
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_fields = torch.zeros(max(1, n) * FIELD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_simple = torch.empty(max(1, pl["simple_bytes"]), dtype=torch.uint8, device=dev)
        Dh = np.broadcast_to(np.asarray(D, dtype=np.int32), (n,))
        self._check(self.simple_pack_async(elem, d_values, _u64(offsets) * np.uint64(elem), n_values, Dh, params, d_work, d_fields, d_simple,
                                           pl["simple_offsets"]), "aec_gpu_grib_simple_pack_async")
        return d_simple[:pl["simple_bytes"]], pl["simple_offsets"], d_fields.cpu().numpy().view(FIELD_DTYPE)[:n]

    def simple_unpack(self, d_simple, simple_offsets, params, n_values, simple_sizes=None, dtype=None):
        """template 7.0 streams -> a float tensor with the fields back to back; params the FIELD_DTYPE records of section 5"""
        torch = self.torch
        dtype = dtype or torch.float32
        elem = F32 if dtype == torch.float32 else F64
        pl = self._simple_plan_or_raise(n_values, elem)
        n = len(n_values)
        dst_offsets = np.concatenate([[0], np.cumsum(np.asarray(n_values, dtype=np.uint64))]).astype(np.uint64) * np.uint64(elem)
        d_dst = torch.empty(int(dst_offsets[-1]) // elem, dtype=dtype, device=d_simple.device)
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=d_simple.device)
        self._check(self.simple_unpack_async(elem, d_simple, d_simple.numel(), simple_offsets, simple_sizes, n_values, params, dst_offsets[:n],
                                             d_work, d_dst), "aec_gpu_grib_simple_unpack_async")
        return d_dst

    def simple_to_ccsds(self, d_simple, simple_offsets, n_values, simple_sizes=None, want_offsets=False):
        """template 7.0 streams -> (d_out, spans, d_table) as pack() gives them: section 7 under template 5.42 of field i is
        d_out[spans[i][0]:][:spans[i][1]].  R, E, D and nbits of section 5 stay as they are."""
        torch = self.torch
        pl = self._simple_plan_or_raise(n_values)
        n, dev = len(n_values), d_simple.device
        d_out = torch.empty(pl["out_bound"], dtype=torch.uint8, device=dev)
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_rec = torch.zeros(max(1, n) * 2, dtype=torch.int64, device=dev)
        d_res = torch.zeros(gpu.ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_table = torch.zeros(max(1, pl["rsi_entries"]), dtype=torch.int64, device=dev) if want_offsets else None
        self._check(self.simple_to_ccsds_async(d_simple, d_simple.numel(), simple_offsets, simple_sizes, n_values, d_work, d_out, d_out.numel(),
                                               d_rec, d_table, d_res), "aec_gpu_grib_simple_to_ccsds_async")
        if n and d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["overflow"]:
            raise RuntimeError("encode overflow")
        rec = d_rec.cpu().numpy().view(np.uint64).view(BATCH_CHUNK_DTYPE)[:n]
        return d_out, [(int(r["base_bits"]) // 8, (int(r["bits"]) + 7) // 8) for r in rec], d_table

    def ccsds_to_simple(self, d_streams, spans, n_values, d_table=None):
        """template 7.42 streams (spans[i] = (start, bytes) of the uint8 tensor d_streams; with d_table no index pass runs) ->
        (d_simple, simple_offsets, per-field decode records)"""
        torch = self.torch
        pl = self._simple_plan_or_raise(n_values)
        n, dev = len(n_values), d_streams.device
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_simple = torch.empty(max(1, pl["simple_bytes"]), dtype=torch.uint8, device=dev)
        have = d_table is not None
        if not have:
            d_table = torch.zeros(max(1, pl["rsi_entries"]), dtype=torch.int64, device=dev)
        d_results = torch.zeros(max(1, n) * gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_result = torch.zeros(gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        in_offs = None if have else [s for s, _ in spans]
        in_sizes = None if have else [b for _, b in spans]
        self._check(self.ccsds_to_simple_async(d_streams, d_streams.numel(), in_offs, in_sizes, n_values, d_table, have, d_work, d_results,
                                               d_result, d_simple, pl["simple_offsets"]), "aec_gpu_grib_ccsds_to_simple_async")
        return d_simple[:pl["simple_bytes"]], pl["simple_offsets"], d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[:n]

    def simple_pack_bitmap(self, d_values, offsets, n_points, d_bitmap, bitmap_offsets, n_values, D, params=None):
        """simple_pack() over whole grids with bitmaps, as the two calls the header names: quantise_bitmap_async, then
        bits_pack_async -> (d_simple, simple_offsets, fields); the streams hold the X of the present points only"""
        torch = self.torch
        elem = _elem_of(d_values)
        if self.bitmap_plan(n_points, n_values, elem) is None:
            raise ValueError("not a batch for one call (aec_gpu_grib_bitmap_plan)")
        pl = self._simple_plan_or_raise(n_values, elem)
        n, dev = len(n_values), d_values.device
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_fields = torch.zeros(max(1, n) * FIELD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_simple = torch.empty(max(1, pl["simple_bytes"]), dtype=torch.uint8, device=dev)
        Dh = np.broadcast_to(np.asarray(D, dtype=np.int32), (n,))
        self._check(self.quantise_bitmap_async(elem, d_values, _u64(offsets) * np.uint64(elem), n_values, Dh, params, d_work, d_fields,
                                               d_bitmap, bitmap_offsets, n_points), "aec_gpu_grib_quantise_bitmap_async")
        self._check(self.bits_pack_async(n_values, d_work, d_simple, pl["simple_offsets"]), "aec_gpu_grib_bits_pack_async")
        return d_simple[:pl["simple_bytes"]], pl["simple_offsets"], d_fields.cpu().numpy().view(FIELD_DTYPE)[:n]

    def simple_unpack_bitmap(self, d_simple, simple_offsets, params, n_values, n_points, d_bitmap, bitmap_offsets, missing=9999.0,
                             simple_sizes=None, dtype=None):
        """simple_unpack() into whole grids: bits_unpack_async, then dequantise_bitmap_async -> (float tensor with the grids
        back to back, per-field status: 0 or MISMATCH)"""
        torch = self.torch
        dtype = dtype or torch.float32
        elem = F32 if dtype == torch.float32 else F64
        if self.bitmap_plan(n_points, n_values, elem) is None:
            raise ValueError("not a batch for one call (aec_gpu_grib_bitmap_plan)")
        pl = self._simple_plan_or_raise(n_values, elem)
        n, dev = len(n_values), d_simple.device
        dst_offsets = np.concatenate([[0], np.cumsum(np.asarray(n_points, dtype=np.uint64))]).astype(np.uint64) * np.uint64(elem)
        d_dst = torch.empty(int(dst_offsets[-1]) // elem, dtype=dtype, device=dev)
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_status = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        self._check(self.bits_unpack_async(n_values, d_simple, d_simple.numel(), simple_offsets, simple_sizes, d_work),
                    "aec_gpu_grib_bits_unpack_async")
        self._check(self.dequantise_bitmap_async(elem, d_work, n_values, params, dst_offsets[:n], d_dst, d_bitmap, bitmap_offsets, n_points,
                                                 missing, d_status), "aec_gpu_grib_dequantise_bitmap_async")
        return d_dst, d_status.cpu().numpy()[:n].astype(np.uint32)

    def bitmap(self, d_values, offsets, n_points, missing):
        """grids of n_points[i] elements at ELEMENT offsets[i] of the float tensor d_values -> (d_bitmap, bitmap_offsets,
        counts): the bitmaps back to back in a uint8 tensor, their byte offsets and the present points of every grid as a
        NumPy array -- the n_values of pack_bitmap.  SYNCHRONISES (the counts come to the host): call it once per mask."""
        torch = self.torch
        elem = _elem_of(d_values)
        npts = _u64(n_points)
        sizes = (npts + np.uint64(7)) // np.uint64(8)
        bm_offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        d_bitmap = torch.zeros(max(1, int(bm_offsets[-1])), dtype=torch.uint8, device=d_values.device)
        d_counts = torch.zeros(max(1, npts.size), dtype=torch.int64, device=d_values.device)
        self._check(self.bitmap_async(elem, d_values, _u64(offsets) * np.uint64(elem), npts, missing, d_bitmap, bm_offsets[:-1], d_counts),
                    "aec_gpu_grib_bitmap_async")
        return d_bitmap, bm_offsets[:-1], d_counts.cpu().numpy()[:npts.size].astype(np.uint64)

    def pack_bitmap(self, d_values, offsets, n_points, d_bitmap, bitmap_offsets, n_values, D, params=None, want_offsets=False):
        """pack() over whole grids with bitmaps (of bitmap(), or a message's): -> (d_out, spans, fields, d_table)"""
        torch = self.torch
        elem = _elem_of(d_values)
        pl = self.bitmap_plan(n_points, n_values, elem)
        if pl is None:
            raise ValueError("not a batch for one call (aec_gpu_grib_bitmap_plan)")
        n, dev = len(n_values), d_values.device
        d_out = torch.empty(pl["out_bound"], dtype=torch.uint8, device=dev)
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_rec = torch.zeros(max(1, n) * 2, dtype=torch.int64, device=dev)
        d_fields = torch.zeros(max(1, n) * FIELD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(gpu.ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_table = torch.zeros(max(1, pl["rsi_entries"]), dtype=torch.int64, device=dev) if want_offsets else None
        Dh = np.broadcast_to(np.asarray(D, dtype=np.int32), (n,))
        self._check(self.pack_bitmap_async(elem, d_values, _u64(offsets) * np.uint64(elem), n_values, Dh, params, d_work, d_out,
                                           d_out.numel(), d_rec, d_table, d_fields, d_res, d_bitmap, bitmap_offsets, n_points),
                    "aec_gpu_grib_pack_bitmap_async")
        if n and d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["overflow"]:
            raise RuntimeError("encode overflow")
        rec = d_rec.cpu().numpy().view(np.uint64).view(BATCH_CHUNK_DTYPE)[:n]
        spans = [(int(r["base_bits"]) // 8, (int(r["bits"]) + 7) // 8) for r in rec]
        return d_out, spans, d_fields.cpu().numpy().view(FIELD_DTYPE)[:n], d_table

    def unpack_bitmap(self, d_streams, spans, params, n_values, n_points, d_bitmap, bitmap_offsets, missing=9999.0, d_table=None,
                      dtype=None):
        """unpack() into whole grids: -> (float tensor with the grids back to back, per-field decode records, per-field
        status: 0 or MISMATCH)"""
        torch = self.torch
        dtype = dtype or torch.float32
        elem = F32 if dtype == torch.float32 else F64
        pl = self.bitmap_plan(n_points, n_values, elem)
        if pl is None:
            raise ValueError("not a batch for one call (aec_gpu_grib_bitmap_plan)")
        n, dev = len(n_values), d_streams.device
        dst_offsets = np.concatenate([[0], np.cumsum(np.asarray(n_points, dtype=np.uint64))]).astype(np.uint64) * np.uint64(elem)
        d_dst = torch.empty(int(dst_offsets[-1]) // elem, dtype=dtype, device=dev)
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        have = d_table is not None
        if not have:
            d_table = torch.zeros(max(1, pl["rsi_entries"]), dtype=torch.int64, device=dev)
        d_results = torch.zeros(max(1, n) * gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_result = torch.zeros(gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_status = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        in_offs = None if have else [s for s, _ in spans]
        in_sizes = None if have else [b for _, b in spans]
        self._check(self.unpack_bitmap_async(elem, d_streams, d_streams.numel(), in_offs, in_sizes, n_values, params, dst_offsets[:n],
                                             d_table, have, d_work, d_dst, d_results, d_result, d_bitmap, bitmap_offsets, n_points, missing,
                                             d_status), "aec_gpu_grib_unpack_bitmap_async")
        return d_dst, d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[:n], d_status.cpu().numpy()[:n].astype(np.uint32)

    def _check(self, rc, what):
        if rc != 0:
            raise ValueError(f"not a batch for one call ({what} -> AEC_CONF_ERROR)") if rc == AEC_CONF_ERROR else \
                RuntimeError(f"{what} failed ({rc})")

    def pack(self, d_values, offsets, n_values, D, params=None, want_offsets=False):
        """fields of n_values[i] elements at ELEMENT offsets[i] of the float tensor d_values -> (d_out, spans, fields,
        d_table): section 7 of field i is d_out[spans[i][0]:][:spans[i][1]] (start, bytes), fields the FIELD_DTYPE records
        (R, E, D, status), d_table the int64 RSI table for unpack (None unless want_offsets)"""
        torch = self.torch
        elem = _elem_of(d_values)
        pl = self.plan(n_values, elem)
        if pl is None:
            raise ValueError("not a batch for one call (aec_gpu_grib_plan)")
        n, dev = len(n_values), d_values.device
        d_out = torch.empty(pl["out_bound"], dtype=torch.uint8, device=dev)
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        d_rec = torch.zeros(max(1, n) * 2, dtype=torch.int64, device=dev)
        d_fields = torch.zeros(max(1, n) * FIELD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(gpu.ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_table = torch.zeros(max(1, pl["rsi_entries"]), dtype=torch.int64, device=dev) if want_offsets else None
        Dh = np.broadcast_to(np.asarray(D, dtype=np.int32), (n,))
        self._check(self.pack_async(elem, d_values, _u64(offsets) * np.uint64(elem), n_values, Dh, params, d_work, d_out,
                                    d_out.numel(), d_rec, d_table, d_fields, d_res), "aec_gpu_grib_pack_async")
        if n and d_res.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]["overflow"]:
            raise RuntimeError("encode overflow")
        rec = d_rec.cpu().numpy().view(np.uint64).view(BATCH_CHUNK_DTYPE)[:n]
        spans = [(int(r["base_bits"]) // 8, (int(r["bits"]) + 7) // 8) for r in rec]
        return d_out, spans, d_fields.cpu().numpy().view(FIELD_DTYPE)[:n], d_table

    def unpack(self, d_streams, spans, params, n_values, d_table=None, dtype=None):
        """streams -> (float tensor with the fields back to back, per-field decode records): stream i is spans[i] = (start,
        bytes) of the uint8 tensor d_streams, params the FIELD_DTYPE records of section 5.  With d_table (of pack(...,
        want_offsets=True), positions relative to d_streams) no index pass runs."""
        torch = self.torch
        dtype = dtype or torch.float32
        elem = F32 if dtype == torch.float32 else F64
        pl = self.plan(n_values, elem)
        if pl is None:
            raise ValueError("not a batch for one call (aec_gpu_grib_plan)")
        n, dev = len(n_values), d_streams.device
        dst_offsets = np.concatenate([[0], np.cumsum(np.asarray(n_values, dtype=np.uint64))]).astype(np.uint64) * np.uint64(elem)
        d_dst = torch.empty(int(dst_offsets[-1]) // elem, dtype=dtype, device=dev)
        d_work = torch.empty(pl["work_bytes"] + 16, dtype=torch.uint8, device=dev)
        have = d_table is not None
        if not have:
            d_table = torch.zeros(max(1, pl["rsi_entries"]), dtype=torch.int64, device=dev)
        d_results = torch.zeros(max(1, n) * gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_result = torch.zeros(gpu.DEC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        in_offs = None if have else [s for s, _ in spans]
        in_sizes = None if have else [b for _, b in spans]
        self._check(self.unpack_async(elem, d_streams, d_streams.numel(), in_offs, in_sizes, n_values, params, dst_offsets[:n], d_table,
                                      have, d_work, d_dst, d_results, d_result), "aec_gpu_grib_unpack_async")
        return d_dst, d_results.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[:n]

    def quantise(self, d_values, offsets, n_values, D, params=None):
        """-> (d_work with the X in the plan's rooms, the plan, the FIELD_DTYPE records)"""
        torch = self.torch
        elem = _elem_of(d_values)
        pl = self.plan(n_values, elem)
        if pl is None:
            raise ValueError("not a batch for one call (aec_gpu_grib_plan)")
        n = len(n_values)
        d_work = torch.zeros(pl["work_bytes"] + 16, dtype=torch.uint8, device=d_values.device)
        d_fields = torch.zeros(max(1, n) * FIELD_DTYPE.itemsize, dtype=torch.uint8, device=d_values.device)
        Dh = np.broadcast_to(np.asarray(D, dtype=np.int32), (n,))
        self._check(self.quantise_async(elem, d_values, _u64(offsets) * np.uint64(elem), n_values, Dh, params, d_work, d_fields),
                    "aec_gpu_grib_quantise_async")
        return d_work, pl, d_fields.cpu().numpy().view(FIELD_DTYPE)[:n]

    def dequantise(self, d_work, n_values, params, dtype=None):
        """X in the plan's rooms of d_work -> a float tensor with the fields back to back"""
        torch = self.torch
        dtype = dtype or torch.float32
        elem = F32 if dtype == torch.float32 else F64
        dst_offsets = np.concatenate([[0], np.cumsum(np.asarray(n_values, dtype=np.uint64))]).astype(np.uint64) * np.uint64(elem)
        d_dst = torch.empty(int(dst_offsets[-1]) // elem, dtype=dtype, device=d_work.device)
        self._check(self.dequantise_async(elem, d_work, n_values, params, dst_offsets[:len(n_values)], d_dst),
                    "aec_gpu_grib_dequantise_async")
        return d_dst
