// aec_gribbits.hip -- GRIB2 simple packing (template 5.0 / 7.0, ecCodes' grid_simple) on the device (include/aec_gpu_grib.h,
// SIMPLE PACKING): the X rooms of the GRIB layer to big-endian strings of nbits-bit integers at any byte and back, and the
// calls that compose them with the quantiser of aec_grib.hip and the chunk coder of aec_gpu.hip.  The arithmetic is
// aec_gribbits.h.
//
// The launch shape is k_grib_quantise's: a field owns whole wavefronts, a wavefront kGribWaveRoom = 1 KiB of its field's
// room, a lane one 16-byte group of it; the field is wave-uniform and comes from a table (one uint32_t per wavefront),
// its descriptor -- GribField, `off` the stream's byte offset -- is read once per wavefront.  A wavefront's share of the
// stream is one contiguous range of 128 / 64 / 32 * nbits bytes for containers of 1 / 2 / 4 bytes.
//   bits_pack    one 16-byte load of the room, the lane's string (at most 128 bits) in registers, its bytes out: aligned
//                words where they lie inside the lane's bytes, single bytes at its two ends.  No byte is stored twice and
//                nothing is read back: a lane of 4 values under an odd nbits shares a byte with its neighbour, which the
//                even lane stores whole after one __shfl_down of the odd lane's first word.
//   bits_unpack  the aligned words around the lane's string (bytes where a word would leave the buffer), two funnel shifts
//                to the string, the values out of it, one 16-byte store; the samples that pad the last block read value
//                n - 1 at its own bit position.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>

#include "../../include/aec_gpu_grib.h"
#include "aec_gribbits.h"
#include "aec_kernels.h"

using namespace aec;

namespace {

constexpr uint32_t kBitsBlock = 256, kBitsWaves = kBitsBlock / 64;

// the field of every wavefront
__global__ void __launch_bounds__(256)
k_grib_bits_setup(const GribField *__restrict__ desc, uint64_t n, uint64_t waves, uint32_t *__restrict__ wave_field)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < waves; i += stride)
        wave_field[i] = (uint32_t)grib_field_of_wave(desc, n, 1, i);
}

// this wavefront's field and its number within the field; false behind the last wavefront
__device__ __forceinline__ bool bits_wave(const GribField *__restrict__ desc, const uint32_t *__restrict__ wave_field, uint64_t nwaves,
                                          GribField &F, uint64_t &in_field)
{
    const uint64_t w = (uint64_t)blockIdx.x * kBitsWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= nwaves) return false;
    const uint32_t field = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_field[w]);
    F = desc[field];
    in_field = w - F.wave0[1];
    return true;
}

// plain loads and stores at byte offsets from the buffer's base (aec_gribbits.h: Mem)
struct BitsMem {
    uint8_t *p;
    __device__ __forceinline__ uint32_t ld8(int64_t o) const { return p[o]; }
    __device__ __forceinline__ uint32_t ld32(int64_t o) const { return *reinterpret_cast<const uint32_t *>(p + o); }
    __device__ __forceinline__ void st8(int64_t o, uint8_t v) const { p[o] = v; }
    __device__ __forceinline__ void st32(int64_t o, uint32_t v) const { *reinterpret_cast<uint32_t *>(p + o) = v; }
};

template <int CONT>
__global__ void __launch_bounds__(kBitsBlock)
k_grib_bits_pack(const GribField *__restrict__ desc, const uint32_t *__restrict__ wave_field, uint64_t nwaves, uint32_t nbits,
                 const uint8_t *__restrict__ work, uint8_t *__restrict__ simple, uint32_t mis)
{
    GribField F;
    uint64_t in_field;
    if (!bits_wave(desc, wave_field, nwaves, F, in_field)) return;
    const uint32_t lane = threadIdx.x & 63u;
    const GribBitsLane L = grib_bits_lane(in_field, lane, 16u / CONT, F.n, F.off, nbits);
    uint64_t hi = 0, lo = 0;
    if (L.cnt) {
        // (a room is followed by the padding to the next one: the 16 bytes are the work buffer's wherever the room ends)
        const uint4 in = *reinterpret_cast<const uint4 *>(work + F.work_off + (in_field * 64u + lane) * 16u);
        const uint32_t w[4] = {in.x, in.y, in.z, in.w};
        grib_bits_of_group<CONT>(w, nbits, L.cnt, &hi, &lo);
    }
    // (the whole wavefront shuffles; a lane without a value hands on 0, lane 63 has no follower in its last byte)
    const uint32_t follower = (uint32_t)__shfl_down((int)grib_bits_head(hi), 1);
    BitsMem m{simple};
    grib_bits_store(m, hi, lo, L.p0, L.p1, lane < 63u ? follower : 0u, mis);
}

template <int CONT>
__global__ void __launch_bounds__(kBitsBlock)
k_grib_bits_unpack(const GribField *__restrict__ desc, const uint32_t *__restrict__ wave_field, uint64_t nwaves, uint32_t nbits,
                   const uint8_t *__restrict__ simple, uint32_t mis, uint64_t simple_bytes, uint8_t *__restrict__ work)
{
    GribField F;
    uint64_t in_field;
    if (!bits_wave(desc, wave_field, nwaves, F, in_field)) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t at = (in_field * 64u + lane) * 16u;
    if (at >= F.room) return;
    const GribBitsLane L = grib_bits_lane(in_field, lane, 16u / CONT, F.n, F.off, nbits);
    BitsMem m{const_cast<uint8_t *>(simple)};
    uint32_t w[4];
    grib_bits_group_of<CONT>(m, L, F.off, F.n, nbits, mis, simple_bytes, w);
    uint8_t *out = work + F.work_off + at;
    if (at + 16u <= F.room) {
        *reinterpret_cast<uint4 *>(out) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            if (at + i < F.room) out[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// host arithmetic of a batch: the plan of aec_gpu_grib_plan, the rooms, their places, the streams' sizes
struct BitsShape {
    aec_gpu_grib_plan_t plan;
    std::unique_ptr<uint64_t[]> own;
    uint64_t *rooms = nullptr, *work_offsets = nullptr, *sizes = nullptr;
    uint64_t waves = 0, simple_bytes = 0;
};

int bits_shape(const aec_gpu_grib_template *t, int elem, const uint64_t *n_values, uint64_t n, BitsShape *s)
{
    if ((n && !n_values) || n > 0x7FFFFFFFull) return RC_CONF_ERROR;
    s->own.reset(new (std::nothrow) uint64_t[3 * n + 1]);
    if (!s->own) return RC_MEM_ERROR;
    s->rooms = s->own.get();
    s->work_offsets = s->rooms + n;
    s->sizes = s->work_offsets + n;
    if (!aec_gpu_grib_plan(t, elem, n_values, n, &s->plan, s->work_offsets)) return RC_CONF_ERROR;
    const uint32_t container = grib_container(t->nbits);
    for (uint64_t i = 0; i < n; i++) {
        s->rooms[i] = grib_room(n_values[i], t->block_size, container);
        s->sizes[i] = grib_bits_bytes(n_values[i], t->nbits);         // (n < 2^35, nbits <= 32: no overflow)
        s->waves += grib_room_waves(s->rooms[i]);
        s->simple_bytes += s->sizes[i];
    }
    return RC_OK;
}

// the template alone, checked before anything else (an empty batch under a bad template is refused)
bool template_ok(const aec_gpu_grib_template *t)
{
    aec_gpu_grib_layout_t L;
    return aec_gpu_grib_layout(t, 0, &L) == RC_OK;
}

// every stream inside [0, simple_bytes) and, where the caller says how long section 7 is, not longer than that
bool streams_inside(const BitsShape &s, uint64_t n, size_t simple_bytes, const uint64_t *simple_offsets, const uint64_t *each)
{
    for (uint64_t i = 0; i < n; i++) {
        if (each && each[i] < s.sizes[i]) return false;
        if (simple_offsets[i] > simple_bytes || s.sizes[i] > simple_bytes - simple_offsets[i]) return false;
    }
    return true;
}

struct BitsOnDevice {
    const GribField *desc;
    const uint32_t *wave_field;
};

// the descriptors of a batch on the device and the wavefront table behind them (one transfer, one launch); they take the
// place of the GRIB layer's in the context's buffer, which aec_gpu_grib_plan counts
int bits_send(aec_gpu_ctx *ctx, const BitsShape &s, const uint64_t *n_values, const uint64_t *simple_offsets, uint64_t n, hipStream_t st,
              BitsOnDevice *on)
{
    const size_t h_need = (size_t)(n + 1) * sizeof(GribField);
    void *h = nullptr;
    void *stage = ctx_sz_stage(ctx, h_need, &h);
    if (!stage) return RC_MEM_ERROR;
    GribField *d = static_cast<GribField *>(h);
    uint64_t w = 0;
    for (uint64_t i = 0; i <= n; i++) {
        d[i] = GribField{};
        d[i].wave0[1] = w;
        if (i == n) break;
        d[i].off = simple_offsets[i];
        d[i].n = n_values[i];
        d[i].work_off = s.work_offsets[i];
        d[i].room = s.rooms[i];
        w += grib_room_waves(s.rooms[i]);
    }
    const size_t desc_bytes = up256(h_need);
    uint8_t *cd = ctx_sz_send(ctx, stage, h_need, desc_bytes + up256((size_t)(w + 1) * 4), st);
    if (!cd) return RC_MEM_ERROR;
    on->desc = reinterpret_cast<const GribField *>(cd);
    uint32_t *table = reinterpret_cast<uint32_t *>(cd + desc_bytes);
    on->wave_field = table;
    const uint64_t grid = (w + 255) / 256;
    hipLaunchKernelGGL(k_grib_bits_setup, dim3((uint32_t)(grid < 4096 ? grid : 4096)), dim3(256), 0, st, on->desc, n, w, table);
    return RC_OK;
}

int bits_pack(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const BitsShape &s, const uint64_t *n_values, uint64_t n, const void *d_work,
              void *d_simple, const uint64_t *simple_offsets, hipStream_t st)
{
    BitsOnDevice on;
    const int rc = bits_send(ctx, s, n_values, simple_offsets, n, st, &on);
    if (rc != RC_OK) return rc;
    const dim3 grid((uint32_t)((s.waves + kBitsWaves - 1) / kBitsWaves)), block(kBitsBlock);
    const uint8_t *work = static_cast<const uint8_t *>(d_work);
    uint8_t *simple = static_cast<uint8_t *>(d_simple);
    const uint32_t container = grib_container(t->nbits), mis = (uint32_t)(reinterpret_cast<uintptr_t>(d_simple) & 3u);
#define BITS_P(C) hipLaunchKernelGGL((k_grib_bits_pack<C>), grid, block, 0, st, on.desc, on.wave_field, s.waves, t->nbits, work, simple, mis)
    if (container == 1) BITS_P(1);
    else if (container == 2) BITS_P(2);
    else BITS_P(4);
#undef BITS_P
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

int bits_unpack(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const BitsShape &s, const uint64_t *n_values, uint64_t n,
                const void *d_simple, size_t simple_bytes, const uint64_t *simple_offsets, void *d_work, hipStream_t st)
{
    BitsOnDevice on;
    const int rc = bits_send(ctx, s, n_values, simple_offsets, n, st, &on);
    if (rc != RC_OK) return rc;
    const dim3 grid((uint32_t)((s.waves + kBitsWaves - 1) / kBitsWaves)), block(kBitsBlock);
    const uint8_t *simple = static_cast<const uint8_t *>(d_simple);
    uint8_t *work = static_cast<uint8_t *>(d_work);
    const uint32_t container = grib_container(t->nbits), mis = (uint32_t)(reinterpret_cast<uintptr_t>(d_simple) & 3u);
#define BITS_U(C) hipLaunchKernelGGL((k_grib_bits_unpack<C>), grid, block, 0, st, on.desc, on.wave_field, s.waves, t->nbits, simple, mis, \
                                     (uint64_t)simple_bytes, work)
    if (container == 1) BITS_U(1);
    else if (container == 2) BITS_U(2);
    else BITS_U(4);
#undef BITS_U
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

// the checks of the calls that read streams; RC_OK with the shape filled
int unpack_args(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const uint64_t *n_values, uint64_t n, const void *d_simple,
                size_t simple_bytes, const uint64_t *simple_offsets, const uint64_t *simple_bytes_each, void *d_work, BitsShape *s)
{
    if (!ctx || !n_values || !d_simple || !simple_offsets || !d_work || !aligned(d_work, 16)) return RC_CONF_ERROR;
    const int rc = bits_shape(t, elem, n_values, n, s);
    if (rc != RC_OK) return rc;
    return streams_inside(*s, n, simple_bytes, simple_offsets, simple_bytes_each) ? RC_OK : RC_CONF_ERROR;
}

// ... and of those that write them
int pack_args(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const uint64_t *n_values, uint64_t n, const void *d_work,
              void *d_simple, const uint64_t *simple_offsets, BitsShape *s)
{
    if (!ctx || !n_values || !d_simple || !simple_offsets || !d_work || !aligned(d_work, 16)) return RC_CONF_ERROR;
    return bits_shape(t, elem, n_values, n, s);
}

aec_gpu_params decoder_of(const aec_gpu_params &p) { return aec_gpu_params{p.bits_per_sample, p.block_size, p.rsi, p.flags & ~(uint32_t)F_NOT_ENFORCE}; }

}  // namespace

extern "C" {

int aec_gpu_grib_simple_plan(const aec_gpu_grib_template *t, int elem, const uint64_t *n_values, uint64_t n_fields,
                             aec_gpu_grib_simple_plan_t *plan, uint64_t *work_offsets, uint64_t *simple_offsets)
{
    BitsShape s;
    if (!plan || bits_shape(t, elem, n_values, n_fields, &s) != RC_OK) return 0;
    plan->plan = s.plan;
    plan->simple_bytes = (size_t)s.simple_bytes;
    if (work_offsets && n_fields) memcpy(work_offsets, s.work_offsets, (size_t)n_fields * sizeof(uint64_t));
    if (simple_offsets) {
        uint64_t at = 0;
        for (uint64_t i = 0; i < n_fields; i++) {
            simple_offsets[i] = at;
            at += s.sizes[i];
        }
    }
    return 1;
}

int aec_gpu_grib_bits_pack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const uint64_t *n_values, uint64_t n_fields,
                                 const void *d_work, void *d_simple, const uint64_t *simple_offsets, void *stream)
{
    if (!template_ok(t)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    BitsShape s;
    const int rc = pack_args(ctx, t, AEC_GPU_GRIB_F32, n_values, n_fields, d_work, d_simple, simple_offsets, &s);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return bits_pack(ctx, t, s, n_values, n_fields, d_work, d_simple, simple_offsets, static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_bits_unpack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const uint64_t *n_values, uint64_t n_fields,
                                   const void *d_simple, size_t simple_bytes, const uint64_t *simple_offsets,
                                   const uint64_t *simple_bytes_each, void *d_work, void *stream)
{
    if (!template_ok(t)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    BitsShape s;
    const int rc = unpack_args(ctx, t, AEC_GPU_GRIB_F32, n_values, n_fields, d_simple, simple_bytes, simple_offsets, simple_bytes_each,
                               d_work, &s);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return bits_unpack(ctx, t, s, n_values, n_fields, d_simple, simple_bytes, simple_offsets, d_work, static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_simple_pack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src,
                                   const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D, int have_params,
                                   const aec_gpu_grib_field *params, uint64_t n_fields, void *d_work, aec_gpu_grib_field *d_fields,
                                   void *d_simple, const uint64_t *simple_offsets, void *stream)
{
    if (!template_ok(t) || (elem != AEC_GPU_GRIB_F32 && elem != AEC_GPU_GRIB_F64)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    BitsShape s;
    int rc = pack_args(ctx, t, elem, n_values, n_fields, d_work, d_simple, simple_offsets, &s);
    if (rc != RC_OK) return rc;
    rc = aec_gpu_grib_quantise_async(ctx, t, elem, d_src, src_offsets, n_values, D, have_params, params, n_fields, d_work, d_fields, stream);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return bits_pack(ctx, t, s, n_values, n_fields, d_work, d_simple, simple_offsets, static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_simple_unpack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_simple, size_t simple_bytes,
                                     const uint64_t *simple_offsets, const uint64_t *simple_bytes_each, const uint64_t *n_values,
                                     const aec_gpu_grib_field *params, const uint64_t *dst_offsets, uint64_t n_fields, void *d_work,
                                     void *d_dst, void *stream)
{
    if (!template_ok(t) || (elem != AEC_GPU_GRIB_F32 && elem != AEC_GPU_GRIB_F64)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    BitsShape s;
    int rc = unpack_args(ctx, t, elem, n_values, n_fields, d_simple, simple_bytes, simple_offsets, simple_bytes_each, d_work, &s);
    if (rc != RC_OK) return rc;
    // (the checks of the second half first: a call it refuses enqueues nothing.  Its launch comes behind the bits.)
    if (!params || !dst_offsets || !d_dst) return RC_CONF_ERROR;
    for (uint64_t i = 0; i < n_fields; i++)
        if ((reinterpret_cast<uintptr_t>(d_dst) + dst_offsets[i]) % (uint32_t)elem || params[i].D > kGribMaxD || params[i].D < -kGribMaxD ||
            params[i].E > 1022 || params[i].E < -1022)
            return RC_CONF_ERROR;
    (void)hipGetLastError();
    rc = bits_unpack(ctx, t, s, n_values, n_fields, d_simple, simple_bytes, simple_offsets, d_work, static_cast<hipStream_t>(stream));
    if (rc != RC_OK) return rc;
    return aec_gpu_grib_dequantise_async(ctx, t, elem, d_work, n_values, params, dst_offsets, n_fields, d_dst, stream);
}

int aec_gpu_grib_simple_to_ccsds_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const void *d_simple, size_t simple_bytes,
                                       const uint64_t *simple_offsets, const uint64_t *simple_bytes_each, const uint64_t *n_values,
                                       uint64_t n_fields, void *d_work, void *d_out, size_t out_cap, aec_gpu_batch_chunk *d_chunks,
                                       uint64_t *d_rsi_bit_offsets, aec_gpu_enc_result *d_result, void *stream)
{
    if (!template_ok(t)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    if (!d_out || !d_chunks || !d_result || !aligned(d_out, 16) || (out_cap & 15u) || out_cap < 16) return RC_CONF_ERROR;
    BitsShape s;
    int rc = unpack_args(ctx, t, AEC_GPU_GRIB_F32, n_values, n_fields, d_simple, simple_bytes, simple_offsets, simple_bytes_each, d_work, &s);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    rc = bits_unpack(ctx, t, s, n_values, n_fields, d_simple, simple_bytes, simple_offsets, d_work, static_cast<hipStream_t>(stream));
    if (rc != RC_OK) return rc;
    return aec_gpu_encode_chunks_async(ctx, &s.plan.coder, d_work, s.work_offsets, s.rooms, n_fields, d_out, out_cap, d_chunks,
                                       d_rsi_bit_offsets, d_result, stream);
}

int aec_gpu_grib_ccsds_to_simple_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const void *d_in, size_t in_bytes,
                                       const uint64_t *in_offsets, const uint64_t *in_bytes_each, const uint64_t *n_values,
                                       uint64_t n_fields, uint64_t *d_rsi_bit_offsets, int have_table, void *d_work,
                                       aec_gpu_dec_result *d_results, aec_gpu_dec_result *d_result, void *d_simple,
                                       const uint64_t *simple_offsets, void *stream)
{
    if (!template_ok(t)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    if (!d_in) return RC_CONF_ERROR;
    BitsShape s;
    int rc = pack_args(ctx, t, AEC_GPU_GRIB_F32, n_values, n_fields, d_work, d_simple, simple_offsets, &s);
    if (rc != RC_OK) return rc;
    const aec_gpu_params p = decoder_of(s.plan.coder);
    rc = aec_gpu_decode_chunks_async(ctx, &p, d_in, in_bytes, in_offsets, in_bytes_each, s.work_offsets, s.rooms, n_fields,
                                     d_rsi_bit_offsets, have_table, d_work, d_results, d_result, stream);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return bits_pack(ctx, t, s, n_values, n_fields, d_work, d_simple, simple_offsets, static_cast<hipStream_t>(stream));
}

}  // extern "C"
