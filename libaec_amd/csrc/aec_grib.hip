// aec_grib.hip -- GRIB2 CCSDS packing on the device (include/aec_gpu_grib.h): what a GRIB writer does between a field of
// floats and its one coder call -- minimum and maximum, R and E, the quantisation to X (WMO regulation 92.9.4) -- and a
// reader behind its decoder call, as kernels, and the one-call forms over the chunk coder of aec_gpu.hip.  The arithmetic
// is aec_grib.h.
//
// Fields are unequal, so a field owns whole wavefronts of a launch and a wavefront reads its field's number from the
// table k_grib_setup wrote (one uint32_t per wavefront: k_grib_minmax's wavefronts, then k_grib_quantise's): the field is
// wave-uniform, its descriptor is read once per wavefront through the scalar cache and so are the three signs of D.
//   minmax      a wavefront reduces 4 KiB of its field: four 16-byte loads a lane where the field's base is 16-byte
//               aligned and the 16 bytes lie inside it, element by element elsewhere (the tail; a field off that
//               boundary).  Keys, not floats: see aec_grib.h.  One atomicMin and one atomicMax per wavefront.
//   quantise    a lane owns one 16-byte group of its field's room (rooms are 16-byte aligned: only a field's last group
//               can be partial): 16 / 8 / 4 values in by 16-byte loads, one 16-byte store out.
//   dequantise  the reverse: one 16-byte load from the room, 16 / 8 / 4 elements out.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <type_traits>

#include "../../include/aec_gpu_grib.h"
#include "aec_grib.h"
#include "aec_kernels.h"

using namespace aec;

static_assert(sizeof(aec_gpu_grib_field) == sizeof(GribRecord) && sizeof(GribRecord) == 16, "record layout");

namespace {

constexpr uint32_t kGribBlock = 256, kGribWaves = kGribBlock / 64;

template <typename T>
using KeyOf = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;

// the table, and the extremes of every field set to "nothing seen" (extremes == null: a call without a minmax)
__global__ void __launch_bounds__(256)
k_grib_setup(const GribField *__restrict__ desc, uint64_t n, uint64_t mm_waves, uint64_t q_waves, uint32_t *__restrict__ wave_field,
             uint64_t *__restrict__ extremes)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < mm_waves + q_waves; i += stride)
        wave_field[i] = i < mm_waves ? (uint32_t)grib_field_of_wave(desc, n, 0, i) : (uint32_t)grib_field_of_wave(desc, n, 1, i - mm_waves);
    if (extremes)
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
            extremes[2 * i] = ~0ull;
            extremes[2 * i + 1] = 0ull;
        }
}

// this wavefront's field and its number within the field; false behind the last wavefront
__device__ __forceinline__ bool grib_wave(const GribField *__restrict__ desc, const uint32_t *__restrict__ wave_field,
                                          uint64_t nwaves, int which, GribField &F, uint32_t &field, uint64_t &in_field)
{
    const uint64_t w = (uint64_t)blockIdx.x * kGribWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= nwaves) return false;
    field = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_field[w]);
    F = desc[field];
    in_field = w - F.wave0[which];
    return true;
}

__device__ __forceinline__ uint32_t grib_shfl(uint32_t v, int off) { return (uint32_t)__shfl_xor((int)v, off); }
__device__ __forceinline__ uint64_t grib_shfl(uint64_t v, int off) { return (uint64_t)__shfl_xor((unsigned long long)v, off); }

template <typename T>
__global__ void __launch_bounds__(kGribBlock)
k_grib_minmax(const GribField *__restrict__ desc, const uint32_t *__restrict__ wave_field, uint64_t nwaves,
              const uint8_t *__restrict__ src, uint64_t *__restrict__ extremes)
{
    typedef KeyOf<T> K;
    constexpr uint32_t per = 16u / sizeof(T);
    GribField F;
    uint32_t field;
    uint64_t in_field;
    if (!grib_wave(desc, wave_field, nwaves, 0, F, field, in_field)) return;
    const T *base = reinterpret_cast<const T *>(src + F.off);
    const uint32_t lane = threadIdx.x & 63u;
    K kmin = ~(K)0, kmax = 0;
    uint64_t first[4];
    uint32_t count[4];
#pragma unroll
    for (uint32_t s = 0; s < 4; s++) grib_minmax_group<T>(in_field, s, lane, F.n, &first[s], &count[s]);
    if ((reinterpret_cast<uintptr_t>(base) & 15u) == 0 && count[3] == per) {       // (the fourth group is whole: so are all)
        uint4 w[4];
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) w[s] = *reinterpret_cast<const uint4 *>(base + first[s]);
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            T v[per];
            memcpy(v, &w[s], 16);
            grib_minmax_take<T, K>(v, per, &kmin, &kmax);
        }
    } else {
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            T v[per];
#pragma unroll
            for (uint32_t i = 0; i < per; i++)
                if (i < count[s]) v[i] = base[first[s] + i];
            grib_minmax_take<T, K>(v, count[s], &kmin, &kmax);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const K a = grib_shfl(kmin, off), b = grib_shfl(kmax, off);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    // (Reading the stored extremes first and sending only the atomics that move one was measured and is slower: 0.95
    // against 0.45 ms for min/max + quantise of 64 fields of 1 038 240 float32, profiles/r20/README.md.)
    if (lane == 0) {
        atomicMin(reinterpret_cast<unsigned long long *>(extremes + 2 * (uint64_t)field), (unsigned long long)grib_widen(kmin));
        atomicMax(reinterpret_cast<unsigned long long *>(extremes + 2 * (uint64_t)field + 1), (unsigned long long)grib_widen(kmax));
    }
}

// a lane per field: the record.  It writes nothing else.
__global__ void __launch_bounds__(256)
k_grib_params(const GribField *__restrict__ desc, uint64_t n, uint32_t nbits, const uint64_t *__restrict__ extremes,
              GribRecord *__restrict__ fields)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GribRecord g = desc[i].given;
    fields[i] = grib_params(extremes[2 * i], extremes[2 * i + 1], g.D, nbits, g.status != 0, g.R, g.E);
}

template <typename T, int CONT>
__global__ void __launch_bounds__(kGribBlock)
k_grib_quantise(const GribField *__restrict__ desc, const uint32_t *__restrict__ wave_field, uint64_t nwaves, uint32_t nbits,
                const uint8_t *__restrict__ src, uint8_t *__restrict__ work, GribRecord *__restrict__ fields)
{
    constexpr uint32_t per = 16u / CONT;                     // values of a group
    constexpr uint32_t loads = per * sizeof(T) / 16u;
    GribField F;
    uint32_t field;
    uint64_t in_field;
    if (!grib_wave(desc, wave_field, nwaves, 1, F, field, in_field)) return;
    const uint64_t g = in_field * 64u + (threadIdx.x & 63u), lo = g * 16u;
    if (lo >= F.room) return;
    const T *base = reinterpret_cast<const T *>(src + F.off);
    const uint64_t j0 = g * per;
    T v[per];
    if ((reinterpret_cast<uintptr_t>(base) & 15u) == 0 && j0 + per <= F.n) {
        uint4 w[loads];
#pragma unroll
        for (uint32_t l = 0; l < loads; l++) w[l] = reinterpret_cast<const uint4 *>(base + j0)[l];
        memcpy(v, w, sizeof(v));
    } else {
#pragma unroll
        for (uint32_t i = 0; i < per; i++) v[i] = base[grib_value_of_sample(j0 + i, F.n)];
    }
    const GribRecord rec = fields[field];
    const bool have = F.given.status != 0;
    const GribQuant q = grib_quant(rec, nbits, have);
    bool clamped = false;
    uint32_t x[per];
    if (rec.D == 0) {
#pragma unroll
        for (uint32_t i = 0; i < per; i++) x[i] = grib_quantise<0>((double)v[i], q, &clamped);
    } else if (rec.D > 0) {
#pragma unroll
        for (uint32_t i = 0; i < per; i++) x[i] = grib_quantise<1>((double)v[i], q, &clamped);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < per; i++) x[i] = grib_quantise<-1>((double)v[i], q, &clamped);
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t i = 0; i < per; i++) w[i * CONT / 4u] |= x[i] << (8u * (i * CONT % 4u));
    uint8_t *out = work + F.work_off + lo;
    if (lo + 16u <= F.room) {
        *reinterpret_cast<uint4 *>(out) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            if (lo + i < F.room) out[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
    // (a field whose record says bad has no X to speak of: its NaNs are not "held")
    if (!(rec.status & kGribBad) && __any(clamped) && (threadIdx.x & 63u) == 0) atomicOr(&fields[field].status, (uint32_t)kGribClamped);
}

template <typename T, int CONT>
__global__ void __launch_bounds__(kGribBlock)
k_grib_dequantise(const GribField *__restrict__ desc, const uint32_t *__restrict__ wave_field, uint64_t nwaves,
                  const uint8_t *__restrict__ work, uint8_t *__restrict__ dst)
{
    constexpr uint32_t per = 16u / CONT;
    constexpr uint32_t stores = per * sizeof(T) / 16u;
    GribField F;
    uint32_t field;
    uint64_t in_field;
    if (!grib_wave(desc, wave_field, nwaves, 1, F, field, in_field)) return;
    const uint64_t g = in_field * 64u + (threadIdx.x & 63u), j0 = g * per;
    if (j0 >= F.n) return;
    // (a room is followed by the padding to the next one: the 16 bytes are the work buffer's wherever the room ends)
    const uint4 in = *reinterpret_cast<const uint4 *>(work + F.work_off + g * 16u);
    const uint32_t w[4] = {in.x, in.y, in.z, in.w};
    const double R = (double)F.given.R, scale = grib_pow2(F.given.E), p = grib_pow10(F.given.D);
    T y[per];
#pragma unroll
    for (uint32_t i = 0; i < per; i++) {
        const uint32_t x = CONT == 4 ? w[i] : (w[i * CONT / 4u] >> (8u * (i * CONT % 4u))) & (CONT == 1 ? 0xFFu : 0xFFFFu);
        y[i] = (T)(F.given.D == 0 ? grib_dequantise<0>(x, R, scale, p)
                                  : F.given.D > 0 ? grib_dequantise<1>(x, R, scale, p) : grib_dequantise<-1>(x, R, scale, p));
    }
    T *out = reinterpret_cast<T *>(dst + F.off) + j0;
    if ((reinterpret_cast<uintptr_t>(out) & 15u) == 0 && j0 + per <= F.n) {
        uint4 o[stores];
        memcpy(o, y, sizeof(y));
#pragma unroll
        for (uint32_t l = 0; l < stores; l++) reinterpret_cast<uint4 *>(out)[l] = o[l];
    } else {
#pragma unroll
        for (uint32_t i = 0; i < per; i++)
            if (j0 + i < F.n) out[i] = y[i];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// No launch counts beyond 2^31 lanes: a batch has at most 2^25 wavefronts in either launch, a field less than 2^35 bytes.
constexpr uint64_t kGribMaxWaves = 1ull << 25, kGribMaxField = 1ull << 35;

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
uint32_t wave_blocks(uint64_t waves) { return (uint32_t)((waves + kGribWaves - 1) / kGribWaves); }

int layout_of(const aec_gpu_grib_template *t, int D, aec_gpu_grib_layout_t *L)
{
    if (!t || !L || (t->options & F_SIGNED) || t->nbits == 0 || t->nbits > 32 || D > kGribMaxD || D < -kGribMaxD) return RC_CONF_ERROR;
    L->coder = aec_gpu_params{t->nbits, t->block_size, t->rsi, grib_flags(t->options)};
    L->container = grib_container(t->nbits);
    return aec_gpu_check_params(&L->coder, 1);
}

aec_gpu_params decoder_of(const aec_gpu_params &p) { return aec_gpu_params{p.bits_per_sample, p.block_size, p.rsi, p.flags & ~(uint32_t)F_NOT_ENFORCE}; }

// the host arrays of a call: rooms and their places in the work buffer
struct GribArrays {
    std::unique_ptr<uint64_t[]> own;
    uint64_t *rooms = nullptr, *work_offsets = nullptr;
    bool make(uint64_t n)
    {
        own.reset(new (std::nothrow) uint64_t[2 * n + 1]);
        rooms = own.get();
        work_offsets = rooms + n;
        return own != nullptr;
    }
};

// host arithmetic of a batch under one template: the plan, the fields' rooms and their places in the work buffer (a,
// allocated here, once, when the arguments have been checked) and the wavefronts of the two launches.  RC_OK, or
// RC_CONF_ERROR = refused.
int fields_shape(const aec_gpu_grib_template *t, int elem, const uint64_t *n_values, uint64_t n, aec_gpu_grib_plan_t *plan,
                 GribArrays *a, uint64_t waves[2])
{
    aec_gpu_grib_layout_t L;
    if (layout_of(t, 0, &L) != RC_OK || (elem != AEC_GPU_GRIB_F32 && elem != AEC_GPU_GRIB_F64) || (n && !n_values) || n > 0x7FFFFFFFull)
        return RC_CONF_ERROR;
    if (!a->make(n)) return RC_MEM_ERROR;
    uint64_t *rooms = a->rooms, *work_offsets = a->work_offsets;
    uint64_t work = 0;
    waves[0] = waves[1] = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (n_values[i] == 0 || n_values[i] >= kGribMaxField || n_values[i] * (uint32_t)elem >= kGribMaxField) return RC_CONF_ERROR;
        rooms[i] = grib_room(n_values[i], t->block_size, L.container);
        if (rooms[i] >= kGribMaxField) return RC_CONF_ERROR;
        work_offsets[i] = work;
        work += (rooms[i] + 15u) & ~(uint64_t)15u;
        waves[0] += grib_minmax_waves(n_values[i], (uint32_t)elem);
        waves[1] += grib_room_waves(rooms[i]);
        if (waves[0] > kGribMaxWaves || waves[1] > kGribMaxWaves) return RC_CONF_ERROR;
    }
    aec_gpu_chunks_plan cp;
    aec_gpu_dchunks_plan dp;
    const aec_gpu_params pd = decoder_of(L.coder);
    if (!aec_gpu_encode_chunks_plan(&L.coder, rooms, n, &cp) || !aec_gpu_decode_chunks_plan(&pd, rooms, n, &dp)) return RC_CONF_ERROR;
    plan->coder = L.coder;
    plan->work_bytes = (size_t)work;
    plan->out_bound = cp.out_bound;
    plan->rsi_entries = cp.rsi_entries;
    plan->workspace_bytes = (cp.workspace_bytes > dp.workspace_bytes ? cp.workspace_bytes : dp.workspace_bytes) +
                            up256((size_t)(n + 1) * sizeof(GribField)) + up256((size_t)(waves[0] + waves[1] + 1) * 4) +
                            up256((size_t)(n ? n : 1) * 16);
    return RC_OK;
}

// every field's place is a multiple of the element size, every D is one the layout takes, every given E one grib_pow2 takes
bool fields_ok(const void *base, const uint64_t *offsets, const int32_t *D, const aec_gpu_grib_field *params, bool use_params_D,
               uint64_t n, int elem)
{
    for (uint64_t i = 0; i < n; i++) {
        if ((reinterpret_cast<uintptr_t>(base) + offsets[i]) % (uint32_t)elem) return false;
        const int d = use_params_D ? params[i].D : D[i];
        if (d > kGribMaxD || d < -kGribMaxD) return false;
        if (params && (params[i].E > 1022 || params[i].E < -1022)) return false;
    }
    return true;
}

// the descriptors of a batch on the device, the wavefront table and the extremes behind them, filled (one transfer, one
// launch)
struct GribOnDevice {
    const GribField *desc;
    const uint32_t *wave_field;         // k_grib_minmax's wavefronts, then k_grib_quantise's
    uint64_t *extremes;                 // per field: the keys of its minimum and maximum
};

int send_fields(aec_gpu_ctx *ctx, const uint64_t *offsets, const uint64_t *n_values, const uint64_t *work_offsets,
                const uint64_t *rooms, const int32_t *D, const aec_gpu_grib_field *params, bool have, uint64_t n, int elem,
                bool minmax, hipStream_t st, GribOnDevice *on)
{
    const size_t h_need = (size_t)(n + 1) * sizeof(GribField);
    void *h = nullptr;
    void *stage = ctx_sz_stage(ctx, h_need, &h);
    if (!stage) return RC_MEM_ERROR;
    GribField *d = static_cast<GribField *>(h);
    uint64_t w0 = 0, w1 = 0;
    for (uint64_t i = 0; i <= n; i++) {
        GribField &f = d[i];
        f = GribField{};
        f.wave0[0] = w0;
        f.wave0[1] = w1;
        if (i == n) break;
        f.off = offsets[i];
        f.n = n_values[i];
        f.work_off = work_offsets[i];
        f.room = rooms[i];
        f.given.D = D ? D[i] : params[i].D;
        if (have) {
            f.given.R = params[i].R;
            f.given.E = params[i].E;
            f.given.status = 1;
        }
        if (minmax) w0 += grib_minmax_waves(f.n, (uint32_t)elem);
        w1 += grib_room_waves(f.room);
    }
    const size_t desc_bytes = up256(h_need), table_bytes = up256((size_t)(w0 + w1 + 1) * 4);
    uint8_t *cd = ctx_sz_send(ctx, stage, h_need, desc_bytes + table_bytes + up256((size_t)n * 16), st);
    if (!cd) return RC_MEM_ERROR;
    on->desc = reinterpret_cast<const GribField *>(cd);
    uint32_t *table = reinterpret_cast<uint32_t *>(cd + desc_bytes);
    on->wave_field = table;
    on->extremes = reinterpret_cast<uint64_t *>(cd + desc_bytes + table_bytes);
    const uint64_t items = w0 + w1 > n ? w0 + w1 : n, grid = (items + 255) / 256;
    hipLaunchKernelGGL(k_grib_setup, dim3((uint32_t)(grid < 4096 ? grid : 4096)), dim3(256), 0, st, on->desc, n, w0, w1, table,
                       minmax ? on->extremes : nullptr);
    return RC_OK;
}

template <typename T>
void launch_quantise(uint32_t container, uint64_t waves, hipStream_t st, const GribOnDevice &on, uint64_t mm_waves, uint32_t nbits,
                     const uint8_t *src, uint8_t *work, GribRecord *fields)
{
    const dim3 grid(wave_blocks(waves)), block(kGribBlock);
    const uint32_t *table = on.wave_field + mm_waves;
    if (container == 1) hipLaunchKernelGGL((k_grib_quantise<T, 1>), grid, block, 0, st, on.desc, table, waves, nbits, src, work, fields);
    else if (container == 2) hipLaunchKernelGGL((k_grib_quantise<T, 2>), grid, block, 0, st, on.desc, table, waves, nbits, src, work, fields);
    else hipLaunchKernelGGL((k_grib_quantise<T, 4>), grid, block, 0, st, on.desc, table, waves, nbits, src, work, fields);
}

template <typename T>
void launch_dequantise(uint32_t container, uint64_t waves, hipStream_t st, const GribOnDevice &on, const uint8_t *work, uint8_t *dst)
{
    const dim3 grid(wave_blocks(waves)), block(kGribBlock);
    if (container == 1) hipLaunchKernelGGL((k_grib_dequantise<T, 1>), grid, block, 0, st, on.desc, on.wave_field, waves, work, dst);
    else if (container == 2) hipLaunchKernelGGL((k_grib_dequantise<T, 2>), grid, block, 0, st, on.desc, on.wave_field, waves, work, dst);
    else hipLaunchKernelGGL((k_grib_dequantise<T, 4>), grid, block, 0, st, on.desc, on.wave_field, waves, work, dst);
}

// minimum and maximum, parameters, quantisation: everything of a pack in front of the encoder
int quantise(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src, const uint64_t *src_offsets,
             const uint64_t *n_values, const int32_t *D, bool have, const aec_gpu_grib_field *params, uint64_t n, void *d_work,
             aec_gpu_grib_field *d_fields, const GribArrays &a, const uint64_t waves[2], hipStream_t st)
{
    GribOnDevice on;
    const int rc = send_fields(ctx, src_offsets, n_values, a.work_offsets, a.rooms, D, params, have, n, elem, true, st, &on);
    if (rc != RC_OK) return rc;
    const uint8_t *src = static_cast<const uint8_t *>(d_src);
    GribRecord *fields = reinterpret_cast<GribRecord *>(d_fields);
    if (elem == AEC_GPU_GRIB_F32)
        hipLaunchKernelGGL(k_grib_minmax<float>, dim3(wave_blocks(waves[0])), dim3(kGribBlock), 0, st, on.desc, on.wave_field, waves[0], src, on.extremes);
    else
        hipLaunchKernelGGL(k_grib_minmax<double>, dim3(wave_blocks(waves[0])), dim3(kGribBlock), 0, st, on.desc, on.wave_field, waves[0], src, on.extremes);
    hipLaunchKernelGGL(k_grib_params, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, on.desc, n, t->nbits, on.extremes, fields);
    const uint32_t container = grib_container(t->nbits);
    if (elem == AEC_GPU_GRIB_F32) launch_quantise<float>(container, waves[1], st, on, waves[0], t->nbits, src, static_cast<uint8_t *>(d_work), fields);
    else launch_quantise<double>(container, waves[1], st, on, waves[0], t->nbits, src, static_cast<uint8_t *>(d_work), fields);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

int dequantise(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_work, const uint64_t *n_values,
               const aec_gpu_grib_field *params, const uint64_t *dst_offsets, uint64_t n, void *d_dst, const GribArrays &a,
               const uint64_t waves[2], hipStream_t st)
{
    GribOnDevice on;
    const int rc = send_fields(ctx, dst_offsets, n_values, a.work_offsets, a.rooms, nullptr, params, true, n, elem, false, st, &on);
    if (rc != RC_OK) return rc;
    const uint32_t container = grib_container(t->nbits);
    if (elem == AEC_GPU_GRIB_F32) launch_dequantise<float>(container, waves[1], st, on, static_cast<const uint8_t *>(d_work), static_cast<uint8_t *>(d_dst));
    else launch_dequantise<double>(container, waves[1], st, on, static_cast<const uint8_t *>(d_work), static_cast<uint8_t *>(d_dst));
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

// the checks the pack-side calls share; RC_OK with *n == 0 handled by the caller
int pack_args(const aec_gpu_grib_template *t, int elem, aec_gpu_ctx *ctx, const void *d_src, const uint64_t *src_offsets,
              const uint64_t *n_values, const int32_t *D, int have_params, const aec_gpu_grib_field *params, uint64_t n,
              void *d_work, aec_gpu_grib_field *d_fields, GribArrays *a, aec_gpu_grib_plan_t *plan, uint64_t waves[2])
{
    if (!ctx || !d_src || !src_offsets || !n_values || !D || (have_params && !params) || !d_work ||
        !aligned(d_work, 16) || !d_fields || !aligned(d_fields, 16) || n > 0x7FFFFFFFull)
        return RC_CONF_ERROR;
    const int rc = fields_shape(t, elem, n_values, n, plan, a, waves);
    if (rc != RC_OK) return rc;
    return fields_ok(d_src, src_offsets, D, have_params ? params : nullptr, false, n, elem) ? RC_OK : RC_CONF_ERROR;
}

int unpack_args(const aec_gpu_grib_template *t, int elem, aec_gpu_ctx *ctx, const void *d_work, const uint64_t *n_values,
                const aec_gpu_grib_field *params, const uint64_t *dst_offsets, uint64_t n, void *d_dst, GribArrays *a,
                aec_gpu_grib_plan_t *plan, uint64_t waves[2])
{
    if (!ctx || !d_work || !aligned(d_work, 16) || !n_values || !params || !dst_offsets || !d_dst || n > 0x7FFFFFFFull)
        return RC_CONF_ERROR;
    const int rc = fields_shape(t, elem, n_values, n, plan, a, waves);
    if (rc != RC_OK) return rc;
    return fields_ok(d_dst, dst_offsets, nullptr, params, true, n, elem) ? RC_OK : RC_CONF_ERROR;
}

}  // namespace

extern "C" {

int aec_gpu_grib_layout(const aec_gpu_grib_template *t, int D, aec_gpu_grib_layout_t *layout) { return layout_of(t, D, layout); }

int aec_gpu_grib_plan(const aec_gpu_grib_template *t, int elem, const uint64_t *n_values, uint64_t n_fields,
                      aec_gpu_grib_plan_t *plan, uint64_t *work_offsets)
{
    uint64_t waves[2];
    GribArrays a;
    if (!plan || fields_shape(t, elem, n_values, n_fields, plan, &a, waves) != RC_OK) return 0;
    if (work_offsets && n_fields) memcpy(work_offsets, a.work_offsets, (size_t)n_fields * sizeof(uint64_t));
    return 1;
}

int aec_gpu_grib_quantise_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src,
                                const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D, int have_params,
                                const aec_gpu_grib_field *params, uint64_t n_fields, void *d_work, aec_gpu_grib_field *d_fields,
                                void *stream)
{
    aec_gpu_grib_layout_t L;
    if (layout_of(t, 0, &L) != RC_OK || (elem != AEC_GPU_GRIB_F32 && elem != AEC_GPU_GRIB_F64)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    GribArrays a;
    aec_gpu_grib_plan_t plan;
    uint64_t waves[2];
    const int rc = pack_args(t, elem, ctx, d_src, src_offsets, n_values, D, have_params, params, n_fields, d_work, d_fields, &a,
                             &plan, waves);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return quantise(ctx, t, elem, d_src, src_offsets, n_values, D, have_params != 0, params, n_fields, d_work,
                    d_fields, a, waves, static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_pack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src,
                            const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D, int have_params,
                            const aec_gpu_grib_field *params, uint64_t n_fields, void *d_work, void *d_out, size_t out_cap,
                            aec_gpu_batch_chunk *d_chunks, uint64_t *d_rsi_bit_offsets, aec_gpu_grib_field *d_fields,
                            aec_gpu_enc_result *d_result, void *stream)
{
    aec_gpu_grib_layout_t L;
    if (layout_of(t, 0, &L) != RC_OK || (elem != AEC_GPU_GRIB_F32 && elem != AEC_GPU_GRIB_F64)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    if (!d_out || !d_chunks || !d_result || !aligned(d_out, 16) || (out_cap & 15u) || out_cap < 16) return RC_CONF_ERROR;
    GribArrays a;
    aec_gpu_grib_plan_t plan;
    uint64_t waves[2];
    int rc = pack_args(t, elem, ctx, d_src, src_offsets, n_values, D, have_params, params, n_fields, d_work, d_fields, &a, &plan,
                       waves);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    rc = quantise(ctx, t, elem, d_src, src_offsets, n_values, D, have_params != 0, params, n_fields, d_work,
                  d_fields, a, waves, static_cast<hipStream_t>(stream));
    if (rc != RC_OK) return rc;
    return aec_gpu_encode_chunks_async(ctx, &plan.coder, d_work, a.work_offsets, a.rooms, n_fields, d_out, out_cap, d_chunks,
                                       d_rsi_bit_offsets, d_result, stream);
}

int aec_gpu_grib_dequantise_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_work,
                                  const uint64_t *n_values, const aec_gpu_grib_field *params, const uint64_t *dst_offsets,
                                  uint64_t n_fields, void *d_dst, void *stream)
{
    aec_gpu_grib_layout_t L;
    if (layout_of(t, 0, &L) != RC_OK || (elem != AEC_GPU_GRIB_F32 && elem != AEC_GPU_GRIB_F64)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    GribArrays a;
    aec_gpu_grib_plan_t plan;
    uint64_t waves[2];
    const int rc = unpack_args(t, elem, ctx, d_work, n_values, params, dst_offsets, n_fields, d_dst, &a, &plan, waves);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return dequantise(ctx, t, elem, d_work, n_values, params, dst_offsets, n_fields, d_dst, a, waves, static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_unpack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_in, size_t in_bytes,
                              const uint64_t *in_offsets, const uint64_t *in_bytes_each, const uint64_t *n_values,
                              const aec_gpu_grib_field *params, const uint64_t *dst_offsets, uint64_t n_fields,
                              uint64_t *d_rsi_bit_offsets, int have_table, void *d_work, void *d_dst, aec_gpu_dec_result *d_results,
                              aec_gpu_dec_result *d_result, void *stream)
{
    aec_gpu_grib_layout_t L;
    if (layout_of(t, 0, &L) != RC_OK || (elem != AEC_GPU_GRIB_F32 && elem != AEC_GPU_GRIB_F64)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    if (!d_in) return RC_CONF_ERROR;
    GribArrays a;
    aec_gpu_grib_plan_t plan;
    uint64_t waves[2];
    int rc = unpack_args(t, elem, ctx, d_work, n_values, params, dst_offsets, n_fields, d_dst, &a, &plan, waves);
    if (rc != RC_OK) return rc;
    const aec_gpu_params p = decoder_of(plan.coder);
    rc = aec_gpu_decode_chunks_async(ctx, &p, d_in, in_bytes, in_offsets, in_bytes_each, a.work_offsets, a.rooms, n_fields,
                                     d_rsi_bit_offsets, have_table, d_work, d_results, d_result, stream);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return dequantise(ctx, t, elem, d_work, n_values, params, dst_offsets, n_fields, d_dst, a, waves, static_cast<hipStream_t>(stream));
}

}  // extern "C"
