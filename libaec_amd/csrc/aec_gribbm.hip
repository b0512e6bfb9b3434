// aec_gribbm.hip -- GRIB2 section 6 bitmaps on the device (include/aec_gpu_grib.h, the *_bitmap_* calls): the pack and the
// unpack of aec_grib.hip for fields with missing points, without a compacted copy of the floats ever being written.  The
// arithmetic is aec_gribbm.h (and aec_grib.h: keys, grib_params, grib_quantise, grib_dequantise, unchanged).
//
// A field owns whole tiles of kGribBmTile = 1024 grid points, a wavefront owns a tile (the table k_grib_bm_setup wrote says
// whose), a lane 16 consecutive points: two bytes of the bitmap, read as bytes, and 64 (float32) or 128 (float64) bytes
// of values, read by 16-byte loads where the field's base is 16-byte aligned and the 16 points exist.
//   pack    setup, k_grib_bm_minmax (keys of the present points, one atomicMin / atomicMax a wavefront, the tile's count),
//           k_grib_bm_scan (a wavefront per field: tile counts -> tile bases, the total against n_values, the record),
//           k_grib_bm_quantise (X of a present point to sample base + rank of the room, by stores of ONE container: two
//           wavefronts meet inside a word, so nothing wider is written and nothing is read back), then the chunk encoder.
//   unpack  the chunk decoder, setup, k_grib_bm_count (bitmap only), the same scan, k_grib_bm_expand (sample base + rank
//           back to its point, the missing value's bits elsewhere).
//   build   k_grib_bm_build: values to bitmap bytes, one 64-bit atomicAdd a wavefront into the field's count.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <type_traits>

#include "../../include/aec_gpu_grib.h"
#include "aec_gribbm.h"
#include "aec_kernels.h"

using namespace aec;

static_assert(AEC_GPU_GRIB_MISMATCH == kGribMismatch && AEC_GPU_GRIB_TILE_POINTS == kGribBmTile, "header and kernels agree");

namespace {

constexpr uint32_t kBmBlock = 256, kBmWaves = kBmBlock / 64;

template <typename T>
using KeyOf = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;

// what a call leaves in the context's descriptor buffer
struct BmOnDevice {
    const GribField *desc;
    const GribBitmap *bm;
    uint32_t *tile_field;        // the field of every tile
    uint64_t *extremes;          // per field: the keys of the minimum and maximum of its present points
    uint32_t *counts;            // per tile: its ones
    uint64_t *bases;             // per tile: the ones of its field in front of it
};

// the tile table; the extremes set to "nothing seen" and the counts of a build cleared (either may be null)
__global__ void __launch_bounds__(256)
k_grib_bm_setup(const GribBitmap *__restrict__ bm, uint64_t n, uint64_t tiles, uint32_t *__restrict__ tile_field,
                uint64_t *__restrict__ extremes, uint64_t *__restrict__ ones)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = first; i < tiles; i += stride) tile_field[i] = (uint32_t)grib_bm_field_of_tile(bm, n, i);
    for (uint64_t i = first; i < n; i += stride) {
        if (extremes) {
            extremes[2 * i] = ~0ull;
            extremes[2 * i + 1] = 0ull;
        }
        if (ones) ones[i] = 0ull;
    }
}

// this wavefront's tile: its field, its descriptors and its number within the field; false behind the last tile
__device__ __forceinline__ bool bm_tile(const BmOnDevice &on, uint64_t tiles, GribField &F, GribBitmap &B, uint32_t &field, uint64_t &tile,
                                        uint64_t &in_field)
{
    tile = (uint64_t)blockIdx.x * kBmWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (tile >= tiles) return false;
    field = (uint32_t)__builtin_amdgcn_readfirstlane((int)on.tile_field[tile]);
    F = on.desc[field];
    B = on.bm[field];
    in_field = tile - B.tile0;
    return true;
}

// the lane's word of its field's bitmap: byte loads, and only of bytes the bitmap has
__device__ __forceinline__ uint32_t bm_word(const uint8_t *__restrict__ bitmap, const GribBitmap &B, const GribBmLane &L)
{
    const uint8_t *p = bitmap + B.bm_off + L.byte0;
    const uint32_t b0 = L.nbytes > 0 ? p[0] : 0u, b1 = L.nbytes > 1 ? p[1] : 0u;
    return grib_bm_word(b0, b1, L.valid);
}

// inclusive sum over the lanes 0 .. lane of the wavefront
__device__ __forceinline__ uint32_t bm_scan(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) v = grib_bm_scan_step(v, (uint32_t)__shfl_up((int)v, off), lane, off);
    return v;
}
__device__ __forceinline__ uint32_t bm_last(uint32_t inclusive) { return (uint32_t)__shfl((int)inclusive, 63); }

// the lane's 16 values: 16-byte loads where the base is aligned and all 16 exist, else the elements the field has
template <typename T>
__device__ __forceinline__ void bm_load(const T *__restrict__ base, const GribBmLane &L, T (&v)[kGribBmLane])
{
    if ((reinterpret_cast<uintptr_t>(base) & 15u) == 0 && L.valid == kGribBmLane) {
        constexpr uint32_t loads = kGribBmLane * sizeof(T) / 16u;
        uint4 w[loads];
#pragma unroll
        for (uint32_t l = 0; l < loads; l++) w[l] = reinterpret_cast<const uint4 *>(base + L.p0)[l];
        memcpy(v, w, sizeof(v));
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kGribBmLane; j++) v[j] = j < L.valid ? base[L.p0 + j] : (T)0;
    }
}

__device__ __forceinline__ uint32_t bm_shfl(uint32_t v, int off) { return (uint32_t)__shfl_xor((int)v, off); }
__device__ __forceinline__ uint64_t bm_shfl(uint64_t v, int off) { return (uint64_t)__shfl_xor((unsigned long long)v, off); }

// WITH_VALUES: the keys of the tile's present points into the field's extremes; always: the tile's count
template <typename T, bool WITH_VALUES>
__global__ void __launch_bounds__(kBmBlock)
k_grib_bm_minmax(BmOnDevice on, uint64_t tiles, const uint8_t *__restrict__ bitmap, const uint8_t *__restrict__ src)
{
    typedef KeyOf<T> K;
    GribField F;
    GribBitmap B;
    uint32_t field;
    uint64_t tile, in_field;
    if (!bm_tile(on, tiles, F, B, field, tile, in_field)) return;
    const uint32_t lane = threadIdx.x & 63u;
    const GribBmLane L = grib_bm_lane(in_field, lane, B.points);
    const uint32_t word = bm_word(bitmap, B, L);
    const uint32_t ones = bm_last(bm_scan(grib_bm_count(word), lane));
    if (lane == 0) on.counts[tile] = ones;
    if (!WITH_VALUES || ones == 0) return;
    K kmin = ~(K)0, kmax = 0;
    if (word) {
        T v[kGribBmLane];
        bm_load(reinterpret_cast<const T *>(src + F.off), L, v);
#pragma unroll
        for (uint32_t j = 0; j < kGribBmLane; j++)
            if (grib_bm_present(word, j)) grib_minmax_take<T, K>(&v[j], 1u, &kmin, &kmax);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const K a = bm_shfl(kmin, off), b = bm_shfl(kmax, off);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if (lane == 0) {
        atomicMin(reinterpret_cast<unsigned long long *>(on.extremes + 2 * (uint64_t)field), (unsigned long long)grib_widen(kmin));
        atomicMax(reinterpret_cast<unsigned long long *>(on.extremes + 2 * (uint64_t)field + 1), (unsigned long long)grib_widen(kmax));
    }
}

// a wavefront per field: tile counts to tile bases, 64 tiles a round; the total against the host's count; with fields the
// record (grib_params of the extremes, plus bit 3), with status the bit alone
__global__ void __launch_bounds__(kBmBlock)
k_grib_bm_scan(BmOnDevice on, uint64_t n, uint32_t nbits, GribRecord *__restrict__ fields, uint32_t *__restrict__ status)
{
    const uint64_t field = (uint64_t)blockIdx.x * kBmWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (field >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t tile0 = on.bm[field].tile0, ntiles = on.bm[field + 1].tile0 - tile0;
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += 64) {
        const uint64_t t = t0 + lane;
        const uint32_t c = t < ntiles ? on.counts[tile0 + t] : 0u;
        const uint32_t incl = bm_scan(c, lane);
        if (t < ntiles) on.bases[tile0 + t] = grib_bm_tile_base(carry, incl, c);
        carry += bm_last(incl);
    }
    if (lane != 0) return;
    const uint32_t bit = grib_bm_mismatch(carry, on.desc[field].n);
    if (status) status[field] = bit;
    if (fields) {
        const GribRecord g = on.desc[field].given;
        GribRecord r = grib_params(on.extremes[2 * field], on.extremes[2 * field + 1], g.D, nbits, g.status != 0, g.R, g.E);
        r.status |= bit;
        fields[field] = r;
    }
}

template <int CONT>
__device__ __forceinline__ void bm_store_x(uint8_t *__restrict__ room, uint64_t sample, uint32_t x)
{
    if (CONT == 1) room[sample] = (uint8_t)x;
    else if (CONT == 2) reinterpret_cast<uint16_t *>(room)[sample] = (uint16_t)x;
    else reinterpret_cast<uint32_t *>(room)[sample] = x;
}

template <typename T, int CONT, int DSIGN>
__device__ __forceinline__ void bm_quantise_lane(const T (&v)[kGribBmLane], uint32_t word, uint64_t r0, const GribField &F, const GribQuant &q,
                                                 uint8_t *__restrict__ room, bool *clamped)
{
#pragma unroll
    for (uint32_t j = 0; j < kGribBmLane; j++) {
        const uint64_t r = r0 + grib_bm_rank(word, j);
        if (!grib_bm_present(word, j) || !grib_bm_kept(r, F.n)) continue;
        const uint32_t x = grib_quantise<DSIGN>((double)v[j], q, clamped);
        bm_store_x<CONT>(room, r, x);
        if (grib_bm_pads(r, F.n))
            for (uint64_t s = F.n; s < F.room / CONT; s++) bm_store_x<CONT>(room, s, x);
    }
}

template <typename T, int CONT>
__global__ void __launch_bounds__(kBmBlock)
k_grib_bm_quantise(BmOnDevice on, uint64_t tiles, uint32_t nbits, const uint8_t *__restrict__ bitmap, const uint8_t *__restrict__ src,
                   uint8_t *__restrict__ work, GribRecord *__restrict__ fields)
{
    GribField F;
    GribBitmap B;
    uint32_t field;
    uint64_t tile, in_field;
    if (!bm_tile(on, tiles, F, B, field, tile, in_field)) return;
    if (on.counts[tile] == 0) return;
    const uint32_t lane = threadIdx.x & 63u;
    const GribBmLane L = grib_bm_lane(in_field, lane, B.points);
    const uint32_t word = bm_word(bitmap, B, L), ones = grib_bm_count(word);
    const uint64_t r0 = on.bases[tile] + (bm_scan(ones, lane) - ones);
    const GribRecord rec = fields[field];
    bool clamped = false;
    if (word && grib_bm_kept(r0, F.n)) {
        T v[kGribBmLane];
        bm_load(reinterpret_cast<const T *>(src + F.off), L, v);
        const GribQuant q = grib_quant(rec, nbits, F.given.status != 0);
        uint8_t *room = work + F.work_off;
        if (rec.D == 0) bm_quantise_lane<T, CONT, 0>(v, word, r0, F, q, room, &clamped);
        else if (rec.D > 0) bm_quantise_lane<T, CONT, 1>(v, word, r0, F, q, room, &clamped);
        else bm_quantise_lane<T, CONT, -1>(v, word, r0, F, q, room, &clamped);
    }
    if (!(rec.status & kGribBad) && __any(clamped) && lane == 0) atomicOr(&fields[field].status, (uint32_t)kGribClamped);
}

template <int CONT>
__device__ __forceinline__ uint32_t bm_load_x(const uint8_t *__restrict__ room, uint64_t sample)
{
    if (CONT == 1) return room[sample];
    if (CONT == 2) return reinterpret_cast<const uint16_t *>(room)[sample];
    return reinterpret_cast<const uint32_t *>(room)[sample];
}

template <typename T, int CONT>
__global__ void __launch_bounds__(kBmBlock)
k_grib_bm_expand(BmOnDevice on, uint64_t tiles, const uint8_t *__restrict__ bitmap, const uint8_t *__restrict__ work,
                 uint8_t *__restrict__ dst, KeyOf<T> missing_bits)
{
    GribField F;
    GribBitmap B;
    uint32_t field;
    uint64_t tile, in_field;
    if (!bm_tile(on, tiles, F, B, field, tile, in_field)) return;
    const uint32_t lane = threadIdx.x & 63u;
    const GribBmLane L = grib_bm_lane(in_field, lane, B.points);
    const uint32_t word = bm_word(bitmap, B, L), ones = grib_bm_count(word);
    const uint64_t r0 = on.bases[tile] + (bm_scan(ones, lane) - ones);       // (the whole wavefront scans; then the lanes
    if (L.valid == 0) return;                                                // behind the field's last point leave)
    const double R = (double)F.given.R, scale = grib_pow2(F.given.E), p = grib_pow10(F.given.D);
    const uint8_t *room = work + F.work_off;
    T missing;
    memcpy(&missing, &missing_bits, sizeof(T));
    T y[kGribBmLane];
#pragma unroll
    for (uint32_t j = 0; j < kGribBmLane; j++) {
        const bool present = grib_bm_present(word, j);
        const uint32_t x = present ? bm_load_x<CONT>(room, grib_bm_sample(r0 + grib_bm_rank(word, j), F.n)) : 0u;
        const T value = (T)(F.given.D == 0 ? grib_dequantise<0>(x, R, scale, p)
                                           : F.given.D > 0 ? grib_dequantise<1>(x, R, scale, p) : grib_dequantise<-1>(x, R, scale, p));
        y[j] = present ? value : missing;
    }
    T *out = reinterpret_cast<T *>(dst + F.off) + L.p0;
    if ((reinterpret_cast<uintptr_t>(out) & 15u) == 0 && L.valid == kGribBmLane) {
        constexpr uint32_t stores = kGribBmLane * sizeof(T) / 16u;
        uint4 o[stores];
        memcpy(o, y, sizeof(y));
#pragma unroll
        for (uint32_t l = 0; l < stores; l++) reinterpret_cast<uint4 *>(out)[l] = o[l];
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kGribBmLane; j++)
            if (j < L.valid) out[j] = y[j];
    }
}

template <typename T>
__global__ void __launch_bounds__(kBmBlock)
k_grib_bm_build(BmOnDevice on, uint64_t tiles, const uint8_t *__restrict__ src, uint8_t *__restrict__ bitmap, KeyOf<T> missing_bits,
                uint64_t *__restrict__ ones_of_field)
{
    GribField F;
    GribBitmap B;
    uint32_t field;
    uint64_t tile, in_field;
    if (!bm_tile(on, tiles, F, B, field, tile, in_field)) return;
    const uint32_t lane = threadIdx.x & 63u;
    const GribBmLane L = grib_bm_lane(in_field, lane, B.points);
    T missing;
    memcpy(&missing, &missing_bits, sizeof(T));
    const bool is_nan = missing != missing;
    uint32_t word = 0;
    if (L.valid) {
        T v[kGribBmLane];
        bm_load(reinterpret_cast<const T *>(src + F.off), L, v);
#pragma unroll
        for (uint32_t j = 0; j < kGribBmLane; j++)
            if (j < L.valid && !grib_bm_is_missing(v[j], missing, is_nan)) word |= 1u << (15u - j);
        uint8_t *p = bitmap + B.bm_off + L.byte0;
        if (L.nbytes > 0) p[0] = (uint8_t)grib_bm_byte(word, 0);
        if (L.nbytes > 1) p[1] = (uint8_t)grib_bm_byte(word, 1);
    }
    const uint32_t ones = bm_last(bm_scan(grib_bm_count(word), lane));
    if (lane == 0 && ones) atomicAdd(reinterpret_cast<unsigned long long *>(ones_of_field + field), (unsigned long long)ones);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
constexpr uint64_t kBmMaxTiles = 1ull << 25, kBmMaxField = 1ull << 35;

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
uint32_t tile_blocks(uint64_t tiles) { return (uint32_t)((tiles + kBmWaves - 1) / kBmWaves); }
bool elem_ok(int elem) { return elem == AEC_GPU_GRIB_F32 || elem == AEC_GPU_GRIB_F64; }

// the tiles of a batch of grids; false = refused
bool tiles_of(const uint64_t *n_points, uint64_t n, int elem, uint64_t *tiles)
{
    *tiles = 0;
    if ((n && !n_points) || n > 0x7FFFFFFFull) return false;
    for (uint64_t i = 0; i < n; i++) {
        if (n_points[i] == 0 || n_points[i] >= kBmMaxField || n_points[i] * (uint32_t)elem >= kBmMaxField) return false;
        *tiles += grib_bm_tiles(n_points[i]);
        if (*tiles > kBmMaxTiles) return false;
    }
    return true;
}

// host arithmetic of a batch with bitmaps: aec_gpu_grib_plan for the present points, the rooms, the tiles
struct BmShape {
    aec_gpu_grib_bitmap_plan_t plan;
    std::unique_ptr<uint64_t[]> own;
    uint64_t *rooms = nullptr, *work_offsets = nullptr;
};

size_t bm_workspace(uint64_t n, uint64_t tiles)
{
    return up256((size_t)(n + 1) * sizeof(GribBitmap)) + up256((size_t)(n + 1) * sizeof(GribField)) + 2 * up256((size_t)(tiles + 1) * 4) +
           up256((size_t)(tiles + 1) * 8) + up256((size_t)(n ? n : 1) * 16);
}

int bm_shape(const aec_gpu_grib_template *t, int elem, const uint64_t *n_points, const uint64_t *n_values, uint64_t n, BmShape *s)
{
    if (!elem_ok(elem) || (n && (!n_points || !n_values)) || n > 0x7FFFFFFFull) return RC_CONF_ERROR;
    s->own.reset(new (std::nothrow) uint64_t[2 * n + 1]);
    if (!s->own) return RC_MEM_ERROR;
    s->rooms = s->own.get();
    s->work_offsets = s->rooms + n;
    if (!aec_gpu_grib_plan(t, elem, n_values, n, &s->plan.plan, s->work_offsets)) return RC_CONF_ERROR;
    uint64_t tiles;
    if (!tiles_of(n_points, n, elem, &tiles)) return RC_CONF_ERROR;
    const uint32_t container = grib_container(t->nbits);
    for (uint64_t i = 0; i < n; i++) {
        if (n_values[i] > n_points[i]) return RC_CONF_ERROR;
        s->rooms[i] = grib_room(n_values[i], t->block_size, container);
    }
    s->plan.tile_points = kGribBmTile;
    s->plan.tiles = tiles;
    s->plan.plan.workspace_bytes += bm_workspace(n, tiles);
    return RC_OK;
}

// every field's place is a multiple of the element size, every D one the layout takes, every given E one grib_pow2 takes
bool places_ok(const void *base, const uint64_t *offsets, const int32_t *D, const aec_gpu_grib_field *params, bool use_params_D, uint64_t n,
               int elem)
{
    for (uint64_t i = 0; i < n; i++) {
        if ((reinterpret_cast<uintptr_t>(base) + offsets[i]) % (uint32_t)elem) return false;
        if (D || use_params_D) {
            const int d = use_params_D ? params[i].D : D[i];
            if (d > kGribMaxD || d < -kGribMaxD) return false;
        }
        if (params && (params[i].E > 1022 || params[i].E < -1022)) return false;
    }
    return true;
}

// the descriptors of a batch on the device and the tables behind them (one transfer, one launch).  n_values, work_offsets,
// rooms, D and params may be null (a build).
int bm_send(aec_gpu_ctx *ctx, const uint64_t *offsets, const uint64_t *n_points, const uint64_t *bitmap_offsets, const uint64_t *n_values,
            const uint64_t *work_offsets, const uint64_t *rooms, const int32_t *D, const aec_gpu_grib_field *params, bool have, uint64_t n,
            uint64_t tiles, bool extremes, uint64_t *d_ones, hipStream_t st, BmOnDevice *on)
{
    const size_t desc_bytes = up256((size_t)(n + 1) * sizeof(GribField)), bm_bytes = up256((size_t)(n + 1) * sizeof(GribBitmap));
    const size_t h_need = desc_bytes + bm_bytes;
    void *h = nullptr;
    void *stage = ctx_sz_stage(ctx, h_need, &h);
    if (!stage) return RC_MEM_ERROR;
    memset(h, 0, h_need);
    GribField *d = static_cast<GribField *>(h);
    GribBitmap *b = reinterpret_cast<GribBitmap *>(static_cast<uint8_t *>(h) + desc_bytes);
    uint64_t t0 = 0;
    for (uint64_t i = 0; i < n; i++) {
        d[i].off = offsets[i];
        d[i].n = n_values ? n_values[i] : 0;
        d[i].work_off = work_offsets ? work_offsets[i] : 0;
        d[i].room = rooms ? rooms[i] : 0;
        d[i].given.D = D ? D[i] : params ? params[i].D : 0;
        if (have) {
            d[i].given.R = params[i].R;
            d[i].given.E = params[i].E;
            d[i].given.status = 1;
        }
        b[i].bm_off = bitmap_offsets[i];
        b[i].points = n_points[i];
        b[i].tile0 = t0;
        t0 += grib_bm_tiles(n_points[i]);
    }
    b[n].tile0 = t0;
    const size_t table_bytes = up256((size_t)(tiles + 1) * 4), ext_bytes = up256((size_t)n * 16), base_bytes = up256((size_t)(tiles + 1) * 8);
    uint8_t *cd = ctx_sz_send(ctx, stage, h_need, h_need + 2 * table_bytes + ext_bytes + base_bytes, st);
    if (!cd) return RC_MEM_ERROR;
    on->desc = reinterpret_cast<const GribField *>(cd);
    on->bm = reinterpret_cast<const GribBitmap *>(cd + desc_bytes);
    on->bases = reinterpret_cast<uint64_t *>(cd + h_need);
    on->extremes = reinterpret_cast<uint64_t *>(cd + h_need + base_bytes);
    on->tile_field = reinterpret_cast<uint32_t *>(cd + h_need + base_bytes + ext_bytes);
    on->counts = reinterpret_cast<uint32_t *>(cd + h_need + base_bytes + ext_bytes + table_bytes);
    const uint64_t items = tiles > n ? tiles : n, grid = (items + 255) / 256;
    hipLaunchKernelGGL(k_grib_bm_setup, dim3((uint32_t)(grid < 4096 ? grid : 4096)), dim3(256), 0, st, on->bm, n, tiles, on->tile_field,
                       extremes ? on->extremes : nullptr, d_ones);
    return RC_OK;
}

template <typename T>
KeyOf<T> missing_bits_of(double missing)
{
    const T m = (T)missing;             // the host's cast, once: a NaN's payload is the host's
    KeyOf<T> b;
    memcpy(&b, &m, sizeof(T));
    return b;
}

// everything of a pack in front of the encoder
int quantise_bm(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src, const uint64_t *src_offsets,
                const uint64_t *n_values, const int32_t *D, bool have, const aec_gpu_grib_field *params, uint64_t n, void *d_work,
                aec_gpu_grib_field *d_fields, const void *d_bitmap, const uint64_t *bitmap_offsets, const uint64_t *n_points, const BmShape &s,
                hipStream_t st)
{
    BmOnDevice on;
    const uint64_t tiles = s.plan.tiles;
    const int rc = bm_send(ctx, src_offsets, n_points, bitmap_offsets, n_values, s.work_offsets, s.rooms, D, params, have, n, tiles, true,
                           nullptr, st, &on);
    if (rc != RC_OK) return rc;
    const uint8_t *src = static_cast<const uint8_t *>(d_src), *bitmap = static_cast<const uint8_t *>(d_bitmap);
    uint8_t *work = static_cast<uint8_t *>(d_work);
    GribRecord *fields = reinterpret_cast<GribRecord *>(d_fields);
    const dim3 grid(tile_blocks(tiles)), block(kBmBlock);
    const uint32_t container = grib_container(t->nbits), nbits = t->nbits;
    if (elem == AEC_GPU_GRIB_F32) hipLaunchKernelGGL((k_grib_bm_minmax<float, true>), grid, block, 0, st, on, tiles, bitmap, src);
    else hipLaunchKernelGGL((k_grib_bm_minmax<double, true>), grid, block, 0, st, on, tiles, bitmap, src);
    hipLaunchKernelGGL(k_grib_bm_scan, dim3(tile_blocks(n)), block, 0, st, on, n, nbits, fields, (uint32_t *)nullptr);
#define BM_Q(T, C) hipLaunchKernelGGL((k_grib_bm_quantise<T, C>), grid, block, 0, st, on, tiles, nbits, bitmap, src, work, fields)
    if (elem == AEC_GPU_GRIB_F32) {
        if (container == 1) BM_Q(float, 1);
        else if (container == 2) BM_Q(float, 2);
        else BM_Q(float, 4);
    } else {
        if (container == 1) BM_Q(double, 1);
        else if (container == 2) BM_Q(double, 2);
        else BM_Q(double, 4);
    }
#undef BM_Q
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

// everything of an unpack behind the decoder
int expand_bm(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_work, const uint64_t *n_values,
              const aec_gpu_grib_field *params, const uint64_t *dst_offsets, uint64_t n, void *d_dst, const void *d_bitmap,
              const uint64_t *bitmap_offsets, const uint64_t *n_points, double missing, uint32_t *d_status, const BmShape &s, hipStream_t st)
{
    BmOnDevice on;
    const uint64_t tiles = s.plan.tiles;
    const int rc = bm_send(ctx, dst_offsets, n_points, bitmap_offsets, n_values, s.work_offsets, s.rooms, nullptr, params, true, n, tiles,
                           false, nullptr, st, &on);
    if (rc != RC_OK) return rc;
    const uint8_t *work = static_cast<const uint8_t *>(d_work), *bitmap = static_cast<const uint8_t *>(d_bitmap);
    uint8_t *dst = static_cast<uint8_t *>(d_dst);
    const dim3 grid(tile_blocks(tiles)), block(kBmBlock);
    const uint32_t container = grib_container(t->nbits);
    hipLaunchKernelGGL((k_grib_bm_minmax<float, false>), grid, block, 0, st, on, tiles, bitmap, (const uint8_t *)nullptr);
    hipLaunchKernelGGL(k_grib_bm_scan, dim3(tile_blocks(n)), block, 0, st, on, n, t->nbits, (GribRecord *)nullptr, d_status);
#define BM_E(T, C) hipLaunchKernelGGL((k_grib_bm_expand<T, C>), grid, block, 0, st, on, tiles, bitmap, work, dst, missing_bits_of<T>(missing))
    if (elem == AEC_GPU_GRIB_F32) {
        if (container == 1) BM_E(float, 1);
        else if (container == 2) BM_E(float, 2);
        else BM_E(float, 4);
    } else {
        if (container == 1) BM_E(double, 1);
        else if (container == 2) BM_E(double, 2);
        else BM_E(double, 4);
    }
#undef BM_E
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

// the checks the pack-side calls share
int pack_args(const aec_gpu_grib_template *t, int elem, aec_gpu_ctx *ctx, const void *d_src, const uint64_t *src_offsets,
              const uint64_t *n_values, const int32_t *D, int have_params, const aec_gpu_grib_field *params, uint64_t n, void *d_work,
              aec_gpu_grib_field *d_fields, const void *d_bitmap, const uint64_t *bitmap_offsets, const uint64_t *n_points, BmShape *s)
{
    if (!ctx || !d_src || !src_offsets || !n_values || !D || (have_params && !params) || !d_work || !aligned(d_work, 16) || !d_fields ||
        !aligned(d_fields, 16) || !d_bitmap || !bitmap_offsets || !n_points)
        return RC_CONF_ERROR;
    const int rc = bm_shape(t, elem, n_points, n_values, n, s);
    if (rc != RC_OK) return rc;
    return places_ok(d_src, src_offsets, D, have_params ? params : nullptr, false, n, elem) ? RC_OK : RC_CONF_ERROR;
}

int unpack_args(const aec_gpu_grib_template *t, int elem, aec_gpu_ctx *ctx, const void *d_work, const uint64_t *n_values,
                const aec_gpu_grib_field *params, const uint64_t *dst_offsets, uint64_t n, void *d_dst, const void *d_bitmap,
                const uint64_t *bitmap_offsets, const uint64_t *n_points, uint32_t *d_status, BmShape *s)
{
    if (!ctx || !d_work || !aligned(d_work, 16) || !n_values || !params || !dst_offsets || !d_dst || !d_bitmap || !bitmap_offsets ||
        !n_points || !d_status || !aligned(d_status, 4))
        return RC_CONF_ERROR;
    const int rc = bm_shape(t, elem, n_points, n_values, n, s);
    if (rc != RC_OK) return rc;
    return places_ok(d_dst, dst_offsets, nullptr, params, true, n, elem) ? RC_OK : RC_CONF_ERROR;
}

// the template and the element type, checked before anything else (an empty batch under a bad template is refused)
bool template_ok(const aec_gpu_grib_template *t, int elem)
{
    aec_gpu_grib_layout_t L;
    return aec_gpu_grib_layout(t, 0, &L) == RC_OK && elem_ok(elem);
}

aec_gpu_params decoder_of(const aec_gpu_params &p) { return aec_gpu_params{p.bits_per_sample, p.block_size, p.rsi, p.flags & ~(uint32_t)F_NOT_ENFORCE}; }

}  // namespace

extern "C" {

int aec_gpu_grib_bitmap_plan(const aec_gpu_grib_template *t, int elem, const uint64_t *n_points, const uint64_t *n_values,
                             uint64_t n_fields, aec_gpu_grib_bitmap_plan_t *plan, uint64_t *work_offsets)
{
    BmShape s;
    if (!plan || bm_shape(t, elem, n_points, n_values, n_fields, &s) != RC_OK) return 0;
    *plan = s.plan;
    if (work_offsets && n_fields) memcpy(work_offsets, s.work_offsets, (size_t)n_fields * sizeof(uint64_t));
    return 1;
}

int aec_gpu_grib_bitmap_async(aec_gpu_ctx *ctx, int elem, const void *d_src, const uint64_t *src_offsets, const uint64_t *n_points,
                              double missing, uint64_t n_fields, void *d_bitmap, const uint64_t *bitmap_offsets, uint64_t *d_counts,
                              void *stream)
{
    if (!elem_ok(elem)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    uint64_t tiles;
    if (!ctx || !d_src || !src_offsets || !d_bitmap || !bitmap_offsets || !d_counts || !aligned(d_counts, 8) ||
        !tiles_of(n_points, n_fields, elem, &tiles) || !places_ok(d_src, src_offsets, nullptr, nullptr, false, n_fields, elem))
        return RC_CONF_ERROR;
    (void)hipGetLastError();
    hipStream_t st = static_cast<hipStream_t>(stream);
    BmOnDevice on;
    const int rc = bm_send(ctx, src_offsets, n_points, bitmap_offsets, nullptr, nullptr, nullptr, nullptr, nullptr, false, n_fields, tiles,
                           false, d_counts, st, &on);
    if (rc != RC_OK) return rc;
    const dim3 grid(tile_blocks(tiles)), block(kBmBlock);
    const uint8_t *src = static_cast<const uint8_t *>(d_src);
    uint8_t *bitmap = static_cast<uint8_t *>(d_bitmap);
    if (elem == AEC_GPU_GRIB_F32) hipLaunchKernelGGL(k_grib_bm_build<float>, grid, block, 0, st, on, tiles, src, bitmap, missing_bits_of<float>(missing), d_counts);
    else hipLaunchKernelGGL(k_grib_bm_build<double>, grid, block, 0, st, on, tiles, src, bitmap, missing_bits_of<double>(missing), d_counts);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

int aec_gpu_grib_quantise_bitmap_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src,
                                       const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D, int have_params,
                                       const aec_gpu_grib_field *params, uint64_t n_fields, void *d_work, aec_gpu_grib_field *d_fields,
                                       const void *d_bitmap, const uint64_t *bitmap_offsets, const uint64_t *n_points, void *stream)
{
    if (!template_ok(t, elem)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    BmShape s;
    const int rc = pack_args(t, elem, ctx, d_src, src_offsets, n_values, D, have_params, params, n_fields, d_work, d_fields, d_bitmap,
                             bitmap_offsets, n_points, &s);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return quantise_bm(ctx, t, elem, d_src, src_offsets, n_values, D, have_params != 0, params, n_fields, d_work, d_fields, d_bitmap,
                       bitmap_offsets, n_points, s, static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_pack_bitmap_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src,
                                   const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D, int have_params,
                                   const aec_gpu_grib_field *params, uint64_t n_fields, void *d_work, void *d_out, size_t out_cap,
                                   aec_gpu_batch_chunk *d_chunks, uint64_t *d_rsi_bit_offsets, aec_gpu_grib_field *d_fields,
                                   aec_gpu_enc_result *d_result, const void *d_bitmap, const uint64_t *bitmap_offsets,
                                   const uint64_t *n_points, void *stream)
{
    if (!template_ok(t, elem)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    if (!d_out || !d_chunks || !d_result || !aligned(d_out, 16) || (out_cap & 15u) || out_cap < 16) return RC_CONF_ERROR;
    BmShape s;
    int rc = pack_args(t, elem, ctx, d_src, src_offsets, n_values, D, have_params, params, n_fields, d_work, d_fields, d_bitmap,
                       bitmap_offsets, n_points, &s);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    rc = quantise_bm(ctx, t, elem, d_src, src_offsets, n_values, D, have_params != 0, params, n_fields, d_work, d_fields, d_bitmap,
                     bitmap_offsets, n_points, s, static_cast<hipStream_t>(stream));
    if (rc != RC_OK) return rc;
    return aec_gpu_encode_chunks_async(ctx, &s.plan.plan.coder, d_work, s.work_offsets, s.rooms, n_fields, d_out, out_cap, d_chunks,
                                       d_rsi_bit_offsets, d_result, stream);
}

int aec_gpu_grib_dequantise_bitmap_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_work,
                                         const uint64_t *n_values, const aec_gpu_grib_field *params, const uint64_t *dst_offsets,
                                         uint64_t n_fields, void *d_dst, const void *d_bitmap, const uint64_t *bitmap_offsets,
                                         const uint64_t *n_points, double missing, uint32_t *d_status, void *stream)
{
    if (!template_ok(t, elem)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    BmShape s;
    const int rc = unpack_args(t, elem, ctx, d_work, n_values, params, dst_offsets, n_fields, d_dst, d_bitmap, bitmap_offsets, n_points,
                               d_status, &s);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return expand_bm(ctx, t, elem, d_work, n_values, params, dst_offsets, n_fields, d_dst, d_bitmap, bitmap_offsets, n_points, missing,
                     d_status, s, static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_unpack_bitmap_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_in, size_t in_bytes,
                                     const uint64_t *in_offsets, const uint64_t *in_bytes_each, const uint64_t *n_values,
                                     const aec_gpu_grib_field *params, const uint64_t *dst_offsets, uint64_t n_fields,
                                     uint64_t *d_rsi_bit_offsets, int have_table, void *d_work, void *d_dst,
                                     aec_gpu_dec_result *d_results, aec_gpu_dec_result *d_result, const void *d_bitmap,
                                     const uint64_t *bitmap_offsets, const uint64_t *n_points, double missing, uint32_t *d_status,
                                     void *stream)
{
    if (!template_ok(t, elem)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    if (!d_in) return RC_CONF_ERROR;
    BmShape s;
    int rc = unpack_args(t, elem, ctx, d_work, n_values, params, dst_offsets, n_fields, d_dst, d_bitmap, bitmap_offsets, n_points,
                         d_status, &s);
    if (rc != RC_OK) return rc;
    const aec_gpu_params p = decoder_of(s.plan.plan.coder);
    rc = aec_gpu_decode_chunks_async(ctx, &p, d_in, in_bytes, in_offsets, in_bytes_each, s.work_offsets, s.rooms, n_fields,
                                     d_rsi_bit_offsets, have_table, d_work, d_results, d_result, stream);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return expand_bm(ctx, t, elem, d_work, n_values, params, dst_offsets, n_fields, d_dst, d_bitmap, bitmap_offsets, n_points, missing,
                     d_status, s, static_cast<hipStream_t>(stream));
}

}  // extern "C"
