// aec_gribcxw.hip -- WRITING GRIB2 complex packing (templates 5.2 / 5.3) on the device (include/aec_gpu_grib.h, COMPLEX PACKING,
// the writer's rule): the X rooms of the GRIB layer to section 7 streams with groups of a fixed length G, and the calls that
// compose that with the quantiser of aec_grib.hip, the chunk decoder of aec_gpu.hip and the bit unpacker of aec_gribbits.hip.
// The arithmetic is aec_gribcxw.h.
//
// Six launches, every one a plain grid; no workgroup waits for another, no atomics, no zero-fill of the output:
//   k_cxw_diff     orders 1 and 2 only.  A wavefront owns a value tile (1 KiB of its field's room), a lane the values of 16
//                  bytes of it; predecessors come through shuffles, the first lane of a tile loads its one or two; leaves the
//                  tile's smallest d
//   k_cxw_minsd    orders 1 and 2 only.  A wavefront a field: minsd from the tile minima
//   k_cxw_groups   the same lanes again: a group is G / per adjacent lanes, a segmented butterfly gives its extremes; leaves
//                  every group's reference, width and first bit inside the tile, and the tile's totals
//   k_cxw_field    a wavefront a field: scans the tile totals 64 at a time (the first bit of every tile), ref_bits, width_ref
//                  and width_bits; one lane writes the field's record and the extra descriptors
//   k_cxw_tables   a wavefront 256 groups, a lane four: references and widths as strings of ref_bits- and width_bits-bit
//                  integers (grib_bits_store: every byte whole and once)
//   k_cxw_values   lanes own OUTPUT bytes, 16 of the packed string each; the launch is sized by the bound and a wavefront
//                  behind the string's end leaves.  Binary search for the group at the lane's first bit, then a walk over
//                  values and groups that recomputes packed_j from the room
// The field of a wavefront is found by binary search over the descriptors (wave-uniform).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>

#include "../../include/aec_gpu_grib.h"
#include "aec_gribcxw.h"
#include "aec_kernels.h"

using namespace aec;

static_assert(sizeof(aec_gpu_grib_complex_write) == 8 && sizeof(aec_gpu_grib_cxw) == 56 && sizeof(CxwRecord) == 56 &&
                  sizeof(aec_gpu_grib_complex_field) == 44,
              "d_cxw");

namespace {

constexpr uint32_t kCxwBlock = 256, kCxwWaves = kCxwBlock / 64;

// the workspace of a batch behind its descriptors
struct CxwOnDevice {
    const CxwField *desc;
    CxwDyn *dyn;             // per field
    int64_t *minsd;          // per field
    int64_t *tmin;           // per value tile
    CxwTile *tile;           // per value tile
    uint32_t *gref, *gwid, *gbit;   // per group
};

// plain loads from a field's room and plain stores at byte offsets from the stream buffer's base (aec_gribcxw.h: Mem)
struct CxwMem {
    const uint8_t *room;
    uint8_t *out;
    __device__ __forceinline__ uint32_t ldx(int64_t o, uint32_t cont) const
    {
        return cont == 1u ? room[o] : cont == 2u ? *reinterpret_cast<const uint16_t *>(room + o) : *reinterpret_cast<const uint32_t *>(room + o);
    }
    __device__ __forceinline__ void ld128(int64_t o, uint32_t (&w)[4]) const
    {
        const uint4 v = *reinterpret_cast<const uint4 *>(room + o);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    }
    __device__ __forceinline__ void st8(int64_t o, uint8_t v) const { out[o] = v; }
    __device__ __forceinline__ void st32(int64_t o, uint32_t v) const { *reinterpret_cast<uint32_t *>(out + o) = v; }
};

__device__ __forceinline__ uint64_t wave_id() { return (uint64_t)blockIdx.x * kCxwWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ int64_t xor64(int64_t v, uint32_t o) { return (int64_t)__shfl_xor((long long)v, (int)o); }
__device__ __forceinline__ uint32_t xor32(uint32_t v, uint32_t o) { return (uint32_t)__shfl_xor((int)v, (int)o); }
__device__ __forceinline__ uint32_t up32(uint32_t v, uint32_t d) { return (uint32_t)__shfl_up((int)v, d); }

__device__ __forceinline__ CxwTile tile_xor(const CxwTile &a, uint32_t o)
{
    return CxwTile{(uint64_t)xor64((int64_t)a.bits, o), xor32(a.max_ref, o), xor32(a.min_w, o), xor32(a.max_w, o), 0u};
}

// smallest and largest d of the lane's counted values (the whole wavefront shuffles)
template <int CONT>
__device__ __forceinline__ void lane_ext(const CxwMem &m, const GribBitsLane &L, const CxwShape &P, uint32_t lane, int64_t *lo, int64_t *hi)
{
    constexpr uint32_t per = 16u / CONT;
    uint32_t x[per];
    cxw_lane_x<CONT>(m, L, P.nbits, x);
    uint32_t p1 = up32(x[per - 1u], 1), p2 = up32(x[per - 2u], 1);
    if (lane == 0u) {
        p1 = p2 = 0u;
        if (L.cnt) cxw_pred<CONT>(m, L.j0, P.order, P.nbits, &p1, &p2);
    }
    cxw_lane_ext<(int)per>(x, L.j0, L.cnt, P.order, p1, p2, lo, hi);
}

template <int CONT>
__global__ void __launch_bounds__(kCxwBlock)
k_cxw_diff(CxwOnDevice on, CxwShape P, uint64_t n, uint64_t vtiles, const uint8_t *__restrict__ work)
{
    const uint64_t w = wave_id();
    if (w >= vtiles) return;
    const uint32_t lane = threadIdx.x & 63u;
    const CxwField F = on.desc[cxw_field_of_tile(on.desc, n, 0, w)];
    const GribBitsLane L = grib_bits_lane(w - F.vtile0, lane, 16u / CONT, F.n, 0, 0);
    const CxwMem m{work + F.work_off, nullptr};
    int64_t lo, hi;
    lane_ext<CONT>(m, L, P, lane, &lo, &hi);
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) {
        const int64_t other = xor64(lo, o);
        lo = other < lo ? other : lo;
    }
    if (lane == 0u) on.tmin[w] = lo;
}

__global__ void __launch_bounds__(kCxwBlock)
k_cxw_minsd(CxwOnDevice on, uint64_t n)
{
    const uint64_t f = wave_id();
    if (f >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t0 = on.desc[f].vtile0, t1 = on.desc[f + 1].vtile0;
    int64_t lo = INT64_MAX;
    for (uint64_t t = t0 + lane; t < t1; t += 64u) {
        const int64_t v = on.tmin[t];
        lo = v < lo ? v : lo;
    }
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) {
        const int64_t other = xor64(lo, o);
        lo = other < lo ? other : lo;
    }
    if (lane == 0u) on.minsd[f] = lo == INT64_MAX ? 0 : lo;
}

template <int CONT>
__global__ void __launch_bounds__(kCxwBlock)
k_cxw_groups(CxwOnDevice on, CxwShape P, uint64_t n, uint64_t vtiles, const uint8_t *__restrict__ work)
{
    constexpr uint32_t per = 16u / CONT;
    const uint64_t w = wave_id();
    if (w >= vtiles) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t f = cxw_field_of_tile(on.desc, n, 0, w);
    const CxwField F = on.desc[f];
    const GribBitsLane L = grib_bits_lane(w - F.vtile0, lane, per, F.n, 0, 0);
    const CxwMem m{work + F.work_off, nullptr};
    const int64_t minsd = P.order ? on.minsd[f] : 0;
    int64_t lo, hi;
    lane_ext<CONT>(m, L, P, lane, &lo, &hi);
    const uint32_t lanes = P.G / per, gpt = 64u / lanes;               // lanes of a group, groups of a tile
    for (uint32_t o = 1; o < lanes; o <<= 1) {                         // (wave-uniform; xor below `lanes` stays inside the group)
        const int64_t a = xor64(lo, o), b = xor64(hi, o);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    const uint64_t g = (w - F.vtile0) * gpt + lane / lanes;
    const bool mine = lane % lanes == 0u && g < F.ng;
    const CxwGroup G = mine ? cxw_group(lo, hi, minsd, cxw_group_len(F, P.G, g)) : CxwGroup{0u, 0u, 0u};
    uint32_t incl = G.bits;
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t left = up32(incl, o);
        if (lane >= o) incl += left;
    }
    if (mine) {
        on.gref[F.group0 + g] = G.ref;
        on.gwid[F.group0 + g] = G.width;
        on.gbit[F.group0 + g] = incl - G.bits;
    }
    CxwTile a = mine ? cxw_tile_of(G) : cxw_tile_none();
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) a = cxw_tile_join(a, tile_xor(a, o));
    if (lane == 0u) on.tile[w] = a;
}

template <int CONT>
__global__ void __launch_bounds__(kCxwBlock)
k_cxw_field(CxwOnDevice on, CxwShape P, uint64_t n, const uint8_t *__restrict__ work, uint8_t *__restrict__ complex, CxwRecord *__restrict__ cxw)
{
    const uint64_t f = wave_id();
    if (f >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const CxwField F = on.desc[f];
    const uint64_t tiles = on.desc[f + 1].vtile0 - F.vtile0;
    uint64_t carry = 0;
    CxwTile all = cxw_tile_none();
    for (uint64_t base = 0; base < tiles; base += 64u) {
        const uint64_t t = base + lane;
        const CxwTile a = t < tiles ? on.tile[F.vtile0 + t] : cxw_tile_none();
        uint64_t incl = a.bits;
#pragma unroll
        for (uint32_t o = 1; o < 64u; o <<= 1) {
            const uint64_t left = (uint64_t)__shfl_up((unsigned long long)incl, o);
            if (lane >= o) incl += left;
        }
        if (t < tiles) on.tile[F.vtile0 + t].bits = carry + incl - a.bits;
        carry += (uint64_t)__shfl((unsigned long long)incl, 63);
        all = cxw_tile_join(all, a);
    }
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) all = cxw_tile_join(all, tile_xor(all, o));
    if (lane == 0u) {
        all.bits = carry;
        const CxwDyn Y = cxw_dyn(F, P, all, P.order ? on.minsd[f] : 0);
        on.dyn[f] = Y;
        cxw[f] = cxw_record(F, P, Y);
        const CxwMem m{work + F.work_off, complex};
        cxw_head_bytes<CONT>(m, F, P, Y);
    }
}

__global__ void __launch_bounds__(kCxwBlock)
k_cxw_tables(CxwOnDevice on, CxwShape P, uint64_t n, uint64_t ttiles, uint8_t *__restrict__ complex, uint32_t mis)
{
    const uint64_t w = wave_id();
    if (w >= ttiles) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t f = cxw_field_of_tile(on.desc, n, 1, w);
    const CxwField F = on.desc[f];
    const CxwDyn Y = on.dyn[f];
    const uint64_t g0 = ((w - F.ttile0) * 64u + lane) * kCxwTableLane;
    const CxwMem m{nullptr, complex};
    uint64_t at = F.off + cxw_head(P.nbits, P.order);
#pragma unroll
    for (int which = 0; which < 2; which++) {
        const uint32_t bits = which ? Y.width_bits : Y.ref_bits;
        if (bits) {                                                    // (wave-uniform)
            uint64_t hi, lo;
            uint32_t cnt;
            cxw_table_string((which ? on.gwid : on.gref) + F.group0, which ? Y.width_ref : 0u, g0, F.ng, bits, &hi, &lo, &cnt);
            const uint32_t follower = (uint32_t)__shfl_down((int)grib_bits_head(hi), 1);
            const uint64_t p0 = at * 8u + g0 * bits;
            grib_bits_store(m, hi, lo, p0, p0 + (uint64_t)cnt * bits, lane < 63u ? follower : 0u, mis);
        }
        at += cxw_table_bytes(F.ng, bits);
    }
}

template <int CONT>
__global__ void __launch_bounds__(kCxwBlock)
k_cxw_values(CxwOnDevice on, CxwShape P, uint64_t n, uint64_t otiles, const uint8_t *__restrict__ work, uint8_t *__restrict__ complex, uint32_t mis)
{
    const uint64_t w = wave_id();
    if (w >= otiles) return;
    const uint64_t f = cxw_field_of_tile(on.desc, n, 2, w);
    const CxwField F = on.desc[f];
    const CxwDyn Y = on.dyn[f];
    if ((w - F.otile0) * (8u * kCxwOutTile) >= Y.bits) return;       // (wave-uniform: behind the string's end)
    const uint64_t lane_in_field = (w - F.otile0) * 64u + (threadIdx.x & 63u);
    const CxwMem m{work + F.work_off, complex};
    const CxwTables T{on.tile + F.vtile0, on.gref + F.group0, on.gwid + F.group0, on.gbit + F.group0};
    uint64_t hi, lo;
    const uint32_t nb = cxw_lane_string<CONT>(m, F, P, Y, T, lane_in_field, &hi, &lo);
    const uint64_t p0 = 8u * (F.off + Y.data_byte + lane_in_field * kCxwOutLane);
    grib_bits_store(m, hi, lo, p0, p0 + 8u * nb, 0u, mis);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
constexpr uint64_t kCxwMaxTiles = 1ull << 25, kCxwMaxGroups = 0x7FFFFFFFull;

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
uint32_t wave_blocks(uint64_t waves) { return (uint32_t)((waves + kCxwWaves - 1) / kCxwWaves); }

bool template_ok(const aec_gpu_grib_template *t)
{
    aec_gpu_grib_layout_t L;
    return aec_gpu_grib_layout(t, 0, &L) == RC_OK;
}

bool write_ok(const aec_gpu_grib_template *t, const aec_gpu_grib_complex_write *w)
{
    if (!w || w->order > 2u || t->nbits + w->order > 32u) return false;
    return w->group_length == 16u || w->group_length == 32u || w->group_length == 64u || w->group_length == 128u || w->group_length == 256u;
}

// host arithmetic of a batch: the plan of aec_gpu_grib_plan, the rooms and their places, the bounds, the tiles
struct CxwBatch {
    aec_gpu_grib_complex_write_plan_t plan;
    std::unique_ptr<uint64_t[]> own;
    uint64_t *rooms = nullptr, *work_offsets = nullptr, *bounds = nullptr;
    uint64_t groups = 0;
    size_t desc_bytes = 0, dyn_bytes = 0, f8_bytes = 0, v8_bytes = 0, tile_bytes = 0, g4_bytes = 0;
    size_t extent() const { return desc_bytes + dyn_bytes + f8_bytes + v8_bytes + tile_bytes + 3 * g4_bytes; }
};

int cxw_batch(const aec_gpu_grib_template *t, const aec_gpu_grib_complex_write *w, int elem, const uint64_t *n_values, uint64_t n, CxwBatch *s)
{
    if ((n && !n_values) || n > 0x7FFFFFFFull) return RC_CONF_ERROR;
    s->own.reset(new (std::nothrow) uint64_t[3 * n + 1]);
    if (!s->own) return RC_MEM_ERROR;
    s->rooms = s->own.get();
    s->work_offsets = s->rooms + n;
    s->bounds = s->work_offsets + n;
    if (!aec_gpu_grib_plan(t, elem, n_values, n, &s->plan.plan, s->work_offsets) || !write_ok(t, w)) return RC_CONF_ERROR;
    const uint32_t container = grib_container(t->nbits);
    uint64_t vtiles = 0, ttiles = 0, otiles = 0, groups = 0, bound = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t ng = cxw_groups(n_values[i], w->group_length);
        s->rooms[i] = grib_room(n_values[i], t->block_size, container);
        s->bounds[i] = cxw_bound(n_values[i], t->nbits, w->order, w->group_length);
        vtiles += grib_room_waves(s->rooms[i]);                              // (aec_gpu_grib_plan holds them to 2^25)
        ttiles += (ng + kCxwTableTile - 1) / kCxwTableTile;
        otiles += (cxw_string_bound(n_values[i], t->nbits, w->order) + kCxwOutTile - 1) / kCxwOutTile;
        groups += ng;
        bound += s->bounds[i];
        if (otiles > kCxwMaxTiles || groups > kCxwMaxGroups) return RC_CONF_ERROR;
    }
    s->groups = groups;
    s->plan.complex_bound = (size_t)bound;
    s->plan.tile_values = kGribWaveRoom / container;
    s->plan.value_tiles = vtiles;
    s->plan.group_tiles = ttiles;
    s->plan.out_tiles = otiles;
    s->desc_bytes = up256((size_t)(n + 1) * sizeof(CxwField));
    s->dyn_bytes = up256((size_t)(n ? n : 1) * sizeof(CxwDyn));
    s->f8_bytes = up256((size_t)(n ? n : 1) * 8);
    s->v8_bytes = up256((size_t)(vtiles ? vtiles : 1) * 8);
    s->tile_bytes = up256((size_t)(vtiles ? vtiles : 1) * sizeof(CxwTile));
    s->g4_bytes = up256((size_t)(groups ? groups : 1) * 4);
    s->plan.plan.workspace_bytes += s->extent();
    return RC_OK;
}

// the checks of every call that writes streams; RC_OK with the batch filled
int cxw_args(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const aec_gpu_grib_complex_write *w, int elem, const uint64_t *n_values, uint64_t n,
             const void *d_work, void *d_complex, size_t complex_cap, const uint64_t *complex_offsets, aec_gpu_grib_cxw *d_cxw, CxwBatch *s)
{
    if (!ctx || !n_values || !d_work || !d_complex || !complex_offsets || !d_cxw || !aligned(d_work, 16) || !aligned(d_cxw, 8)) return RC_CONF_ERROR;
    const int rc = cxw_batch(t, w, elem, n_values, n, s);
    if (rc != RC_OK) return rc;
    // every range inside [0, complex_cap), no two of them overlapping
    std::unique_ptr<uint64_t[]> order(new (std::nothrow) uint64_t[n]);
    if (!order) return RC_MEM_ERROR;
    for (uint64_t i = 0; i < n; i++) {
        order[i] = i;
        if (complex_offsets[i] > complex_cap || s->bounds[i] > complex_cap - complex_offsets[i]) return RC_CONF_ERROR;
    }
    std::sort(order.get(), order.get() + n, [&](uint64_t a, uint64_t b) { return complex_offsets[a] < complex_offsets[b]; });
    for (uint64_t k = 1; k < n; k++)
        if (complex_offsets[order[k - 1]] + s->bounds[order[k - 1]] > complex_offsets[order[k]]) return RC_CONF_ERROR;
    return RC_OK;
}

int cxw_write(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const aec_gpu_grib_complex_write *w, const CxwBatch &s, const uint64_t *n_values,
              uint64_t n, const void *d_work, void *d_complex, const uint64_t *complex_offsets, aec_gpu_grib_cxw *d_cxw, hipStream_t st)
{
    const size_t h_need = (size_t)(n + 1) * sizeof(CxwField);
    void *h = nullptr;
    void *stage = ctx_sz_stage(ctx, h_need, &h);
    if (!stage) return RC_MEM_ERROR;
    CxwField *d = static_cast<CxwField *>(h);
    uint64_t vt = 0, tt = 0, ot = 0, g0 = 0;
    for (uint64_t i = 0; i <= n; i++) {
        CxwField &f = d[i];
        f = CxwField{};
        f.vtile0 = vt;
        f.ttile0 = tt;
        f.otile0 = ot;
        f.group0 = g0;
        if (i == n) break;
        f.off = complex_offsets[i];
        f.n = n_values[i];
        f.work_off = s.work_offsets[i];
        f.room = s.rooms[i];
        f.ng = (uint32_t)cxw_groups(f.n, w->group_length);
        vt += grib_room_waves(f.room);
        tt += ((uint64_t)f.ng + kCxwTableTile - 1) / kCxwTableTile;
        ot += (cxw_string_bound(f.n, t->nbits, w->order) + kCxwOutTile - 1) / kCxwOutTile;
        g0 += f.ng;
    }
    uint8_t *cd = ctx_sz_send(ctx, stage, h_need, s.extent(), st);
    if (!cd) return RC_MEM_ERROR;
    CxwOnDevice on;
    on.desc = reinterpret_cast<const CxwField *>(cd);
    cd += s.desc_bytes;
    on.dyn = reinterpret_cast<CxwDyn *>(cd);
    cd += s.dyn_bytes;
    on.minsd = reinterpret_cast<int64_t *>(cd);
    cd += s.f8_bytes;
    on.tmin = reinterpret_cast<int64_t *>(cd);
    cd += s.v8_bytes;
    on.tile = reinterpret_cast<CxwTile *>(cd);
    cd += s.tile_bytes;
    on.gref = reinterpret_cast<uint32_t *>(cd);
    cd += s.g4_bytes;
    on.gwid = reinterpret_cast<uint32_t *>(cd);
    cd += s.g4_bytes;
    on.gbit = reinterpret_cast<uint32_t *>(cd);
    const uint8_t *work = static_cast<const uint8_t *>(d_work);
    uint8_t *complex = static_cast<uint8_t *>(d_complex);
    CxwRecord *rec = reinterpret_cast<CxwRecord *>(d_cxw);
    const CxwShape P{w->order, w->group_length, t->nbits, cxw_extra(t->nbits, w->order)};
    const dim3 block(kCxwBlock), by_value(wave_blocks(vt)), by_field(wave_blocks(n)), by_table(wave_blocks(tt)), by_out(wave_blocks(ot));
    const uint32_t container = grib_container(t->nbits), mis = (uint32_t)(reinterpret_cast<uintptr_t>(d_complex) & 3u);
#define CXW_W(C)                                                                                              \
    do {                                                                                                      \
        if (P.order) {                                                                                        \
            hipLaunchKernelGGL((k_cxw_diff<C>), by_value, block, 0, st, on, P, n, vt, work);                  \
            hipLaunchKernelGGL(k_cxw_minsd, by_field, block, 0, st, on, n);                                   \
        }                                                                                                     \
        hipLaunchKernelGGL((k_cxw_groups<C>), by_value, block, 0, st, on, P, n, vt, work);                    \
        hipLaunchKernelGGL((k_cxw_field<C>), by_field, block, 0, st, on, P, n, work, complex, rec);           \
        hipLaunchKernelGGL(k_cxw_tables, by_table, block, 0, st, on, P, n, tt, complex, mis);                 \
        hipLaunchKernelGGL((k_cxw_values<C>), by_out, block, 0, st, on, P, n, ot, work, complex, mis);        \
    } while (0)
    if (container == 1) CXW_W(1);
    else if (container == 2) CXW_W(2);
    else CXW_W(4);
#undef CXW_W
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

aec_gpu_params decoder_of(const aec_gpu_params &p) { return aec_gpu_params{p.bits_per_sample, p.block_size, p.rsi, p.flags & ~(uint32_t)F_NOT_ENFORCE}; }

}  // namespace

extern "C" {

int aec_gpu_grib_complex_write_plan(const aec_gpu_grib_template *t, const aec_gpu_grib_complex_write *w, int elem, const uint64_t *n_values,
                                    uint64_t n_fields, aec_gpu_grib_complex_write_plan_t *plan, uint64_t *work_offsets, uint64_t *complex_offsets)
{
    CxwBatch s;
    if (!plan || !t || cxw_batch(t, w, elem, n_values, n_fields, &s) != RC_OK) return 0;
    *plan = s.plan;
    if (work_offsets && n_fields) memcpy(work_offsets, s.work_offsets, (size_t)n_fields * sizeof(uint64_t));
    if (complex_offsets) {
        uint64_t at = 0;
        for (uint64_t i = 0; i < n_fields; i++) {
            complex_offsets[i] = at;
            at += s.bounds[i];
        }
    }
    return 1;
}

int aec_gpu_grib_complex_write_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const aec_gpu_grib_complex_write *w,
                                     const uint64_t *n_values, uint64_t n_fields, const void *d_work, void *d_complex, size_t complex_cap,
                                     const uint64_t *complex_offsets, aec_gpu_grib_cxw *d_cxw, void *stream)
{
    if (!template_ok(t) || !write_ok(t, w)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    CxwBatch s;
    const int rc = cxw_args(ctx, t, w, AEC_GPU_GRIB_F32, n_values, n_fields, d_work, d_complex, complex_cap, complex_offsets, d_cxw, &s);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return cxw_write(ctx, t, w, s, n_values, n_fields, d_work, d_complex, complex_offsets, d_cxw, static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_complex_pack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const aec_gpu_grib_complex_write *w, int elem,
                                    const void *d_src, const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D, int have_params,
                                    const aec_gpu_grib_field *params, uint64_t n_fields, void *d_work, aec_gpu_grib_field *d_fields,
                                    void *d_complex, size_t complex_cap, const uint64_t *complex_offsets, aec_gpu_grib_cxw *d_cxw, void *stream)
{
    if (!template_ok(t) || !write_ok(t, w) || (elem != AEC_GPU_GRIB_F32 && elem != AEC_GPU_GRIB_F64)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    CxwBatch s;
    int rc = cxw_args(ctx, t, w, elem, n_values, n_fields, d_work, d_complex, complex_cap, complex_offsets, d_cxw, &s);
    if (rc != RC_OK) return rc;
    rc = aec_gpu_grib_quantise_async(ctx, t, elem, d_src, src_offsets, n_values, D, have_params, params, n_fields, d_work, d_fields, stream);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return cxw_write(ctx, t, w, s, n_values, n_fields, d_work, d_complex, complex_offsets, d_cxw, static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_ccsds_to_complex_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const aec_gpu_grib_complex_write *w, const void *d_in,
                                        size_t in_bytes, const uint64_t *in_offsets, const uint64_t *in_bytes_each, const uint64_t *n_values,
                                        uint64_t n_fields, uint64_t *d_rsi_bit_offsets, int have_table, void *d_work,
                                        aec_gpu_dec_result *d_results, aec_gpu_dec_result *d_result, void *d_complex, size_t complex_cap,
                                        const uint64_t *complex_offsets, aec_gpu_grib_cxw *d_cxw, void *stream)
{
    if (!template_ok(t) || !write_ok(t, w)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    if (!d_in) return RC_CONF_ERROR;
    CxwBatch s;
    int rc = cxw_args(ctx, t, w, AEC_GPU_GRIB_F32, n_values, n_fields, d_work, d_complex, complex_cap, complex_offsets, d_cxw, &s);
    if (rc != RC_OK) return rc;
    const aec_gpu_params p = decoder_of(s.plan.plan.coder);
    rc = aec_gpu_decode_chunks_async(ctx, &p, d_in, in_bytes, in_offsets, in_bytes_each, s.work_offsets, s.rooms, n_fields, d_rsi_bit_offsets,
                                     have_table, d_work, d_results, d_result, stream);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return cxw_write(ctx, t, w, s, n_values, n_fields, d_work, d_complex, complex_offsets, d_cxw, static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_simple_to_complex_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const aec_gpu_grib_complex_write *w,
                                         const void *d_simple, size_t simple_bytes, const uint64_t *simple_offsets,
                                         const uint64_t *simple_bytes_each, const uint64_t *n_values, uint64_t n_fields, void *d_work,
                                         void *d_complex, size_t complex_cap, const uint64_t *complex_offsets, aec_gpu_grib_cxw *d_cxw,
                                         void *stream)
{
    if (!template_ok(t) || !write_ok(t, w)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    CxwBatch s;
    int rc = cxw_args(ctx, t, w, AEC_GPU_GRIB_F32, n_values, n_fields, d_work, d_complex, complex_cap, complex_offsets, d_cxw, &s);
    if (rc != RC_OK) return rc;
    rc = aec_gpu_grib_bits_unpack_async(ctx, t, n_values, n_fields, d_simple, simple_bytes, simple_offsets, simple_bytes_each, d_work, stream);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return cxw_write(ctx, t, w, s, n_values, n_fields, d_work, d_complex, complex_offsets, d_cxw, static_cast<hipStream_t>(stream));
}

}  // extern "C"
