// aec_gribcx.hip -- GRIB2 complex packing (templates 5.2 / 5.3, what every NCEP product is written in) on the device
// (include/aec_gpu_grib.h, COMPLEX PACKING): section 7 streams to the X rooms of the GRIB layer, and the calls that compose
// that with the dequantiser of aec_grib.hip and the chunk coder of aec_gpu.hip.  The arithmetic is aec_gribcx.h.
//
// Seven launches, every one a plain grid; no workgroup waits for another (reduce, scan the aggregates, apply):
//   k_cx_groups        a wavefront a tile of 64 groups, a lane a group: reference, width, length (saturated); the tile's
//                      exclusive saturating scan of (len, len * width) and its total
//   k_cx_group_scan    a wavefront a field: scans its tile totals, 64 at a time; the field's totals decide MALFORMED; lane 0
//                      reads the extra descriptors once
//   k_cx_group_apply   adds the tile's base: every group's first value and first bit
//   k_cx_values        orders 1 and 2 only.  A wavefront owns 1 KiB of its field's room (a value tile), a lane the values
//                      of 16 bytes of it: binary search for the group of its first value, walk, extract; leaves the tile's
//                      aggregate (Y, X at its end from a zero state)
//   k_cx_value_scan    a wavefront a field: the state in front of every value tile, and X of value n - 1
//   k_cx_apply         every order.  Extracts again (the stream is the small side; s_j is kept nowhere), integrates inside the
//                      tile from the tile's carry, stores the lane's 16 bytes once -- the last block padded with X of value
//                      n - 1 -- and leaves the tile's minimum and maximum
//   k_cx_records       a wavefront a field: x_min, x_max and status from the tile extremes.  No atomics anywhere.
// The field of a wavefront is found by binary search over the descriptors (wave-uniform).
#include <hip/hip_runtime.h>

#include <memory>
#include <new>

#include "../../include/aec_gpu_grib.h"
#include "aec_gribcx.h"
#include "aec_kernels.h"

using namespace aec;

static_assert(sizeof(aec_gpu_grib_cx) == 24 && AEC_GPU_GRIB_CX_RANGE == kCxRange && AEC_GPU_GRIB_CX_MALFORMED == kCxMalformed, "d_cx");

namespace {

constexpr uint32_t kCxBlock = 256, kCxWaves = kCxBlock / 64;

// the workspace of a batch behind its descriptors
struct CxOnDevice {
    const CxField *desc;
    CxDyn *dyn;              // per field
    CxSum *gagg;             // per group tile: its total, then its base
    uint64_t *gval, *gbit;   // per group
    uint32_t *gref, *gwid;
    CxAgg *vagg;             // per value tile: its aggregate, then the state in front of it
    int64_t *vmin, *vmax;    // per value tile
};

// plain byte loads from a stream's first byte (aec_gribcx.h: Mem)
struct CxMem {
    const uint8_t *p;
    __device__ __forceinline__ uint32_t ld8(int64_t o) const { return p[o]; }
};

__device__ __forceinline__ uint64_t wave_id() { return (uint64_t)blockIdx.x * kCxWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ uint64_t up64(uint64_t v, uint32_t d) { return (uint64_t)__shfl_up((unsigned long long)v, d); }
__device__ __forceinline__ uint64_t from64(uint64_t v, uint32_t lane) { return (uint64_t)__shfl((unsigned long long)v, (int)lane); }

// inclusive scans over the 64 lanes; *excl: what lies in front of the lane
__device__ __forceinline__ CxSum scan_sum(CxSum v, uint32_t lane, uint64_t capv, uint64_t capb, CxSum *excl)
{
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const CxSum left{up64(v.v, o), up64(v.b, o)};
        if (lane >= o) v = cx_sum_add(left, v, capv, capb);
    }
    const CxSum e{up64(v.v, 1), up64(v.b, 1)};
    *excl = lane ? e : CxSum{0, 0};
    return v;
}

// (lanes hold runs of L values each: after the step of o the lane's aggregate covers o lanes)
__device__ __forceinline__ CxAgg scan_agg(CxAgg v, uint32_t lane, uint64_t L, CxAgg *excl)
{
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const CxAgg left{up64(v.s, o), up64(v.w, o)};
        if (lane >= o) v = cx_combine(left, v, o * L);
    }
    const CxAgg e{up64(v.s, 1), up64(v.w, 1)};
    *excl = lane ? e : CxAgg{0, 0};
    return v;
}

__global__ void __launch_bounds__(kCxBlock)
k_cx_groups(CxOnDevice on, uint64_t n, uint64_t gtiles, const uint8_t *__restrict__ complex)
{
    const uint64_t w = wave_id();
    if (w >= gtiles) return;
    const uint32_t lane = threadIdx.x & 63u;
    const CxField F = on.desc[cx_field_of_tile(on.desc, n, 0, w)];
    const uint64_t g = (w - F.gtile0) * kCxGroupTile + lane;
    CxMem m{complex + F.off};
    CxGroup G{0, 0, CxSum{0, 0}};
    if (g < F.ng) G = cx_group(m, F, g);
    CxSum excl;
    const CxSum incl = scan_sum(G.s, lane, cx_cap_values(F), cx_cap_bits(F), &excl);
    if (g < F.ng) {
        on.gval[F.group0 + g] = excl.v;
        on.gbit[F.group0 + g] = excl.b;
        on.gref[F.group0 + g] = G.ref;
        on.gwid[F.group0 + g] = G.width;
    }
    if (lane == 63u) on.gagg[w] = incl;
}

__global__ void __launch_bounds__(kCxBlock)
k_cx_group_scan(CxOnDevice on, uint64_t n, const uint8_t *__restrict__ complex)
{
    const uint64_t f = wave_id();
    if (f >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const CxField F = on.desc[f];
    const uint64_t tiles = on.desc[f + 1].gtile0 - F.gtile0, capv = cx_cap_values(F), capb = cx_cap_bits(F);
    CxSum carry{0, 0};
    for (uint64_t base = 0; base < tiles; base += 64u) {
        const uint64_t t = base + lane;
        CxSum excl;
        const CxSum incl = scan_sum(t < tiles ? on.gagg[F.gtile0 + t] : CxSum{0, 0}, lane, capv, capb, &excl);
        if (t < tiles) on.gagg[F.gtile0 + t] = cx_sum_add(carry, excl, capv, capb);
        carry = cx_sum_add(carry, CxSum{from64(incl.v, 63), from64(incl.b, 63)}, capv, capb);
    }
    if (lane == 0u) {
        CxMem m{complex + F.off};
        on.dyn[f] = cx_dyn(m, F, carry);
    }
}

__global__ void __launch_bounds__(kCxBlock)
k_cx_group_apply(CxOnDevice on, uint64_t n, uint64_t gtiles)
{
    const uint64_t w = wave_id();
    if (w >= gtiles) return;
    const CxField F = on.desc[cx_field_of_tile(on.desc, n, 0, w)];
    const uint64_t g = (w - F.gtile0) * kCxGroupTile + (threadIdx.x & 63u);
    if (g >= F.ng) return;
    const CxSum at = cx_sum_add(on.gagg[w], CxSum{on.gval[F.group0 + g], on.gbit[F.group0 + g]}, cx_cap_values(F), cx_cap_bits(F));
    on.gval[F.group0 + g] = at.v;
    on.gbit[F.group0 + g] = at.b;
}

__device__ __forceinline__ CxTables tables_of(const CxOnDevice &on, const CxField &F)
{
    return CxTables{on.gval + F.group0, on.gbit + F.group0, on.gref + F.group0, on.gwid + F.group0};
}

template <int CONT>
__global__ void __launch_bounds__(kCxBlock)
k_cx_values(CxOnDevice on, uint64_t n, uint64_t vtiles, const uint8_t *__restrict__ complex)
{
    constexpr uint32_t per = 16u / CONT;
    const uint64_t w = wave_id();
    if (w >= vtiles) return;
    const uint64_t f = cx_field_of_tile(on.desc, n, 1, w);
    const CxField F = on.desc[f];
    if (F.order == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const CxDyn Y = on.dyn[f];
    const GribBitsLane L = grib_bits_lane(w - F.vtile0, lane, per, F.n, 0, 0);
    CxMem m{complex + F.off};
    uint64_t d[per];
    cx_lane_values<(int)per>(m, F, Y, tables_of(on, F), L.j0, L.cnt, d);
    CxAgg excl;
    const CxAgg incl = scan_agg(cx_lane_agg<(int)per>(d), lane, per, &excl);
    if (lane == 63u) on.vagg[w] = incl;
}

template <int CONT>
__global__ void __launch_bounds__(kCxBlock)
k_cx_value_scan(CxOnDevice on, uint64_t n)
{
    constexpr uint64_t T = kGribWaveRoom / CONT;
    const uint64_t f = wave_id();
    if (f >= n) return;
    const CxField F = on.desc[f];
    if (F.order == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t tiles = on.desc[f + 1].vtile0 - F.vtile0;
    CxAgg carry{0, 0};
    uint64_t covered = 0;
    for (uint64_t base = 0; base < tiles; base += 64u) {
        const uint64_t t = base + lane;
        CxAgg excl;
        const CxAgg incl = scan_agg(t < tiles ? on.vagg[F.vtile0 + t] : CxAgg{0, 0}, lane, T, &excl);
        if (t < tiles) on.vagg[F.vtile0 + t] = cx_combine(carry, excl, lane * T);
        carry = cx_combine(carry, CxAgg{from64(incl.s, 63), from64(incl.w, 63)}, 64u * T);
        covered += 64u * T;
    }
    if (lane == 0u) on.dyn[f].xlast = cx_last_x(carry, F.order, covered, F.n);
}

template <int CONT>
__global__ void __launch_bounds__(kCxBlock)
k_cx_apply(CxOnDevice on, uint64_t n, uint64_t vtiles, uint32_t nbits, const uint8_t *__restrict__ complex, uint8_t *__restrict__ work)
{
    constexpr uint32_t per = 16u / CONT;
    const uint64_t w = wave_id();
    if (w >= vtiles) return;
    const uint64_t f = cx_field_of_tile(on.desc, n, 1, w);
    const CxField F = on.desc[f];
    const uint32_t lane = threadIdx.x & 63u;
    const CxDyn Y = on.dyn[f];
    const uint64_t in_field = w - F.vtile0, at = (in_field * 64u + lane) * 16u;
    const GribBitsLane L = grib_bits_lane(in_field, lane, per, F.n, 0, 0);
    const CxTables T = tables_of(on, F);
    CxMem m{complex + F.off};
    uint64_t d[per];
    cx_lane_values<(int)per>(m, F, Y, T, L.j0, L.cnt, d);
    CxAgg in{0, 0};
    if (F.order) {                                    // (wave-uniform)
        CxAgg excl;
        scan_agg(cx_lane_agg<(int)per>(d), lane, per, &excl);
        in = cx_combine(on.vagg[w], excl, (uint64_t)lane * per);
    }
    cx_lane_x<(int)per>(d, F.order, in);
    uint64_t last = Y.xlast;
    if (F.order == 0u && L.cnt < per && at < F.room) {          // value n - 1 by its own place in the stream
        uint64_t one[1];
        cx_lane_values<1>(m, F, Y, T, F.n - 1u, 1u, one);
        last = one[0];
    }
    CxExt e = cx_ext_none();
    uint32_t words[4];
    cx_lane_words<CONT>(d, L.cnt, last, nbits, &e, words);
    if (at < F.room) {
        uint8_t *out = work + F.work_off + at;
        if (at + 16u <= F.room) {
            *reinterpret_cast<uint4 *>(out) = make_uint4(words[0], words[1], words[2], words[3]);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 16; i++)
                if (at + i < F.room) out[i] = (uint8_t)(words[i >> 2] >> (8 * (i & 3)));
        }
    }
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1)
        e = cx_ext_join(e, CxExt{(int64_t)__shfl_xor((long long)e.lo, (int)o), (int64_t)__shfl_xor((long long)e.hi, (int)o)});
    if (lane == 0u) {
        on.vmin[w] = e.lo;
        on.vmax[w] = e.hi;
    }
}

__global__ void __launch_bounds__(kCxBlock)
k_cx_records(CxOnDevice on, uint64_t n, uint32_t nbits, aec_gpu_grib_cx *__restrict__ cx)
{
    const uint64_t f = wave_id();
    if (f >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t0 = on.desc[f].vtile0, t1 = on.desc[f + 1].vtile0;
    CxExt e = cx_ext_none();
    for (uint64_t t = t0 + lane; t < t1; t += 64u) e = cx_ext_join(e, CxExt{on.vmin[t], on.vmax[t]});
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1)
        e = cx_ext_join(e, CxExt{(int64_t)__shfl_xor((long long)e.lo, (int)o), (int64_t)__shfl_xor((long long)e.hi, (int)o)});
    if (lane == 0u) cx[f] = aec_gpu_grib_cx{e.lo, e.hi, cx_status(on.dyn[f], e, nbits), 0u};
}

// ---- host side ------------------------------------------------------------------------------------------------------------
constexpr uint64_t kCxMaxTiles = 1ull << 25, kCxMaxGroups = 0x7FFFFFFFull;

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
uint32_t wave_blocks(uint64_t waves) { return (uint32_t)((waves + kCxWaves - 1) / kCxWaves); }

bool template_ok(const aec_gpu_grib_template *t)
{
    aec_gpu_grib_layout_t L;
    return aec_gpu_grib_layout(t, 0, &L) == RC_OK;
}

// bytes of a stream in front of its packed values: the extra descriptors and the three tables
uint64_t head_bytes(const aec_gpu_grib_complex_field &c)
{
    return (c.order ? (uint64_t)(c.order + 1u) * c.extra_octets : 0u) + cx_table_bytes(c.n_groups, c.ref_bits) +
           cx_table_bytes(c.n_groups, c.width_bits) + cx_table_bytes(c.n_groups, c.length_bits);
}

// host arithmetic of a batch: the plan of aec_gpu_grib_plan, the rooms and their places, the tiles
struct CxShape {
    aec_gpu_grib_complex_plan_t plan;
    std::unique_ptr<uint64_t[]> own;
    uint64_t *rooms = nullptr, *work_offsets = nullptr;
    uint64_t groups = 0;
    size_t desc_bytes = 0, dyn_bytes = 0, gagg_bytes = 0, g8_bytes = 0, g4_bytes = 0, vagg_bytes = 0, v8_bytes = 0;
    size_t extent() const { return desc_bytes + dyn_bytes + gagg_bytes + 2 * g8_bytes + 2 * g4_bytes + vagg_bytes + 2 * v8_bytes; }
};

int cx_shape(const aec_gpu_grib_template *t, int elem, const uint64_t *n_values, const aec_gpu_grib_complex_field *fields, uint64_t n,
             CxShape *s)
{
    if ((n && (!n_values || !fields)) || n > 0x7FFFFFFFull) return RC_CONF_ERROR;
    s->own.reset(new (std::nothrow) uint64_t[2 * n + 1]);
    if (!s->own) return RC_MEM_ERROR;
    s->rooms = s->own.get();
    s->work_offsets = s->rooms + n;
    if (!aec_gpu_grib_plan(t, elem, n_values, n, &s->plan.plan, s->work_offsets)) return RC_CONF_ERROR;
    const uint32_t container = grib_container(t->nbits);
    uint64_t vtiles = 0, gtiles = 0, groups = 0;
    for (uint64_t i = 0; i < n; i++) {
        const aec_gpu_grib_complex_field &c = fields[i];
        if (c.missing != 0 || c.order > 2 || (c.order && c.extra_octets > 8) || c.ref_bits > 32 || c.width_bits > 32 || c.length_bits > 32 ||
            c.n_groups == 0 || c.n_groups > n_values[i])
            return RC_CONF_ERROR;
        s->rooms[i] = grib_room(n_values[i], t->block_size, container);
        vtiles += grib_room_waves(s->rooms[i]);                                  // (aec_gpu_grib_plan holds them to 2^25)
        gtiles += (c.n_groups + kCxGroupTile - 1) / kCxGroupTile;
        groups += c.n_groups;
        if (gtiles > kCxMaxTiles || groups > kCxMaxGroups) return RC_CONF_ERROR;
    }
    s->groups = groups;
    s->plan.tile_values = kGribWaveRoom / container;
    s->plan.value_tiles = vtiles;
    s->plan.group_tiles = gtiles;
    s->desc_bytes = up256((size_t)(n + 1) * sizeof(CxField));
    s->dyn_bytes = up256((size_t)(n ? n : 1) * sizeof(CxDyn));
    s->gagg_bytes = up256((size_t)(gtiles ? gtiles : 1) * sizeof(CxSum));
    s->g8_bytes = up256((size_t)(groups ? groups : 1) * 8);
    s->g4_bytes = up256((size_t)(groups ? groups : 1) * 4);
    s->vagg_bytes = up256((size_t)(vtiles ? vtiles : 1) * sizeof(CxAgg));
    s->v8_bytes = up256((size_t)(vtiles ? vtiles : 1) * 8);
    s->plan.plan.workspace_bytes += s->extent();
    return RC_OK;
}

// the checks of the calls that read streams; RC_OK with the shape filled
int cx_args(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const aec_gpu_grib_complex_field *fields, const uint64_t *n_values,
            uint64_t n, const void *d_complex, size_t complex_bytes, const uint64_t *complex_offsets, const uint64_t *complex_bytes_each,
            void *d_work, aec_gpu_grib_cx *d_cx, CxShape *s)
{
    if (!ctx || !n_values || !fields || !d_complex || !complex_offsets || !complex_bytes_each || !d_work || !d_cx || !aligned(d_work, 16) ||
        !aligned(d_cx, 8))
        return RC_CONF_ERROR;
    const int rc = cx_shape(t, elem, n_values, fields, n, s);
    if (rc != RC_OK) return rc;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t each = complex_bytes_each[i];
        if (each >= kCxMaxBytes || each < head_bytes(fields[i]) || complex_offsets[i] > complex_bytes || each > complex_bytes - complex_offsets[i])
            return RC_CONF_ERROR;
    }
    return RC_OK;
}

int cx_expand(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const CxShape &s, const aec_gpu_grib_complex_field *fields,
              const uint64_t *n_values, uint64_t n, const void *d_complex, const uint64_t *complex_offsets, const uint64_t *complex_bytes_each,
              void *d_work, aec_gpu_grib_cx *d_cx, hipStream_t st)
{
    const size_t h_need = (size_t)(n + 1) * sizeof(CxField);
    void *h = nullptr;
    void *stage = ctx_sz_stage(ctx, h_need, &h);
    if (!stage) return RC_MEM_ERROR;
    CxField *d = static_cast<CxField *>(h);
    uint64_t vt = 0, gt = 0, g0 = 0;
    bool differenced = false;
    for (uint64_t i = 0; i <= n; i++) {
        CxField &f = d[i];
        f = CxField{};
        f.vtile0 = vt;
        f.gtile0 = gt;
        f.group0 = g0;
        if (i == n) break;
        const aec_gpu_grib_complex_field &c = fields[i];
        f.off = complex_offsets[i];
        f.bytes = complex_bytes_each[i];
        f.n = n_values[i];
        f.work_off = s.work_offsets[i];
        f.room = s.rooms[i];
        f.ng = c.n_groups;
        f.ref_bits = c.ref_bits;
        f.width_ref = c.width_ref;
        f.width_bits = c.width_bits;
        f.length_ref = c.length_ref;
        f.length_inc = c.length_inc;
        f.last_length = c.last_length;
        f.length_bits = c.length_bits;
        f.order = c.order;
        f.extra = c.order ? c.extra_octets : 0u;
        f.refs_bit = 8u * (c.order ? (uint64_t)(c.order + 1u) * c.extra_octets : 0u);
        f.widths_bit = f.refs_bit + 8u * cx_table_bytes(c.n_groups, c.ref_bits);
        f.lengths_bit = f.widths_bit + 8u * cx_table_bytes(c.n_groups, c.width_bits);
        f.data_bit = f.lengths_bit + 8u * cx_table_bytes(c.n_groups, c.length_bits);
        differenced |= c.order != 0;
        vt += grib_room_waves(f.room);
        gt += (c.n_groups + kCxGroupTile - 1) / kCxGroupTile;
        g0 += c.n_groups;
    }
    uint8_t *cd = ctx_sz_send(ctx, stage, h_need, s.extent(), st);
    if (!cd) return RC_MEM_ERROR;
    CxOnDevice on;
    on.desc = reinterpret_cast<const CxField *>(cd);
    cd += s.desc_bytes;
    on.dyn = reinterpret_cast<CxDyn *>(cd);
    cd += s.dyn_bytes;
    on.gagg = reinterpret_cast<CxSum *>(cd);
    cd += s.gagg_bytes;
    on.gval = reinterpret_cast<uint64_t *>(cd);
    cd += s.g8_bytes;
    on.gbit = reinterpret_cast<uint64_t *>(cd);
    cd += s.g8_bytes;
    on.vagg = reinterpret_cast<CxAgg *>(cd);
    cd += s.vagg_bytes;
    on.vmin = reinterpret_cast<int64_t *>(cd);
    cd += s.v8_bytes;
    on.vmax = reinterpret_cast<int64_t *>(cd);
    cd += s.v8_bytes;
    on.gref = reinterpret_cast<uint32_t *>(cd);
    cd += s.g4_bytes;
    on.gwid = reinterpret_cast<uint32_t *>(cd);
    const uint8_t *complex = static_cast<const uint8_t *>(d_complex);
    uint8_t *work = static_cast<uint8_t *>(d_work);
    const dim3 block(kCxBlock), by_group(wave_blocks(gt)), by_value(wave_blocks(vt)), by_field(wave_blocks(n));
    const uint32_t container = grib_container(t->nbits), nbits = t->nbits;
    hipLaunchKernelGGL(k_cx_groups, by_group, block, 0, st, on, n, gt, complex);
    hipLaunchKernelGGL(k_cx_group_scan, by_field, block, 0, st, on, n, complex);
    hipLaunchKernelGGL(k_cx_group_apply, by_group, block, 0, st, on, n, gt);
#define CX_V(C)                                                                                        \
    do {                                                                                               \
        if (differenced) {                                                                             \
            hipLaunchKernelGGL((k_cx_values<C>), by_value, block, 0, st, on, n, vt, complex);          \
            hipLaunchKernelGGL((k_cx_value_scan<C>), by_field, block, 0, st, on, n);                   \
        }                                                                                              \
        hipLaunchKernelGGL((k_cx_apply<C>), by_value, block, 0, st, on, n, vt, nbits, complex, work);  \
    } while (0)
    if (container == 1) CX_V(1);
    else if (container == 2) CX_V(2);
    else CX_V(4);
#undef CX_V
    hipLaunchKernelGGL(k_cx_records, by_field, block, 0, st, on, n, nbits, d_cx);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

}  // namespace

extern "C" {

int aec_gpu_grib_complex_plan(const aec_gpu_grib_template *t, int elem, const uint64_t *n_values, const aec_gpu_grib_complex_field *fields,
                              uint64_t n_fields, aec_gpu_grib_complex_plan_t *plan, uint64_t *work_offsets)
{
    CxShape s;
    if (!plan || cx_shape(t, elem, n_values, fields, n_fields, &s) != RC_OK) return 0;
    *plan = s.plan;
    if (work_offsets && n_fields) memcpy(work_offsets, s.work_offsets, (size_t)n_fields * sizeof(uint64_t));
    return 1;
}

int aec_gpu_grib_complex_expand_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const aec_gpu_grib_complex_field *fields,
                                      const uint64_t *n_values, uint64_t n_fields, const void *d_complex, size_t complex_bytes,
                                      const uint64_t *complex_offsets, const uint64_t *complex_bytes_each, void *d_work,
                                      aec_gpu_grib_cx *d_cx, void *stream)
{
    if (!template_ok(t)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    CxShape s;
    const int rc = cx_args(ctx, t, AEC_GPU_GRIB_F32, fields, n_values, n_fields, d_complex, complex_bytes, complex_offsets, complex_bytes_each,
                           d_work, d_cx, &s);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    return cx_expand(ctx, t, s, fields, n_values, n_fields, d_complex, complex_offsets, complex_bytes_each, d_work, d_cx,
                     static_cast<hipStream_t>(stream));
}

int aec_gpu_grib_complex_unpack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const aec_gpu_grib_complex_field *fields,
                                      const void *d_complex, size_t complex_bytes, const uint64_t *complex_offsets,
                                      const uint64_t *complex_bytes_each, const uint64_t *n_values, const aec_gpu_grib_field *params,
                                      const uint64_t *dst_offsets, uint64_t n_fields, void *d_work, void *d_dst, aec_gpu_grib_cx *d_cx,
                                      void *stream)
{
    if (!template_ok(t) || (elem != AEC_GPU_GRIB_F32 && elem != AEC_GPU_GRIB_F64)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    CxShape s;
    int rc = cx_args(ctx, t, elem, fields, n_values, n_fields, d_complex, complex_bytes, complex_offsets, complex_bytes_each, d_work, d_cx, &s);
    if (rc != RC_OK) return rc;
    // (the checks of the second half first: a call it refuses enqueues nothing.  Its launch comes behind the expansion.)
    if (!params || !dst_offsets || !d_dst) return RC_CONF_ERROR;
    for (uint64_t i = 0; i < n_fields; i++)
        if ((reinterpret_cast<uintptr_t>(d_dst) + dst_offsets[i]) % (uint32_t)elem || params[i].D > kGribMaxD || params[i].D < -kGribMaxD ||
            params[i].E > 1022 || params[i].E < -1022)
            return RC_CONF_ERROR;
    (void)hipGetLastError();
    rc = cx_expand(ctx, t, s, fields, n_values, n_fields, d_complex, complex_offsets, complex_bytes_each, d_work, d_cx,
                   static_cast<hipStream_t>(stream));
    if (rc != RC_OK) return rc;
    return aec_gpu_grib_dequantise_async(ctx, t, elem, d_work, n_values, params, dst_offsets, n_fields, d_dst, stream);
}

int aec_gpu_grib_complex_to_ccsds_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const aec_gpu_grib_complex_field *fields,
                                        const void *d_complex, size_t complex_bytes, const uint64_t *complex_offsets,
                                        const uint64_t *complex_bytes_each, const uint64_t *n_values, uint64_t n_fields, void *d_work,
                                        void *d_out, size_t out_cap, aec_gpu_batch_chunk *d_chunks, uint64_t *d_rsi_bit_offsets,
                                        aec_gpu_enc_result *d_result, aec_gpu_grib_cx *d_cx, void *stream)
{
    if (!template_ok(t)) return RC_CONF_ERROR;
    if (n_fields == 0) return RC_OK;
    if (!d_out || !d_chunks || !d_result || !aligned(d_out, 16) || (out_cap & 15u) || out_cap < 16) return RC_CONF_ERROR;
    CxShape s;
    int rc = cx_args(ctx, t, AEC_GPU_GRIB_F32, fields, n_values, n_fields, d_complex, complex_bytes, complex_offsets, complex_bytes_each, d_work,
                     d_cx, &s);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    rc = cx_expand(ctx, t, s, fields, n_values, n_fields, d_complex, complex_offsets, complex_bytes_each, d_work, d_cx,
                   static_cast<hipStream_t>(stream));
    if (rc != RC_OK) return rc;
    return aec_gpu_encode_chunks_async(ctx, &s.plan.plan.coder, d_work, s.work_offsets, s.rooms, n_fields, d_out, out_cap, d_chunks,
                                       d_rsi_bit_offsets, d_result, stream);
}

}  // extern "C"
