// aec_szest.hip -- aec_gpu_sz_estimate_async (include/aec_gpu_sz.h): the length of SZ_BufftoBuffCompress's stream of every
// chunk of a batch under pixels_per_block 8, 16, 32 and 64, from one read of the chunks and with nothing marshalled to
// memory.  The arithmetic is aec_szest.h's over aec_est.h and aec_szmap.h (it runs on the CPU in
// tests/emul/sz_est_emul.cpp); what is here is how a chunk's bytes reach a lane and how the records are summed.
// No reference counterpart.  Per pass (the sizes that share a scan line):
//
//   k_szest_setup    the wavefront table of the pass (one uint32_t per wavefront: its chunk); the first pass's also clears
//                    the per-chunk sums and the record.
//   k_szest_pieces   lane = one piece: 64 coder samples of one scan line, from the line's start.  A wavefront takes 64
//                    pieces of ONE chunk and brings their bytes into LDS rows (one row per piece, padded by 16 bytes so that
//                    one-lane-per-row 16-byte reads are conflict free) on the chunk's path --
//                      generic    every lane walks the map of aec_szmap.h byte by byte: planes of any shape, lines that
//                                 straddle planes, unaligned chunks;
//                      straight   no planes, chunk base and line bytes multiples of 16: the wavefront's 16-byte groups that
//                                 are 16 bytes of a line as the chunk holds it are loaded as such (coalesced where the pieces
//                                 are neighbours in the chunk); line tails and the fill go through the map;
//                      planes4    4-byte pixels, whole lines per plane: a wavefront takes 16 units of 64 pixels, every
//                                 lane loads four quads of four pixels once and transposes them in registers
//                                 (sz_transpose4) into the rows of the pieces of all four planes, fill included
//                    -- then each lane reads its row and codes its 8 + 4 + 2 + 1 blocks with est_piece: one 16-bit record
//                    per block and size, those inside the line's padded length stored at line * rsi + block.
//   k_szest_sum      blockIdx.y = size.  A wavefront takes the lines of its chunk that start among its 64 pieces: a
//                    contiguous run of 64-block segments inside one chunk, a lane a block; zero runs by __ballot +
//                    est_seg_lane; wave sum; one 64-bit atomicAdd per wavefront into the chunk's sum.  Integer addition
//                    commutes: the sums do not depend on the order in which the wavefronts arrive.
// and at the end k_szest_finish (lane = chunk: its bits to d_chunk_bits, its stream bytes into the totals) and
// k_szest_best (one lane).
#include <hip/hip_runtime.h>

#include "../../include/aec_gpu_sz.h"
#include "aec_kernels.h"
#include "aec_szest.h"

namespace aec {
namespace {

constexpr uint32_t kPieceWaves = 2;        // wavefronts per workgroup of k_szest_pieces (LDS: 2 x 64 rows of up to 272 bytes)
constexpr uint32_t kSumWaves = 4;
constexpr uint32_t kSumAhead = 4;          // segments a wavefront of k_szest_sum has in flight
constexpr uint32_t kFinishBlock = 256;

static_assert(sizeof(aec_gpu_sz_estimate_t) == sizeof(SzEstResult) && AEC_GPU_SZ_ESTIMATE_SIZES == kEstSizes, "result layout");

__device__ __forceinline__ void lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void clear_result(uint32_t mask, SzEstResult *est)
{
    for (uint32_t i = 0; i < kEstSizes; i++) est->total_bytes[i] = ((mask >> i) & 1u) ? 0ull : ~0ull;
    const uint64_t zero[kEstSizes] = {0, 0, 0, 0};
    est->best = est_best(zero, mask);
    est->pad = 0;
}

// clear != 0: the call's first launch -- also the per-chunk sums (n * 4) and the record, for all sizes of the call (mask)
__global__ void __launch_bounds__(256)
k_szest_setup(const SzChunk *__restrict__ desc, uint64_t n, uint64_t waves, uint32_t *__restrict__ wave_chunk, uint32_t clear,
              uint32_t mask, unsigned long long *__restrict__ sums, SzEstResult *__restrict__ est)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = t; i < waves; i += stride) wave_chunk[i] = (uint32_t)sz_chunk_of_wave(desc, n, 0, i);
    if (clear) {
        for (uint64_t i = t; i < n * kEstSizes; i += stride) sums[i] = 0ull;
        if (t == 0) clear_result(mask, est);
    }
}

// this wavefront's chunk, the chunk's number and the wavefront's number within the chunk; false behind the last wavefront
template <uint32_t WAVES>
__device__ __forceinline__ bool wave_chunk_of(const SzChunk *__restrict__ desc, const uint32_t *__restrict__ wave_chunk,
                                              uint64_t nwaves, SzChunk &D, uint32_t &c, uint64_t &j)
{
    const uint64_t w = (uint64_t)blockIdx.x * WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= nwaves) return false;
    c = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_chunk[w]);
    D = desc[c];
    j = w - D.wave0[0];
    return true;
}

template <int BYTES>
__global__ void __launch_bounds__(kPieceWaves * 64)
k_szest_pieces(const SzEstPass s, const SzChunk *__restrict__ desc, const uint32_t *__restrict__ wave_chunk,
               const uint8_t *__restrict__ src, uint8_t *__restrict__ ws)
{
    constexpr uint32_t RW = 16u * BYTES;       // words of a piece
    constexpr uint32_t STRIDE = RW + 4u;       // ... and of its LDS row
    constexpr uint32_t CPP = 4u * BYTES;       // 16-byte groups of a piece
    __shared__ __attribute__((aligned(16))) uint32_t smem[kPieceWaves * 64u * STRIDE];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    SzChunk D;
    uint32_t c;
    uint64_t j;
    if (!wave_chunk_of<kPieceWaves>(desc, wave_chunk, s.waves, D, c, j)) return;
    uint32_t *rows = smem + wave * 64u * STRIDE;
    uint32_t *row = rows + lane * STRIDE;

    // the lane's own piece: scan line l of the chunk, piece g of the line
    bool live;
    uint64_t l = 0;
    uint32_t g = 0;
    if (BYTES == 1 && D.planes == kSzEstPlanes4) {
        const uint64_t lpp = D.lines / 4u, q = 16u * j + (lane & 15u);
        live = q < lpp * s.ppl;
        uint64_t r;
        szest_piece_at(s, live ? q : 0u, r, g);
        l = (lane >> 4) * lpp + r;
    } else {
        const uint64_t p = 64u * j + lane;
        live = p < D.coder_bytes;
        szest_piece_at(s, live ? p : 0u, l, g);
    }

    if (BYTES == 1 && D.planes == kSzEstPlanes4) {
        // quad tt of the wavefront's 16 units: unit tt / 16, its pixels 4 (tt % 16) ...; all four loads in flight at once
        const uint64_t units = D.lines / 4u * s.ppl;
        uint4 v[4];
        bool fill[4], have[4];
#pragma unroll
        for (uint32_t it = 0; it < 4u; it++) {
            const uint32_t tt = it * 64u + lane;
            const uint64_t q = 16u * j + tt / 16u;
            have[it] = q < units;
            uint64_t r;
            uint32_t gq;
            szest_piece_at(s, have[it] ? q : 0u, r, gq);
            const uint64_t at = szest_quad_at(s, D, r, gq, tt % 16u, fill[it]);
            v[it] = have[it] ? *reinterpret_cast<const uint4 *>(src + at) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (uint32_t it = 0; it < 4u; it++) {
            const uint32_t tt = it * 64u + lane;
            uint32_t out[4];
            szest_quad_planes(s.L, v[it].x, v[it].y, v[it].z, v[it].w, fill[it], out);
            if (have[it]) {
#pragma unroll
                for (uint32_t pl = 0; pl < 4u; pl++) rows[(pl * 16u + tt / 16u) * STRIDE + tt % 16u] = out[pl];
            }
        }
    } else if (D.planes == kSzEstStraight) {
        // group ci of the wavefront's 64 pieces: group ci % CPP of piece ci / CPP; all loads in flight at once
        uint4 v[CPP];
        bool have[CPP];
#pragma unroll
        for (uint32_t it = 0; it < CPP; it++) {
            const uint32_t ci = it * 64u + lane;
            const uint64_t p = 64u * j + ci / CPP;
            uint64_t lp;
            uint32_t gp;
            szest_piece_at(s, p < D.coder_bytes ? p : 0u, lp, gp);
            have[it] = p < D.coder_bytes && ci % CPP < szest_straight_groups(s.L, D, lp, gp);
            v[it] = have[it] ? *reinterpret_cast<const uint4 *>(src + szest_straight_at(s.L, D, lp, gp, ci % CPP))
                             : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (uint32_t it = 0; it < CPP; it++) {
            const uint32_t ci = it * 64u + lane;
            if (have[it]) *reinterpret_cast<uint4 *>(&rows[(ci / CPP) * STRIDE + (ci % CPP) * 4u]) = v[it];
        }
        lds_fence();
        // line tails and the fill (the lanes whose piece the line's own bytes do not fill)
        if (live) {
            const uint32_t groups = szest_straight_groups(s.L, D, l, g);
            if (groups < CPP) szest_fill_row(s.L, D, src, l, g, 16u * groups, reinterpret_cast<uint8_t *>(row));
        }
    } else if (live) {
        szest_fill_row(s.L, D, src, l, g, 0u, reinterpret_cast<uint8_t *>(row));
    }
    lds_fence();
    if (!live) return;

    uint32_t loc[RW];
#pragma unroll
    for (uint32_t q = 0; q < RW / 4u; q++) {
        const uint4 t = *reinterpret_cast<const uint4 *>(row + 4u * q);
        loc[4 * q] = t.x; loc[4 * q + 1] = t.y; loc[4 * q + 2] = t.z; loc[4 * q + 3] = t.w;
    }
    uint16_t rec[16];
    est_piece<BYTES>(s.e, loc, szest_prev(s.L, D, src, l, g), g, rec);
    szest_store(s, ws, D.work_off + l, g, rec);
}

__global__ void __launch_bounds__(kSumWaves * 64)
k_szest_sum(const SzEstPass s, const SzChunk *__restrict__ desc, const uint32_t *__restrict__ wave_chunk,
            const uint8_t *__restrict__ ws, unsigned long long *__restrict__ sums)
{
    const uint32_t i = blockIdx.y, lane = threadIdx.x & 63u;
    if (!((s.e.mask >> i) & 1u)) return;
    SzChunk D;
    uint32_t c;
    uint64_t j, lo, hi;
    if (!wave_chunk_of<kSumWaves>(desc, wave_chunk, s.waves, D, c, j)) return;
    szest_wave_lines(s, D, j, lo, hi);
    if (lo >= hi) return;
    const uint16_t *__restrict__ recs = reinterpret_cast<const uint16_t *>(ws + s.e.rec_off[i]);
    const uint64_t spr = s.e.segs_per_rsi[i], end = (D.work_off + hi) * spr;
    unsigned long long acc = 0;
    // kSumAhead segments per round, their loads issued together
    for (uint64_t s0 = (D.work_off + lo) * spr; s0 < end; s0 += kSumAhead) {
        EstSeg g[kSumAhead];
        uint32_t rec[kSumAhead];
#pragma unroll
        for (uint32_t k = 0; k < kSumAhead; k++) {
            const bool on = s0 + k < end;
            g[k] = est_seg(s.e, i, on ? s0 + k : s0);
            if (!on) g[k].nv = 0;
            rec[k] = lane < g[k].nv ? recs[g[k].blk0 + lane] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kSumAhead; k++) {
            const uint64_t zmask = __ballot(lane < g[k].nv && (rec[k] & kEstZero));
            acc += est_seg_lane(s.e, g[k], lane, rec[k], zmask);
        }
    }
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if (lane == 0 && acc) atomicAdd(&sums[(uint64_t)c * kEstSizes + i], acc);
}

// lane = chunk: bits per size to chunk_bits (optional), stream bytes into the totals (one atomicAdd per workgroup and size)
__global__ void __launch_bounds__(kFinishBlock)
k_szest_finish(uint64_t n, uint32_t mask, const unsigned long long *__restrict__ sums, uint64_t *__restrict__ chunk_bits,
               SzEstResult *__restrict__ est)
{
    __shared__ unsigned long long part[kFinishBlock / 64][kEstSizes];
    const uint64_t c = (uint64_t)blockIdx.x * kFinishBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t i = 0; i < kEstSizes; i++) {
        const bool asked = (mask >> i) & 1u;
        unsigned long long bytes = 0;
        if (c < n) {
            const uint64_t bits = asked ? sums[c * kEstSizes + i] : ~0ull;
            if (chunk_bits) chunk_bits[c * kEstSizes + i] = bits;
            if (asked) bytes = szest_stream_bytes(bits);
        }
#pragma unroll
        for (uint32_t o = 32; o > 0; o >>= 1) bytes += __shfl_down(bytes, o);
        if (lane == 0) part[wave][i] = bytes;
    }
    __syncthreads();
    if (threadIdx.x < kEstSizes && ((mask >> threadIdx.x) & 1u)) {
        unsigned long long sum = 0;
        for (uint32_t w = 0; w < kFinishBlock / 64; w++) sum += part[w][threadIdx.x];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(&est->total_bytes[threadIdx.x]), sum);
    }
}

__global__ void __launch_bounds__(64) k_szest_best(uint32_t mask, SzEstResult *__restrict__ est)
{
    if (threadIdx.x == 0) {
        uint64_t t[kEstSizes];
        for (uint32_t i = 0; i < kEstSizes; i++) t[i] = est->total_bytes[i];
        est->best = est_best(t, mask);
    }
}

__global__ void __launch_bounds__(64) k_szest_empty(uint32_t mask, SzEstResult *__restrict__ est)
{
    if (threadIdx.x == 0) clear_result(mask, est);
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- host side ---------------------------------------------------------------------------------------------------------------
// The passes of a call: the sizes asked, grouped by scan line in the order of their first size.
struct SzEstCall {
    SzEstPass pass[kEstSizes];
    uint32_t passes, mask;
    uint64_t pieces;
    size_t desc_bytes;               // all passes' descriptors, (n + 1) each
    size_t table_off[kEstSizes];     // the passes' wavefront tables
    size_t sums_off, rec_off, d_need;
};

// host arithmetic of a call; with desc (passes * (n + 1) entries) the descriptors are written too.  RC_CONF_ERROR = refused.
int shape(const SZ_com_t *sz, const unsigned int *pps, uint64_t base, const uint64_t *offsets, const uint64_t *chunk_bytes,
          uint64_t n, SzEstCall *call, SzChunk *desc)
{
    if (!sz || (n && !chunk_bytes) || n > 0x7FFFFFFFull) return RC_CONF_ERROR;
    *call = SzEstCall{};
    unsigned int line[kEstSizes];
    for (uint32_t i = 0; i < kEstSizes; i++) {
        line[i] = pps ? pps[i] : (sz->pixels_per_scanline > 0 ? (unsigned int)sz->pixels_per_scanline : 0u);
        if (line[i]) call->mask |= 1u << i;
    }
    if (!call->mask) return RC_CONF_ERROR;
    uint32_t done = 0;
    for (uint32_t i = 0; i < kEstSizes; i++) {
        if (!((call->mask >> i) & 1u) || ((done >> i) & 1u)) continue;
        uint32_t m = 0;
        for (uint32_t k = i; k < kEstSizes; k++) m |= line[k] == line[i] ? 1u << k : 0u;
        done |= m;
        SzEstPass &s = call->pass[call->passes];
        if (szest_make_pass(sz->options_mask, sz->bits_per_pixel, line[i], m, &s) != RC_OK) return RC_CONF_ERROR;
        if (!szest_make_chunks(&s, base, offsets, chunk_bytes, n, desc ? desc + call->passes * (n + 1) : nullptr))
            return RC_CONF_ERROR;
        // aec_gpu_sz_chunks_plan's count of what marshalling the batch under each candidate would launch
        for (uint32_t k = 0; k < kEstSizes; k++) {
            if (!((m >> k) & 1u)) continue;
            const uint64_t padded = (uint64_t)s.e.rsi[k] * (8u << k) * s.L.pixel;
            uint64_t group_waves = 0;
            for (uint64_t ch = 0; ch < n; ch++) {
                SzChunk D;
                sz_chunk_sizes(s.L, chunk_bytes[ch], D);
                const uint64_t coder = D.lines * padded;
                group_waves += sz_group_waves(coder > D.chunk_bytes ? coder : D.chunk_bytes, 15u);
                if (group_waves > kSzEstMaxWaves) return RC_CONF_ERROR;
            }
        }
        call->pieces += s.e.pieces;
        call->passes++;
    }
    call->desc_bytes = up256((size_t)call->passes * (size_t)(n + 1) * sizeof(SzChunk));
    size_t off = call->desc_bytes, rec = 0;
    for (uint32_t p = 0; p < call->passes; p++) {
        call->table_off[p] = off;
        off += up256((size_t)(call->pass[p].waves ? call->pass[p].waves : 1) * 4);
        rec = call->pass[p].rec_bytes > rec ? (size_t)call->pass[p].rec_bytes : rec;
    }
    call->sums_off = off;
    off += up256((size_t)(n ? n : 1) * kEstSizes * 8);
    call->rec_off = off;
    call->d_need = off + up256(rec);
    return RC_OK;
}

}  // namespace
}  // namespace aec

using namespace aec;

extern "C" {

int aec_gpu_sz_estimate_plan(const SZ_com_t *sz, const unsigned int *pixels_per_scanline, const uint64_t *chunk_bytes,
                             uint64_t n_chunks, struct aec_gpu_sz_estimate_plan *plan)
{
    SzEstCall call;
    if (!plan || shape(sz, pixels_per_scanline, 0, nullptr, chunk_bytes, n_chunks, &call, nullptr) != RC_OK) return 0;
    plan->evaluated = call.mask;
    plan->passes = call.passes;
    plan->pieces = call.pieces;
    plan->workspace_bytes = n_chunks ? ctx_desc_room(call.d_need) : 0;
    return 1;
}

int aec_gpu_sz_estimate_async(aec_gpu_ctx *ctx, const SZ_com_t *sz, const unsigned int *pixels_per_scanline, const void *d_src,
                              const uint64_t *src_offsets, const uint64_t *chunk_bytes, uint64_t n_chunks,
                              uint64_t *d_chunk_bits, aec_gpu_sz_estimate_t *d_estimate, void *stream)
{
    if (!ctx || !d_estimate || (n_chunks && (!d_src || !src_offsets))) return RC_CONF_ERROR;
    SzEstCall on_stack, *call = &on_stack;
    const uint64_t n = n_chunks, base = reinterpret_cast<uintptr_t>(d_src);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    SzEstResult *est = reinterpret_cast<SzEstResult *>(d_estimate);
    if (n == 0) {
        const int rc = shape(sz, pixels_per_scanline, base, nullptr, nullptr, 0, call, nullptr);
        if (rc != RC_OK) return rc;
        (void)hipGetLastError();
        hipLaunchKernelGGL(k_szest_empty, dim3(1), dim3(64), 0, st, call->mask, est);
        return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
    }
    // the descriptors of all passes (as many as there are distinct scan lines): one pinned buffer, one transfer
    if (!sz || !chunk_bytes || n > 0x7FFFFFFFull) return RC_CONF_ERROR;
    uint32_t passes = 0;
    for (uint32_t i = 0; i < kEstSizes; i++) {
        bool first = pixels_per_scanline ? pixels_per_scanline[i] != 0 : i == 0;
        for (uint32_t k = 0; k < i && pixels_per_scanline; k++) first &= pixels_per_scanline[k] != pixels_per_scanline[i];
        passes += first ? 1u : 0u;
    }
    const size_t h_need = (size_t)(passes ? passes : 1u) * (size_t)(n + 1) * sizeof(SzChunk);
    void *h = nullptr;
    void *stage = ctx_sz_stage(ctx, h_need, &h);
    if (!stage) return RC_MEM_ERROR;
    const int rc = shape(sz, pixels_per_scanline, base, src_offsets, chunk_bytes, n, call, static_cast<SzChunk *>(h));
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    uint8_t *d = ctx_sz_send(ctx, stage, h_need, call->d_need, st);
    if (!d) return RC_MEM_ERROR;
    const uint8_t *src = static_cast<const uint8_t *>(d_src);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(d + call->sums_off);
    uint8_t *recs = d + call->rec_off;
    for (uint32_t p = 0; p < call->passes; p++) {
        const SzEstPass &s = call->pass[p];
        const SzChunk *desc = reinterpret_cast<const SzChunk *>(d) + (size_t)p * (size_t)(n + 1);
        uint32_t *table = reinterpret_cast<uint32_t *>(d + call->table_off[p]);
        const uint64_t items = s.waves > n * kEstSizes ? s.waves : n * kEstSizes, grid = (items + 255) / 256;
        hipLaunchKernelGGL(k_szest_setup, dim3((uint32_t)(grid < 4096 ? grid : 4096)), dim3(256), 0, st, desc, n, s.waves, table,
                           p == 0 ? 1u : 0u, call->mask, sums, est);
        const dim3 pg((uint32_t)((s.waves + kPieceWaves - 1) / kPieceWaves)), pb(kPieceWaves * 64u);
        switch (s.L.pixel) {
        case 1: hipLaunchKernelGGL(k_szest_pieces<1>, pg, pb, 0, st, s, desc, table, src, recs); break;
        case 2: hipLaunchKernelGGL(k_szest_pieces<2>, pg, pb, 0, st, s, desc, table, src, recs); break;
        default: hipLaunchKernelGGL(k_szest_pieces<4>, pg, pb, 0, st, s, desc, table, src, recs); break;
        }
        hipLaunchKernelGGL(k_szest_sum, dim3((uint32_t)((s.waves + kSumWaves - 1) / kSumWaves), kEstSizes), dim3(kSumWaves * 64u), 0,
                           st, s, desc, table, recs, sums);
    }
    hipLaunchKernelGGL(k_szest_finish, dim3((uint32_t)((n + kFinishBlock - 1) / kFinishBlock)), dim3(kFinishBlock), 0, st, n,
                       call->mask, sums, d_chunk_bits, est);
    hipLaunchKernelGGL(k_szest_best, dim3(1), dim3(64), 0, st, call->mask, est);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

}  // extern "C"
