// aec_est.hip -- kernels of aec_gpu_estimate_async (include/aec_gpu.h): the exact coded size of one input under block
// sizes 8, 16, 32 and 64 from one read of the input.  The arithmetic is aec_est.h's (it runs on the CPU in
// tests/emul/est_emul.cpp); what is here is how the samples reach a lane, where the records go and how they are summed.
// No reference counterpart.
//
//   k_est_blocks   lane = one piece of 64 samples.  A wavefront loads its 64 pieces with coalesced 16-byte loads into LDS
//                  rows (one row per piece, padded by 16 bytes so that one-lane-per-row 16-byte reads are conflict free),
//                  each lane then reads its row, maps it through the predictor once and codes its 8 + 4 + 2 + 1 blocks:
//                  one 16-bit record per block and size (the length in bits, or the zero-block mark).
//   k_est_sum      blockIdx.y = size.  A wavefront takes 64-block segments of that size's RSIs, a lane a block; zero runs by
//                  __ballot + zero_run_at; wave sum, workgroup sum, one 64-bit atomicAdd per workgroup into the record.
//                  Integer addition commutes: the total does not depend on the order in which the workgroups arrive.
//   k_est_best     one lane: the index of the smallest total.
#include <hip/hip_runtime.h>

#include "aec_est.h"

namespace aec {
namespace {

constexpr uint32_t kEstWaves = 2;          // wavefronts per workgroup of k_est_blocks (LDS: 2 x 64 rows of up to 272 bytes)
constexpr uint32_t kSumWaves = 4;
constexpr uint32_t kSumAhead = 4;          // segments a wavefront of k_est_sum has in flight
constexpr uint32_t kSumMaxGroups = 2048;   // workgroups of k_est_sum per size: as many atomics into one 64-bit word

__device__ __forceinline__ void est_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void est_clear(const EstCfg &e, EstResult *est)
{
    for (uint32_t i = 0; i < kEstSizes; i++) est->total_bits[i] = ((e.mask >> i) & 1u) ? 0ull : ~0ull;
    uint64_t zero[kEstSizes] = {0, 0, 0, 0};
    est->best = est_best(zero, e.mask);
    est->pad = 0;
}

// an input without a whole sample: 0 for every size asked for
__global__ void __launch_bounds__(64) k_est_empty(const EstCfg e, EstResult *__restrict__ est)
{
    if (threadIdx.x == 0) est_clear(e, est);
}

template <int BYTES>
__global__ void __launch_bounds__(kEstWaves * 64)
k_est_blocks(const EstCfg e, const uint8_t *__restrict__ in, uint8_t *__restrict__ ws, EstResult *__restrict__ est)
{
    constexpr uint32_t RW = 16u * BYTES;       // words of a piece
    constexpr uint32_t STRIDE = RW + 4u;       // ... and of its LDS row
    constexpr uint32_t CPP = 4u * BYTES;       // 16-byte chunks of a piece
    __shared__ __attribute__((aligned(16))) uint32_t smem[kEstWaves * 64u * STRIDE];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) est_clear(e, est);      // (k_est_sum adds into it behind this kernel)

    const uint64_t p0 = ((uint64_t)blockIdx.x * kEstWaves + wave) * 64u;      // the wavefront's first piece
    if (p0 >= e.pieces) return;
    uint32_t *rows = smem + wave * 64u * STRIDE;
    // whole pieces go through coalesced loads: chunk ci of the wavefront's stretch is chunk ci % CPP of its piece ci / CPP
    const uint64_t full = e.c.total_samples / kEstPiece;
    const uint32_t nfull = full > p0 ? (full - p0 < 64u ? (uint32_t)(full - p0) : 64u) : 0u;
    const uint4 *src = reinterpret_cast<const uint4 *>(in) + p0 * CPP;
    if (nfull) {
        // (addresses clamped to the stretch's last chunk: the loads are unconditional and all in flight at once)
        const uint32_t nchunks = nfull * CPP;
        uint4 v[CPP];
#pragma unroll
        for (uint32_t it = 0; it < CPP; it++) {
            const uint32_t ci = it * 64u + lane;
            v[it] = src[ci < nchunks ? ci : nchunks - 1u];
        }
#pragma unroll
        for (uint32_t it = 0; it < CPP; it++) {
            const uint32_t ci = it * 64u + lane;
            if (ci < nchunks) *reinterpret_cast<uint4 *>(&rows[(ci / CPP) * STRIDE + (ci % CPP) * 4u]) = v[it];
        }
    }
    const uint64_t pi = p0 + lane;
    uint32_t *row = rows + lane * STRIDE;
    if (pi == full && pi < e.pieces) {
        // the piece the input ends in (one lane of the grid): byte by byte, the last sample repeated (encode.c:676-684)
        uint8_t *rb = reinterpret_cast<uint8_t *>(row);
        const uint64_t last = e.c.total_samples - 1;
        for (uint32_t i = 0; i < kEstPiece; i++) {
            uint64_t s = pi * kEstPiece + i;
            if (s > last) s = last;
            for (uint32_t b = 0; b < (uint32_t)BYTES; b++) rb[i * BYTES + b] = in[s * BYTES + b];
        }
    }
    est_lds_fence();
    if (pi >= e.pieces) return;

    uint32_t loc[RW];
#pragma unroll
    for (uint32_t q = 0; q < RW / 4u; q++) {
        const uint4 t = *reinterpret_cast<const uint4 *>(row + 4u * q);
        loc[4 * q] = t.x; loc[4 * q + 1] = t.y; loc[4 * q + 2] = t.z; loc[4 * q + 3] = t.w;
    }
    const uint32_t prev = pi ? load_sample_bytes(in + (pi * kEstPiece - 1) * BYTES, BYTES, e.c.flags & F_MSB) : 0u;
    uint16_t rec[16];
    est_piece<BYTES>(e, loc, prev, pi, rec);

    auto two = [&](uint32_t j) { return (uint32_t)rec[j] | ((uint32_t)rec[j + 1] << 16); };
    if (e.rsi[0]) *reinterpret_cast<uint4 *>(ws + e.rec_off[0] + pi * 16u) = make_uint4(two(0), two(2), two(4), two(6));
    if (e.rsi[1]) *reinterpret_cast<uint2 *>(ws + e.rec_off[1] + pi * 8u) = make_uint2(two(8), two(10));
    if (e.rsi[2]) *reinterpret_cast<uint32_t *>(ws + e.rec_off[2] + pi * 4u) = two(12);
    if (e.rsi[3]) *reinterpret_cast<uint16_t *>(ws + e.rec_off[3] + pi * 2u) = rec[14];
}

__global__ void __launch_bounds__(kSumWaves * 64)
k_est_sum(const EstCfg e, const uint8_t *__restrict__ ws, EstResult *__restrict__ est)
{
    __shared__ unsigned long long part[kSumWaves];
    const uint32_t i = blockIdx.y;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool asked = (e.mask >> i) & 1u;
    unsigned long long acc = 0;
    if (asked) {
        const uint16_t *__restrict__ recs = reinterpret_cast<const uint16_t *>(ws + e.rec_off[i]);
        const uint64_t nwaves = (uint64_t)gridDim.x * kSumWaves;
        // kSumAhead segments per round, their loads issued together: a round is one trip to memory, not four
        for (uint64_t s0 = (uint64_t)blockIdx.x * kSumWaves + wave; s0 < e.segs[i]; s0 += nwaves * kSumAhead) {
            EstSeg g[kSumAhead];
            uint32_t rec[kSumAhead];
#pragma unroll
            for (uint32_t j = 0; j < kSumAhead; j++) {
                const uint64_t sg = s0 + j * nwaves;
                const bool live = sg < e.segs[i];
                g[j] = est_seg(e, i, live ? sg : 0);
                if (!live) g[j].nv = 0;
                rec[j] = lane < g[j].nv ? recs[g[j].blk0 + lane] : 0u;
            }
#pragma unroll
            for (uint32_t j = 0; j < kSumAhead; j++) {
                const uint64_t zmask = __ballot(lane < g[j].nv && (rec[j] & kEstZero));
                acc += est_seg_lane(e, g[j], lane, rec[j], zmask);
            }
        }
    }
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && asked) {
        unsigned long long sum = 0;
        for (uint32_t w = 0; w < kSumWaves; w++) sum += part[w];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(&est->total_bits[i]), sum);
    }
}

__global__ void __launch_bounds__(64) k_est_best(const EstCfg e, EstResult *__restrict__ est)
{
    if (threadIdx.x == 0) {
        uint64_t t[kEstSizes];
        for (uint32_t i = 0; i < kEstSizes; i++) t[i] = est->total_bits[i];
        est->best = est_best(t, e.mask);
    }
}

}  // namespace

void launch_estimate(const EstCfg &e, const uint8_t *d_in, uint8_t *ws, EstResult *d_est, hipStream_t stream)
{
    if (e.pieces == 0) {
        hipLaunchKernelGGL(k_est_empty, dim3(1), dim3(64), 0, stream, e, d_est);
        return;
    }
    const dim3 grid((uint32_t)((e.pieces + 64u * kEstWaves - 1) / (64u * kEstWaves))), block(kEstWaves * 64u);
    switch (e.c.bytes) {
    case 1: hipLaunchKernelGGL(k_est_blocks<1>, grid, block, 0, stream, e, d_in, ws, d_est); break;
    case 2: hipLaunchKernelGGL(k_est_blocks<2>, grid, block, 0, stream, e, d_in, ws, d_est); break;
    case 3: hipLaunchKernelGGL(k_est_blocks<3>, grid, block, 0, stream, e, d_in, ws, d_est); break;
    default: hipLaunchKernelGGL(k_est_blocks<4>, grid, block, 0, stream, e, d_in, ws, d_est); break;
    }
    uint64_t most = 0;
    for (uint32_t i = 0; i < kEstSizes; i++) most = e.segs[i] > most ? e.segs[i] : most;
    // eight segments and more per wavefront where there are many: fewer atomics, the same bytes read
    uint64_t groups = (most + kSumWaves * 8u - 1) / (kSumWaves * 8u);
    groups = groups < 1 ? 1 : (groups > kSumMaxGroups ? kSumMaxGroups : groups);
    hipLaunchKernelGGL(k_est_sum, dim3((uint32_t)groups, kEstSizes), dim3(kSumWaves * 64u), 0, stream, e, ws, d_est);
    hipLaunchKernelGGL(k_est_best, dim3(1), dim3(64), 0, stream, e, d_est);
}

}  // namespace aec
