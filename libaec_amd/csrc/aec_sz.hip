// aec_sz.hip -- SZIP chunks on the device (include/aec_gpu_sz.h): the marshalling the reference's shim does on the
// host around its one coder call (reference src/sz_compat.c:39-108, 134-166, 208-261; here: sz_abi.cpp) as kernels,
// and the two one-call forms over the batch coder of aec_gpu.hip.  The index arithmetic is aec_szmap.h.
//
// Pure data movement.  Two paths:
//   bytes   a lane owns one 16-byte group of the OUTPUT (groups lie on 16-byte boundaries of the output's address, so
//           every whole group is one 16-byte store).  Where its 16 bytes are 16 consecutive bytes of one scan line at
//           a 16-byte aligned source address it moves them with one 16-byte load; else it walks the map byte by byte
//           (line tails, padding, partial last lines, unaligned chunk bases, planes of odd length).
//   planes  whole chunks of 32- / 64-bit pixels whose planes and lines are multiples of 4 bytes: a lane takes four
//           pixels (one or two 16-byte loads), transposes them in registers (v_perm_b32) and stores a 4-byte piece to
//           each plane; the merge reads those pieces and stores the pixels 16 bytes at a time.  The padding of such
//           chunks is written by k_sz_fill.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>

#include "../../include/aec_gpu_sz.h"
#include "aec_kernels.h"
#include "aec_szmap.h"

using namespace aec;

namespace {

constexpr uint32_t kSzBlock = 256;

// the run [0, total) of output bytes at `out` in 16-byte groups of its ADDRESS: group g covers run bytes
// [16 g - head, 16 g - head + 16), head = out & 15
struct SzGroup {
    uint64_t first, end;    // the group's bytes of the run
    int64_t lo;             // run byte of the group's byte 0 (may be negative in group 0)
    bool whole;
};

__device__ __forceinline__ bool sz_group_at(uint64_t i, uint64_t total, uint32_t head, SzGroup &g)
{
    g.lo = (int64_t)(i * 16u) - (int64_t)head;
    if (g.lo >= (int64_t)total) return false;
    g.first = g.lo < 0 ? 0u : (uint64_t)g.lo;
    g.end = (uint64_t)(g.lo + 16) < total ? (uint64_t)(g.lo + 16) : total;
    g.whole = g.lo >= 0 && (uint64_t)(g.lo + 16) <= total;
    return true;
}

__device__ __forceinline__ bool sz_group(uint64_t total, uint32_t head, SzGroup &g)
{
    return sz_group_at((uint64_t)blockIdx.x * kSzBlock + threadIdx.x, total, head, g);
}

__device__ __forceinline__ void sz_store_group(uint8_t *out, const SzGroup &g, const uint32_t (&w)[4])
{
    if (g.whole) {
        *reinterpret_cast<uint4 *>(out + g.lo) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < 16; i++)
        if (g.lo + i >= (int64_t)g.first && g.lo + i < (int64_t)g.end) out[g.lo + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// chunks -> coder inputs
__global__ void __launch_bounds__(kSzBlock)
k_sz_marshal(const SzLayout L, const uint8_t *__restrict__ src, uint8_t *__restrict__ out, uint64_t total, uint32_t head)
{
    SzGroup g;
    if (!sz_group(total, head, g)) return;
    SzInCursor c;
    sz_in_seek(L, g.first, c);
    if (g.whole) {
        const uint64_t at = sz_in_straight(L, c);
        if (at != kSzZero && (reinterpret_cast<uintptr_t>(src + at) & 15u) == 0) {
            *reinterpret_cast<uint4 *>(out + g.lo) = *reinterpret_cast<const uint4 *>(src + at);
            return;
        }
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (g.lo + i >= (int64_t)g.first && g.lo + i < (int64_t)g.end) {
            w[i >> 2] |= (uint32_t)sz_in_byte(L, src, c) << (8 * (i & 3));
            sz_in_next(L, c);
        }
    }
    sz_store_group(out, g, w);
}

// coder outputs -> chunks
__global__ void __launch_bounds__(kSzBlock)
k_sz_unmarshal(const SzLayout L, const uint8_t *__restrict__ coder_out, uint8_t *__restrict__ dst, uint64_t total,
               uint32_t head)
{
    SzGroup g;
    if (!sz_group(total, head, g)) return;
    uint64_t chunk, d;
    sz_divmod(g.first, L.chunk_bytes, chunk, d);
    if (g.whole) {
        const uint64_t at = sz_out_straight(L, chunk, d);
        if (at != kSzZero && (reinterpret_cast<uintptr_t>(coder_out + at) & 15u) == 0) {
            *reinterpret_cast<uint4 *>(dst + g.lo) = *reinterpret_cast<const uint4 *>(coder_out + at);
            return;
        }
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (g.lo + i >= (int64_t)g.first && g.lo + i < (int64_t)g.end) {
            w[i >> 2] |= (uint32_t)sz_out_byte(L, coder_out, chunk, d) << (8 * (i & 3));
            if (++d == L.chunk_bytes) {
                d = 0;
                chunk++;
            }
        }
    }
    sz_store_group(dst, g, w);
}

// byte planes, sz_planes_fast(L) chunks: lane = four pixels
template <int WORD>
__global__ void __launch_bounds__(kSzBlock)
k_sz_split(const SzLayout L, const uint8_t *__restrict__ src, uint8_t *__restrict__ out, uint64_t nquads)
{
    const uint64_t t = (uint64_t)blockIdx.x * kSzBlock + threadIdx.x;
    if (t >= nquads) return;
    uint64_t chunk, m;
    sz_divmod(t, L.pixels / 4u, chunk, m);
    const uint4 *p = reinterpret_cast<const uint4 *>(src + chunk * L.chunk_bytes + m * (4u * WORD));
    uint32_t piece[WORD];
    if constexpr (WORD == 4) {
        const uint4 a = p[0];
        sz_transpose4(a.x, a.y, a.z, a.w, piece);
    } else {
        const uint4 a = p[0], b = p[1];                       // pixels 4m, 4m+1 | 4m+2, 4m+3: low word, high word
        sz_transpose4(a.x, a.z, b.x, b.z, piece);
        sz_transpose4(a.y, a.w, b.y, b.w, piece + 4);
    }
    uint8_t *base = out + chunk * L.coder_bytes;
#pragma unroll
    for (int j = 0; j < WORD; j++) *reinterpret_cast<uint32_t *>(base + sz_piece_at(L, (uint32_t)j, m)) = piece[j];
}

template <int WORD>
__global__ void __launch_bounds__(kSzBlock)
k_sz_merge(const SzLayout L, const uint8_t *__restrict__ coder_out, uint8_t *__restrict__ dst, uint64_t nquads)
{
    const uint64_t t = (uint64_t)blockIdx.x * kSzBlock + threadIdx.x;
    if (t >= nquads) return;
    uint64_t chunk, m;
    sz_divmod(t, L.pixels / 4u, chunk, m);
    const uint8_t *base = coder_out + chunk * L.coder_bytes;
    uint32_t piece[WORD];
#pragma unroll
    for (int j = 0; j < WORD; j++) piece[j] = *reinterpret_cast<const uint32_t *>(base + sz_piece_at(L, (uint32_t)j, m));
    uint4 *p = reinterpret_cast<uint4 *>(dst + chunk * L.chunk_bytes + m * (4u * WORD));
    uint32_t lo[4];
    sz_transpose4(piece[0], piece[1], piece[2], piece[3], lo);
    if constexpr (WORD == 4) {
        p[0] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    } else {
        uint32_t hi[4];
        sz_transpose4(piece[4], piece[5], piece[6], piece[7], hi);
        p[0] = make_uint4(lo[0], hi[0], lo[1], hi[1]);
        p[1] = make_uint4(lo[2], hi[2], lo[3], hi[3]);
    }
}

// the padding of sz_planes_fast(L) chunks: block = scan line, a lane writes 4 bytes (take and padded_line are
// multiples of 4 there)
__global__ void __launch_bounds__(64)
k_sz_fill(const SzLayout L, const uint8_t *__restrict__ src, uint8_t *__restrict__ out)
{
    SzInCursor c;
    sz_divmod(blockIdx.x, L.lines, c.chunk, c.l);
    c.take = sz_take(L, c.l);
    uint8_t *row = out + c.chunk * L.coder_bytes + c.l * L.padded_line;
    for (uint64_t k = c.take + 4u * threadIdx.x; k < L.padded_line; k += 4u * 64u) {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            c.k = k + i;
            w |= (uint32_t)sz_in_byte(L, src, c) << (8 * i);
        }
        *reinterpret_cast<uint32_t *>(row + k) = w;
    }
}

// ---- batches of unequal chunks (aec_szmap.h: SzChunk) ----------------------------------------------------------------------
// The same two paths, chosen per chunk.  A chunk owns whole wavefronts of its path's launch; a wavefront reads its chunk's
// number from the table k_sz_chunks_setup wrote (one uint32_t per wavefront: the byte path's wavefronts, then the plane
// path's), so the chunk is wave-uniform, its descriptor is read once per wavefront through the scalar cache and no lane
// searches in front of its 16-byte move.
constexpr uint32_t kSzWaves = kSzBlock / 64;

__global__ void __launch_bounds__(256)
k_sz_chunks_setup(const SzChunk *__restrict__ desc, uint64_t n, uint64_t byte_waves, uint64_t plane_waves,
                  uint32_t *__restrict__ wave_chunk)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < byte_waves + plane_waves; i += stride)
        wave_chunk[i] = i < byte_waves ? (uint32_t)sz_chunk_of_wave(desc, n, kSzBytes, i)
                                       : (uint32_t)sz_chunk_of_wave(desc, n, kSzPlanes, i - byte_waves);
}

// this wavefront's chunk and the lane's number within the chunk; false behind the last wavefront
__device__ __forceinline__ bool sz_wave_chunk(const SzChunk *__restrict__ desc, const uint32_t *__restrict__ wave_chunk,
                                              uint64_t nwaves, int path, SzChunk &D, uint64_t &lane)
{
    const uint64_t w = (uint64_t)blockIdx.x * kSzWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= nwaves) return false;
    D = desc[(uint32_t)__builtin_amdgcn_readfirstlane((int)wave_chunk[w])];
    lane = (w - D.wave0[path]) * 64u + (threadIdx.x & 63u);
    return true;
}

// chunks -> their rooms in the work buffer (rooms are 16-byte aligned: only a chunk's last group can be partial)
__global__ void __launch_bounds__(kSzBlock)
k_sz_marshal_chunks(const SzLayout L, const SzChunk *__restrict__ desc, const uint32_t *__restrict__ wave_chunk, uint64_t nwaves,
                    const uint8_t *__restrict__ src, uint8_t *__restrict__ work)
{
    SzChunk D;
    uint64_t lane;
    SzGroup g;
    if (!sz_wave_chunk(desc, wave_chunk, nwaves, kSzBytes, D, lane) || !sz_group_at(lane, D.coder_bytes, 0u, g)) return;
    uint8_t *out = work + D.work_off;
    SzInCursor c;
    sz_in_seek(L, D, g.first, c);
    if (g.whole) {
        const uint64_t at = sz_in_straight(L, D, c);
        if (at != kSzZero && (reinterpret_cast<uintptr_t>(src + at) & 15u) == 0) {
            *reinterpret_cast<uint4 *>(out + g.lo) = *reinterpret_cast<const uint4 *>(src + at);
            return;
        }
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (g.lo + i >= (int64_t)g.first && g.lo + i < (int64_t)g.end) {
            w[i >> 2] |= (uint32_t)sz_in_byte(L, D, src, c) << (8 * (i & 3));
            sz_in_next(L, D, c);
        }
    }
    sz_store_group(out, g, w);
}

// rooms of the work buffer -> chunks: every chunk has its own head, its first and last groups store bytes (two chunks
// that share a 16-byte line of the destination write disjoint bytes of it)
__global__ void __launch_bounds__(kSzBlock)
k_sz_unmarshal_chunks(const SzLayout L, const SzChunk *__restrict__ desc, const uint32_t *__restrict__ wave_chunk,
                      uint64_t nwaves, const uint8_t *__restrict__ work, uint8_t *__restrict__ dst)
{
    SzChunk D;
    uint64_t lane;
    SzGroup g;
    if (!sz_wave_chunk(desc, wave_chunk, nwaves, kSzBytes, D, lane) || !sz_group_at(lane, D.chunk_bytes, D.head, g)) return;
    uint8_t *out = dst + D.off;
    uint64_t d = g.first;
    if (g.whole) {
        const uint64_t at = sz_out_straight(L, D, d);
        if (at != kSzZero && (reinterpret_cast<uintptr_t>(work + at) & 15u) == 0) {
            *reinterpret_cast<uint4 *>(out + g.lo) = *reinterpret_cast<const uint4 *>(work + at);
            return;
        }
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++)
        if (g.lo + i >= (int64_t)g.first && g.lo + i < (int64_t)g.end)
            w[i >> 2] |= (uint32_t)sz_out_byte(L, D, work, d++) << (8 * (i & 3));
    sz_store_group(out, g, w);
}

template <int WORD>
__global__ void __launch_bounds__(kSzBlock)
k_sz_split_chunks(const SzLayout L, const SzChunk *__restrict__ desc, const uint32_t *__restrict__ wave_chunk, uint64_t nwaves,
                  const uint8_t *__restrict__ src, uint8_t *__restrict__ work)
{
    SzChunk D;
    uint64_t m;
    if (!sz_wave_chunk(desc, wave_chunk, nwaves, kSzPlanes, D, m) || m >= D.pixels / 4u) return;
    const uint4 *p = reinterpret_cast<const uint4 *>(src + D.off + m * (4u * WORD));
    uint32_t piece[WORD];
    if constexpr (WORD == 4) {
        const uint4 a = p[0];
        sz_transpose4(a.x, a.y, a.z, a.w, piece);
    } else {
        const uint4 a = p[0], b = p[1];
        sz_transpose4(a.x, a.z, b.x, b.z, piece);
        sz_transpose4(a.y, a.w, b.y, b.w, piece + 4);
    }
#pragma unroll
    for (int j = 0; j < WORD; j++) *reinterpret_cast<uint32_t *>(work + sz_piece_at(L, D, (uint32_t)j, m)) = piece[j];
}

template <int WORD>
__global__ void __launch_bounds__(kSzBlock)
k_sz_merge_chunks(const SzLayout L, const SzChunk *__restrict__ desc, const uint32_t *__restrict__ wave_chunk, uint64_t nwaves,
                  const uint8_t *__restrict__ work, uint8_t *__restrict__ dst)
{
    SzChunk D;
    uint64_t m;
    if (!sz_wave_chunk(desc, wave_chunk, nwaves, kSzPlanes, D, m) || m >= D.pixels / 4u) return;
    uint32_t piece[WORD];
#pragma unroll
    for (int j = 0; j < WORD; j++) piece[j] = *reinterpret_cast<const uint32_t *>(work + sz_piece_at(L, D, (uint32_t)j, m));
    uint4 *p = reinterpret_cast<uint4 *>(dst + D.off + m * (4u * WORD));
    uint32_t lo[4];
    sz_transpose4(piece[0], piece[1], piece[2], piece[3], lo);
    if constexpr (WORD == 4) {
        p[0] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    } else {
        uint32_t hi[4];
        sz_transpose4(piece[4], piece[5], piece[6], piece[7], hi);
        p[0] = make_uint4(lo[0], hi[0], lo[1], hi[1]);
        p[1] = make_uint4(lo[2], hi[2], lo[3], hi[3]);
    }
}

// the padding of the plane path's chunks: the chunk's wavefronts take its scan lines in turn, a lane writes 4 bytes
__global__ void __launch_bounds__(kSzBlock)
k_sz_fill_chunks(const SzLayout L, const SzChunk *__restrict__ desc, const uint32_t *__restrict__ wave_chunk, uint64_t nwaves,
                 const uint8_t *__restrict__ src, uint8_t *__restrict__ work)
{
    SzChunk D;
    uint64_t lane;
    if (!sz_wave_chunk(desc, wave_chunk, nwaves, kSzPlanes, D, lane) || D.coder_bytes == D.coded_bytes) return;
    SzInCursor c;
    c.chunk = 0;
    for (c.l = lane >> 6; c.l < D.lines; c.l += sz_quad_waves(D)) {
        c.take = sz_take(L, D, c.l);
        uint8_t *row = work + D.work_off + c.l * L.padded_line;
        for (uint64_t k = c.take + 4u * (lane & 63u); k < L.padded_line; k += 4u * 64u) {
            uint32_t w = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                c.k = k + i;
                w |= (uint32_t)sz_in_byte(L, D, src, c) << (8 * i);
            }
            *reinterpret_cast<uint32_t *>(row + k) = w;
        }
    }
}

int layout_of(const SZ_com_t *sz, size_t chunk_bytes, SzLayout *L)
{
    if (!sz) return RC_CONF_ERROR;
    return sz_make_layout(sz->options_mask, sz->bits_per_pixel, sz->pixels_per_block, sz->pixels_per_scanline, chunk_bytes, L);
}

aec_gpu_params coder_of(const SzLayout &L, bool for_encode)
{
    return aec_gpu_params{L.bps, L.bs, L.rsi, for_encode ? L.flags : L.flags & ~(uint32_t)F_NOT_ENFORCE};
}

bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

uint32_t blocks_for(uint64_t items) { return (uint32_t)((items + kSzBlock - 1) / kSzBlock); }

int marshal(const SzLayout &L, const uint8_t *src, uint64_t n, uint8_t *out, hipStream_t st)
{
    if (!src || !out || !aligned(out, 16)) return RC_CONF_ERROR;
    if (n == 0) return RC_OK;
    (void)hipGetLastError();
    if (sz_planes_fast(L) && aligned(src, 16)) {
        const uint64_t nquads = n * (L.pixels / 4u);
        if (L.word == 4) hipLaunchKernelGGL(k_sz_split<4>, dim3(blocks_for(nquads)), dim3(kSzBlock), 0, st, L, src, out, nquads);
        else hipLaunchKernelGGL(k_sz_split<8>, dim3(blocks_for(nquads)), dim3(kSzBlock), 0, st, L, src, out, nquads);
        if (L.coder_bytes != L.coded_bytes)
            hipLaunchKernelGGL(k_sz_fill, dim3((uint32_t)(n * L.lines)), dim3(64), 0, st, L, src, out);
    } else {
        const uint64_t total = n * L.coder_bytes;
        hipLaunchKernelGGL(k_sz_marshal, dim3(blocks_for((total + 15) / 16)), dim3(kSzBlock), 0, st, L, src, out, total, 0u);
    }
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

int unmarshal(const SzLayout &L, const uint8_t *coder_out, uint64_t n, uint8_t *dst, hipStream_t st)
{
    if (!coder_out || !dst) return RC_CONF_ERROR;
    if (n == 0) return RC_OK;
    (void)hipGetLastError();
    if (sz_planes_fast(L) && aligned(dst, 16) && aligned(coder_out, 4)) {
        const uint64_t nquads = n * (L.pixels / 4u);
        if (L.word == 4) hipLaunchKernelGGL(k_sz_merge<4>, dim3(blocks_for(nquads)), dim3(kSzBlock), 0, st, L, coder_out, dst, nquads);
        else hipLaunchKernelGGL(k_sz_merge<8>, dim3(blocks_for(nquads)), dim3(kSzBlock), 0, st, L, coder_out, dst, nquads);
    } else {
        const uint64_t total = n * L.chunk_bytes;
        const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
        hipLaunchKernelGGL(k_sz_unmarshal, dim3(blocks_for((head + total + 15) / 16)), dim3(kSzBlock), 0, st, L, coder_out,
                           dst, total, head);
    }
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

// n chunks of this layout in one call: at most 32 GiB either way and 2^25 scan lines, so that no launch above counts
// beyond 2^31 lanes
bool sizes_ok(const SzLayout &L, uint64_t n)
{
    const uint64_t most = L.coder_bytes > L.chunk_bytes ? L.coder_bytes : L.chunk_bytes;
    return n <= (1ull << 35) / most && n <= (1ull << 25) / L.lines;
}

// ---- batches of unequal chunks: host side ---------------------------------------------------------------------------------
// No launch counts beyond 2^31 lanes: the wavefronts of a batch -- per chunk, the 16-byte groups of the larger of its
// coder bytes and its chunk bytes behind a head of 15, rounded up to whole wavefronts; the plane path's quads are never
// more than these -- are at most 2^25, and a chunk has less than 2^35 bytes.
constexpr uint64_t kSzMaxWaves = 1ull << 25, kSzMaxChunk = 1ull << 35;

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// host arithmetic of a batch under one SZ_com_t: the plan, and (each optional, n entries) the chunks' rooms and coder
// sizes.  false = refused.
bool chunks_shape(const SZ_com_t *sz, const uint64_t *chunk_bytes, uint64_t n, SzLayout *L, aec_gpu_sz_chunks_plan_t *plan,
                  uint64_t *work_offsets, uint64_t *coder_bytes)
{
    if (layout_of(sz, 64, L) != RC_OK || (n && !chunk_bytes) || n > 0x7FFFFFFFull) return false;   // (64: whole pixels of any width)
    std::unique_ptr<uint64_t[]> own;
    if (!coder_bytes && n) {
        own.reset(new (std::nothrow) uint64_t[n]);
        if (!(coder_bytes = own.get())) return false;
    }
    uint64_t work = 0, waves = 0;
    unsigned direct = 1;
    for (uint64_t i = 0; i < n; i++) {
        SzChunk D;
        if (chunk_bytes[i] >= kSzMaxChunk || !sz_chunk_sizes(*L, chunk_bytes[i], D)) return false;
        if (work_offsets) work_offsets[i] = work;
        coder_bytes[i] = D.coder_bytes;
        work += (D.coder_bytes + 15u) & ~(uint64_t)15u;
        waves += sz_group_waves(D.coder_bytes > D.chunk_bytes ? D.coder_bytes : D.chunk_bytes, 15u);
        if (waves > kSzMaxWaves) return false;
        direct &= sz_chunk_passthrough(*L, D) ? 1u : 0u;
    }
    const aec_gpu_params p = coder_of(*L, true);
    aec_gpu_chunks_plan cp;
    if (!aec_gpu_encode_chunks_plan(&p, coder_bytes, n, &cp)) return false;
    plan->coder = p;
    plan->work_bytes = (size_t)work;
    plan->out_bound = cp.out_bound;
    plan->rsi_entries = cp.rsi_entries;
    plan->workspace_bytes = cp.workspace_bytes + up256((size_t)(n + 1) * sizeof(SzChunk)) + up256((size_t)(waves ? waves : 1) * 4);
    plan->direct = direct;
    return true;
}

bool all_aligned(const void *base, const uint64_t *offsets, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++)
        if ((reinterpret_cast<uintptr_t>(base) + offsets[i]) & 15u) return false;
    return true;
}

// the descriptors of a batch on the device and the wavefront table behind them, filled (one transfer, one launch)
struct SzChunksOnDevice {
    const SzChunk *desc;
    const uint32_t *wave_chunk;         // the byte path's wavefronts, then the plane path's
    uint64_t waves[2];
    bool fill;                          // a chunk of the plane path has padding
};

int send_chunks(aec_gpu_ctx *ctx, const SzLayout &L, const void *base, const uint64_t *offsets, const uint64_t *chunk_bytes,
                uint64_t n, bool unmarshal, hipStream_t st, SzChunksOnDevice *on)
{
    const size_t h_need = (size_t)(n + 1) * sizeof(SzChunk);
    void *h = nullptr;
    void *stage = ctx_sz_stage(ctx, h_need, &h);
    if (!stage) return RC_MEM_ERROR;
    SzChunk *d = static_cast<SzChunk *>(h);
    if (!sz_make_chunks(L, reinterpret_cast<uintptr_t>(base), offsets, chunk_bytes, n, unmarshal, d)) return RC_CONF_ERROR;
    on->waves[kSzBytes] = d[n].wave0[kSzBytes];
    on->waves[kSzPlanes] = d[n].wave0[kSzPlanes];
    on->fill = false;
    for (uint64_t i = 0; i < n; i++) on->fill |= d[i].planes && d[i].coder_bytes != d[i].coded_bytes;
    const uint64_t waves = on->waves[kSzBytes] + on->waves[kSzPlanes];
    const size_t desc_bytes = up256(h_need);
    uint8_t *cd = ctx_sz_send(ctx, stage, h_need, desc_bytes + up256((size_t)(waves ? waves : 1) * 4), st);
    if (!cd) return RC_MEM_ERROR;
    on->desc = reinterpret_cast<const SzChunk *>(cd);
    uint32_t *table = reinterpret_cast<uint32_t *>(cd + desc_bytes);
    on->wave_chunk = table;
    if (waves) {
        const uint64_t grid = (waves + 255) / 256;
        hipLaunchKernelGGL(k_sz_chunks_setup, dim3((uint32_t)(grid < 4096 ? grid : 4096)), dim3(256), 0, st, on->desc, n,
                           on->waves[kSzBytes], on->waves[kSzPlanes], table);
    }
    return RC_OK;
}

uint32_t wave_blocks(uint64_t waves) { return (uint32_t)((waves + kSzWaves - 1) / kSzWaves); }

}  // namespace

extern "C" {

int aec_gpu_sz_layout(const SZ_com_t *sz, size_t chunk_bytes, aec_gpu_sz_layout_t *layout)
{
    SzLayout L;
    if (!layout) return RC_CONF_ERROR;
    const int rc = layout_of(sz, chunk_bytes, &L);
    if (rc != RC_OK) return rc;
    layout->coder = coder_of(L, true);
    layout->word = L.word;
    layout->pixel = L.pixel;
    layout->fill_repeat = L.repeat;
    layout->passthrough = L.passthrough;
    layout->line = L.line;
    layout->padded_line = L.padded_line;
    layout->lines = L.lines;
    layout->coder_bytes = L.coder_bytes;
    layout->coded_bytes = L.coded_bytes;
    return RC_OK;
}

int aec_gpu_sz_marshal_async(const SZ_com_t *sz, const void *d_src, size_t chunk_bytes, uint64_t n_chunks, void *d_coder_in,
                             void *stream)
{
    SzLayout L;
    const int rc = layout_of(sz, chunk_bytes, &L);
    if (rc != RC_OK) return rc;
    if (!sizes_ok(L, n_chunks)) return RC_CONF_ERROR;
    return marshal(L, static_cast<const uint8_t *>(d_src), n_chunks, static_cast<uint8_t *>(d_coder_in),
                   static_cast<hipStream_t>(stream));
}

int aec_gpu_sz_unmarshal_async(const SZ_com_t *sz, const void *d_coder_out, size_t chunk_bytes, uint64_t n_chunks, void *d_dst,
                               void *stream)
{
    SzLayout L;
    const int rc = layout_of(sz, chunk_bytes, &L);
    if (rc != RC_OK) return rc;
    if (!sizes_ok(L, n_chunks)) return RC_CONF_ERROR;
    return unmarshal(L, static_cast<const uint8_t *>(d_coder_out), n_chunks, static_cast<uint8_t *>(d_dst),
                     static_cast<hipStream_t>(stream));
}

int aec_gpu_sz_batch_ok(const SZ_com_t *sz, size_t chunk_bytes, uint64_t n_chunks)
{
    SzLayout L;
    if (layout_of(sz, chunk_bytes, &L) != RC_OK || n_chunks == 0 || !sizes_ok(L, n_chunks)) return 0;
    const aec_gpu_params p = coder_of(L, true);
    return aec_gpu_uniform_batch_ok(&p, (size_t)L.coder_bytes, n_chunks);
}

int aec_gpu_sz_compress_batch_async(aec_gpu_ctx *ctx, const SZ_com_t *sz, const void *d_src, size_t chunk_bytes,
                                    uint64_t n_chunks, void *d_work, void *d_out, size_t out_cap, aec_gpu_batch_chunk *d_chunks,
                                    aec_gpu_enc_result *d_result, void *stream)
{
    SzLayout L;
    int rc = layout_of(sz, chunk_bytes, &L);
    if (rc != RC_OK) return rc;
    if (!ctx || !d_src || !aec_gpu_sz_batch_ok(sz, chunk_bytes, n_chunks)) return RC_CONF_ERROR;
    const aec_gpu_params p = coder_of(L, true);
    const void *coder_in = d_src;
    if (!L.passthrough) {
        rc = marshal(L, static_cast<const uint8_t *>(d_src), n_chunks, static_cast<uint8_t *>(d_work),
                     static_cast<hipStream_t>(stream));
        if (rc != RC_OK) return rc;
        coder_in = d_work;
    }
    return aec_gpu_encode_uniform_batch_async(ctx, &p, coder_in, (size_t)L.coder_bytes, n_chunks, d_out, out_cap, d_chunks,
                                              d_result, stream);
}

int aec_gpu_sz_decompress_batch_async(aec_gpu_ctx *ctx, const SZ_com_t *sz, const void *d_in, size_t in_bytes,
                                      const uint64_t *d_chunk_offsets, uint64_t n_chunks, size_t chunk_bytes,
                                      uint64_t *d_rsi_bit_offsets, void *d_work, void *d_dst, aec_gpu_dec_result *d_results,
                                      aec_gpu_dec_result *d_result, void *stream)
{
    SzLayout L;
    int rc = layout_of(sz, chunk_bytes, &L);
    if (rc != RC_OK) return rc;
    if (!ctx || !d_dst || !sizes_ok(L, n_chunks)) return RC_CONF_ERROR;
    const aec_gpu_params p = coder_of(L, false);
    const bool direct = L.passthrough && aligned(d_dst, 16);
    if (!direct && (!d_work || !aligned(d_work, 16))) return RC_CONF_ERROR;
    void *coder_out = direct ? d_dst : d_work;
    rc = aec_gpu_decode_batch_async(ctx, &p, d_in, in_bytes, d_chunk_offsets, n_chunks, L.lines, d_rsi_bit_offsets, coder_out,
                                    d_results, d_result, stream);
    if (rc != RC_OK || direct) return rc;
    return unmarshal(L, static_cast<const uint8_t *>(d_work), n_chunks, static_cast<uint8_t *>(d_dst),
                     static_cast<hipStream_t>(stream));
}

int aec_gpu_sz_chunks_plan(const SZ_com_t *sz, const uint64_t *chunk_bytes, uint64_t n_chunks, aec_gpu_sz_chunks_plan_t *plan,
                           uint64_t *work_offsets)
{
    SzLayout L;
    return plan && chunks_shape(sz, chunk_bytes, n_chunks, &L, plan, work_offsets, nullptr) ? 1 : 0;
}

int aec_gpu_sz_compress_chunks_async(aec_gpu_ctx *ctx, const SZ_com_t *sz, const void *d_src, const uint64_t *src_offsets,
                                     const uint64_t *chunk_bytes, uint64_t n_chunks, void *d_work, void *d_out, size_t out_cap,
                                     aec_gpu_batch_chunk *d_chunks, uint64_t *d_rsi_bit_offsets, aec_gpu_enc_result *d_result,
                                     void *stream)
{
    SzLayout L;
    if (layout_of(sz, 64, &L) != RC_OK) return RC_CONF_ERROR;
    if (n_chunks == 0) return RC_OK;
    if (!ctx || !d_src || !src_offsets || !chunk_bytes || !d_out || !d_chunks || !d_result || !aligned(d_out, 16) ||
        (out_cap & 15u) || out_cap < 16 || n_chunks > 0x7FFFFFFFull)
        return RC_CONF_ERROR;
    // (host arrays of the call: coder sizes, rooms, and the chunks' offsets from a 16-byte aligned base when coded in place)
    std::unique_ptr<uint64_t[]> arrays(new (std::nothrow) uint64_t[3 * n_chunks]);
    if (!arrays) return RC_MEM_ERROR;
    uint64_t *coder_bytes = arrays.get(), *work_offsets = coder_bytes + n_chunks, *in_place = work_offsets + n_chunks;
    aec_gpu_sz_chunks_plan_t plan;
    if (!chunks_shape(sz, chunk_bytes, n_chunks, &L, &plan, work_offsets, coder_bytes)) return RC_CONF_ERROR;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t *src = static_cast<const uint8_t *>(d_src);
    if (plan.direct && all_aligned(d_src, src_offsets, n_chunks)) {
        const uint64_t skew = reinterpret_cast<uintptr_t>(d_src) & 15u;
        for (uint64_t i = 0; i < n_chunks; i++) in_place[i] = src_offsets[i] + skew;
        return aec_gpu_encode_chunks_async(ctx, &plan.coder, src - skew, in_place, coder_bytes, n_chunks, d_out, out_cap,
                                           d_chunks, d_rsi_bit_offsets, d_result, stream);
    }
    if (!d_work || !aligned(d_work, 16)) return RC_CONF_ERROR;
    uint8_t *work = static_cast<uint8_t *>(d_work);
    SzChunksOnDevice on;
    const int rc = send_chunks(ctx, L, d_src, src_offsets, chunk_bytes, n_chunks, false, st, &on);
    if (rc != RC_OK) return rc;
    const uint64_t nb = on.waves[kSzBytes], np = on.waves[kSzPlanes];
    if (np) {
        if (L.word == 4)
            hipLaunchKernelGGL(k_sz_split_chunks<4>, dim3(wave_blocks(np)), dim3(kSzBlock), 0, st, L, on.desc, on.wave_chunk + nb, np, src, work);
        else
            hipLaunchKernelGGL(k_sz_split_chunks<8>, dim3(wave_blocks(np)), dim3(kSzBlock), 0, st, L, on.desc, on.wave_chunk + nb, np, src, work);
        if (on.fill)
            hipLaunchKernelGGL(k_sz_fill_chunks, dim3(wave_blocks(np)), dim3(kSzBlock), 0, st, L, on.desc, on.wave_chunk + nb, np, src, work);
    }
    if (nb)
        hipLaunchKernelGGL(k_sz_marshal_chunks, dim3(wave_blocks(nb)), dim3(kSzBlock), 0, st, L, on.desc, on.wave_chunk, nb, src, work);
    if (hipGetLastError() != hipSuccess) return RC_MEM_ERROR;
    return aec_gpu_encode_chunks_async(ctx, &plan.coder, d_work, work_offsets, coder_bytes, n_chunks, d_out, out_cap, d_chunks,
                                       d_rsi_bit_offsets, d_result, stream);
}

int aec_gpu_sz_decompress_chunks_async(aec_gpu_ctx *ctx, const SZ_com_t *sz, const void *d_in, size_t in_bytes,
                                       const uint64_t *in_offsets, const uint64_t *in_bytes_each, const uint64_t *dst_offsets,
                                       const uint64_t *chunk_bytes, uint64_t n_chunks, uint64_t *d_rsi_bit_offsets,
                                       int have_table, void *d_work, void *d_dst, aec_gpu_dec_result *d_results,
                                       aec_gpu_dec_result *d_result, void *stream)
{
    SzLayout L;
    if (layout_of(sz, 64, &L) != RC_OK) return RC_CONF_ERROR;
    if (n_chunks == 0) return RC_OK;
    if (!ctx || !d_in || !d_dst || !dst_offsets || !chunk_bytes || n_chunks > 0x7FFFFFFFull) return RC_CONF_ERROR;
    std::unique_ptr<uint64_t[]> arrays(new (std::nothrow) uint64_t[3 * n_chunks]);
    if (!arrays) return RC_MEM_ERROR;
    uint64_t *coder_bytes = arrays.get(), *work_offsets = coder_bytes + n_chunks, *in_place = work_offsets + n_chunks;
    aec_gpu_sz_chunks_plan_t plan;
    if (!chunks_shape(sz, chunk_bytes, n_chunks, &L, &plan, work_offsets, coder_bytes)) return RC_CONF_ERROR;
    const aec_gpu_params p = coder_of(L, false);
    uint8_t *dst = static_cast<uint8_t *>(d_dst);
    if (plan.direct && all_aligned(d_dst, dst_offsets, n_chunks)) {
        const uint64_t skew = reinterpret_cast<uintptr_t>(d_dst) & 15u;
        for (uint64_t i = 0; i < n_chunks; i++) in_place[i] = dst_offsets[i] + skew;
        return aec_gpu_decode_chunks_async(ctx, &p, d_in, in_bytes, in_offsets, in_bytes_each, in_place, coder_bytes, n_chunks,
                                           d_rsi_bit_offsets, have_table, dst - skew, d_results, d_result, stream);
    }
    if (!d_work || !aligned(d_work, 16)) return RC_CONF_ERROR;
    int rc = aec_gpu_decode_chunks_async(ctx, &p, d_in, in_bytes, in_offsets, in_bytes_each, work_offsets, coder_bytes, n_chunks,
                                         d_rsi_bit_offsets, have_table, d_work, d_results, d_result, stream);
    if (rc != RC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t *work = static_cast<const uint8_t *>(d_work);
    SzChunksOnDevice on;
    rc = send_chunks(ctx, L, d_dst, dst_offsets, chunk_bytes, n_chunks, true, st, &on);
    if (rc != RC_OK) return rc;
    const uint64_t nb = on.waves[kSzBytes], np = on.waves[kSzPlanes];
    if (np) {
        if (L.word == 4)
            hipLaunchKernelGGL(k_sz_merge_chunks<4>, dim3(wave_blocks(np)), dim3(kSzBlock), 0, st, L, on.desc, on.wave_chunk + nb, np, work, dst);
        else
            hipLaunchKernelGGL(k_sz_merge_chunks<8>, dim3(wave_blocks(np)), dim3(kSzBlock), 0, st, L, on.desc, on.wave_chunk + nb, np, work, dst);
    }
    if (nb)
        hipLaunchKernelGGL(k_sz_unmarshal_chunks, dim3(wave_blocks(nb)), dim3(kSzBlock), 0, st, L, on.desc, on.wave_chunk, nb, work, dst);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

}  // extern "C"
