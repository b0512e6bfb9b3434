// aec_est.h -- the arithmetic of aec_gpu_estimate_async: the exact stream length of one input under block sizes
// 8, 16, 32 and 64 from ONE pass over the samples.  No reference counterpart (the reference codes; it does not estimate).
//
// What makes one pass enough ("Estimate"):
//   * the mapped residual of a sample depends on the sample and its predecessor only, so it is the same under every block
//     size -- except in the slot that starts an RSI of that size, which holds 0 there (the raw sample goes out as the
//     reference sample) and the ordinary residual under the three other sizes;
//   * blocks of every size are aligned to their own size from sample 0, so 64 samples from a multiple of 64 -- a PIECE --
//     hold exactly 8 / 4 / 2 / 1 blocks of sizes 8 / 16 / 32 / 64, and a lane that holds a piece holds whole blocks only;
//   * a block's length does not depend on the k carried into it: it is id_len + ref * bps + min(split, second extension,
//     uncompressed), the split term the minimum of the convex fs(k) + n(k + 1);
//   * zero blocks only form runs inside a 64-block segment of their own size's RSI, which is the second, small pass.
// est_piece() is what one lane of k_est_blocks does, est_seg_lane() what one lane of k_est_sum does; both are
// __host__ __device__ and run block by block on the CPU in tests/emul/est_emul.cpp.
#pragma once
#include "aec_cfg.h"
#include "aec_lane.h"

namespace aec {

constexpr uint32_t kEstSizes = 4;          // block sizes 8 << i
constexpr uint32_t kEstPiece = 64;         // samples per piece
constexpr uint32_t kEstZero = 0x8000u;     // record of an all-zero block; any other record is the block's length in bits

// the public record (include/aec_gpu.h: aec_gpu_estimate)
struct EstResult {
    uint64_t total_bits[kEstSizes];
    uint32_t best;
    uint32_t pad;
};

// One call: the parameters that all candidates share (c: block_size 8, rsi unused) and, per size, the RSI in blocks
// (0: not evaluated), the counts that follow from it and where its records lie in the workspace.
struct EstCfg {
    Cfg c;
    uint32_t rsi[kEstSizes];
    uint32_t segs_per_rsi[kEstSizes];
    uint64_t blocks[kEstSizes];        // ceil(samples / (8 << i)): the last block is padded (encode.c:676-684)
    uint64_t segs[kEstSizes];          // segments of 64 blocks of this size's RSIs (the last of an RSI may be short)
    uint64_t rec_off[kEstSizes];       // byte offset of the size's records: pieces * (64 / size) of 16 bits
    uint64_t pieces;                   // ceil(samples / 64)
    uint32_t mask;                     // bit i: size i is evaluated
    uint32_t pad;
};

// RC_OK, or RC_CONF_ERROR where a candidate asked for is refused or none is asked for.  rsi == nullptr: rsi_all for all.
inline int make_est_cfg(uint32_t bps, uint32_t flags, const unsigned int *rsi, uint32_t rsi_all, size_t in_bytes,
                        EstCfg *e, size_t *workspace_bytes)
{
    *e = EstCfg{};
    size_t off = 0;
    for (uint32_t i = 0; i < kEstSizes; i++) {
        const uint32_t r = rsi ? rsi[i] : rsi_all;
        if (r == 0) {
            if (!rsi) return RC_CONF_ERROR;
            continue;
        }
        Cfg c;
        const int rc = make_cfg(bps, 8u << i, r, flags, in_bytes, true, &c);
        if (rc != RC_OK) return rc;
        e->mask |= 1u << i;
        e->rsi[i] = r;
        e->segs_per_rsi[i] = c.segs_per_rsi;
        e->blocks[i] = c.total_blocks;
        e->segs[i] = c.total_segs;
        e->c = c;
        e->pieces = (c.total_samples + kEstPiece - 1) / kEstPiece;
        e->rec_off[i] = off;
        off += (size_t)((e->pieces * (kEstPiece >> (3 + i)) * 2u + 15u) & ~(uint64_t)15);
    }
    if (!e->mask) return RC_CONF_ERROR;
    e->c.bs = 8;
    e->c.rsi = 0;
    e->c.segs_per_rsi = 0;
    e->c.total_blocks = e->c.total_segs = e->c.rsi_count = 0;
    if (workspace_bytes) *workspace_bytes = off;
    return RC_OK;
}

// ---- samples of a piece as they lie in memory: `row` = its 64 * BYTES bytes as little-endian 32-bit words ------------
// byte order of a loaded word: both 16-bit halves (BYTES == 2) or the whole word (BYTES == 4) of MSB data
AEC_HD uint32_t est_swap16x2(uint32_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, w, 0x02030001u);
#else
    return ((w & 0x00FF00FFu) << 8) | ((w >> 8) & 0x00FF00FFu);
#endif
}
AEC_HD uint32_t est_swap32(uint32_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, w, 0x00010203u);
#else
    return bswap32(w);
#endif
}

template <int BYTES>
AEC_HD uint32_t est_sample(const uint32_t *row, uint32_t i, bool msb)
{
    if (BYTES == 1) return (row[i / 4u] >> (8u * (i % 4u))) & 0xFFu;
    if (BYTES == 2) {
        const uint32_t w = msb ? est_swap16x2(row[i / 2u]) : row[i / 2u];
        return (i & 1u) ? w >> 16 : w & 0xFFFFu;
    }
    if (BYTES == 4) return msb ? est_swap32(row[i]) : row[i];
    const uint32_t o = 3u * i, q = o / 4u, sh = 8u * (o % 4u);      // three bytes from one word or across two
    const uint32_t lo = row[q], hi = sh > 8u ? row[q + 1u] : 0u;     // (sample 63 ends with the row's last word)
    const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & 0xFFFFFFu;
    return msb ? est_swap32(v) >> 8 : v;
}

// ---- one block ---------------------------------------------------------------------------------------------------------
// The split option's minimum over a window of four k: with ks = bit_length(fs(0)) - bit_length(n) - 2 (aec_lane.h
// assess_split_with starts its climb there), fs(ks) < 8n, so fs(ks + 3) < n and the climb, which goes on while
// fs(k) - fs(k + 1) > n, has stopped by ks + 3: the minimum of the convex length lies in [ks, ks + 3], and the plain
// minimum over those k -- no compare-and-branch per step -- is the length the climb returns.  Every sample >> ks is below
// 8n <= 512 (or below 8 where ks was clamped to kmax), so the four sums fit 32 bits whatever the sample width: only fs(0)
// needs 64.
AEC_HD uint32_t est_ks(uint64_t s0, uint32_t n, uint32_t kmax)
{
    int ks = bit_length64(s0) - bit_length64(n) - 2;
    if (ks < 0) ks = 0;
    return (uint32_t)ks > kmax ? kmax : (uint32_t)ks;
}
AEC_HD uint32_t est_window_min(const uint32_t f[4], uint32_t ks, uint32_t n, uint32_t kmax)
{
    uint32_t best = f[0] + n * (ks + 1u);
#pragma unroll
    for (uint32_t t = 1; t < 4u; t++) {
        const uint32_t len = f[t] + n * (ks + t + 1u);
        best = (ks + t <= kmax && len < best) ? len : best;
    }
    return best;
}

// Samples of more than 16 bits: d = the piece's 64 residuals, the block is d[START .. START + N).
template <int N, int START>
AEC_HD uint32_t est_block_wide(const uint32_t *d, const Cfg &c, uint32_t ref)
{
    uint32_t b[N];
    uint32_t any = 0;
    uint64_t s0 = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        b[i] = (i == 0 && ref) ? 0u : d[START + i];        // the reference slot holds 0 (encode.c:254)
        any |= b[i];
        s0 += b[i];
    }
    if (any == 0) return kEstZero;
    const uint32_t n = (uint32_t)N - ref;
    uint32_t split_len = 0xFFFFFFFFu;
    if (c.id_len > 1) {
        const uint32_t ks = est_ks(s0, n, c.kmax);
        uint32_t f[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < N; i++) {
            const uint32_t t = b[i] >> ks;
            f[0] += t; f[1] += t >> 1; f[2] += t >> 2; f[3] += t >> 3;
        }
        split_len = est_window_min(f, ks, n, c.kmax);
    }
    // Second extension, the length aec_lane.h's assess_se gives.  Its limit is at most 64 x 32 bits, which one residual of
    // 64 and more exceeds by itself ((s + 1) s / 2 >= 2080 for the pair sum s it is part of): the option is out unless every
    // residual is below 64 -- then nothing wraps and the in-order sum with its early exit is the plain sum -- or unless a
    // pair sums to 2^32 and more, whose 64-bit product wraps in the reference (encode.c:428-429): those blocks, entered
    // once per wavefront and practically never, go through assess_se itself.
    const uint32_t limit = n * c.bps;
    uint32_t se_len = 0xFFFFFFFFu, wraps = 0;
#pragma unroll
    for (int i = 0; i < N; i += 2) wraps |= (b[i] + b[i + 1] < b[i]) ? 1u : 0u;
    if (AEC_ANY(any < 64u)) {
        uint32_t len = 1;
#pragma unroll
        for (int i = 0; i < N; i += 2) {
            const uint32_t s = b[i] + b[i + 1];
            len += s * (s + 1u) / 2u + b[i + 1] + 1u;
        }
        if (any < 64u && len <= limit) se_len = len;
    }
    if (AEC_ANY(wraps != 0u)) {
        if (wraps) se_len = assess_se<N>(b, (uint32_t)N, limit);
    }
    return choose_from(c, (uint32_t)N, ref, split_len, se_len, 0u, 0u).bits;
}

// Samples of at most 16 bits: w = the piece as 32 words of two residuals each (stream order: low half first); the block is
// words [START / 2, (START + N) / 2).  fs(k) is one packed shift and one dot product per pair and k (v_pk_lshrrev_b16,
// v_dot2_u32_u16), the second extension the closed form of the encoder's choose_option_pk: the reference's running sum
// passes the limit exactly when the whole sum does, the whole sum is 1 + (sum s^2 + sum s) / 2 + sum b + pairs, and a pair
// sum of 2^13 and more is beyond any limit by itself.
#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short est_u16x2 __attribute__((ext_vector_type(2)));
AEC_HD uint32_t est_pk_shr(uint32_t w, uint32_t k)
{
    const est_u16x2 kk = {(unsigned short)k, (unsigned short)k};
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(est_u16x2, w) >> kk);
}
AEC_HD uint32_t est_dot2(uint32_t w, uint32_t m, uint32_t acc)
{
    return __builtin_amdgcn_udot2(__builtin_bit_cast(est_u16x2, w), __builtin_bit_cast(est_u16x2, m), acc, false);
}
#else
AEC_HD uint32_t est_pk_shr(uint32_t w, uint32_t k) { return ((w & 0xFFFFu) >> k) | (((w >> 16) >> k) << 16); }
AEC_HD uint32_t est_dot2(uint32_t w, uint32_t m, uint32_t acc)
{
    return acc + (w & 0xFFFFu) * (m & 0xFFFFu) + (w >> 16) * (m >> 16);
}
#endif

template <int N, int START>
AEC_HD uint32_t est_block_pk(const uint32_t *w, const Cfg &c, uint32_t ref)
{
    constexpr uint32_t ONES = 0x00010001u, SECOND = 0x00010000u;
    uint32_t b[N / 2];
    uint32_t any = 0, s0 = 0, s_sq = 0, s_b = 0, s_or = 0;
#pragma unroll
    for (int j = 0; j < N / 2; j++) {
        b[j] = (j == 0 && ref) ? w[START / 2] & 0xFFFF0000u : w[START / 2 + j];
        any |= b[j];
        const uint32_t sum = est_dot2(b[j], ONES, 0u);
        s_or |= sum;
        s0 += sum;
        s_sq += (sum & 0xFFFFFFu) * (sum & 0xFFFFFFu);      // (sum < 2^13 wherever the result is used)
        s_b = est_dot2(b[j], SECOND, s_b);
    }
    if (any == 0) return kEstZero;
    const uint32_t n = (uint32_t)N - ref;
    uint32_t split_len = 0xFFFFFFFFu;
    if (c.id_len > 1) {
        const uint32_t ks = est_ks(s0, n, c.kmax);
        uint32_t f[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < N / 2; j++) {
            uint32_t t = est_pk_shr(b[j], ks);
            f[0] = est_dot2(t, ONES, f[0]);
            t = est_pk_shr(t, 1u); f[1] = est_dot2(t, ONES, f[1]);
            t = est_pk_shr(t, 1u); f[2] = est_dot2(t, ONES, f[2]);
            t = est_pk_shr(t, 1u); f[3] = est_dot2(t, ONES, f[3]);
        }
        split_len = est_window_min(f, ks, n, c.kmax);
    }
    const uint32_t len = 1u + (s_sq + s0) / 2u + s_b + (uint32_t)N / 2u;
    const bool over = (s_or >> 13) != 0u || len > n * c.bps;
    return choose_from(c, (uint32_t)N, ref, split_len, over ? 0xFFFFFFFFu : len, 0u, 0u).bits;
}

// position of a piece's first block of size i inside its RSI (32-bit division whenever possible)
AEC_HD uint32_t est_first_in_rsi(uint64_t piece, uint32_t i, uint32_t rsi)
{
    const uint64_t b0 = piece * (kEstPiece >> (3u + i));
    return (b0 >> 32) ? (uint32_t)(b0 % rsi) : (uint32_t)b0 % rsi;
}

// records of the 64 / N blocks of one piece into out16[J ...]; r = block J's position in its RSI
template <int N, bool PK, int J = 0>
AEC_HD void est_blocks(const uint32_t *d, const Cfg &c, bool pp, uint32_t r, uint32_t rsi, uint16_t *out16)
{
    if constexpr (J < 64 / N) {
        const uint32_t ref = (pp && r == 0) ? 1u : 0u;
        if constexpr (PK) out16[J] = (uint16_t)est_block_pk<N, J * N>(d, c, ref);
        else out16[J] = (uint16_t)est_block_wide<N, J * N>(d, c, ref);
        est_blocks<N, PK, J + 1>(d, c, pp, r + 1u == rsi ? 0u : r + 1u, rsi, out16);
    }
}

// One piece.  row: its bytes as est_sample reads them, the samples behind the end of the input filled with the last one
// (encode.c:676-684); prev: the sample in front of the piece in host order (any value for piece 0).  rec[0..8) receive the
// records of the blocks of 8, rec[8..12) of 16, rec[12..14) of 32, rec[14] of 64; the records of a size that is not
// evaluated, and of blocks behind that size's last block, are not meaningful.
template <int BYTES>
AEC_HD void est_piece(const EstCfg &e, const uint32_t *row, uint32_t prev, uint64_t piece, uint16_t rec[16])
{
    constexpr bool PK = BYTES <= 2;
    const Cfg &c = e.c;
    const bool msb = c.flags & F_MSB, pp = c.flags & F_PREPROCESS;
    uint32_t d[PK ? 32 : 64];
    uint32_t last = prev;
#pragma unroll
    for (uint32_t i = 0; i < kEstPiece; i++) {
        const uint32_t x = est_sample<BYTES>(row, i, msb);
        uint32_t v = pp ? pp_any(last, x, c) : x;
        if (i == 0 && piece == 0) v = pp ? 0u : x;       // sample 0 has nothing in front of it: a reference slot for every size
        last = x;
        if (PK) {
            v &= 0xFFFFu;
            if (i & 1u) d[i / 2u] |= v << 16; else d[i / 2u] = v;
        } else {
            d[i] = v;
        }
    }
    if (e.rsi[0]) est_blocks<8, PK>(d, c, pp, est_first_in_rsi(piece, 0, e.rsi[0]), e.rsi[0], rec);
    if (e.rsi[1]) est_blocks<16, PK>(d, c, pp, est_first_in_rsi(piece, 1, e.rsi[1]), e.rsi[1], rec + 8);
    if (e.rsi[2]) est_blocks<32, PK>(d, c, pp, est_first_in_rsi(piece, 2, e.rsi[2]), e.rsi[2], rec + 12);
    if (e.rsi[3]) est_blocks<64, PK>(d, c, pp, est_first_in_rsi(piece, 3, e.rsi[3]), e.rsi[3], rec + 14);
}

// ---- the sum over one size's blocks: a segment = 64 consecutive blocks of one RSI of that size ---------------------------
struct EstSeg {
    uint64_t blk0;      // global index of its first block
    uint32_t b0;        // index of its first block inside the RSI (multiple of 64)
    uint32_t nv;        // blocks in the segment (1..64)
};
AEC_HD EstSeg est_seg(const EstCfg &e, uint32_t i, uint64_t sg)
{
    const uint32_t spr = e.segs_per_rsi[i];
    const uint64_t rsi_idx = (sg >> 32) ? sg / spr : (uint64_t)((uint32_t)sg / spr);
    EstSeg g;
    g.b0 = (uint32_t)(sg - rsi_idx * spr) * 64u;
    uint64_t nb = e.blocks[i] - rsi_idx * e.rsi[i];
    if (nb > e.rsi[i]) nb = e.rsi[i];
    const uint64_t left = nb - g.b0;
    g.nv = left < 64 ? (uint32_t)left : 64u;
    g.blk0 = rsi_idx * e.rsi[i] + g.b0;
    return g;
}

// Bits that block `l` of segment g contributes: its record's length, or for a zero block the coded data set of the run it
// starts (id_len + 1 + ref * bps + fs + 1, encode.c:565-583) and nothing where a run that started earlier swallows it.
// zmask: bit j set <=> block j of the segment is a zero block (a __ballot on the device).
AEC_HD uint32_t est_seg_lane(const EstCfg &e, const EstSeg &g, uint32_t l, uint32_t rec, uint64_t zmask)
{
    if (l >= g.nv) return 0;
    if (!(rec & kEstZero)) return rec;
    uint32_t fs = 0;
    const uint32_t run = zero_run_at(zmask, l, g.nv, fs);
    if (!run) return 0;
    const uint32_t ref = ((e.c.flags & F_PREPROCESS) && g.b0 == 0 && l == 0) ? 1u : 0u;
    return e.c.id_len + 1u + ref * e.c.bps + fs + 1u;
}

// index of the smallest total among the sizes asked for; ties: the lowest index
AEC_HD uint32_t est_best(const uint64_t total[kEstSizes], uint32_t mask)
{
    uint32_t best = 0;
    bool have = false;
    for (uint32_t i = 0; i < kEstSizes; i++)
        if (((mask >> i) & 1u) && (!have || total[i] < total[best])) {
            best = i;
            have = true;
        }
    return best;
}

#if defined(__HIPCC__)
// Enqueues the call (aec_est.hip): ws = the workspace of make_est_cfg's size, 16-byte aligned.
void launch_estimate(const EstCfg &e, const uint8_t *d_in, uint8_t *ws, EstResult *d_est, hipStream_t stream);
#endif

}  // namespace aec
