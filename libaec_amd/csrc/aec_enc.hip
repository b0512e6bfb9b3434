// aec_enc.hip -- gfx950 encoder kernels for the CCSDS 121.0-B-2 adaptive entropy coder.
//
// Work decomposition (MI355X: 64-lane wavefronts, 160 KiB LDS per CU):
//   segment  = up to 64 consecutive blocks of one RSI = one wavefront pass, ONE LANE PER BLOCK.
//              It is exactly the CCSDS zero-run segment (reference src/encode.c:649), so zero-block
//              aggregation is a 64-bit ballot per wavefront and never crosses a wavefront.
//   phase A  (lane = 16-byte chunk) coalesced global loads, byte-order fix-up, unit-delay
//            predictor + sign map (reference encode.c:235-311, encode_accessors.c:145-269),
//            results written to padded LDS rows [block][sample].
//   phase B  (lane = block) option / k-plateau / length selection (encode.c:313-434, 585-659).
//
//   k_analyze   phase A+B, writes a 4-byte summary per block and (bits, k clamp) per segment.
//   k_scan_*    device-wide exclusive scan of segment bit lengths (absolute bit offsets) and of
//               the k clamp composition (replaces the serial state->k / state->bits carry).
//               (k_scan_apply also zeroes the few output words that two waves of k_pack share)
//   k_pack      phase A again (input is re-read; the per-block summaries are not recomputed),
//               per-lane bit emission into an LDS image of the segment via ds_or_b32, then a
//               coalesced byte-swapped copy to HBM; only the first/last word of a segment can be
//               shared with a neighbour and uses a global atomic OR.
//
//   k_encode_local / k_encode_redo / k_place   large encodes of blocks held in registers code every block ONCE
//               (aec_enc_local.h): analysis and emission together into a slot per wavefront with a guessed carried k,
//               the scan, the runs whose guess missed coded again, the slots shifted to their places in the stream.
//
//   k_analyze_chunks / k_pack_chunks   the same bodies (aec_enc_analyze.inc / aec_enc_pack.inc) behind a prologue that
//               gives a wave ONE chunk of a batch of unequal chunks; k_chunks_* is the scan that restarts at every
//               chunk (aec_chunks.h).
//
// HBM traffic per input byte: 2 reads of the input + 4/(bs*bytes) summary write+read
// + 1 write of the compressed stream.  Algorithmic bytes are N + C.
//
// Compiled once per templated block size with -DAEC_ENC_PART=<0|8|16|32|64> (k_analyze / k_pack / k_encode_local of that block
// size: objects aec_enc_bs<N>.o) and once without (scans, batch kernels, dispatch), as aec_dec.hip is.
#include <hip/hip_runtime.h>

#include "aec_chunks.h"
#include "aec_enc_local.h"
#include "aec_kernels.h"
#include "aec_lane.h"
#include "aec_tune.h"

namespace aec {

// The launches of one block size's kernels (defined in the object compiled with -DAEC_ENC_PART=BS)
template <int BS> void enc_part(bool pack, const Cfg &c, const uint8_t *in, const EncWorkspace &ws, uint32_t *out_words,
                                uint64_t cap_words, uint32_t fast_ok, hipStream_t st);
struct LocalLaunch {
    uint32_t *image;         // [waves * slot_words]
    uint16_t *seg_first;     // [total_segs] own clamp of the segment's first k-updating block (kLocalNoClamp: none)
    uint8_t *seg_kused;      // [total_segs] the k carried into the segment as k_encode_local had it
    uint32_t slot_words, segs_per_wave, k_in, guess;
};

// (defined for the block sizes that have a DIRECT instantiation: 8, 16, 32)
template <int BS> void enc_part_local(bool redo, const Cfg &c, const uint8_t *in, const EncWorkspace &ws, const LocalLaunch &l,
                                      uint32_t fast_ok, hipStream_t st);

template <int BS> void enc_part_chunks(bool pack, const Cfg &c, const uint8_t *in, const ChunksLaunch &k, const EncWorkspace &ws,
                                       uint32_t *out_words, uint64_t cap_words, uint32_t fast_ok, hipStream_t st);

namespace {

constexpr uint32_t kWave = 64;

// LDS rows [block][sample] of preprocessed samples.  Samples of at most 16 bits are kept as
// uint16 (half the LDS, which is what bounds the waves per CU of k_pack); wider ones as uint32.
// A row is padded by 16 bytes so that one-lane-per-row ds_read_b128 accesses are conflict free.
template <int BS, int BYTES>
struct Rows {
    static constexpr bool HALF = BS > 0 && (BYTES == 1 || BYTES == 2);
    __host__ __device__ static constexpr uint32_t stride_words(uint32_t bs) { return HALF ? bs / 2 + 4 : bs + 4; }
    __device__ static __forceinline__ void put(uint32_t *rows, uint32_t stride_w, uint32_t row, uint32_t col, uint32_t v)
    {
        if (HALF) reinterpret_cast<uint16_t *>(rows + row * stride_w)[col] = (uint16_t)v;
        else rows[row * stride_w + col] = v;
    }
};

__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

struct LdsSink {
    uint32_t *w;
    __device__ __forceinline__ void or_word(uint32_t i, uint32_t v)
    {
        __hip_atomic_fetch_or(&w[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

// Wave-wide inclusive scan on the DPP network (row_shr within 16-lane rows, then row_bcast:15/31
// across rows): six cross-lane moves, no LDS traffic and no waits (the __shfl_up based version
// costs a dozen ds_bpermute round trips per scan).  op(earlier, later) may be non-commutative.
template <class Op>
__device__ __forceinline__ uint32_t wave_scan_dpp(uint32_t v, uint32_t ident, Op op)
{
    uint32_t t;
    t = __builtin_amdgcn_update_dpp(ident, v, 0x111, 0xf, 0xf, false); v = op(t, v);   // row_shr:1
    t = __builtin_amdgcn_update_dpp(ident, v, 0x112, 0xf, 0xf, false); v = op(t, v);   // row_shr:2
    t = __builtin_amdgcn_update_dpp(ident, v, 0x114, 0xf, 0xf, false); v = op(t, v);   // row_shr:4
    t = __builtin_amdgcn_update_dpp(ident, v, 0x118, 0xf, 0xf, false); v = op(t, v);   // row_shr:8
    t = __builtin_amdgcn_update_dpp(ident, v, 0x142, 0xa, 0xf, false); v = op(t, v);   // row_bcast:15
    t = __builtin_amdgcn_update_dpp(ident, v, 0x143, 0xc, 0xf, false); v = op(t, v);   // row_bcast:31
    return v;
}
// value of lane-1 (lane 0 receives `fill`)
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v, uint32_t fill)
{
    return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false);               // wave_shr:1
}
__device__ __forceinline__ uint32_t wave_last(uint32_t v) { return __builtin_amdgcn_readlane(v, 63); }
// a wave-uniform value the optimiser cannot trace to its source from here on (no instruction; it stays a scalar register):
// what is derived from it is computed where it is used and not hoisted to live across a whole loop
__device__ __forceinline__ void uniform_opaque(uint32_t &v) { asm volatile("" : "+s"(v)); }
__device__ __forceinline__ void uniform_opaque(uint64_t &v) { asm volatile("" : "+s"(v)); }
// lane l's 64-bit value, wave-uniform
__device__ __forceinline__ uint64_t wave_get64(uint64_t v, uint32_t l)
{
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), (int)l);     // (the builtin returns an int)
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, (int)l);
    return (uint64_t)hi << 32 | lo;
}
// `v` with lane l's value replaced by `x`
__device__ __forceinline__ uint32_t wave_set_lane(uint32_t v, uint32_t lane, uint32_t l, uint32_t x)
{
    return lane == l ? x : v;
}

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, uint32_t)
{
    return wave_scan_dpp(v, 0u, [](uint32_t a, uint32_t b) { return a + b; });
}

// ordered inclusive scan of k clamps packed as lo | hi << 8
__device__ __forceinline__ uint32_t clamp_pack(KClamp c) { return c.lo | (c.hi << 8); }
__device__ __forceinline__ KClamp clamp_unpack(uint32_t p) { return KClamp{p & 0xFFu, (p >> 8) & 0xFFu}; }

// Inclusive scan of clamp compositions ("first a, then b": both bounds of a are clamped by b).
// Inside the scan a clamp is a pair of 16-bit halves (lo, hi), so one step is two byte permutes
// that replicate b's bounds and a packed max and min -- instead of unpacking, four compares /
// selects and repacking.  In and out: the lo | hi << 8 form of clamp_pack.
__device__ __forceinline__ uint32_t wave_incl_clamp(uint32_t v, uint32_t)
{
    typedef unsigned short cl16x2 __attribute__((ext_vector_type(2)));
    const uint32_t wide = (v & 0xFFu) | ((v & 0xFF00u) << 8);
    const KClamp id = kclamp_identity();
    const uint32_t r = wave_scan_dpp(wide, id.lo | (id.hi << 16), [](uint32_t a, uint32_t b) {
        const uint32_t blo = __builtin_amdgcn_perm(b, b, 0x01000100u), bhi = __builtin_amdgcn_perm(b, b, 0x03020302u);
        const cl16x2 t = __builtin_elementwise_min(
            __builtin_elementwise_max(__builtin_bit_cast(cl16x2, a), __builtin_bit_cast(cl16x2, blo)),
            __builtin_bit_cast(cl16x2, bhi));
        return __builtin_bit_cast(uint32_t, t);
    });
    return (r & 0xFFu) | ((r >> 8) & 0xFF00u);
}

struct Seg {
    uint64_t rsi_idx;   // RSI this segment belongs to
    uint64_t blk0;      // global index of its first block
    uint64_t samp0;     // global index of its first sample
    uint32_t b0;        // index of its first block inside the RSI (multiple of 64)
    uint32_t nv;        // blocks in the segment (1..64)
    bool full;          // every sample of the segment exists (no end-of-data padding)
};

// everything that follows from (RSI, segment inside the RSI)
__device__ __forceinline__ Seg seg_at(const Cfg &c, uint64_t rsi_idx, uint32_t s);

__device__ __forceinline__ Seg seg_geom(const Cfg &c, uint64_t sg)
{
    // 32-bit division whenever possible (a 64-bit one costs ~100 instructions per segment)
    const uint64_t rsi_idx = (sg >> 32) ? sg / c.segs_per_rsi : (uint64_t)((uint32_t)sg / c.segs_per_rsi);
    return seg_at(c, rsi_idx, (uint32_t)(sg - rsi_idx * c.segs_per_rsi));
}

// the segment after g: a wave walks consecutive segments, so the division is paid once per wave
__device__ __forceinline__ Seg seg_next(const Cfg &c, const Seg &g)
{
    const uint32_t s = g.b0 / 64u + 1u;
    return s == c.segs_per_rsi ? seg_at(c, g.rsi_idx + 1, 0u) : seg_at(c, g.rsi_idx, s);
}

__device__ __forceinline__ Seg seg_at(const Cfg &c, uint64_t rsi_idx, uint32_t s)
{
    Seg g;
    g.rsi_idx = rsi_idx;
    g.b0 = s * 64u;
    uint64_t nb = c.total_blocks - g.rsi_idx * c.rsi;
    if (nb > c.rsi) nb = c.rsi;
    const uint64_t left = nb - g.b0;
    g.nv = left < 64 ? (uint32_t)left : 64u;
    g.blk0 = g.rsi_idx * c.rsi + g.b0;
    g.samp0 = g.blk0 * c.bs;
    // "full": every sample exists and the segment is a whole number of 16-byte chunks (a short
    // final RSI may end on half a chunk)
    g.full = g.samp0 + (uint64_t)g.nv * c.bs <= c.total_samples &&
             ((uint64_t)g.nv * c.bs * c.bytes) % 16 == 0;
    return g;
}

// ---- phase A, fast path: whole 16-byte chunks, segment 16-byte aligned in HBM ----------------
// Split into ISSUE (global loads into registers) and FINISH (byte order, predictor, LDS rows) so
// that the loads of segment i+1 are in flight while segment i is analysed / packed: a wavefront
// otherwise exposes a full HBM round trip several times per segment.
template <int BYTES>
__device__ __forceinline__ uint32_t load_sample_raw(const uint8_t *p)
{
    if (BYTES == 1) return *p;
    if (BYTES == 2) return *reinterpret_cast<const uint16_t *>(p);
    return *reinterpret_cast<const uint32_t *>(p);
}

// byte order of a sample loaded with load_sample_raw -- applied where the value is CONSUMED: done
// at the load it makes the prefetch wait for its own data (a full HBM round trip per segment)
template <int BYTES>
__device__ __forceinline__ uint32_t sample_byte_order(uint32_t v, bool msb)
{
    if (BYTES == 1) return v;
    if (BYTES == 2) return msb ? ((v >> 8) | ((v & 0xFFu) << 8)) : v;
    return msb ? bswap32(v) : v;
}

// ---- two 16-bit samples per instruction ------------------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 pk(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t unpk(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }

// The unsigned predictor mapping (reference encode.c:255-269; aec_lane.h pp_unsigned) for both
// halves of a word: prev = the two preceding samples, cur = the two samples, xm = (xmax, xmax).
// With D = |cur - prev|, neg = cur < prev and room = min(prev, xmax - prev) the mapped value is
// 2D - neg while D <= room and room + D beyond; the first grows twice as fast as the second and
// they cross exactly at the switch, so it is min(2D - neg, room + D) -- no compare, no select,
// and everything stays below 2^16 (the doubling saturates, which the min absorbs).
__device__ __forceinline__ uint32_t pp_unsigned_pk(uint32_t prev, uint32_t cur, uint32_t xm)
{
    const u16x2 a = pk(prev), b = pk(cur), one = {1, 1};
    const u16x2 d = __builtin_elementwise_max(a, b) - __builtin_elementwise_min(a, b);
    const u16x2 neg = __builtin_elementwise_min(__builtin_elementwise_sub_sat(a, b), one);
    const u16x2 room = __builtin_elementwise_min(a, pk(xm) - a);
    const u16x2 folded = __builtin_elementwise_add_sat(d, d - neg);
    return unpk(__builtin_elementwise_min(folded, room + d));
}

// The mapped residuals of NW words of sample pairs in stream order (pw; `before` holds the sample in front of them in its
// upper half).  Where nothing can clip -- every step of the stretch is at most the distance between its smallest and its
// largest sample, R, and R fits the room between those and the ends of the range: one test per stretch, wave-wide -- a
// residual is the zigzag of the difference (subtract, shift, sign, exclusive or: 4 packed instructions per pair against
// 11 for pp_unsigned_pk, which the wavefronts with a lane near the ends of the range run as before).  |difference| <= R <=
// xmax / 2 < 2^15, so the difference is exact as a signed 16-bit value and twice it fits 16 bits.
// (try_fast: wave-uniform, the caller's; a stretch that does not pass ends the tests for the caller's remaining stretches
// -- data that lives near an end of its range pays one test per segment, not one per stretch)
template <uint32_t NW>
__device__ __forceinline__ void pp_words_pk(const uint32_t *pw, uint32_t before, uint32_t xm, bool act, uint32_t *out,
                                            bool &try_fast)
{
    typedef short i16x2 __attribute__((ext_vector_type(2)));
    if (!try_fast) {
#pragma unroll
        for (uint32_t j = 0; j < NW; j++)
            out[j] = pp_unsigned_pk(__builtin_amdgcn_alignbit(pw[j], j ? pw[j - 1] : before, 16), pw[j], xm);
        return;
    }
    u16x2 lo = pk((before >> 16) * 0x00010001u), hi = lo;
#pragma unroll
    for (uint32_t j = 0; j < NW; j++) {
        lo = __builtin_elementwise_min(lo, pk(pw[j]));
        hi = __builtin_elementwise_max(hi, pk(pw[j]));
    }
    const uint32_t lo_s = lo.x < lo.y ? lo.x : lo.y, hi_s = hi.x > hi.y ? hi.x : hi.y, range = hi_s - lo_s;
    const bool fits = range <= lo_s && range <= (xm & 0xFFFFu) - hi_s;
    if (!__any(act && !fits)) {
        const u16x2 one = {1, 1}, fifteen = {15, 15};
#pragma unroll
        for (uint32_t j = 0; j < NW; j++) {
            const u16x2 d = pk(pw[j]) - pk(__builtin_amdgcn_alignbit(pw[j], j ? pw[j - 1] : before, 16));
            const i16x2 sign = __builtin_bit_cast(i16x2, d) >> __builtin_bit_cast(i16x2, fifteen);
            out[j] = unpk(d << one) ^ (uint32_t)__builtin_bit_cast(uint32_t, sign);
        }
        return;
    }
    try_fast = false;
#pragma unroll
    for (uint32_t j = 0; j < NW; j++)
        out[j] = pp_unsigned_pk(__builtin_amdgcn_alignbit(pw[j], j ? pw[j - 1] : before, 16), pw[j], xm);
}

template <int BS, int BYTES>
struct FastSeg {
    static constexpr uint32_t CHUNKS = (uint32_t)BS * BYTES * 64u / 16u;       // per full segment
    static constexpr uint32_t NIT = (CHUNKS + 63u) / 64u;                      // chunk rounds per lane
    uint4 v[NIT];
    uint32_t carry;   // sample just before the segment, as loaded (byte order not yet resolved)
};

// max_chunk = index of the last whole 16-byte chunk of the input (addresses are clamped to it, so
// the loads are unconditional and can be issued for a segment that later takes the generic path)
template <int BS, int BYTES>
__device__ __forceinline__ void fast_issue(const Cfg &c, const uint8_t *in, const Seg &g, uint32_t lane,
                                           uint64_t max_chunk, FastSeg<BS, BYTES> &f)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(in);
    const uint64_t first = g.samp0 * BYTES / 16u;
#pragma unroll
    for (uint32_t it = 0; it < FastSeg<BS, BYTES>::NIT; it++) {
        uint64_t ci = first + it * kWave + lane;
        if (ci > max_chunk) ci = max_chunk;
        f.v[it] = src[ci];
    }
    const uint64_t prev = g.samp0 ? g.samp0 - 1 : 0;
    f.carry = load_sample_raw<BYTES>(in + prev * BYTES);
}

template <int BS, int BYTES>
__device__ __forceinline__ void fast_finish(const Cfg &c, const Seg &g, const FastSeg<BS, BYTES> &f,
                                            uint32_t *rows, uint32_t lane)
{
    constexpr uint32_t SPC = 16 / BYTES;           // samples per chunk
    constexpr uint32_t STRIDE = Rows<BS, BYTES>::stride_words(BS);
    const bool msb = c.flags & F_MSB, pp = c.flags & F_PREPROCESS;
    const uint32_t nchunks = g.nv * (uint32_t)BS * BYTES / 16u;
    uint32_t carry = sample_byte_order<BYTES>(f.carry, msb);
    bool try_fast = true;                          // (pp_words_pk)

#pragma unroll
    for (uint32_t it = 0; it < FastSeg<BS, BYTES>::NIT; it++) {
        const uint32_t ci = it * kWave + lane;
        const bool act = ci < nchunks;
        const uint4 v = f.v[it];
        const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
        if (Rows<BS, BYTES>::HALF && pp) {
            // samples of at most 16 bits stay packed, two per instruction, from the loaded words to the
            // uint16 rows (pw[] = sample pairs in stream order).  Signed samples are biased by
            // 2^(bps-1) first -- flip the sign bit, drop the sign copies above it -- which turns
            // [xmin, xmax] into [0, 2^bps - 1] and leaves differences and distances to the bounds,
            // hence the mapped values (reference encode.c:294-309), unchanged.
            constexpr uint32_t NW = SPC / 2;
            uint32_t pw[NW];
            if (BYTES == 2) {
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    pw[j] = msb ? (((vw[j] & 0x00FF00FFu) << 8) | ((vw[j] >> 8) & 0x00FF00FFu)) : vw[j];
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {      // bytes 0,1 and 2,3 widened to 16 bits each
                    pw[2 * j] = __builtin_amdgcn_perm(0u, vw[j], 0x0c010c00u);
                    pw[2 * j + 1] = __builtin_amdgcn_perm(0u, vw[j], 0x0c030c02u);
                }
            }
            const bool sgn = c.flags & F_SIGNED;
            const uint32_t full = low_mask32(c.bps);
            if (sgn) {
                const uint32_t flip = (1u << (c.bps - 1)) * 0x00010001u, keep = full * 0x00010001u;
#pragma unroll
                for (uint32_t j = 0; j < NW; j++) pw[j] = (pw[j] ^ flip) & keep;
            }
            // the word before this chunk: the neighbour lane's last word, or the carried sample
            const uint32_t cbias = sgn ? (carry ^ (1u << (c.bps - 1))) & full : carry;
            const uint32_t before = wave_shr1(pw[NW - 1], cbias << 16);
            carry = wave_last(pw[NW - 1]) >> 16;
            if (sgn) carry ^= 1u << (c.bps - 1);       // back to the raw form the next round expects
            const uint32_t xm = (sgn ? full : c.xmax) * 0x00010001u;
            uint32_t dw[NW];
            pp_words_pk<NW>(pw, before, xm, act, dw, try_fast);
            if (act) {
                if (g.b0 == 0 && ci == 0) dw[0] &= 0xFFFF0000u;      // reference sample slot, encode.c:254
#pragma unroll
                for (uint32_t q = 0; q < NW / 4; q++) {
                    const uint32_t i = ci * SPC + q * 8;
                    const uint32_t row = i / BS, col = i % BS;
                    *reinterpret_cast<uint4 *>(&rows[row * STRIDE + col / 2]) =
                        make_uint4(dw[4 * q], dw[4 * q + 1], dw[4 * q + 2], dw[4 * q + 3]);
                }
            }
            continue;
        }
        uint32_t x[SPC];
        if (BYTES == 4) {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) x[j] = msb ? bswap32(vw[j]) : vw[j];
        } else if (BYTES == 2) {
            uint32_t sw[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)   // swap the bytes of both halves at once for MSB data
                sw[j] = msb ? (((vw[j] & 0x00FF00FFu) << 8) | ((vw[j] >> 8) & 0x00FF00FFu)) : vw[j];
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) x[j] = (j & 1) ? sw[j >> 1] >> 16 : sw[j >> 1] & 0xFFFFu;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 16; j++) x[j] = (vw[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
        }
        const uint32_t last = x[SPC - 1];
        const uint32_t prev = wave_shr1(last, carry);
        carry = wave_last(last);
        if (act) {
            uint32_t dd[SPC];
            // the three flavours are selected once per chunk (wave-uniform), not per sample
            if (!pp) {
#pragma unroll
                for (uint32_t j = 0; j < SPC; j++) dd[j] = x[j];
            } else {
                // as pp_words_pk, for samples of more than 16 bits: the values as distances from xmin, their smallest and
                // largest, the zigzag of the differences where nothing can clip (|difference| <= the stretch's range <=
                // half the sample range < 2^31), the exact mapping otherwise -- and then for the rest of the segment
                const bool sgn = c.flags & F_SIGNED;
                bool fast = try_fast;
                uint32_t u[SPC];
                const uint32_t up = sgn ? sign_extend(prev, c.bps) - c.xmin : prev;
                if (fast) {
                    uint32_t lo = up, hi = up;
#pragma unroll
                    for (uint32_t j = 0; j < SPC; j++) {
                        u[j] = sgn ? sign_extend(x[j], c.bps) - c.xmin : x[j];
                        lo = u[j] < lo ? u[j] : lo;
                        hi = u[j] > hi ? u[j] : hi;
                    }
                    const uint32_t range = hi - lo;
                    fast = !__any(!(range <= lo && range <= (c.xmax - c.xmin) - hi));
                    try_fast = fast;
                }
                if (fast) {
#pragma unroll
                    for (uint32_t j = 0; j < SPC; j++) {
                        const uint32_t diff = u[j] - (j ? u[j - 1] : up);
                        dd[j] = (diff << 1) ^ (uint32_t)((int32_t)diff >> 31);
                    }
                } else if (sgn) {
                    uint32_t pv = sign_extend(prev, c.bps);
#pragma unroll
                    for (uint32_t j = 0; j < SPC; j++) {
                        const uint32_t cv = sign_extend(x[j], c.bps);
                        dd[j] = pp_signed(pv, cv, c.xmin, c.xmax);
                        pv = cv;
                    }
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < SPC; j++) dd[j] = pp_unsigned(j ? x[j - 1] : prev, x[j], c.xmax);
                }
            }
            if (pp && g.b0 == 0 && ci == 0) dd[0] = 0;   // reference sample slot, encode.c:254
            if (Rows<BS, BYTES>::HALF) {
#pragma unroll
                for (uint32_t q = 0; q < SPC / 8; q++) {
                    const uint32_t i = ci * SPC + q * 8;
                    const uint32_t row = i / BS, col = i % BS;
                    *reinterpret_cast<uint4 *>(&rows[row * STRIDE + col / 2]) =
                        make_uint4(dd[8 * q] | (dd[8 * q + 1] << 16), dd[8 * q + 2] | (dd[8 * q + 3] << 16),
                                   dd[8 * q + 4] | (dd[8 * q + 5] << 16), dd[8 * q + 6] | (dd[8 * q + 7] << 16));
                }
            } else {
#pragma unroll
                for (uint32_t q = 0; q < SPC / 4; q++) {
                    const uint32_t i = ci * SPC + q * 4;
                    const uint32_t row = i / BS, col = i % BS;
                    *reinterpret_cast<uint4 *>(&rows[row * STRIDE + col]) =
                        make_uint4(dd[4 * q], dd[4 * q + 1], dd[4 * q + 2], dd[4 * q + 3]);
                }
            }
        }
    }
}

// ---- phase A, direct path: blocks of at most 32 bytes of samples of at most 16 bits ------------------
// Every lane loads ITS block (lane = block from the start: no chunk -> row transposition through the LDS),
// maps it with the packed predictor in its own registers -- the sample before the block comes from the
// neighbour lane -- and hands the sample pairs to the analysis / emission as they are.  The differential
// profile (profiles/r02/differential_profile_c2.txt) put the LDS feed at 0.69 + 0.78 ms of the 3.6 ms the two
// encoder kernels take at C2; most of it was not the predictor but the way through the rows.
template <int BS, int BYTES>
struct DirectSeg {
    static constexpr uint32_t NRAW = (uint32_t)BS * BYTES / 4u;      // 2, 4 or 8 words per block
    uint32_t raw[NRAW];
    uint32_t carry;   // sample just before the segment, as loaded
};

// max_blk = index of the last whole block of the input (lanes beyond the segment re-read a valid block)
template <int BS, int BYTES>
__device__ __forceinline__ void direct_issue(const Cfg &c, const uint8_t *in, const Seg &g, uint32_t lane,
                                             uint64_t max_blk, DirectSeg<BS, BYTES> &f)
{
    constexpr uint32_t BLK = (uint32_t)BS * BYTES;
    uint64_t bi = g.blk0 + lane;
    if (bi > max_blk) bi = max_blk;
    const uint8_t *p = in + bi * BLK;
    if (BLK == 8) {
        const uint2 a = *reinterpret_cast<const uint2 *>(p);
        f.raw[0] = a.x; f.raw[1] = a.y;
    } else {
#pragma unroll
        for (uint32_t q = 0; q < BLK / 16u; q++) {
            const uint4 a = reinterpret_cast<const uint4 *>(p)[q];
            f.raw[4 * q] = a.x; f.raw[4 * q + 1] = a.y; f.raw[4 * q + 2] = a.z; f.raw[4 * q + 3] = a.w;
        }
    }
    const uint64_t prev = g.samp0 ? g.samp0 - 1 : 0;
    f.carry = load_sample_raw<BYTES>(in + prev * BYTES);
}

// the lane's block as BS / 2 words of two mapped 16-bit samples each (what the uint16 rows hold)
template <int BS, int BYTES>
__device__ __forceinline__ void direct_finish(const Cfg &c, const Seg &g, const DirectSeg<BS, BYTES> &f,
                                              uint32_t lane, uint32_t *w)
{
    constexpr uint32_t NW = (uint32_t)BS / 2u;
    const bool msb = c.flags & F_MSB, sgn = c.flags & F_SIGNED;
    uint32_t pw[NW];
    if (BYTES == 2) {
#pragma unroll
        for (uint32_t j = 0; j < NW; j++)
            pw[j] = msb ? (((f.raw[j] & 0x00FF00FFu) << 8) | ((f.raw[j] >> 8) & 0x00FF00FFu)) : f.raw[j];
    } else {
#pragma unroll
        for (uint32_t j = 0; j < NW / 2u; j++) {      // bytes 0,1 and 2,3 widened to 16 bits each
            pw[2 * j] = __builtin_amdgcn_perm(0u, f.raw[j], 0x0c010c00u);
            pw[2 * j + 1] = __builtin_amdgcn_perm(0u, f.raw[j], 0x0c030c02u);
        }
    }
    // signed samples biased by 2^(bps-1) as in fast_finish
    const uint32_t full = low_mask32(c.bps);
    uint32_t carry = sample_byte_order<BYTES>(f.carry, msb);
    if (sgn) {
        const uint32_t flip = (1u << (c.bps - 1)) * 0x00010001u, keep = full * 0x00010001u;
#pragma unroll
        for (uint32_t j = 0; j < NW; j++) pw[j] = (pw[j] ^ flip) & keep;
        carry = (carry ^ (1u << (c.bps - 1))) & full;
    }
    const uint32_t before = wave_shr1(pw[NW - 1], carry << 16);
    const uint32_t xm = (sgn ? full : c.xmax) * 0x00010001u;
    bool try_fast = true;
    pp_words_pk<NW>(pw, before, xm, lane < g.nv, w, try_fast);
    if (g.b0 == 0 && lane == 0) w[0] &= 0xFFFF0000u;      // reference sample slot, encode.c:254
}

// ---- phase A, generic path: lane = sample, byte loads, end-of-data padding -------------------
template <int BS, int BYTES>
__device__ __forceinline__ void load_segment_generic(const Cfg &c, const uint8_t *in, const Seg &g,
                                                     uint32_t *rows, uint32_t stride, uint32_t lane)
{
    const bool msb = c.flags & F_MSB, pp = c.flags & F_PREPROCESS;
    const uint32_t ns = g.nv * c.bs;
    const uint64_t last = c.total_samples - 1;
    for (uint32_t i = lane; i < ns; i += kWave) {
        const uint64_t gi = g.samp0 + i;
        const uint64_t gc = gi < last ? gi : last;            // encode.c:676-684: repeat last sample
        const uint32_t cur = load_sample_bytes(in + gc * c.bytes, c.bytes, msb);
        uint32_t dv;
        if (!pp) {
            dv = cur;
        } else if (g.b0 == 0 && i == 0) {
            dv = 0;
        } else {
            const uint64_t gp = gi - 1 < last ? gi - 1 : last;
            dv = pp_any(load_sample_bytes(in + gp * c.bytes, c.bytes, msb), cur, c);
        }
        Rows<BS, BYTES>::put(rows, stride, i / c.bs, i % c.bs, dv);
    }
}

// the shapes of the direct path (Feeder::DIRECT; the host asks too: local_plan)
constexpr bool direct_shape(uint32_t bs, uint32_t bytes) { return bs > 0 && (bytes == 1 || bytes == 2) && bs * bytes <= 32; }

// Segment feeder: owns the prefetched registers of the NEXT segment.  fast == templated block
// size, 1/2/4-byte containers, 16-byte aligned RSIs; everything else takes the generic loader.
template <int BS, int BYTES>
struct Feeder {
    static constexpr bool FAST_T = BS > 0 && (BYTES == 1 || BYTES == 2 || BYTES == 4);
    static constexpr int FBS = FAST_T ? BS : 8, FBY = FAST_T ? BYTES : 1;
    // prefetch across segments only while it is cheap in registers (<= 4 x 16 bytes per lane)
    static constexpr bool PIPE = FAST_T && FastSeg<FBS, FBY>::NIT <= 4;
    FastSeg<(PIPE ? FBS : 8), (PIPE ? FBY : 1)> pre;
    bool fast;            // run-time half of the decision (alignment, at least one whole chunk)
    uint64_t max_chunk;

    __device__ __forceinline__ void init(const Cfg &c, uint32_t fast_ok)
    {
        const uint64_t total_bytes = c.total_samples * c.bytes;
        fast = FAST_T && fast_ok && total_bytes >= 16;
        max_chunk = total_bytes >= 16 ? total_bytes / 16 - 1 : 0;
        const uint64_t whole_blocks = c.total_samples / (BS ? (uint32_t)BS : c.bs);
        max_blk = whole_blocks ? whole_blocks - 1 : 0;
        if (whole_blocks == 0) fast = false;
    }
    __device__ __forceinline__ void prefetch(const Cfg &c, const uint8_t *in, const Seg &g, uint32_t lane)
    {
        if (PIPE) {
            if (fast) fast_issue<(PIPE ? FBS : 8), (PIPE ? FBY : 1)>(c, in, g, lane, max_chunk, pre);
        }
    }
    // ---- direct path (see DirectSeg): kernels that take it prefetch with prefetch_direct and fall back to
    // feed_now for the segments it does not cover (end-of-data padding, no preprocessing)
    static constexpr bool DIRECT = FAST_T && Rows<BS, BYTES>::HALF && direct_shape(BS, BYTES);
    DirectSeg<(DIRECT ? BS : 8), (DIRECT ? BYTES : 1)> pre_direct;
    uint64_t max_blk;
    __device__ __forceinline__ bool direct_ok(const Cfg &c, const Seg &g) const
    {
        return DIRECT && fast && g.full && (c.flags & F_PREPROCESS);
    }
    __device__ __forceinline__ void prefetch_direct(const Cfg &c, const uint8_t *in, const Seg &g, uint32_t lane)
    {
        if (DIRECT) {
            if (fast) direct_issue<(DIRECT ? BS : 8), (DIRECT ? BYTES : 1)>(c, in, g, lane, max_blk, pre_direct);
        }
    }
    // rows of g without a prefetch (fallback of the direct kernels)
    __device__ __forceinline__ void feed_now(const Cfg &c, const uint8_t *in, const Seg &g, uint32_t *rows,
                                             uint32_t stride, uint32_t lane)
    {
        if (FAST_T) {
            if (fast && g.full) {
                FastSeg<FBS, FBY> now;
                fast_issue<FBS, FBY>(c, in, g, lane, max_chunk, now);
                fast_finish<FBS, FBY>(c, g, now, rows, lane);
                return;
            }
        }
        load_segment_generic<BS, BYTES>(c, in, g, rows, stride, lane);
    }
    // consumes the registers prefetched for g (call prefetch(next) BEFORE this to overlap)
    __device__ __forceinline__ void feed(const Cfg &c, const uint8_t *in, const Seg &g,
                                         const FastSeg<(PIPE ? FBS : 8), (PIPE ? FBY : 1)> &cur, uint32_t *rows,
                                         uint32_t stride, uint32_t lane)
    {
        if (PIPE) {
            if (fast && g.full) {
                fast_finish<(PIPE ? FBS : 8), (PIPE ? FBY : 1)>(c, g, cur, rows, lane);
                return;
            }
        } else if (FAST_T) {
            if (fast && g.full) {          // big blocks: load and use in place
                FastSeg<FBS, FBY> now;
                fast_issue<FBS, FBY>(c, in, g, lane, max_chunk, now);
                fast_finish<FBS, FBY>(c, g, now, rows, lane);
                return;
            }
        }
        load_segment_generic<BS, BYTES>(c, in, g, rows, stride, lane);
    }
};

// copy a block's LDS row into registers (BS > 0) or alias the row (BS == 0)
template <int BS, bool HALF>
struct BlockRegs {
    uint32_t v[BS];
    __device__ __forceinline__ const uint32_t *load(const uint32_t *row)
    {
        if (HALF) {
#pragma unroll
            for (int q = 0; q < BS / 8; q++) {
                const uint4 t = *reinterpret_cast<const uint4 *>(row + 4 * q);
                const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    v[8 * q + 2 * j] = w[j] & 0xFFFFu;
                    v[8 * q + 2 * j + 1] = w[j] >> 16;
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < BS / 4; q++) {
                const uint4 t = *reinterpret_cast<const uint4 *>(row + 4 * q);
                v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
            }
        }
        return v;
    }
};
template <bool HALF>
struct BlockRegs<0, HALF> {
    __device__ __forceinline__ const uint32_t *load(const uint32_t *row) { return row; }
};

template <int BS>
__device__ __forceinline__ bool block_is_zero(const uint32_t *d, uint32_t bs_rt)
{
    const uint32_t bs = BS ? (uint32_t)BS : bs_rt;
    uint32_t any = 0;
#pragma unroll
    for (uint32_t i = 0; i < bs; i++) any |= d[i];
    return any == 0;
}

// Option selection on a block held as BS/2 words of two 16-bit residuals each (uint16 rows):
// fs(k) = sum of (sample >> k) costs one packed shift and one dot product per PAIR
// (v_pk_lshrrev_b16, v_dot2_u32_u16 with (1, 1)); the control flow is aec_lane.h's.
template <int BS>
__device__ __forceinline__ BlockChoice choose_option_pk(const uint32_t *w, const Cfg &c, uint32_t ref)
{
    const uint32_t n = (uint32_t)BS - ref;
    const u16x2 ones = {1, 1};
    auto fs = [&](uint32_t k) -> uint32_t {       // at most 64 * 65535 < 2^22
        const u16x2 kk = {(unsigned short)k, (unsigned short)k};
        uint32_t s = 0;
#pragma unroll
        for (int j = 0; j < BS / 2; j++) s = __builtin_amdgcn_udot2(pk(w[j]) >> kk, ones, s, false);
        return s;
    };
    uint32_t split_len = 0xFFFFFFFFu, klo = 0, khi = 31;
    if (c.id_len > 1) assess_split_with(fs, n, c.kmax, klo, khi, split_len);
    // second extension (aec_lane.h assess_se): a pair is the two halves of a word; their sum stays
    // below 2^17, so the reference's 64-bit wrap case cannot occur here
    // (round 6) The reference adds (a + b)(a + b + 1) / 2 + b + 1 pair by pair and gives up once the length passes the
    // limit (encode.c:412-434); the terms are positive, so that is "the whole sum passes the limit", and the whole sum is
    // 1 + (sum of s^2 + sum of s) / 2 + sum of b + pairs with s = a + b: per pair two dot products, a multiply-add, an or
    // and an add instead of a dozen instructions with their compares and selects.  A pair sum of 2^13 and more is beyond
    // any limit (<= 64 x 16 bits) by itself -- the or of all pair sums tells -- and below that nothing overflows 32 bits.
    const uint32_t limit = n * c.bps;
    const u16x2 second = {0, 1};
    uint32_t s_all = 0, s_sq = 0, s_b = 0, s_or = 0;
#pragma unroll
    for (int j = 0; j < BS / 2; j++) {
        const uint32_t sum = __builtin_amdgcn_udot2(pk(w[j]), ones, 0u, false);
        s_or |= sum;
        s_all += sum;
        s_sq += __umul24(sum, sum);                                   // (sum < 2^13 wherever the result is used)
        s_b = __builtin_amdgcn_udot2(pk(w[j]), second, s_b, false);
    }
    const uint32_t len = 1u + (s_sq + s_all) / 2u + s_b + (uint32_t)BS / 2u;
    const bool over = (s_or >> 13) != 0u || len > limit;
    return choose_from(c, (uint32_t)BS, ref, split_len, over ? 0xFFFFFFFFu : len, klo, khi);
}

// ----------------------------------------------------------------------------------------------
// K1: analysis
// ----------------------------------------------------------------------------------------------
template <int BS, int BYTES>
__device__ __forceinline__ void analyze_body(const Cfg &c, const Seg &g, uint32_t *rows, uint32_t stride,
                                             uint32_t lane, uint64_t sg, uint32_t *__restrict__ meta,
                                             uint32_t *__restrict__ seg_bits, uint16_t *__restrict__ seg_clamp,
                                             const uint32_t *direct = nullptr);

template <int BS, int BYTES>
__global__ void __launch_bounds__(256)
k_analyze(const Cfg c, const uint8_t *__restrict__ in, uint32_t *__restrict__ meta,
          uint32_t *__restrict__ seg_bits, uint16_t *__restrict__ seg_clamp, uint32_t segs_per_wave,
          uint32_t fast_ok)
{
#define AEC_WAVE_INDEX ((uint64_t)blockIdx.x * (blockDim.x >> 6) + wave)
#include "aec_enc_analyze.inc"
#undef AEC_WAVE_INDEX
}

// A wavefront of a batch of unequal chunks (aec_chunks.h): its chunk from the per-wave table that k_chunks_setup wrote,
// then the chunk's counts, input and array bases in scalar registers -- the body then runs on the chunk as on an input of
// its own.  A chunk has ceil(segs / segs_per_wave) waves, so no wave works across a chunk border.
struct ChunkWave {
    Cfg c;
    const uint8_t *in;
    uint64_t blk0, seg0, wave;      // bases in the workspace arrays, wave number inside the chunk
};
__device__ __forceinline__ ChunkWave chunk_wave(const Cfg &call, const uint8_t *d_in, const ChunkDesc *__restrict__ desc,
                                                const uint32_t *__restrict__ wave_chunk, uint64_t gwave)
{
    const uint32_t ci = __builtin_amdgcn_readfirstlane(wave_chunk[gwave]);
    const ChunkDesc d = desc[ci], next = desc[ci + 1];     // (the prefix sums of the next one give this one's counts)
    ChunkWave w;
    w.c = call;
    w.c.total_samples = d.samples;
    w.c.total_blocks = next.blk0 - d.blk0;
    w.c.total_segs = next.seg0 - d.seg0;
    w.c.rsi_count = next.rsi0 - d.rsi0 - 1;
    w.in = d_in + d.in_off;
    w.blk0 = d.blk0;
    w.seg0 = d.seg0;
    w.wave = gwave - d.wave0;
    return w;
}

template <int BS, int BYTES>
__global__ void __launch_bounds__(256)
k_analyze_chunks(const Cfg call, const uint8_t *__restrict__ d_in, const ChunkDesc *__restrict__ desc,
                 const uint32_t *__restrict__ wave_chunk, uint64_t nwaves, uint32_t *__restrict__ meta_all,
                 uint32_t *__restrict__ seg_bits_all, uint16_t *__restrict__ seg_clamp_all, uint32_t segs_per_wave,
                 uint32_t fast_ok)
{
    const uint64_t gw = (uint64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (gw >= nwaves) return;
    const ChunkWave cw = chunk_wave(call, d_in, desc, wave_chunk, gw);
    const Cfg &c = cw.c;
    const uint8_t *__restrict__ in = cw.in;
    uint32_t *__restrict__ meta = meta_all + cw.blk0;
    uint32_t *__restrict__ seg_bits = seg_bits_all + cw.seg0;
    uint16_t *__restrict__ seg_clamp = seg_clamp_all + cw.seg0;
#define AEC_WAVE_INDEX cw.wave
#include "aec_enc_analyze.inc"
#undef AEC_WAVE_INDEX
}

// Phase B of one segment (rows already in LDS): this lane's block summary (meta_pack), the segment's
// bit length and its k clamp (lo | hi << 8), both wave-uniform.
template <int BS, int BYTES>
__device__ __forceinline__ uint32_t analyze_segment(const Cfg &c, const Seg &g, const uint32_t *rows, uint32_t stride,
                                                    uint32_t lane, uint32_t &tot, uint32_t &cl,
                                                    const uint32_t *direct = nullptr,   // the lane's block from direct_finish
                                                    uint32_t *len_incl = nullptr)       // out: inclusive sums of the lengths
{
    const uint32_t bs = BS ? (uint32_t)BS : c.bs;
    const bool pp = c.flags & F_PREPROCESS;
    constexpr bool WIDE_T = (BYTES >= 3);
    BlockRegs<BS, Rows<BS, BYTES>::HALF && BS != 0 ? false : Rows<BS, BYTES>::HALF> regs;
    constexpr bool PK = Rows<BS, BYTES>::HALF && BS != 0;   // uint16 rows: analysed two samples at a time
    const bool valid = lane < g.nv;
    // every lane loads a row (idle lanes re-read the last valid one) so that the block lives in
    // registers instead of behind a conditionally assigned pointer
    const uint32_t *row = rows + (valid ? lane : g.nv - 1) * stride;
    uint32_t w[PK ? BS / 2 : 1];                            // the block as sample pairs
    const uint32_t *d = nullptr;
    bool zero;
    if (PK) {
        if (direct) {
#pragma unroll
            for (int j = 0; j < (PK ? BS / 2 : 0); j++) w[j] = direct[j];
        } else {
#pragma unroll
            for (int q = 0; q < (PK ? BS / 8 : 0); q++) {
                const uint4 t = *reinterpret_cast<const uint4 *>(row + 4 * q);
                w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
            }
        }
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < (PK ? BS / 2 : 0); j++) any |= w[j];
        zero = valid && any == 0;
    } else {
        d = regs.load(row);
        zero = valid && block_is_zero<BS>(d, bs);
    }
    const uint64_t zmask = __ballot(zero);

    uint32_t m = meta_pack(0, OPT_ZCONT, 0, 0);
    KClamp kc = kclamp_identity();
    if (valid) {
        const uint32_t ref = (pp && g.b0 == 0 && lane == 0) ? 1u : 0u;
        if (zero) {
            uint32_t fs = 0;
            const uint32_t run = zero_run_at(zmask, lane, g.nv, fs);
            if (run) m = meta_pack(c.id_len + 1 + ref * c.bps + fs + 1, OPT_ZERO, fs, 0);
        } else {
            BlockChoice ch;
            if (PK)
                ch = choose_option_pk<(PK ? BS : 8)>(w, c, ref);
            else if (BS == 0)
                ch = (c.bps > 16) ? choose_option<BS, true>(d, c, ref) : choose_option<BS, false>(d, c, ref);
            else
                ch = choose_option<BS, WIDE_T>(d, c, ref);
            m = meta_pack(ch.bits, ch.opt, ch.klo, ch.khi);
            if (c.id_len > 1) kc = KClamp{ch.klo, ch.khi};
        }
    }
    const uint32_t incl_l = wave_incl_sum(meta_len(m), lane);
    if (len_incl) *len_incl = incl_l;
    tot = wave_last(incl_l);
    // The summary of a block that updates k carries the COMPOSITION of the clamps of the segment's blocks up to
    // and including it (not its own plateau): the pack kernel then gets the block's k as one clamp of the
    // segment's carried-in k, without scanning the clamps a second time.
    const uint32_t incl_c = wave_incl_clamp(clamp_pack(kc), lane);
    cl = wave_last(incl_c);
    const uint32_t opt = meta_opt(m);
    // (clamp_pack is lo | hi << 8, the summary keeps them in its two upper bytes: one byte permute)
    if (valid && opt != OPT_ZERO && opt != OPT_ZCONT && c.id_len > 1) m = __builtin_amdgcn_perm(incl_c, m, 0x05040100u);
    return m;
}

template <int BS, int BYTES>
__device__ __forceinline__ void analyze_body(const Cfg &c, const Seg &g, uint32_t *rows, uint32_t stride,
                                             uint32_t lane, uint64_t sg, uint32_t *__restrict__ meta,
                                             uint32_t *__restrict__ seg_bits, uint16_t *__restrict__ seg_clamp,
                                             const uint32_t *direct)
{
    wave_lds_fence();
    uint32_t tot, cl;
    const uint32_t m = analyze_segment<BS, BYTES>(c, g, rows, stride, lane, tot, cl, direct);
    if (lane < g.nv) meta[g.blk0 + lane] = m;
    if (lane == 0) {
        seg_bits[sg] = tot;
        seg_clamp[sg] = (uint16_t)cl;
    }
    wave_lds_fence();
}

// ----------------------------------------------------------------------------------------------
// K2: scan of (bits, clamp) over segments -- reduce / scan partials / apply
// ----------------------------------------------------------------------------------------------
struct ScanVal {
    uint64_t bits;
    uint32_t cl;   // packed clamp
};
__device__ __forceinline__ ScanVal scan_then(ScanVal a, ScanVal b)
{
    return ScanVal{a.bits + b.bits, clamp_pack(kclamp_then(clamp_unpack(a.cl), clamp_unpack(b.cl)))};
}
__device__ __forceinline__ ScanVal scan_identity() { return ScanVal{0, clamp_pack(kclamp_identity())}; }

// ordered inclusive scan across the 256 threads of a workgroup; returns this thread's
// EXCLUSIVE prefix and the workgroup total
__device__ __forceinline__ ScanVal block_excl_scan(ScanVal v, ScanVal &total, ScanVal *sh /*[4]*/)
{
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (scalar: segment geometry and addresses then run on the SALU)
    ScanVal inc = v;
#pragma unroll
    for (uint32_t o = 1; o < kWave; o <<= 1) {
        ScanVal t;
        t.bits = __shfl_up((unsigned long long)inc.bits, o);
        t.cl = __shfl_up(inc.cl, o);
        if (lane >= o) inc = scan_then(t, inc);
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    ScanVal wprefix = scan_identity();
    for (uint32_t w = 0; w < wave; w++) wprefix = scan_then(wprefix, sh[w]);
    total = scan_identity();
    for (uint32_t w = 0; w < (blockDim.x >> 6); w++) total = scan_then(total, sh[w]);
    ScanVal exc;
    exc.bits = __shfl_up((unsigned long long)inc.bits, 1);
    exc.cl = __shfl_up(inc.cl, 1);
    if (lane == 0) exc = scan_identity();
    __syncthreads();
    return scan_then(wprefix, exc);
}

#ifndef AEC_ENC_PART                  // (what does not depend on the block size)
constexpr uint32_t kScanItems = 8;   // kScanChunk = 256 * 8

__global__ void __launch_bounds__(256)
k_scan_reduce(const uint32_t *__restrict__ seg_bits, const uint16_t *__restrict__ seg_clamp,
              uint64_t nseg, ScanPartial *__restrict__ partials)
{
    __shared__ ScanVal sh[4];
    const uint64_t base = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kScanItems;
    ScanVal acc = scan_identity();
#pragma unroll
    for (uint32_t i = 0; i < kScanItems; i++) {
        const uint64_t s = base + i;
        if (s < nseg) acc = scan_then(acc, ScanVal{seg_bits[s], seg_clamp[s]});
    }
    ScanVal total;
    block_excl_scan(acc, total, sh);
    if (threadIdx.x == 0) {
        const KClamp k = clamp_unpack(total.cl);
        partials[blockIdx.x] = ScanPartial{total.bits, k.lo, k.hi};
    }
}

// single workgroup: exclusive scan of the chunk partials in place, final totals to *res
__global__ void __launch_bounds__(256)
k_scan_partials(ScanPartial *partials, uint64_t nchunks, uint32_t start_bit, uint32_t k_in,
                EncResult *res)
{
    __shared__ ScanVal sh[4];
    const uint64_t per = (nchunks + 255) / 256;
    const uint64_t lo = (uint64_t)threadIdx.x * per;
    uint64_t hi = lo + per;
    if (hi > nchunks) hi = nchunks;
    ScanVal acc = scan_identity();
    for (uint64_t i = lo; i < hi; i++)
        acc = scan_then(acc, ScanVal{partials[i].bits, clamp_pack(KClamp{partials[i].lo, partials[i].hi})});
    ScanVal total;
    ScanVal run = block_excl_scan(acc, total, sh);
    for (uint64_t i = lo; i < hi; i++) {
        const ScanVal cur{partials[i].bits, clamp_pack(KClamp{partials[i].lo, partials[i].hi})};
        const KClamp k = clamp_unpack(run.cl);
        partials[i] = ScanPartial{run.bits, k.lo, k.hi};
        run = scan_then(run, cur);
    }
    if (threadIdx.x == 0) {
        const KClamp t = clamp_unpack(total.cl);
        res->total_bits = total.bits;
        res->k_out = kclamp_apply(t, k_in);
        res->overflow = 0;
        res->k_lo = t.lo;
        res->k_hi = t.hi;
    }
    (void)start_bit;
}

__global__ void __launch_bounds__(256)
k_scan_apply(const uint32_t *__restrict__ seg_bits, const uint16_t *__restrict__ seg_clamp,
             uint64_t nseg, const ScanPartial *__restrict__ partials, uint32_t start_bit, uint32_t k_in,
             uint32_t segs_per_rsi, uint64_t rsi_count, uint64_t *__restrict__ seg_start,
             uint8_t *__restrict__ seg_kin, uint64_t *__restrict__ rsi_off, EncResult *res,
             uint32_t *__restrict__ out_words, uint64_t cap_words, uint32_t segs_per_wave,
             const ShardCarry *__restrict__ carry)
{
    __shared__ ScanVal sh[4];
    if (carry) {                       // one stream over several devices: what precedes this shard
        start_bit = (uint32_t)(carry->start_bit & 7u);
        k_in = carry->k_in;
    }
    const uint64_t base = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kScanItems;
    ScanVal item[kScanItems];
    ScanVal acc = scan_identity();
#pragma unroll
    for (uint32_t i = 0; i < kScanItems; i++) {
        const uint64_t s = base + i;
        item[i] = (s < nseg) ? ScanVal{seg_bits[s], seg_clamp[s]} : scan_identity();
        acc = scan_then(acc, item[i]);
    }
    ScanVal total;
    ScanVal run = block_excl_scan(acc, total, sh);
    const ScanPartial cp = partials[blockIdx.x];
    run = scan_then(ScanVal{cp.bits, clamp_pack(KClamp{cp.lo, cp.hi})}, run);
#pragma unroll
    for (uint32_t i = 0; i < kScanItems; i++) {
        const uint64_t s = base + i;
        if (s < nseg) {
            const uint64_t bit = (uint64_t)start_bit + run.bits;
            seg_start[s] = bit;
            seg_kin[s] = (uint8_t)kclamp_apply(clamp_unpack(run.cl), k_in);
            if (rsi_off && (s % segs_per_rsi) == 0) rsi_off[s / segs_per_rsi] = bit;
            // k_pack writes every word of the stream with plain stores except the words two of its
            // waves share -- the one a wave's first segment starts in -- which both OR into: those
            // (and the last word of the stream, below) are all that has to be zero beforehand
            if ((s % segs_per_wave) == 0 && (bit >> 5) < cap_words) out_words[bit >> 5] = 0u;
        }
        run = scan_then(run, item[i]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        res->k_out = kclamp_apply(KClamp{res->k_lo, res->k_hi}, k_in);   // k_in is only known now
        if (rsi_off) rsi_off[rsi_count] = (uint64_t)start_bit + res->total_bits;
        const uint64_t end = (uint64_t)start_bit + res->total_bits;
        if ((end + 7) / 8 > cap_words * 4) res->overflow = 1;
        for (uint64_t w = end >> 5; w <= (end >> 5) + 1; w++)      // open last word (+ one of padding)
            if (w < cap_words) out_words[w] = 0u;
    }
}

// ---- a batch of equal, RSI-aligned chunks as ONE launch set ---------------------------------------------
// The chunks of a batch (aec_gpu_encode_uniform_batch_async) lie back to back in the input and are analysed
// and packed as one long input -- an RSI never looks across its borders -- with two differences, both in the
// scan: the k carried into a chunk is 0, and a chunk's stream starts on the byte behind the end of the one in
// front (every stream zero-padded to a byte as aec_buffer_encode pads it).  A chunk has at most kScanChunk
// segments, so one workgroup scans one chunk: totals, then the chunks' bases (one workgroup), then the start
// bit and k of every segment.
__global__ void __launch_bounds__(256)
k_batch_reduce(const uint32_t *__restrict__ seg_bits, uint32_t segs, BatchChunk *__restrict__ chunks)
{
    __shared__ ScanVal sh[4];
    const uint64_t first = (uint64_t)blockIdx.x * segs;
    ScanVal acc = scan_identity();
#pragma unroll
    for (uint32_t i = 0; i < kScanItems; i++) {
        const uint32_t s = threadIdx.x * kScanItems + i;
        if (s < segs) acc.bits += seg_bits[first + s];
    }
    ScanVal total;
    block_excl_scan(acc, total, sh);
    if (threadIdx.x == 0) chunks[blockIdx.x].bits = total.bits;
}

__global__ void __launch_bounds__(256)
k_batch_bases(BatchChunk *chunks, uint64_t n, uint64_t cap_bytes, EncResult *res)
{
    __shared__ ScanVal sh[4];
    const uint64_t per = (n + 255) / 256;
    const uint64_t lo = (uint64_t)threadIdx.x * per;
    uint64_t hi = lo + per;
    if (hi > n) hi = n;
    ScanVal acc = scan_identity();
    for (uint64_t i = lo; i < hi; i++) acc.bits += (chunks[i].bits + 7) / 8;
    ScanVal total;
    ScanVal run = block_excl_scan(acc, total, sh);
    for (uint64_t i = lo; i < hi; i++) {
        chunks[i].base_bits = run.bits * 8;
        run.bits += (chunks[i].bits + 7) / 8;
    }
    if (threadIdx.x == 0) {
        res->total_bits = total.bits * 8;
        res->k_out = 0;
        res->overflow = total.bits > cap_bytes ? 1u : 0u;
        res->k_lo = 0;
        res->k_hi = 0;
    }
}

__global__ void __launch_bounds__(256)
k_batch_apply(const uint32_t *__restrict__ seg_bits, const uint16_t *__restrict__ seg_clamp, uint32_t segs,
              const BatchChunk *__restrict__ chunks, uint64_t *__restrict__ seg_start, uint8_t *__restrict__ seg_kin,
              uint32_t *__restrict__ out_words, uint64_t cap_words, uint32_t segs_per_wave)
{
    __shared__ ScanVal sh[4];
    const uint64_t first = (uint64_t)blockIdx.x * segs;
    ScanVal item[kScanItems];
    ScanVal acc = scan_identity();
#pragma unroll
    for (uint32_t i = 0; i < kScanItems; i++) {
        const uint32_t s = threadIdx.x * kScanItems + i;
        item[i] = (s < segs) ? ScanVal{seg_bits[first + s], seg_clamp[first + s]} : scan_identity();
        acc = scan_then(acc, item[i]);
    }
    ScanVal total;
    ScanVal run = block_excl_scan(acc, total, sh);
    const uint64_t base = chunks[blockIdx.x].base_bits;
#pragma unroll
    for (uint32_t i = 0; i < kScanItems; i++) {
        const uint32_t s = threadIdx.x * kScanItems + i;
        if (s < segs) {
            const uint64_t bit = base + run.bits;
            seg_start[first + s] = bit;
            seg_kin[first + s] = (uint8_t)kclamp_apply(clamp_unpack(run.cl), 0u);
            // (as k_scan_apply: the word a wave's first segment starts in is shared with its neighbour)
            if (((first + s) % segs_per_wave) == 0 && (bit >> 5) < cap_words) out_words[bit >> 5] = 0u;
        }
        run = scan_then(run, item[i]);
    }
    if (threadIdx.x == 0) {                         // the chunk's open last word (+ one: its byte padding)
        const uint64_t end = base + total.bits;
        for (uint64_t w = end >> 5; w <= (end >> 5) + 1; w++)
            if (w < cap_words) out_words[w] = 0u;
    }
}

// ---- a batch of UNEQUAL chunks as one launch set (aec_chunks.h) ---------------------------------------------------------
// The segmented scan over tiles of kScanChunk segments of the concatenated numbering: three launches like the scans
// above, a chunk may span any number of tiles and a tile any number of chunks.
__device__ __forceinline__ CkVal ck_shfl_up(CkVal v, uint32_t o)
{
    CkVal t;
    t.bits = __shfl_up((unsigned long long)v.bits, o);
    t.cl = __shfl_up(v.cl, o);
    t.head = __shfl_up(v.head, o);
    return t;
}
// block_excl_scan for the restarting operator
__device__ __forceinline__ CkVal block_excl_scan_ck(CkVal v, CkVal &total, CkVal *sh /*[4]*/)
{
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    CkVal inc = v;
#pragma unroll
    for (uint32_t o = 1; o < kWave; o <<= 1) {
        const CkVal t = ck_shfl_up(inc, o);
        if (lane >= o) inc = ck_then(t, inc);
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    CkVal wprefix = ck_identity();
    for (uint32_t w = 0; w < wave; w++) wprefix = ck_then(wprefix, sh[w]);
    total = ck_identity();
    for (uint32_t w = 0; w < (blockDim.x >> 6); w++) total = ck_then(total, sh[w]);
    CkVal exc = ck_shfl_up(inc, 1);
    if (lane == 0) exc = ck_identity();
    __syncthreads();
    return ck_then(wprefix, exc);
}

// the per-wave table of the chunk kernels (4 bytes per wave), and the chunk totals cleared for k_chunks_reduce
__global__ void __launch_bounds__(256)
k_chunks_setup(const ChunkDesc *__restrict__ desc, uint64_t n, uint64_t nwaves, uint32_t *__restrict__ wave_chunk,
               BatchChunk *__restrict__ chunks)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwaves || i < n; i += stride) {
        if (i < nwaves) wave_chunk[i] = (uint32_t)chunk_of_wave(desc, n, i);
        if (i < n) chunks[i] = BatchChunk{0, 0};
    }
}

__global__ void __launch_bounds__(256)
k_chunks_reduce(const ChunkDesc *__restrict__ desc, uint64_t n, const uint32_t *__restrict__ seg_bits,
                const uint16_t *__restrict__ seg_clamp, uint64_t nseg, CkVal *__restrict__ tiles,
                BatchChunk *__restrict__ chunks)
{
    __shared__ CkVal sh[4];
    const uint64_t tile0 = (uint64_t)blockIdx.x * kScanChunk;
    const uint64_t tile_end = tile0 + kScanChunk < nseg ? tile0 + kScanChunk : nseg;
    uint64_t s0 = tile0 + (uint64_t)threadIdx.x * kScanItems, s1 = s0 + kScanItems;
    if (s0 > tile_end) s0 = tile_end;
    if (s1 > tile_end) s1 = tile_end;
    const CkVal acc = ck_reduce_items(desc, n, seg_bits, seg_clamp, s0, s1);
    CkVal total;
    const CkVal run = block_excl_scan_ck(acc, total, sh);
    ck_flush_totals(desc, n, seg_bits, seg_clamp, s0, s1, tile_end, run, [&](uint64_t chunk, uint64_t bits) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&chunks[chunk].bits), (unsigned long long)bits);
    });
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// one workgroup: the chunks' bases from their totals, the empty chunks' byte and table entry, the tile carries
__global__ void __launch_bounds__(256)
k_chunks_bases(const ChunkDesc *__restrict__ desc, BatchChunk *chunks, uint64_t n, CkVal *tiles, uint64_t ntiles,
               uint8_t *__restrict__ out, uint64_t cap_bytes, uint64_t *__restrict__ rsi_off, EncResult *res)
{
    __shared__ ScanVal sh[4];
    __shared__ CkVal shc[4];
    const uint64_t per = (n + 255) / 256;
    const uint64_t lo = (uint64_t)threadIdx.x * per < n ? (uint64_t)threadIdx.x * per : n;
    const uint64_t hi = lo + per < n ? lo + per : n;
    ScanVal acc = scan_identity();
    for (uint64_t i = lo; i < hi; i++) acc.bits += chunk_stream_bytes(chunks[i].bits);
    ScanVal total;
    ScanVal run = block_excl_scan(acc, total, sh);
    for (uint64_t i = lo; i < hi; i++) {
        uint64_t base_bits;
        const uint64_t before = run.bits;
        run.bits = ck_base(run.bits, chunks[i].bits, &base_bits);
        chunks[i].base_bits = base_bits;
        if (desc[i + 1].seg0 == desc[i].seg0) {       // an empty chunk: no segment, so nobody else writes for it
            if (before < cap_bytes) out[before] = 0;
            if (rsi_off) rsi_off[desc[i].rsi0] = base_bits;
        }
    }
    if (threadIdx.x == 0) {
        res->total_bits = total.bits * 8;
        res->k_out = 0;
        res->overflow = total.bits > cap_bytes ? 1u : 0u;
        res->k_lo = 0;
        res->k_hi = 0;
    }
    // exclusive scan of the tile aggregates in place: what the chunk open at a tile's start has in front of the tile
    const uint64_t tper = (ntiles + 255) / 256;
    const uint64_t tlo = (uint64_t)threadIdx.x * tper < ntiles ? (uint64_t)threadIdx.x * tper : ntiles;
    const uint64_t thi = tlo + tper < ntiles ? tlo + tper : ntiles;
    CkVal tacc = ck_identity();
    for (uint64_t t = tlo; t < thi; t++) tacc = ck_then(tacc, tiles[t]);
    CkVal ttotal;
    CkVal trun = block_excl_scan_ck(tacc, ttotal, shc);
    for (uint64_t t = tlo; t < thi; t++) {
        const CkVal cur = tiles[t];
        tiles[t] = trun;
        trun = ck_then(trun, cur);
    }
}

__global__ void __launch_bounds__(256)
k_chunks_apply(const ChunkDesc *__restrict__ desc, uint64_t n, const uint32_t *__restrict__ seg_bits,
               const uint16_t *__restrict__ seg_clamp, uint64_t nseg, const CkVal *__restrict__ tiles,
               const BatchChunk *__restrict__ chunks, uint32_t segs_per_rsi, uint32_t segs_per_wave,
               uint64_t *__restrict__ seg_start, uint8_t *__restrict__ seg_kin, uint64_t *__restrict__ rsi_off,
               uint32_t *__restrict__ out_words, uint64_t cap_words)
{
    __shared__ CkVal sh[4];
    const uint64_t tile0 = (uint64_t)blockIdx.x * kScanChunk;
    const uint64_t tile_end = tile0 + kScanChunk < nseg ? tile0 + kScanChunk : nseg;
    uint64_t s0 = tile0 + (uint64_t)threadIdx.x * kScanItems, s1 = s0 + kScanItems;
    if (s0 > tile_end) s0 = tile_end;
    if (s1 > tile_end) s1 = tile_end;
    const CkVal acc = ck_reduce_items(desc, n, seg_bits, seg_clamp, s0, s1);
    CkVal total;
    CkVal run = block_excl_scan_ck(acc, total, sh);
    run = ck_then(tiles[blockIdx.x], run);
    if (s0 >= s1) return;
    CkCursor cur = ck_cursor(desc, n, s0);
    for (uint64_t s = s0; s < s1; s++) {
        ck_advance(desc, n, s, cur);
        const CkVal item = ck_item(desc, cur, s, seg_bits[s], seg_clamp[s]);
        const CkSeg g = ck_segment(desc, cur, s, run, item, chunks[cur.chunk].base_bits, segs_per_rsi, segs_per_wave);
        seg_start[s] = g.start;
        seg_kin[s] = (uint8_t)g.kin;
        if (rsi_off && g.first_rsi) rsi_off[g.rsi_entry] = g.start;
        // (as k_scan_apply: the word a wave's first segment starts in is shared with its neighbour ...
        if (g.wave_first && (g.start >> 5) < cap_words) out_words[g.start >> 5] = 0u;
        if (g.last) {                                  // ... and the chunk's open last word, + one: its byte padding)
            if (rsi_off) rsi_off[g.rsi_entry_end] = g.end;
            for (uint64_t w = g.end >> 5; w <= (g.end >> 5) + 1; w++)
                if (w < cap_words) out_words[w] = 0u;
        }
        run = ck_then(run, item);
    }
}

// segment table for segment-parallel decoding: start bit + preceding raw sample per segment
__global__ void __launch_bounds__(256)
k_seg_table(const Cfg c, const uint8_t *__restrict__ in, const uint64_t *__restrict__ seg_start,
            SegEntry *__restrict__ table)
{
    const uint64_t sg = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sg >= c.total_segs) return;
    const Seg g = seg_geom(c, sg);
    uint32_t prev = 0;
    if (g.b0 != 0) {
        uint64_t i = g.samp0 - 1;
        if (i >= c.total_samples) i = c.total_samples - 1;
        prev = load_sample_bytes(in + i * c.bytes, c.bytes, (c.flags & F_MSB) != 0);
    }
    table[sg] = SegEntry{seg_start[sg], prev, 0u};
}

// The slots of k_encode_local to their places in the stream (aec_enc_local.h): a wavefront takes kPlaceSlots consecutive
// slots.  A run starts where the scan put its first segment and ends where the next run starts (the last one: at the end
// of the stream); its words are shifted by the start's position in a 32-bit word, byte-swapped and stored, the first and
// the last by atomic OR where the run does not own them alone -- k_scan_apply zeroed those, and the words behind cap_words
// are nobody's, as in k_pack.
// A lane takes four slot words at a time (the slots are 128-byte aligned) and the word in front of them from the lane
// below: a ROUND is the wavefront's 256 words.  The order is: the run edges (one load), then the loads of kPlaceRounds
// rounds of every one of the wavefront's runs, and only then the shifts and stores, run by run and round by round from
// the registers; a round needs nothing of the one in front but its last word (`carry`, a register).  At C2 a run is
// three rounds, 11.6 KB a wavefront, 7 wavefronts a SIMD.  A longer run goes on in groups of kPlaceRounds rounds, each
// group's loads in front of its first store.  What this bought is small (profiles/r15/README.md: 0.56 ms at C2 against
// 0.58 - 0.59 with one round in flight per run): the copy is not bound by what it has in flight, nor by the
// instructions of a round; 4 x 4 and 2 x 4 measured no better.
constexpr uint32_t kPlaceSlots = 4, kPlaceRounds = 3;
constexpr uint32_t kPlaceRound = 4u * kWave;      // slot words of a round

// Quad `q` of a slot of which `have` words count.  The words behind them are stale and would cost HBM traffic: a lane
// whose quad lies there reads the last quad that counts once more, a line its wavefront fetches anyway.  So every load
// is issued whatever the run's length, with no branch around it (loads under a branch measured 0.01 ms slower at C2).
__device__ __forceinline__ uint4 place_load(const uint4 *__restrict__ slot, uint32_t q, uint32_t have)
{
    const uint32_t last = have ? (have - 1u) >> 2 : 0u;
    return slot[q < last ? q : last];
}

// What the rounds of a run need besides its span, wave-uniform and relative to the run's first word, so that a lane
// decides with 32-bit compares: the words [plain_lo, plain_hi) are the run's alone and inside the buffer (a plain store),
// the words up to `end` are written at all (those that are not plain: by atomic OR, local_word_shared).
struct PlaceRun {
    LocalSpan sp;
    uint32_t plain_lo, plain_hi, end;
};
__device__ __forceinline__ PlaceRun place_run(const LocalSpan &sp, uint64_t cap_words)
{
    PlaceRun r;
    r.sp = sp;
    const uint64_t room = cap_words > sp.word0 ? cap_words - sp.word0 : 0u;
    const uint32_t cap = room < sp.nwords ? (uint32_t)room : sp.nwords;
    const uint32_t own = sp.nwords - (sp.tail_shared && sp.nwords ? 1u : 0u);
    r.plain_lo = sp.head_shared ? 1u : 0u;
    r.plain_hi = own < cap ? own : cap;
    r.end = cap;
    return r;
}

// the round of a run that starts at slot word `base`, from the lane's quad `cur` of it
__device__ __forceinline__ void place_round(const PlaceRun &run, uint32_t base, uint32_t lane, const uint4 &cur,
                                            uint32_t &carry, uint32_t *__restrict__ out_words)
{
    typedef uint32_t words4 __attribute__((ext_vector_type(4), aligned(4)));
    const LocalSpan &sp = run.sp;
    const uint32_t j0 = base + 4u * lane;
    uint32_t a0 = cur.x, a1 = cur.y, a2 = cur.z, a3 = cur.w;
    if (base + kPlaceRound > sp.nslot) {            // (what lies behind the run's last slot word is stale)
        a0 = j0 < sp.nslot ? a0 : 0u; a1 = j0 + 1 < sp.nslot ? a1 : 0u;
        a2 = j0 + 2 < sp.nslot ? a2 : 0u; a3 = j0 + 3 < sp.nslot ? a3 : 0u;
    }
    const uint32_t before = wave_shr1(a3, carry);       // carry: the slot word in front of this round's first
    carry = wave_last(a3);
    const uint32_t v0 = local_word(sp, before, a0), v1 = local_word(sp, a0, a1), v2 = local_word(sp, a1, a2),
                   v3 = local_word(sp, a2, a3);
    uint32_t *__restrict__ dst = out_words + sp.word0 + base + 4u * lane;
    const words4 quad = words4{bswap32(v0), bswap32(v1), bswap32(v2), bswap32(v3)};
    if (base >= run.plain_lo && base + kPlaceRound <= run.plain_hi) {      // a round in the run's middle: no lane asks
        *reinterpret_cast<words4 *>(dst) = quad;
        return;
    }
    auto one = [&](uint32_t q, uint32_t v) {        // a word at an end of the run, or of the buffer
        if (j0 + q < run.end) {
            if (!local_word_shared(sp, j0 + q))
                dst[q] = bswap32(v);
            else if (v != 0)
                __hip_atomic_fetch_or(&dst[q], bswap32(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if (j0 >= run.plain_lo && j0 + 4u <= run.plain_hi) {
        *reinterpret_cast<words4 *>(dst) = quad;
    } else {
        one(0, v0); one(1, v1); one(2, v2); one(3, v3);
    }
}

__global__ void __launch_bounds__(256)
k_place(const uint32_t *__restrict__ image, uint32_t slot_words, const uint64_t *__restrict__ seg_start, uint64_t nseg,
        uint32_t segs_per_wave, uint64_t nslots, uint32_t start_bit, const EncResult *__restrict__ res,
        uint32_t *__restrict__ out_words, uint64_t cap_words)
{
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t first = ((uint64_t)blockIdx.x * (blockDim.x >> 6) + wave) * kPlaceSlots;
    if (first >= nslots) return;
    // where the runs start, and where the last one ends: lane g reads the edge in front of run g, one load for all
    uint64_t mine = 0u;
    if (lane <= kPlaceSlots && first + lane <= nslots) {
        const uint64_t s = (first + lane) * segs_per_wave;
        mine = s < nseg ? seg_start[s] : (uint64_t)start_bit + res->total_bits;
    }
    PlaceRun run[kPlaceSlots];
    const uint4 *__restrict__ slot[kPlaceSlots];
    uint32_t have[kPlaceSlots];
#pragma unroll
    for (uint32_t g = 0; g < kPlaceSlots; g++) {
        const uint64_t from = wave_get64(mine, g), to = wave_get64(mine, g + 1);
        const bool live = first + g < nslots && to > from;
        LocalSpan sp = local_span(from, live ? to - from : 0u);
        if (!live) sp.nwords = 0u;
        run[g] = place_run(sp, cap_words);
        have[g] = sp.nslot < slot_words ? sp.nslot : slot_words;
        slot[g] = reinterpret_cast<const uint4 *>(image + (first + g < nslots ? first + g : first) * slot_words);
    }
    uint4 w[kPlaceSlots][kPlaceRounds];
#pragma unroll
    for (uint32_t g = 0; g < kPlaceSlots; g++)
#pragma unroll
        for (uint32_t r = 0; r < kPlaceRounds; r++) w[g][r] = place_load(slot[g], r * kWave + lane, have[g]);
#pragma unroll
    for (uint32_t g = 0; g < kPlaceSlots; g++) {
        uint32_t carry = 0u;
#pragma unroll
        for (uint32_t r = 0; r < kPlaceRounds; r++)
            if (r * kPlaceRound < run[g].sp.nwords) place_round(run[g], r * kPlaceRound, lane, w[g][r], carry, out_words);
        // the groups behind the first (C2 has none; data that does not compress fills the slot: about 18 rounds)
        for (uint32_t base = kPlaceRounds * kPlaceRound; base < run[g].sp.nwords; base += kPlaceRounds * kPlaceRound) {
            uint4 t[kPlaceRounds];
#pragma unroll
            for (uint32_t r = 0; r < kPlaceRounds; r++) t[r] = place_load(slot[g], (base >> 2) + r * kWave + lane, have[g]);
#pragma unroll
            for (uint32_t r = 0; r < kPlaceRounds; r++)
                if (base + r * kPlaceRound < run[g].sp.nwords)
                    place_round(run[g], base + r * kPlaceRound, lane, t[r], carry, out_words);
        }
    }
}
#endif

// Emission of one segment into its LDS image (rows in LDS, block summaries in registers): offsets
// inside the segment by a DPP prefix sum of the lengths, k by the DPP clamp scan from the k carried
// into the segment.  Word 0 of the image continues `pending`, the open tail word of the wave's
// previous segment.  Returns the segment's bit length and clamp (wave-uniform).
template <int BS, int BYTES>
__device__ __forceinline__ void emit_segment(const Cfg &c, const Seg &g, const uint32_t *rows, uint32_t stride,
                                             uint32_t *obuf, uint32_t lane, uint32_t m, uint32_t kin, uint32_t lead,
                                             uint32_t ref_sample, uint32_t pending, uint32_t &total,
                                             const uint32_t *direct = nullptr,     // the lane's block from direct_finish
                                             const uint32_t *len_incl = nullptr)   // analyze_segment's sums (else scanned here)
{
    const uint32_t bs = BS ? (uint32_t)BS : c.bs;
    const bool pp = c.flags & F_PREPROCESS;
    const bool valid = lane < g.nv;
    const uint32_t len = meta_len(m), opt = meta_opt(m);
    const uint32_t incl = len_incl ? *len_incl : wave_incl_sum(len, lane);
    total = wave_last(incl);
    const uint32_t excl = incl - len;

    // (the summary holds the composition of the segment's clamps up to and including this block, see
    // analyze_segment: the block's k is one clamp of the k carried into the segment)
    const bool updates_k = valid && opt != OPT_ZERO && opt != OPT_ZCONT && c.id_len > 1;
    const uint32_t k = updates_k ? kclamp_apply(KClamp{meta_a(m), meta_b(m)}, kin) : kin;

    // image of the segment; its first word continues the previous segment of this wave, whose
    // open tail word was kept in `pending` instead of being written out
    if (lane == 0) obuf[0] = pending;
    wave_lds_fence();
    {
        const bool emits = valid && opt != OPT_ZCONT;
        const uint32_t ref = (pp && g.b0 == 0 && lane == 0) ? 1u : 0u;
        const uint32_t karg = opt == OPT_ZERO ? meta_a(m) : k;
        constexpr bool PAIRS = BS > 0 && BS <= 16 && Rows<BS, BYTES>::HALF;
        if (PAIRS) {
            // small blocks of 16-bit residuals: emitted from the sample pairs as they are, one placement a block
            // (aec_lane.h emit_small_pairs); the few lanes that are not eligible unpack them for emit_block
            constexpr int NW = PAIRS ? BS / 2 : 1;
            uint32_t pw[NW];
            if (direct) {
#pragma unroll
                for (int j = 0; j < NW; j++) pw[j] = direct[j];
            } else {
                const uint32_t *row = rows + (valid ? lane : 0u) * stride;
#pragma unroll
                for (int q = 0; q < NW / 4; q++) {
                    const uint4 t = *reinterpret_cast<const uint4 *>(row + 4 * q);
                    pw[4 * q] = t.x; pw[4 * q + 1] = t.y; pw[4 * q + 2] = t.z; pw[4 * q + 3] = t.w;
                }
            }
            LdsSink sink{obuf};
            uint32_t ubits = 0, fbits = 0;
            const bool small = emits && pairs_eligible(c, bs, opt, karg, ref, len, ubits, fbits);
            emit_small_pairs<(PAIRS ? BS : 8)>(sink, lead + excl, pw, c, opt, karg, ref, ref_sample, ubits, fbits, small);
            if (__any(emits && !small)) {
                if (emits && !small) {
                    uint32_t dv[2 * NW];
#pragma unroll
                    for (int j = 0; j < NW; j++) {
                        dv[2 * j] = pw[j] & 0xFFFFu;
                        dv[2 * j + 1] = pw[j] >> 16;
                    }
                    BitWriter<LdsSink> bw(sink, lead + excl);
                    emit_block<BS>(bw, dv, c, opt, karg, ref, ref_sample);
                }
            }
            wave_lds_fence();
            return;
        }
        BlockRegs<BS, Rows<BS, BYTES>::HALF> regs;
        const uint32_t *d;
        uint32_t dv[BS ? BS : 1];
        if (direct && BS > 0 && Rows<BS, BYTES>::HALF) {
#pragma unroll
            for (int j = 0; j < (BS ? BS / 2 : 0); j++) {
                dv[2 * j] = direct[j] & 0xFFFFu;
                dv[2 * j + 1] = direct[j] >> 16;
            }
            d = dv;
        } else {
            d = regs.load(rows + (valid ? lane : 0u) * stride);
        }
        LdsSink sink{obuf};
        BitWriter<LdsSink> bw(sink, lead + excl);
        bool done = !emits;
        if (BS > 0 && BS <= 16) {
            // small blocks: unary and field regions assembled in registers (aec_lane.h emit_small)
            uint32_t ubits = 0, fbits = 0;
            const bool small = emits && small_eligible(c, bs, opt, karg, ref, len, ubits, fbits);
            emit_small<(BS > 0 && BS <= 16 ? BS : 8)>(bw, d, c, opt, karg, ref, ref_sample, ubits, fbits, small);
            done = done || small;
        }
        if (BS == 32) {   // (not 64: grouped emission measured slower there -- typical.dat shape 4.53 against 4.36 ms)
            // blocks of 32: the split option appended in groups (aec_lane.h emit_split_groups;
            // C3 pack 2.40 -> 2.19 ms)
            const bool grp = !done && opt == OPT_SPLIT;
            emit_split_groups<(BS == 32 || BS == 64 ? BS : 32)>(bw, d, c, karg, ref, ref_sample, grp);
            done = done || grp;
        }
        if (__any(!done)) {
            if (!done) emit_block<BS>(bw, d, c, opt, karg, ref, ref_sample);
        }
    }
    wave_lds_fence();
}

// ----------------------------------------------------------------------------------------------
// K3: pack
// ----------------------------------------------------------------------------------------------
template <int BS, int BYTES>
__global__ void __launch_bounds__(256)
k_pack(const Cfg c, const uint8_t *__restrict__ in, const uint32_t *__restrict__ meta,
       const uint64_t *__restrict__ seg_start, const uint8_t *__restrict__ seg_kin,
       uint32_t *__restrict__ out_words, uint64_t cap_words, uint32_t segs_per_wave, uint32_t obuf_words,
       uint32_t fast_ok)
{
#define AEC_WAVE_INDEX ((uint64_t)blockIdx.x * (blockDim.x >> 6) + wave)
#include "aec_enc_pack.inc"
#undef AEC_WAVE_INDEX
}

template <int BS, int BYTES>
__global__ void __launch_bounds__(256)
k_pack_chunks(const Cfg call, const uint8_t *__restrict__ d_in, const ChunkDesc *__restrict__ desc,
              const uint32_t *__restrict__ wave_chunk, uint64_t nwaves, const uint32_t *__restrict__ meta_all,
              const uint64_t *__restrict__ seg_start_all, const uint8_t *__restrict__ seg_kin_all,
              uint32_t *__restrict__ out_words, uint64_t cap_words, uint32_t segs_per_wave, uint32_t obuf_words,
              uint32_t fast_ok)
{
    const uint64_t gw = (uint64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (gw >= nwaves) return;
    const ChunkWave cw = chunk_wave(call, d_in, desc, wave_chunk, gw);
    const Cfg &c = cw.c;
    const uint8_t *__restrict__ in = cw.in;
    const uint32_t *__restrict__ meta = meta_all + cw.blk0;
    const uint64_t *__restrict__ seg_start = seg_start_all + cw.seg0;
    const uint8_t *__restrict__ seg_kin = seg_kin_all + cw.seg0;
#define AEC_WAVE_INDEX cw.wave
#include "aec_enc_pack.inc"
#undef AEC_WAVE_INDEX
}

// The kernel's arguments are ONE struct, so that the kernel's argument segment is this struct: what only the end of a run
// needs -- the four per-segment arrays the first pass stores behind its run -- is read from there where it is used
// (local_args) instead of holding eight scalar registers through the segment loop.
struct LocalArgs {
    Cfg c;
    const uint8_t *in;
    uint32_t *seg_bits;
    uint16_t *seg_clamp;
    const uint8_t *seg_kin;
    const uint64_t *seg_start;
    LocalLaunch l;
    uint32_t obuf_words, fast_ok;
};
typedef const __attribute__((address_space(4))) LocalArgs LocalArgsK;
__device__ __forceinline__ LocalArgsK *local_args()
{
    uint64_t p = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    uniform_opaque(p);           // (a load through it is no copy of one the compiler did at the kernel's start)
    return (LocalArgsK *)p;
}

// ----------------------------------------------------------------------------------------------
// K1 and the emission of K3 on the block while it is in registers (aec_enc_local.h)
// ----------------------------------------------------------------------------------------------
// A wavefront analyses segments [wave * segs_per_wave, + segs_per_wave) as k_analyze does and emits each of them at once,
// as k_pack does, into its own slot of `image`, from bit 0 of the slot on.  The k carried into the run is a guess
// (local_guess), inside the run the carry is exact given the guess.  REDO: the same text after the scan, for the runs
// where the guess made a block take another k than the true one (local_missed) -- the carry then comes from seg_kin,
// the positions inside the slot from seg_start, and nothing is written but the slot, whose layout the carried k does
// not move.
// (The redo of blocks of 16 8-bit samples is told to stay at the seven waves per SIMD it had: left alone the allocator takes
// 73 registers, one more than seven waves allow; with the hint 71, no scratch -- that was with 46 scalar registers spilled;
// without them it takes 60 with the hint and 62 without, and the hint has stayed.  The other instantiations are not bound.)
template <int BS, int BYTES, bool REDO>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(REDO && BS == 16 && BYTES == 1 ? 7 : 1)))
k_encode_local(const LocalArgs a)
{
    const LocalLaunch &l = a.l;
    const uint8_t *__restrict__ in = a.in;
    const uint8_t *__restrict__ seg_kin = a.seg_kin;
    const uint64_t *__restrict__ seg_start = a.seg_start;
    const uint32_t obuf_words = a.obuf_words;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr uint32_t stride = Rows<BS, BYTES>::stride_words(BS);
    const uint32_t per_wave = 64u * stride + obuf_words;
    uint32_t rows_at = wave * per_wave;             // the wavefront's rows in smem, the segment's image behind them
    uint32_t *rows = smem + rows_at, *obuf = rows + 64u * stride;
    Cfg c = a.c;                 // (these pass through uniform_opaque once a segment, see the loop)
    c.bs = BS;                   // what the instantiation fixes: sample and byte offsets by shifts, two registers fewer
    c.bytes = BYTES;
    uint32_t guess = l.guess, fast_ok = a.fast_ok;

    const uint64_t gwave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    const uint64_t run0 = gwave * l.segs_per_wave;      // the run's first segment
    if (run0 >= c.total_segs) return;
    // a run is at most 32 segments (local_plan): inside it a segment is a 32-bit index from run0
    const uint64_t left = c.total_segs - run0;
    const uint32_t nrun = left < l.segs_per_wave ? (uint32_t)left : l.segs_per_wave;
    uint32_t si = 0, si_end = nrun;                     // segments [si, si_end) of the run are coded
    uint32_t *__restrict__ slot = l.image + gwave * l.slot_words;
    uint32_t pending = 0;        // open tail word of the previous segment
    uint32_t pos = 0;            // bits of the run so far = where the segment starts in the slot
    bool merge_tail = false;     // REDO: the last segment coded again ends in a word that goes on with an untouched one
    uint32_t keep_bk = 0, keep_cf = 0;      // lane s: bits | k used << 24 and clamp | first clamp << 16 of segment run0 + s
    if (REDO) {
        bool miss = false;
        const uint64_t s = run0 + lane;
        if (lane < nrun) miss = local_missed(l.seg_first[s], l.seg_kused[s], seg_kin[s]);
        const uint64_t missed = __ballot(miss);
        if (!missed) return;
        // only the segments from the first to the last miss (aec_enc_local.h): positions from the scan, the open words
        // at both ends shared with what stays in the slot
        const LocalRedo range = local_redo_range(missed);
        merge_tail = range.end < nrun;
        si_end = range.end;
        si = range.first;
        pos = (uint32_t)(seg_start[run0 + si] - seg_start[run0]);
        if (pos & 31u) pending = local_redo_head(slot[pos >> 5], pos);
    }

    Feeder<BS, BYTES> feeder;
    feeder.init(c, fast_ok);
    Seg gnext = seg_geom(c, run0 + si);
    feeder.prefetch_direct(c, in, gnext, lane);
    uint32_t k = l.k_in;         // carried k (exact from the first k-updating block on)
    bool have_k = gwave == 0;    // ... or from the start, for the call's first wavefront
    for (uint32_t w = lane; w < obuf_words; w += kWave) obuf[w] = 0u;

    auto do_segment = [&](const Seg &g, uint32_t ref_sample, uint32_t at, const uint32_t *direct) {
        wave_lds_fence();
        uint32_t tot, cl, incl;
        const uint32_t m = analyze_segment<BS, BYTES>(c, g, rows, stride, lane, tot, cl, direct, &incl);
        const uint32_t opt = meta_opt(m);
        const uint64_t upd = __ballot(lane < g.nv && opt != OPT_ZERO && opt != OPT_ZCONT && c.id_len > 1);
        // (the summary of the FIRST block that updates k holds that block's own clamp: nothing is composed in front)
        uint32_t first = kLocalNoClamp;
        if (upd) first = __builtin_amdgcn_readlane(__builtin_amdgcn_perm(0u, m, 0x0c0c0302u), (int)__builtin_ctzll(upd));
        uint32_t kin;
        if (REDO) {
            kin = seg_kin[run0 + at];
        } else {
            if (!have_k && upd) {
                k = local_guess(first, guess);
                have_k = true;
            }
            kin = k;
            // what the segment leaves for the scan and the redo: lane s keeps segment s of the run (all four are
            // wave-uniform; a segment is less than 2^24 bits, a k less than 2^8), stored once behind the run
            keep_bk = wave_set_lane(keep_bk, lane, at, tot | (kin << 24));
            keep_cf = wave_set_lane(keep_cf, lane, at, (cl & 0xFFFFu) | (first << 16));
            k = kclamp_apply(clamp_unpack(cl), k);
        }
        const uint32_t lead = pos & 31u;
        uint32_t total;
        // (the lengths were scanned for `tot`: emit_segment takes the sums as they are)
        emit_segment<BS, BYTES>(c, g, rows, stride, obuf, lane, m, kin, lead, ref_sample, pending, total, direct, &incl);
        // copy-out as k_pack's, without its shared words: the slot is this wavefront's alone
        const uint32_t nwords = (lead + total + 31u) >> 5, gw = pos >> 5;
        const bool carry_tail = ((lead + total) & 31u) != 0 && at + 1 != si_end && nwords > 0;
        const uint32_t tail_word = carry_tail ? obuf[nwords - 1] : 0u;
        const uint32_t tail = (lead + total) & 31u;
        for (uint32_t w = lane; w < nwords; w += kWave) {
            uint32_t v = obuf[w];
            obuf[w] = 0u;
            if (REDO && merge_tail && tail != 0 && at + 1 == si_end && w == nwords - 1)
                v = local_redo_tail(v, slot[gw + w], tail);
            if (!(carry_tail && w == nwords - 1)) slot[gw + w] = v;
        }
        pending = tail_word;
        pos += total;
        wave_lds_fence();
    };

    for (; si < si_end; si++) {
        // What follows from the parameters alone -- masks, sums, shifted constants, every flag as a 64-bit lane mask -- the
        // compiler computes in front of the loop and keeps for all of it: some forty scalar registers more than there are,
        // spilled to the lanes of a vector register and read back one v_readlane at a time inside the segment.  Behind
        // uniform_opaque the values are the segment's own: computed where a segment uses them, on the scalar unit.
        uniform_opaque(c.bps); uniform_opaque(c.flags); uniform_opaque(c.id_len); uniform_opaque(c.kmax);
        uniform_opaque(c.xmax); uniform_opaque(guess); uniform_opaque(rows_at);
        uniform_opaque(c.total_samples); uniform_opaque(fast_ok);
        rows = smem + rows_at;
        obuf = rows + 64u * stride;
        feeder.init(c, fast_ok);          // (the feeder's limits and its flag, a lane mask, are derived values too)
        const bool pp = c.flags & F_PREPROCESS, msb = c.flags & F_MSB;
        const auto cur = feeder.pre_direct;
        const Seg g = gnext;
        const bool direct = feeder.direct_ok(c, g);
        uint32_t ref_sample = 0;
        if (pp && g.b0 == 0) {
            // the reference sample of an RSI is the first sample of lane 0's block: on the direct path from the words
            // the lane holds (as load_sample_raw has it), else by a load of lane 0's own
            constexpr uint32_t one = BYTES == 2 ? 0xFFFFu : 0xFFu;
            if (direct)
                ref_sample = __builtin_amdgcn_readfirstlane(sample_byte_order<BYTES>(cur.raw[0] & one, msb)) & low_mask32(c.bps);
            else if (lane == 0)
                ref_sample = load_sample_bytes(in + g.samp0 * c.bytes, c.bytes, msb) & low_mask32(c.bps);
        }
        if (si + 1 < si_end) gnext = seg_next(c, gnext);
        feeder.prefetch_direct(c, in, gnext, lane);       // the next segment's loads fly during this one
        if (direct) {
            uint32_t w[BS / 2];
            direct_finish<BS, BYTES>(c, g, cur, lane, w);
            do_segment(g, ref_sample, si, w);
        } else {
            feeder.feed_now(c, in, g, rows, stride, lane);
            do_segment(g, ref_sample, si, nullptr);
        }
    }
    if (!REDO && lane < si_end) {
        const LocalArgsK *k_args = local_args();
        k_args->seg_bits[run0 + lane] = keep_bk & 0xFFFFFFu;
        k_args->seg_clamp[run0 + lane] = (uint16_t)keep_cf;
        k_args->l.seg_first[run0 + lane] = (uint16_t)(keep_cf >> 16);
        k_args->l.seg_kused[run0 + lane] = (uint8_t)(keep_bk >> 24);
    }
}

// ----------------------------------------------------------------------------------------------
// dispatch
// ----------------------------------------------------------------------------------------------
struct LaunchGeom {
    uint32_t waves_per_block;
    uint32_t segs_per_wave;
    uint32_t grid;
    size_t lds_bytes;
    uint32_t obuf_words;
};

LaunchGeom make_geom(const Cfg &c, bool with_obuf)
{
    LaunchGeom g;
    const bool templated = c.bs == 8 || c.bs == 16 || c.bs == 32 || c.bs == 64;
    const uint32_t stride = (templated && c.bytes <= 2) ? c.bs / 2 + 4 : c.bs + 4;   // Rows<>::stride_words
    const uint32_t maxlen = c.id_len + c.bs * c.bps + 2 + c.bps;
    g.obuf_words = with_obuf ? ((64u * maxlen + 62u) / 32u + 4u) & ~3u : 0u;
    const size_t per_wave = ((size_t)64 * stride + g.obuf_words) * 4;
    uint32_t wpb = (uint32_t)(65536 / per_wave);
    if (wpb > 4) wpb = 4;
    if (wpb < 1) wpb = 1;
    g.waves_per_block = wpb;
    g.lds_bytes = per_wave * wpb;
    // A wave walks a run of consecutive segments: interior word boundaries then stay inside the
    // wave (no atomics) and the next segment's loads overlap the current one.  Small inputs are
    // spread over the chip instead.
    uint32_t spw = 8;
    while (spw > 1 && c.total_segs < (uint64_t)spw * wpb * 2048) spw >>= 1;
    g.segs_per_wave = spw;
    const uint64_t waves = (c.total_segs + spw - 1) / spw;
    g.grid = (uint32_t)((waves + wpb - 1) / wpb);
    return g;
}

template <int BS, int BYTES>
void launch_analyze_t(const Cfg &c, const uint8_t *in, const EncWorkspace &ws, uint32_t fast_ok,
                      hipStream_t st)
{
    const LaunchGeom g = make_geom(c, false);
    hipLaunchKernelGGL((k_analyze<BS, BYTES>), dim3(g.grid), dim3(64 * g.waves_per_block), g.lds_bytes, st,
                       c, in, ws.meta, ws.seg_bits, ws.seg_clamp, g.segs_per_wave, fast_ok);
}

template <int BS, int BYTES>
void launch_pack_t(const Cfg &c, const uint8_t *in, const EncWorkspace &ws, uint32_t *out_words,
                   uint64_t cap_words, uint32_t fast_ok, hipStream_t st)
{
    const LaunchGeom g = make_geom(c, true);
    hipLaunchKernelGGL((k_pack<BS, BYTES>), dim3(g.grid), dim3(64 * g.waves_per_block), g.lds_bytes, st,
                       c, in, ws.meta, ws.seg_start, ws.seg_kin, out_words, cap_words, g.segs_per_wave,
                       g.obuf_words, fast_ok);
}

template <int BS, int BYTES>
void launch_local_t(bool redo, const Cfg &c, const uint8_t *in, const EncWorkspace &ws, const LocalLaunch &l, uint32_t fast_ok,
                    hipStream_t st)
{
    if constexpr (Feeder<BS, BYTES>::DIRECT) {
        const LaunchGeom g = make_geom(c, true);
        const uint64_t waves = (c.total_segs + l.segs_per_wave - 1) / l.segs_per_wave;
        const uint32_t grid = (uint32_t)((waves + g.waves_per_block - 1) / g.waves_per_block);
        const LocalArgs a{c, in, ws.seg_bits, ws.seg_clamp, ws.seg_kin, ws.seg_start, l, g.obuf_words, fast_ok};
        if (redo)
            hipLaunchKernelGGL((k_encode_local<BS, BYTES, true>), dim3(grid), dim3(64 * g.waves_per_block), g.lds_bytes, st, a);
        else
            hipLaunchKernelGGL((k_encode_local<BS, BYTES, false>), dim3(grid), dim3(64 * g.waves_per_block), g.lds_bytes, st, a);
    } else {
        // local_plan opens the route for direct_shape() only: a launch without a kernel leaves the call's launch error set
        (void)hipLaunchKernel(nullptr, dim3(1), dim3(1), nullptr, 0, st);
    }
}

template <int BS, int BYTES>
void launch_chunks_t(bool pack, const Cfg &c, const uint8_t *in, const ChunksLaunch &k, const EncWorkspace &ws,
                     uint32_t *out_words, uint64_t cap_words, uint32_t fast_ok, hipStream_t st)
{
    const LaunchGeom g = make_geom(c, pack);
    const uint32_t grid = (uint32_t)((k.nwaves + g.waves_per_block - 1) / g.waves_per_block);
    if (pack)
        hipLaunchKernelGGL((k_pack_chunks<BS, BYTES>), dim3(grid), dim3(64 * g.waves_per_block), g.lds_bytes, st, c, in,
                           k.desc, k.wave_chunk, k.nwaves, ws.meta, ws.seg_start, ws.seg_kin, out_words, cap_words,
                           k.segs_per_wave, g.obuf_words, fast_ok);
    else
        hipLaunchKernelGGL((k_analyze_chunks<BS, BYTES>), dim3(grid), dim3(64 * g.waves_per_block), g.lds_bytes, st, c, in,
                           k.desc, k.wave_chunk, k.nwaves, ws.meta, ws.seg_bits, ws.seg_clamp, k.segs_per_wave, fast_ok);
}

template <int BS>
void dispatch_bytes(bool pack, const Cfg &c, const uint8_t *in, const EncWorkspace &ws,
                    uint32_t *out_words, uint64_t cap_words, uint32_t fast_ok, hipStream_t st)
{
#define AEC_GO(B)                                                                     \
    do {                                                                              \
        if (pack) launch_pack_t<BS, B>(c, in, ws, out_words, cap_words, fast_ok, st); \
        else launch_analyze_t<BS, B>(c, in, ws, fast_ok, st);                         \
    } while (0)
    switch (c.bytes) {
    case 1: AEC_GO(1); break;
    case 2: AEC_GO(2); break;
    case 3: AEC_GO(3); break;
    default: AEC_GO(4); break;
    }
#undef AEC_GO
}

}  // namespace

#ifdef AEC_ENC_PART
// ---- the kernels of ONE block size (this object: -DAEC_ENC_PART=<block size>, 0 = any other) --------------------------------
template <int BS>
void enc_part(bool pack, const Cfg &c, const uint8_t *in, const EncWorkspace &ws, uint32_t *out_words, uint64_t cap_words,
              uint32_t fast_ok, hipStream_t st)
{
    if constexpr (BS == 0) {
        if (pack) launch_pack_t<0, 0>(c, in, ws, out_words, cap_words, 0, st);
        else launch_analyze_t<0, 0>(c, in, ws, 0, st);
    } else {
        dispatch_bytes<BS>(pack, c, in, ws, out_words, cap_words, fast_ok, st);
    }
}
template void enc_part<AEC_ENC_PART>(bool, const Cfg &, const uint8_t *, const EncWorkspace &, uint32_t *, uint64_t, uint32_t,
                                     hipStream_t);
template <int BS>
void enc_part_chunks(bool pack, const Cfg &c, const uint8_t *in, const ChunksLaunch &k, const EncWorkspace &ws, uint32_t *out_words,
                     uint64_t cap_words, uint32_t fast_ok, hipStream_t st)
{
    if constexpr (BS == 0) {
        launch_chunks_t<0, 0>(pack, c, in, k, ws, out_words, cap_words, 0, st);
    } else {
        switch (c.bytes) {
        case 1: launch_chunks_t<BS, 1>(pack, c, in, k, ws, out_words, cap_words, fast_ok, st); break;
        case 2: launch_chunks_t<BS, 2>(pack, c, in, k, ws, out_words, cap_words, fast_ok, st); break;
        case 3: launch_chunks_t<BS, 3>(pack, c, in, k, ws, out_words, cap_words, fast_ok, st); break;
        default: launch_chunks_t<BS, 4>(pack, c, in, k, ws, out_words, cap_words, fast_ok, st); break;
        }
    }
}
template void enc_part_chunks<AEC_ENC_PART>(bool, const Cfg &, const uint8_t *, const ChunksLaunch &, const EncWorkspace &,
                                            uint32_t *, uint64_t, uint32_t, hipStream_t);
#if AEC_ENC_PART == 8 || AEC_ENC_PART == 16 || AEC_ENC_PART == 32
template <int BS>
void enc_part_local(bool redo, const Cfg &c, const uint8_t *in, const EncWorkspace &ws, const LocalLaunch &l, uint32_t fast_ok,
                    hipStream_t st)
{
    if (c.bytes == 1) launch_local_t<BS, 1>(redo, c, in, ws, l, fast_ok, st);
    else launch_local_t<BS, 2>(redo, c, in, ws, l, fast_ok, st);
}
template void enc_part_local<AEC_ENC_PART>(bool, const Cfg &, const uint8_t *, const EncWorkspace &, const LocalLaunch &, uint32_t,
                                           hipStream_t);
#endif

#else       // ---- the object without a part ------------------------------------------------------------------------
#define AEC_ENC_EXTERN(BS)                                                                                                  \
    extern template void enc_part<BS>(bool, const Cfg &, const uint8_t *, const EncWorkspace &, uint32_t *, uint64_t, uint32_t, \
                                      hipStream_t);
AEC_ENC_EXTERN(0) AEC_ENC_EXTERN(8) AEC_ENC_EXTERN(16) AEC_ENC_EXTERN(32) AEC_ENC_EXTERN(64)
#undef AEC_ENC_EXTERN
#define AEC_ENC_EXTERN(BS)                                                                                                  \
    extern template void enc_part_local<BS>(bool, const Cfg &, const uint8_t *, const EncWorkspace &, const LocalLaunch &,    \
                                            uint32_t, hipStream_t);
AEC_ENC_EXTERN(8) AEC_ENC_EXTERN(16) AEC_ENC_EXTERN(32)
#undef AEC_ENC_EXTERN

#define AEC_ENC_EXTERN(BS)                                                                                                  \
    extern template void enc_part_chunks<BS>(bool, const Cfg &, const uint8_t *, const ChunksLaunch &, const EncWorkspace &, \
                                             uint32_t *, uint64_t, uint32_t, hipStream_t);
AEC_ENC_EXTERN(0) AEC_ENC_EXTERN(8) AEC_ENC_EXTERN(16) AEC_ENC_EXTERN(32) AEC_ENC_EXTERN(64)
#undef AEC_ENC_EXTERN

static void dispatch_chunks(bool pack, const Cfg &c, const uint8_t *in, const ChunksLaunch &k, const EncWorkspace &ws,
                            uint32_t *out_words, uint64_t cap_words, uint32_t fast_ok, hipStream_t st)
{
    switch (c.bs) {
    case 8: enc_part_chunks<8>(pack, c, in, k, ws, out_words, cap_words, fast_ok, st); break;
    case 16: enc_part_chunks<16>(pack, c, in, k, ws, out_words, cap_words, fast_ok, st); break;
    case 32: enc_part_chunks<32>(pack, c, in, k, ws, out_words, cap_words, fast_ok, st); break;
    case 64: enc_part_chunks<64>(pack, c, in, k, ws, out_words, cap_words, fast_ok, st); break;
    default: enc_part_chunks<0>(pack, c, in, k, ws, out_words, cap_words, fast_ok, st); break;
    }
}

static void dispatch(bool pack, const Cfg &c, const uint8_t *in, const EncWorkspace &ws, uint32_t *out_words,
                     uint64_t cap_words, uint32_t fast_ok, hipStream_t st)
{
    switch (c.bs) {
    case 8: enc_part<8>(pack, c, in, ws, out_words, cap_words, fast_ok, st); break;
    case 16: enc_part<16>(pack, c, in, ws, out_words, cap_words, fast_ok, st); break;
    case 32: enc_part<32>(pack, c, in, ws, out_words, cap_words, fast_ok, st); break;
    case 64: enc_part<64>(pack, c, in, ws, out_words, cap_words, fast_ok, st); break;
    default: enc_part<0>(pack, c, in, ws, out_words, cap_words, fast_ok, st); break;
    }
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- the route that codes every block once (aec_enc_local.h) ------------------------------------------------------------
// Open to a plain whole encode (launch_encode: ENC_ALL, no ShardCarry) of a shape whose kernels hold the block in the
// lane's registers (Feeder::DIRECT, preprocessor on).  Taken where it was measured to win (profiles/r11/README.md):
// 16-bit samples in blocks of 16 in RSIs of whole segments (rsi a multiple of 64: every segment has its 64 blocks, as at
// the measured rsi 128), from kLocalMinSegs such segments (256 MiB) on -- below, the additional launch and the copy of
// the stream cost more than the second feed of the input.  8-bit samples in blocks of 8 lose at every size (their runs
// are a quarter as long, and the placement pays per run); RSIs of part segments have shorter runs still and were not
// measured.  The tuning build takes it for every open shape with AEC_ENC_LOCAL=1.
// A wavefront's run is the 8 segments of the other kernels, and kLocalLongRun segments from kLocalLongSegs segments
// (2 GiB) on: a quarter as many run starts -- guesses, candidates for the redo, shared words and part lines for the
// placement -- take 0.08 ms off 2.72 at 2 GiB and 0.22 off 5.35 at 4 GiB (placement 0.39 - 0.42 against 0.53 - 0.56 ms),
// while at 1 GiB and below the fewer, longer wavefronts of k_encode_local cost what the placement saves, or more
// (profiles/r15/README.md).
static const uint64_t kLocalMinSegs = 131072;
static const uint64_t kLocalLongSegs = 1u << 20;
static const uint32_t kLocalLongRun = 32;

struct LocalPlan {
    bool on;
    uint32_t segs_per_wave, slot_words, guess;
    uint64_t waves;
    size_t off_first, off_kused, bytes;        // inside the area: the image at 0, then the two per-segment arrays
};

static LocalPlan local_plan(const Cfg &c)
{
    LocalPlan p{};
    const bool direct = (c.bs == 8 || c.bs == 16 || c.bs == 32) && direct_shape(c.bs, c.bytes);
    const uint32_t force = tune("AEC_ENC_LOCAL", 2);
    const bool wins = c.bs == 16 && c.bytes == 2 && c.rsi % 64 == 0 && c.total_segs >= kLocalMinSegs;
    p.on = direct && (c.flags & F_PREPROCESS) && c.total_segs != 0 && force != 0 && (force == 1 || wins);
    if (!p.on) return p;
    p.segs_per_wave = wins && c.total_segs >= kLocalLongSegs ? kLocalLongRun : make_geom(c, true).segs_per_wave;
    const uint32_t spw = tune("AEC_ENC_LOCAL_SPW", 0);
    if (spw == 1 || spw == 2 || spw == 4 || spw == 8 || spw == 16 || spw == 32) p.segs_per_wave = spw;
    p.guess = tune_set("AEC_ENC_LOCAL_GUESS") ? tune("AEC_ENC_LOCAL_GUESS", 0) & 0xFFu : kLocalGuessRule;
    p.slot_words = local_slot_words(c.id_len, c.bs, c.bps, c.rsi, p.segs_per_wave);
    p.waves = (c.total_segs + p.segs_per_wave - 1) / p.segs_per_wave;
    p.off_first = align_up((size_t)p.waves * p.slot_words * 4, 256);
    p.off_kused = align_up(p.off_first + c.total_segs * 2, 256);
    p.bytes = align_up(p.off_kused + c.total_segs, 256);
    return p;
}

// off_local (optional): the caller is a plain whole encode.  Where that takes the route above, *off_local is where its
// area starts (image, first clamps, used k: 17.4 KiB per 16 KiB of input at 16 bits, block 16 -- 4.66 GB at 4 GiB) and
// the per-block summaries, which it does not write, take no room; 0 otherwise.
size_t enc_workspace_bytes(const Cfg &c, size_t *off_meta, size_t *off_bits, size_t *off_clamp,
                           size_t *off_start, size_t *off_kin, size_t *off_part, size_t *off_local)
{
    size_t o = 0;
    const uint64_t nseg = c.total_segs ? c.total_segs : 1;
    const uint64_t nchunks = (nseg + kScanChunk - 1) / kScanChunk + 1;
    const LocalPlan lp = off_local ? local_plan(c) : LocalPlan{};
    *off_meta = o;  o = align_up(o + (lp.on ? 1 : c.total_blocks + 1) * 4, 256);
    *off_bits = o;  o = align_up(o + nseg * 4, 256);
    *off_clamp = o; o = align_up(o + nseg * 2, 256);
    *off_start = o; o = align_up(o + nseg * 8, 256);
    *off_kin = o;   o = align_up(o + nseg, 256);
    *off_part = o;  o = align_up(o + nchunks * sizeof(ScanPartial), 256);
    if (off_local) {
        *off_local = lp.on ? o : 0;
        o += lp.bytes;
    }
    return o;
}

void launch_encode(const Cfg &c, const uint8_t *d_in, uint8_t *d_out, size_t out_cap,
                   uint32_t start_bit, uint32_t k_in, const EncWorkspace &ws, uint64_t *d_rsi_off,
                   EncResult *d_res, hipStream_t st, const PhaseEvents *prof, uint32_t phases,
                   SegEntry *d_seg_table, const ShardCarry *d_carry)
{
    auto mark = [&](int i) { if (prof) (void)hipEventRecord(prof->ev[i], st); };
    uint32_t *out_words = reinterpret_cast<uint32_t *>(d_out);
    const uint64_t cap_words = out_cap / 4;
    const uint64_t nseg = c.total_segs;
    const uint64_t nchunks = (nseg + kScanChunk - 1) / kScanChunk;
    // fast loads need every segment to start on a 16-byte boundary of a 16-byte aligned buffer
    const uint32_t fast_ok = ((reinterpret_cast<uintptr_t>(d_in) & 15u) == 0 &&
                              ((uint64_t)c.rsi * c.bs * c.bytes) % 16 == 0) ? 1u : 0u;

    if (phases == ENC_ALL && ws.local && !d_carry) {
        // every block coded once: local encode | scan | redo of the missed runs | placement
        const LocalPlan lp = local_plan(c);
        const LocalLaunch l{reinterpret_cast<uint32_t *>(ws.local), reinterpret_cast<uint16_t *>(ws.local + lp.off_first),
                            ws.local + lp.off_kused, lp.slot_words, lp.segs_per_wave, k_in, lp.guess};
        auto part = [&](bool redo) {
            switch (c.bs) {
            case 8: enc_part_local<8>(redo, c, d_in, ws, l, fast_ok, st); break;
            case 16: enc_part_local<16>(redo, c, d_in, ws, l, fast_ok, st); break;
            default: enc_part_local<32>(redo, c, d_in, ws, l, fast_ok, st); break;
            }
        };
        mark(0);
        part(false);
        mark(1);
        hipLaunchKernelGGL(k_scan_reduce, dim3((uint32_t)nchunks), dim3(256), 0, st, ws.seg_bits, ws.seg_clamp, nseg,
                           ws.partials);
        hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(256), 0, st, ws.partials, nchunks, start_bit, k_in, d_res);
        hipLaunchKernelGGL(k_scan_apply, dim3((uint32_t)nchunks), dim3(256), 0, st, ws.seg_bits, ws.seg_clamp, nseg,
                           ws.partials, start_bit, k_in, c.segs_per_rsi, c.rsi_count, ws.seg_start, ws.seg_kin, d_rsi_off,
                           d_res, out_words, cap_words, lp.segs_per_wave, d_carry);
        if (d_seg_table)
            hipLaunchKernelGGL(k_seg_table, dim3((uint32_t)((nseg + 255) / 256)), dim3(256), 0, st, c, d_in, ws.seg_start,
                               d_seg_table);
        mark(2);
        part(true);
        mark(3);
        hipLaunchKernelGGL(k_place, dim3((uint32_t)((lp.waves + 4 * kPlaceSlots - 1) / (4 * kPlaceSlots))), dim3(256), 0, st,
                           l.image, lp.slot_words, ws.seg_start, nseg, lp.segs_per_wave, lp.waves, start_bit, d_res,
                           out_words, cap_words);
        mark(4);
        return;
    }
    if (phases & ENC_PLAN) {
        mark(0);
        if (nseg) dispatch(false, c, d_in, ws, nullptr, 0, fast_ok, st);
        mark(1);
        if (nchunks)
            hipLaunchKernelGGL(k_scan_reduce, dim3((uint32_t)nchunks), dim3(256), 0, st, ws.seg_bits,
                               ws.seg_clamp, nseg, ws.partials);
        hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(256), 0, st, ws.partials, nchunks, start_bit, k_in,
                           d_res);
    }
    if (phases & ENC_EMIT) {
        if (nchunks)
            hipLaunchKernelGGL(k_scan_apply, dim3((uint32_t)nchunks), dim3(256), 0, st, ws.seg_bits,
                               ws.seg_clamp, nseg, ws.partials, start_bit, k_in, c.segs_per_rsi, c.rsi_count,
                               ws.seg_start, ws.seg_kin, d_rsi_off, d_res, out_words, cap_words,
                               make_geom(c, true).segs_per_wave, d_carry);
        else {
            if (d_rsi_off) (void)hipMemsetAsync(d_rsi_off, 0, sizeof(uint64_t), st);   // empty batch: single entry
            if (out_cap >= 16) (void)hipMemsetAsync(d_out, 0, 16, st);
        }
        if (d_seg_table && nseg)
            hipLaunchKernelGGL(k_seg_table, dim3((uint32_t)((nseg + 255) / 256)), dim3(256), 0, st, c, d_in,
                               ws.seg_start, d_seg_table);
        mark(2);
        mark(3);   // (the buffer is no longer cleared: k_scan_apply zeroes the few shared words)
        if (nseg) dispatch(true, c, d_in, ws, out_words, cap_words, fast_ok, st);
        mark(4);
    }
}

// c describes the concatenation of n_chunks chunks of segs_per_chunk segments each (whole RSIs)
bool batch_uniform_ok(const Cfg &c, uint64_t segs_per_chunk)
{
    if (segs_per_chunk == 0 || segs_per_chunk > kScanChunk || c.total_segs % segs_per_chunk) return false;
    return segs_per_chunk % make_geom(c, true).segs_per_wave == 0;       // no wavefront works across a chunk border
}

void launch_encode_uniform_batch(const Cfg &c, const uint8_t *d_in, uint64_t segs_per_chunk, uint8_t *d_out,
                                 size_t out_cap, const EncWorkspace &ws, BatchChunk *d_chunks, EncResult *d_res,
                                 hipStream_t st)
{
    uint32_t *out_words = reinterpret_cast<uint32_t *>(d_out);
    const uint64_t cap_words = out_cap / 4;
    const uint32_t n = (uint32_t)(c.total_segs / segs_per_chunk);
    const uint32_t fast_ok = ((reinterpret_cast<uintptr_t>(d_in) & 15u) == 0 &&
                              ((uint64_t)c.rsi * c.bs * c.bytes) % 16 == 0) ? 1u : 0u;
    dispatch(false, c, d_in, ws, nullptr, 0, fast_ok, st);
    hipLaunchKernelGGL(k_batch_reduce, dim3(n), dim3(256), 0, st, ws.seg_bits, (uint32_t)segs_per_chunk, d_chunks);
    hipLaunchKernelGGL(k_batch_bases, dim3(1), dim3(256), 0, st, d_chunks, (uint64_t)n, (uint64_t)out_cap, d_res);
    hipLaunchKernelGGL(k_batch_apply, dim3(n), dim3(256), 0, st, ws.seg_bits, ws.seg_clamp, (uint32_t)segs_per_chunk,
                       d_chunks, ws.seg_start, ws.seg_kin, out_words, cap_words, make_geom(c, true).segs_per_wave);
    dispatch(true, c, d_in, ws, out_words, cap_words, fast_ok, st);
}

// c describes the sum of the chunks (total_blocks, total_segs, rsi_count summed over them)
uint32_t chunks_segs_per_wave(const Cfg &c)
{
    return make_geom(c, true).segs_per_wave;
}

void launch_encode_chunks(const Cfg &c, const uint8_t *d_in, const ChunksLaunch &k, uint8_t *d_out, size_t out_cap,
                          const EncWorkspace &ws, BatchChunk *d_chunks, uint64_t *d_rsi_off, EncResult *d_res, hipStream_t st)
{
    static_assert(sizeof(CkVal) == sizeof(ScanPartial), "the tile aggregates live where the scan partials do");
    uint32_t *out_words = reinterpret_cast<uint32_t *>(d_out);
    const uint64_t cap_words = out_cap / 4;
    const uint64_t nseg = c.total_segs, ntiles = (nseg + kScanChunk - 1) / kScanChunk;
    CkVal *tiles = reinterpret_cast<CkVal *>(ws.partials);
    // (chunk offsets are multiples of 16, so a chunk's segments start on 16-byte boundaries as a single input's do)
    const uint32_t fast_ok = ((reinterpret_cast<uintptr_t>(d_in) & 15u) == 0 &&
                              ((uint64_t)c.rsi * c.bs * c.bytes) % 16 == 0) ? 1u : 0u;
    const uint64_t most = k.nwaves > k.n ? k.nwaves : k.n;
    uint64_t setup_grid = (most + 255) / 256;
    if (setup_grid > 4096) setup_grid = 4096;
    hipLaunchKernelGGL(k_chunks_setup, dim3((uint32_t)setup_grid), dim3(256), 0, st, k.desc, k.n, k.nwaves, k.wave_chunk,
                       d_chunks);
    if (nseg) {
        dispatch_chunks(false, c, d_in, k, ws, nullptr, 0, fast_ok, st);
        hipLaunchKernelGGL(k_chunks_reduce, dim3((uint32_t)ntiles), dim3(256), 0, st, k.desc, k.n, ws.seg_bits, ws.seg_clamp,
                           nseg, tiles, d_chunks);
    }
    hipLaunchKernelGGL(k_chunks_bases, dim3(1), dim3(256), 0, st, k.desc, d_chunks, k.n, tiles, ntiles, d_out,
                       (uint64_t)out_cap, d_rsi_off, d_res);
    if (nseg) {
        hipLaunchKernelGGL(k_chunks_apply, dim3((uint32_t)ntiles), dim3(256), 0, st, k.desc, k.n, ws.seg_bits, ws.seg_clamp,
                           nseg, tiles, d_chunks, c.segs_per_rsi, k.segs_per_wave, ws.seg_start, ws.seg_kin, d_rsi_off,
                           out_words, cap_words);
        dispatch_chunks(true, c, d_in, k, ws, out_words, cap_words, fast_ok, st);
    }
}

#endif      // AEC_ENC_PART

}  // namespace aec
