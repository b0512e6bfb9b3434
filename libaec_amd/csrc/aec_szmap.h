// aec_szmap.h -- the index arithmetic of the SZIP layer on the device (aec_sz.hip; include/aec_gpu_sz.h; DESIGN.md §2
// "SZIP chunks on the device").  Restates prepare_compress / finish_decompress of sz_abi.cpp (reference
// src/sz_compat.c:39-108, 134-166, 208-261) as two maps over the bytes of ONE chunk:
//   coder-input byte  -> chunk byte to copy (a byte of the scan line, or of the pixel the padding repeats), or zero
//   chunk byte        -> coder-output byte (or zero: the trailing fraction of a pixel, which is never coded)
// The kernels are loops of these over 16-byte groups; tests/emul/sz_emul.cpp runs the same functions on the CPU
// against vectors the reference's shim produced.
#pragma once

#include "aec_cfg.h"

namespace aec {

constexpr int kSzMsbOption = 16, kSzNnOption = 32;      // SZ_MSB_OPTION_MASK, SZ_NN_OPTION_MASK (szlib.h)
constexpr uint64_t kSzZero = ~0ull;                     // "no source byte: zero"

// One chunk under one SZ_com_t.  With byte planes (32- / 64-bit pixels, sz_compat.c:134) the coder sees 8-bit samples
// and a scan line is `line` BYTES of the concatenated planes: it may start in one plane and end in the next.
struct SzLayout {
    uint32_t bps, bs, rsi, flags;   // the coder's parameters (flags with F_NOT_ENFORCE: what the encoder is given)
    uint32_t word;                  // 0, or bytes per pixel (4 / 8) when byte planes are used
    uint32_t pixel;                 // container bytes of a coded sample: 1 / 2 / 4
    uint32_t repeat;                // padding repeats the last pixel (NN) instead of zero
    uint32_t passthrough;           // no planes, no padding, whole lines, whole pixels: the chunk IS the coder's input
    uint64_t line, padded_line;     // bytes of a scan line, and of the RSI it becomes
    uint64_t lines;                 // scan lines (= RSIs) per chunk, the last one may be partial
    uint64_t coder_bytes;           // lines * padded_line
    uint64_t coded_bytes;           // the whole pixels of the chunk (sz_abi.cpp:87-90)
    uint64_t chunk_bytes;
    uint64_t pixels;                // planes: pixels per chunk = length of one plane
};

inline int sz_make_layout(int options, int bpp, int ppb, int pps, uint64_t chunk_bytes, SzLayout *L)
{
    if (ppb <= 0 || pps <= 0 || bpp <= 0) return RC_CONF_ERROR;                 // sz_abi.cpp: prepare_compress
    const bool planes = bpp == 32 || bpp == 64;                                  // sz_compat.c:134
    const uint32_t bps = planes ? 8u : (uint32_t)bpp;
    const uint32_t rsi = (uint32_t)(((int64_t)pps + ppb - 1) / ppb);
    uint32_t flags = F_NOT_ENFORCE;                                               // sz_compat.c:128
    if (options & kSzMsbOption) flags |= F_MSB;                                   // sz_compat.c:12-27
    if (options & kSzNnOption) flags |= F_PREPROCESS;
    Cfg c;
    if (make_cfg(bps, (uint32_t)ppb, rsi, flags, 0, true, &c) != RC_OK) return RC_CONF_ERROR;
    L->bps = bps; L->bs = (uint32_t)ppb; L->rsi = rsi; L->flags = flags;
    L->word = planes ? (uint32_t)bpp / 8u : 0u;
    L->pixel = bps > 16 ? 4u : (bps > 8 ? 2u : 1u);                               // sz_compat.c:29-37
    L->repeat = (flags & F_PREPROCESS) ? 1u : 0u;
    L->line = (uint64_t)pps * L->pixel;
    L->padded_line = (uint64_t)rsi * (uint32_t)ppb * L->pixel;
    L->chunk_bytes = chunk_bytes;
    L->coded_bytes = chunk_bytes - chunk_bytes % (planes ? L->word : L->pixel);
    if (L->coded_bytes == 0) return RC_CONF_ERROR;                                // nothing to code
    L->pixels = planes ? L->coded_bytes / L->word : 0;
    L->lines = (L->coded_bytes + L->line - 1) / L->line;
    L->coder_bytes = L->lines * L->padded_line;
    L->passthrough = (!planes && L->padded_line == L->line && L->coded_bytes % L->line == 0 &&
                      L->coded_bytes == chunk_bytes) ? 1u : 0u;
    return RC_OK;
}

// (chunks below 4 GiB divide in 32 bits)
AEC_HD void sz_divmod(uint64_t a, uint64_t b, uint64_t &q, uint64_t &r)
{
    if (((a | b) >> 32) == 0) {
        q = (uint32_t)a / (uint32_t)b;
        r = (uint32_t)a % (uint32_t)b;
    } else {
        q = a / b;
        r = a % b;
    }
}

// byte q of the (concatenated planes of the) chunk -> byte of the chunk as it lies: to_planes, sz_compat.c:39-53
AEC_HD uint64_t sz_planar_to_chunk(const SzLayout &L, uint64_t q)
{
    if (!L.word) return q;
    uint64_t j, i;
    sz_divmod(q, L.pixels, j, i);
    return i * L.word + j;
}

// bytes of scan line l that come from the chunk (the last line may be partial)
AEC_HD uint64_t sz_take(const SzLayout &L, uint64_t l)
{
    const uint64_t left = L.coded_bytes - l * L.line;
    return left < L.line ? left : L.line;
}

// ---- map 1: byte r of the coder's input of one chunk -> byte of the chunk, or kSzZero ---------------------------
AEC_HD uint64_t sz_src_at(const SzLayout &L, uint64_t l, uint64_t k, uint64_t take)
{
    if (k < take) return sz_planar_to_chunk(L, l * L.line + k);
    if (!L.repeat) return kSzZero;
    // the pixel in front of the padding, byte for byte (take is whole pixels): sz_compat.c:71-94
    return sz_planar_to_chunk(L, l * L.line + take - L.pixel + (k & (L.pixel - 1u)));   // (pixel is 1, 2 or 4)
}

AEC_HD uint64_t sz_src_of(const SzLayout &L, uint64_t r)
{
    uint64_t l, k;
    sz_divmod(r, L.padded_line, l, k);
    return sz_src_at(L, l, k, sz_take(L, l));
}

// ---- map 2: byte d of the chunk -> byte of the coder's output of that chunk, or kSzZero ---------------------------
AEC_HD uint64_t sz_dst_from(const SzLayout &L, uint64_t d)
{
    if (d >= L.coded_bytes) return kSzZero;
    uint64_t q = d;
    if (L.word) {                                           // from_planes, sz_compat.c:55-69
        const uint64_t i = L.word == 8 ? d >> 3 : d >> 2, j = d & (L.word - 1u);
        q = j * L.pixels + i;
    }
    uint64_t l, k;
    sz_divmod(q, L.line, l, k);                             // un-padding, sz_compat.c:96-108
    return l * L.padded_line + k;
}

// ---- the same over a run of chunks lying back to back, byte after byte (what a lane of the generic path does) ----
struct SzInCursor {
    uint64_t chunk, l, k, take;
};

AEC_HD void sz_in_seek(const SzLayout &L, uint64_t o, SzInCursor &c)     // o: byte of the run of coder inputs
{
    uint64_t r;
    sz_divmod(o, L.coder_bytes, c.chunk, r);
    sz_divmod(r, L.padded_line, c.l, c.k);
    c.take = sz_take(L, c.l);
}

AEC_HD uint8_t sz_in_byte(const SzLayout &L, const uint8_t *src, const SzInCursor &c)
{
    const uint64_t s = sz_src_at(L, c.l, c.k, c.take);
    return s == kSzZero ? (uint8_t)0 : src[c.chunk * L.chunk_bytes + s];
}

AEC_HD void sz_in_next(const SzLayout &L, SzInCursor &c)
{
    if (++c.k < L.padded_line) return;
    c.k = 0;
    if (++c.l == L.lines) {
        c.l = 0;
        c.chunk++;
    }
    c.take = sz_take(L, c.l);
}

// 16 bytes from c on are 16 consecutive bytes of one scan line as the chunk holds them: where (else kSzZero)
AEC_HD uint64_t sz_in_straight(const SzLayout &L, const SzInCursor &c)
{
    if (L.word || c.k + 16u > c.take) return kSzZero;
    return c.chunk * L.chunk_bytes + c.l * L.line + c.k;
}

AEC_HD uint8_t sz_out_byte(const SzLayout &L, const uint8_t *coder_out, uint64_t chunk, uint64_t d)
{
    const uint64_t s = sz_dst_from(L, d);
    return s == kSzZero ? (uint8_t)0 : coder_out[chunk * L.coder_bytes + s];
}

// 16 bytes from byte d of chunk `chunk` on are 16 consecutive bytes of one RSI of the coder's output: where
AEC_HD uint64_t sz_out_straight(const SzLayout &L, uint64_t chunk, uint64_t d)
{
    if (L.word || d + 16u > L.coded_bytes) return kSzZero;
    uint64_t l, k;
    sz_divmod(d, L.line, l, k);
    if (k + 16u > L.line) return kSzZero;
    return chunk * L.coder_bytes + l * L.padded_line + k;
}

// ---- byte planes in registers -----------------------------------------------------------------------------------------
// v_perm_b32: byte i of the result is byte sel[i] of the eight bytes {hi, lo} (0..3 = lo, 4..7 = hi)
AEC_HD uint32_t sz_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) r |= (uint32_t)((both >> (8u * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
    return r;
#endif
}

// 4 x 4 byte transpose: byte i of out[j] = byte j of in_i.  Four pixels of 4 bytes -> their 4-byte piece of each plane,
// and (it is its own inverse) four such pieces -> four pixels.  Eight permutes.
AEC_HD void sz_transpose4(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t *out)
{
    const uint32_t a = sz_perm(y, x, 0x05010400u), b = sz_perm(y, x, 0x07030602u);   // x0 y0 x1 y1 | x2 y2 x3 y3
    const uint32_t c = sz_perm(w, z, 0x05010400u), d = sz_perm(w, z, 0x07030602u);   // z0 w0 z1 w1 | z2 w2 z3 w3
    out[0] = sz_perm(c, a, 0x05040100u);
    out[1] = sz_perm(c, a, 0x07060302u);
    out[2] = sz_perm(d, b, 0x05040100u);
    out[3] = sz_perm(d, b, 0x07060302u);
}

// where the 4-byte piece of plane j that starts at pixel 4 m lies in the coder's buffer of its chunk
AEC_HD uint64_t sz_piece_at(const SzLayout &L, uint32_t j, uint64_t m)
{
    uint64_t l, k;
    sz_divmod(j * L.pixels + 4u * m, L.line, l, k);
    return l * L.padded_line + k;
}

// Whole chunks take the register path when every 4-byte piece of a plane lies in one scan line at a 4-byte boundary
// (the chunk's and the coder buffer's base alignment are the caller's to check).
inline bool sz_planes_fast(const SzLayout &L)
{
    return L.word && L.coded_bytes == L.chunk_bytes && L.chunk_bytes % 16 == 0 && L.pixels % 4 == 0 && L.line % 4 == 0 &&
           L.padded_line % 4 == 0;
}

// ---- batches of UNEQUAL chunks under one SZ_com_t (aec_gpu_sz_*_chunks_async) -----------------------------------------
// The SZ_com_t fixes line, padded_line, pixel, word and repeat (an SzLayout made for any chunk size holds them); a
// chunk's size fixes the rest, which travels in a descriptor per chunk.  Every chunk has a room of its own in the work
// buffer, at a 16-byte aligned offset.  A chunk owns whole wavefronts of a launch: on the byte path one lane per 16-byte
// group of what is written, on the plane path one lane per four pixels; wave0 holds the running sums of both, so a chunk
// that takes the other path owns no wavefront of this one.  The maps below are those above with the descriptor in place
// of chunk * L.chunk_bytes / chunk * L.coder_bytes: they give bytes of the caller's buffer and of the work buffer.
// tests/emul/sz_chunks_emul.cpp runs them on the CPU.
constexpr int kSzBytes = 0, kSzPlanes = 1;              // the two paths

struct SzChunk {
    uint64_t off;               // the chunk in the caller's buffer (d_src / d_dst): any byte offset
    uint64_t chunk_bytes;
    uint64_t work_off;          // its room in the work buffer: the running sum of up16(coder_bytes)
    uint64_t coded_bytes, pixels, lines, coder_bytes;   // as in SzLayout, of this chunk
    uint64_t wave0[2];          // its first wavefront on the byte path / on the plane path (entry n: the totals)
    uint32_t planes;            // 1: the chunk takes the plane path in this call
    uint32_t head;              // un-marshal: (d_dst + off) & 15, the bytes in front of the chunk in its first group
};

// what the chunk's size fixes (sz_make_layout's arithmetic); false for a chunk without a whole pixel
AEC_HD bool sz_chunk_sizes(const SzLayout &L, uint64_t chunk_bytes, SzChunk &D)
{
    D.chunk_bytes = chunk_bytes;
    D.coded_bytes = chunk_bytes - chunk_bytes % (L.word ? L.word : L.pixel);
    D.pixels = L.word ? D.coded_bytes / L.word : 0;
    D.lines = (D.coded_bytes + L.line - 1) / L.line;
    D.coder_bytes = D.lines * L.padded_line;
    return D.coded_bytes != 0;
}

AEC_HD bool sz_chunk_passthrough(const SzLayout &L, const SzChunk &D)
{
    return !L.word && L.padded_line == L.line && D.coded_bytes % L.line == 0 && D.coded_bytes == D.chunk_bytes;
}

// sz_planes_fast of this chunk (its base alignment is the caller's to check)
AEC_HD bool sz_chunk_planes_fast(const SzLayout &L, const SzChunk &D)
{
    return L.word && D.coded_bytes == D.chunk_bytes && D.chunk_bytes % 16 == 0 && D.pixels % 4 == 0 && L.line % 4 == 0 &&
           L.padded_line % 4 == 0;
}

// wavefronts of 64 lanes a chunk owns: groups of `bytes` output bytes that start `head` bytes into a group / quads
AEC_HD uint64_t sz_group_waves(uint64_t bytes, uint32_t head) { return ((head + bytes + 15u) / 16u + 63u) / 64u; }
AEC_HD uint64_t sz_quad_waves(const SzChunk &D) { return (D.pixels / 4u + 63u) / 64u; }

// the chunk that owns wavefront w of a path: the LAST chunk whose first wavefront is <= w (chunks that own none share
// the first wavefront of the next one that does).  w must be below d[n].wave0[path].
AEC_HD uint64_t sz_chunk_of_wave(const SzChunk *d, uint64_t n, int path, uint64_t w)
{
    uint64_t lo = 0, hi = n;            // invariant: d[lo].wave0 <= w < d[hi].wave0
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (d[mid].wave0[path] <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

AEC_HD uint64_t sz_planar_to_chunk(const SzLayout &L, const SzChunk &D, uint64_t q)
{
    if (!L.word) return q;
    uint64_t j, i;
    sz_divmod(q, D.pixels, j, i);
    return i * L.word + j;
}

AEC_HD uint64_t sz_take(const SzLayout &L, const SzChunk &D, uint64_t l)
{
    const uint64_t left = D.coded_bytes - l * L.line;
    return left < L.line ? left : L.line;
}

// map 1: byte k of scan line l of the chunk's coder input -> byte of the caller's buffer, or kSzZero
AEC_HD uint64_t sz_src_at(const SzLayout &L, const SzChunk &D, uint64_t l, uint64_t k, uint64_t take)
{
    if (k < take) return D.off + sz_planar_to_chunk(L, D, l * L.line + k);
    if (!L.repeat) return kSzZero;
    return D.off + sz_planar_to_chunk(L, D, l * L.line + take - L.pixel + (k & (L.pixel - 1u)));
}

// map 2: byte d of the chunk -> byte of the work buffer (the coder's output), or kSzZero
AEC_HD uint64_t sz_dst_from(const SzLayout &L, const SzChunk &D, uint64_t d)
{
    if (d >= D.coded_bytes) return kSzZero;
    uint64_t q = d;
    if (L.word) {
        const uint64_t i = L.word == 8 ? d >> 3 : d >> 2, j = d & (L.word - 1u);
        q = j * D.pixels + i;
    }
    uint64_t l, k;
    sz_divmod(q, L.line, l, k);
    return D.work_off + l * L.padded_line + k;
}

// the cursor over the coder input of ONE chunk (c.chunk is not used: a lane never leaves its chunk)
AEC_HD void sz_in_seek(const SzLayout &L, const SzChunk &D, uint64_t r, SzInCursor &c)    // r: byte of the chunk's coder input
{
    c.chunk = 0;
    sz_divmod(r, L.padded_line, c.l, c.k);
    c.take = sz_take(L, D, c.l);
}

AEC_HD uint8_t sz_in_byte(const SzLayout &L, const SzChunk &D, const uint8_t *src, const SzInCursor &c)
{
    const uint64_t s = sz_src_at(L, D, c.l, c.k, c.take);
    return s == kSzZero ? (uint8_t)0 : src[s];
}

AEC_HD void sz_in_next(const SzLayout &L, const SzChunk &D, SzInCursor &c)
{
    if (++c.k < L.padded_line) return;
    c.k = 0;
    if (++c.l < D.lines) c.take = sz_take(L, D, c.l);       // (behind the last line: the end of the chunk's input)
}

AEC_HD uint64_t sz_in_straight(const SzLayout &L, const SzChunk &D, const SzInCursor &c)
{
    if (L.word || c.k + 16u > c.take) return kSzZero;
    return D.off + c.l * L.line + c.k;
}

AEC_HD uint8_t sz_out_byte(const SzLayout &L, const SzChunk &D, const uint8_t *coder_out, uint64_t d)
{
    const uint64_t s = sz_dst_from(L, D, d);
    return s == kSzZero ? (uint8_t)0 : coder_out[s];
}

AEC_HD uint64_t sz_out_straight(const SzLayout &L, const SzChunk &D, uint64_t d)
{
    if (L.word || d + 16u > D.coded_bytes) return kSzZero;
    uint64_t l, k;
    sz_divmod(d, L.line, l, k);
    if (k + 16u > L.line) return kSzZero;
    return D.work_off + l * L.padded_line + k;
}

// where the 4-byte piece of plane j that starts at pixel 4 m of the chunk lies in the work buffer
AEC_HD uint64_t sz_piece_at(const SzLayout &L, const SzChunk &D, uint32_t j, uint64_t m)
{
    uint64_t l, k;
    sz_divmod(j * D.pixels + 4u * m, L.line, l, k);
    return D.work_off + l * L.padded_line + k;
}

// The descriptors of a batch: sizes, rooms, paths and the two wavefront prefixes; d[n] holds the totals.  base: the
// caller's buffer (its low four bits decide alignment and heads); unmarshal: groups are cut on the destination.
// false for a chunk without a whole pixel.
inline bool sz_make_chunks(const SzLayout &L, uint64_t base, const uint64_t *offsets, const uint64_t *chunk_bytes, uint64_t n,
                           bool unmarshal, SzChunk *d)
{
    uint64_t work = 0, waves[2] = {0, 0};
    for (uint64_t i = 0; i < n; i++) {
        SzChunk &D = d[i];
        if (!sz_chunk_sizes(L, chunk_bytes[i], D)) return false;
        D.off = offsets[i];
        D.work_off = work;
        const uint32_t low = (uint32_t)((base + D.off) & 15u);
        D.planes = sz_chunk_planes_fast(L, D) && low == 0 ? 1u : 0u;
        D.head = unmarshal ? low : 0u;
        D.wave0[kSzBytes] = waves[kSzBytes];
        D.wave0[kSzPlanes] = waves[kSzPlanes];
        if (D.planes) waves[kSzPlanes] += sz_quad_waves(D);
        else waves[kSzBytes] += unmarshal ? sz_group_waves(D.chunk_bytes, D.head) : sz_group_waves(D.coder_bytes, 0u);
        work += (D.coder_bytes + 15u) & ~(uint64_t)15u;
    }
    d[n] = SzChunk{0, 0, work, 0, 0, 0, 0, {waves[kSzBytes], waves[kSzPlanes]}, 0u, 0u};
    return true;
}

}  // namespace aec
