// aec_szest.h -- the arithmetic of aec_gpu_sz_estimate_async (include/aec_gpu_sz.h): the length of SZ_BufftoBuffCompress's
// stream of every chunk of a batch under pixels_per_block 8, 16, 32 and 64 from ONE read of the chunks, nothing marshalled
// to memory.  No reference counterpart.  DESIGN.md section 2, "Estimate through the SZIP marshal".
//
// SZIP pads every scan line to whole blocks of the candidate size, so the coder's input differs per candidate and the
// estimate of aec_est.h, which answers for ONE input, does not apply to it.  What makes one pass enough all the same:
//   * every candidate divides 64, so roundup(pps, 8 << i) <= roundup(pps, 64): a PIECE -- 64 coder samples of one scan
//     line counted from the line's start -- holds whole blocks of every size, and the pieces of a line are the same for
//     all candidates; only the number of blocks that count in a line's last piece differs: ceil((pps - 64 g) / (8 << i));
//   * the fill behind a line's pixels is the same for every candidate (the last pixel with NN, else zero), and it is what
//     the map of aec_szmap.h (sz_src_at) gives for any byte behind the line's own;
//   * every line starts an RSI under every candidate: the reference slot is sample 0 of the line for all four sizes, and
//     piece g of a line is to est_piece (aec_est.h) what piece g of an input is whose RSI is the line.
// The record of block b of line l, lines counted through all chunks, lies at l * rsi_i + b with rsi_i = ceil(pps / (8 << i)):
// with EstCfg.blocks = lines * rsi_i every line is a full RSI to est_seg / est_seg_lane, which apply as they are.
// Sizes that share a scan line share a PASS; tests/emul/sz_est_emul.cpp runs all of this on the CPU.
#pragma once
#include "aec_est.h"
#include "aec_szmap.h"

namespace aec {

constexpr uint32_t kSzEstGeneric = 0, kSzEstStraight = 1, kSzEstPlanes4 = 2;     // how a chunk's bytes reach the rows
constexpr uint64_t kSzEstMaxWaves = 1ull << 25, kSzEstMaxChunk = 1ull << 35;     // (aec_gpu_sz_chunks_plan's bounds)

// the public record (include/aec_gpu_sz.h: aec_gpu_sz_estimate_t)
struct SzEstResult {
    uint64_t total_bytes[kEstSizes];
    uint32_t best;
    uint32_t pad;
};

// One pass: the candidates that share pixels_per_scanline.
struct SzEstPass {
    SzLayout L;          // line, pixel, word, repeat, bps, flags (block size: the smallest of the pass; padded_line is not used)
    EstCfg e;            // c, mask, rsi[], segs_per_rsi[], and over all chunks blocks[] = lines * rsi, segs[], rec_off[], pieces
    uint32_t pps, ppl;   // pixels per scan line (with planes: bytes); pieces per line = ceil(pps / 64)
    uint64_t lines;      // scan lines of all chunks
    uint64_t waves;      // wavefronts of 64 pieces, every chunk rounded up to whole ones
    uint64_t rec_bytes;  // the pass's records
};

// The parameters of a pass; RC_CONF_ERROR where aec_gpu_sz_layout rejects one of its candidates.
inline int szest_make_pass(int options, int bpp, unsigned int pps, uint32_t mask, SzEstPass *s)
{
    *s = SzEstPass{};
    for (uint32_t i = 0; i < kEstSizes; i++) {
        if (!((mask >> i) & 1u)) continue;
        SzLayout L;
        if (pps > 0x7FFFFFFFu || sz_make_layout(options, bpp, 8 << i, (int)pps, 64, &L) != RC_OK) return RC_CONF_ERROR;
        Cfg c;
        if (make_cfg(L.bps, L.bs, L.rsi, L.flags, 0, true, &c) != RC_OK) return RC_CONF_ERROR;
        if (!s->e.mask) {
            s->L = L;
            s->e.c = c;
        }
        s->e.mask |= 1u << i;
        s->e.rsi[i] = L.rsi;
        s->e.segs_per_rsi[i] = c.segs_per_rsi;
    }
    if (!s->e.mask) return RC_CONF_ERROR;
    s->e.c.bs = 8;
    s->e.c.rsi = 0;
    s->e.c.segs_per_rsi = 0;
    s->pps = pps;
    s->ppl = (pps + kEstPiece - 1) / kEstPiece;
    return RC_OK;
}

// The descriptors of a pass's chunks (n + 1 entries; SzChunk with work_off = the chunk's first line among all lines,
// coder_bytes = its pieces, wave0[0] = its first wavefront, planes = its path) and the pass's totals.  base: the caller's
// buffer.  false for a chunk without a whole pixel or of kSzEstMaxChunk bytes and more, and beyond kSzEstMaxWaves wavefronts.
inline bool szest_make_chunks(SzEstPass *s, uint64_t base, const uint64_t *offsets, const uint64_t *chunk_bytes, uint64_t n,
                              SzChunk *d)
{
    const SzLayout &L = s->L;
    uint64_t lines = 0, waves = 0;
    for (uint64_t i = 0; i < n; i++) {
        SzChunk D;
        if (chunk_bytes[i] >= kSzEstMaxChunk || !sz_chunk_sizes(L, chunk_bytes[i], D)) return false;
        D.off = offsets ? offsets[i] : 0;
        D.work_off = lines;
        D.coder_bytes = D.lines * s->ppl;
        D.wave0[0] = waves;
        D.wave0[1] = 0;
        D.head = 0;
        const bool at16 = ((base + D.off) & 15u) == 0;
        D.planes = kSzEstGeneric;
        if (at16 && !L.word && L.line % 16 == 0) D.planes = kSzEstStraight;
        if (at16 && L.word == 4 && D.coded_bytes == D.chunk_bytes && s->pps % 4 == 0 && D.pixels % s->pps == 0)
            D.planes = kSzEstPlanes4;
        lines += D.lines;
        waves += (D.coder_bytes + 63u) / 64u;
        if (waves > kSzEstMaxWaves) return false;
        if (d) d[i] = D;
    }
    if (d) d[n] = SzChunk{0, 0, lines, 0, 0, 0, 0, {waves, 0}, 0u, 0u};
    s->lines = lines;
    s->waves = waves;
    s->e.pieces = lines * s->ppl;
    uint64_t off = 0;
    for (uint32_t i = 0; i < kEstSizes; i++) {
        if (!s->e.rsi[i]) continue;
        s->e.blocks[i] = lines * s->e.rsi[i];
        s->e.segs[i] = lines * s->e.segs_per_rsi[i];
        s->e.rec_off[i] = off;
        off += (s->e.blocks[i] * 2u + 15u) & ~(uint64_t)15;
    }
    s->rec_bytes = off;
    return true;
}

// ---- a piece ----------------------------------------------------------------------------------------------------------
// piece p of a chunk: its scan line and its place in the line
AEC_HD void szest_piece_at(const SzEstPass &s, uint64_t p, uint64_t &l, uint32_t &g)
{
    uint64_t r;
    sz_divmod(p, s.ppl, l, r);
    g = (uint32_t)r;
}

// bytes [from, 64 * pixel) of the row of piece g of line l, through the map: the line's own bytes, then the fill
AEC_HD void szest_fill_row(const SzLayout &L, const SzChunk &D, const uint8_t *src, uint64_t l, uint32_t g, uint32_t from,
                           uint8_t *row)
{
    const uint64_t take = sz_take(L, D, l), k0 = (uint64_t)g * kEstPiece * L.pixel;
    for (uint32_t b = from; b < kEstPiece * L.pixel; b++) {
        const uint64_t at = sz_src_at(L, D, l, k0 + b, take);
        row[b] = at == kSzZero ? (uint8_t)0 : src[at];
    }
}

// the sample in front of piece g inside its line (any value for g == 0: est_piece does not use it there)
AEC_HD uint32_t szest_prev(const SzLayout &L, const SzChunk &D, const uint8_t *src, uint64_t l, uint32_t g)
{
    if (!g) return 0;
    const uint64_t take = sz_take(L, D, l), k0 = (uint64_t)g * kEstPiece * L.pixel - L.pixel;
    uint32_t v = 0;
    for (uint32_t i = 0; i < L.pixel; i++) {                 // (load_sample_bytes, byte by byte through the map)
        const uint64_t at = sz_src_at(L, D, l, k0 + i, take);
        const uint32_t b = at == kSzZero ? 0u : src[at];
        v = (L.flags & F_MSB) ? (v << 8) | b : v | (b << (8u * i));
    }
    return v;
}

// blocks of size i of piece g that lie inside the line's padded length: ceil((pps - 64 g) / (8 << i)), at most 64 >> (3 + i)
AEC_HD uint32_t szest_count(const SzEstPass &s, uint32_t i, uint32_t g)
{
    const uint32_t per = kEstPiece >> (3u + i), left = s.e.rsi[i] - g * per;
    return left < per ? left : per;
}

// n of the PER records rec[0 .. PER) to out: all of them in one store where they are there and out is aligned for it
template <int PER>
AEC_HD void szest_store_size(uint16_t *out, uint32_t n, const uint16_t *rec)
{
    if (n == (uint32_t)PER && (reinterpret_cast<uintptr_t>(out) & (2u * PER - 1u)) == 0) {
        uint16_t all[PER];
#pragma unroll
        for (int j = 0; j < PER; j++) all[j] = rec[j];
        __builtin_memcpy(__builtin_assume_aligned(out, 2 * PER), all, 2 * PER);
        return;
    }
#pragma unroll
    for (int j = 0; j < PER; j++)
        if ((uint32_t)j < n) out[j] = rec[j];
}

// est_piece's records of piece g of line `line` (counted through all chunks) to the workspace
AEC_HD void szest_store(const SzEstPass &s, uint8_t *ws, uint64_t line, uint32_t g, const uint16_t rec[16])
{
    auto at = [&](uint32_t i) {
        return reinterpret_cast<uint16_t *>(ws + s.e.rec_off[i]) + line * s.e.rsi[i] + g * (kEstPiece >> (3u + i));
    };
    if (s.e.rsi[0]) szest_store_size<8>(at(0), szest_count(s, 0, g), rec);
    if (s.e.rsi[1]) szest_store_size<4>(at(1), szest_count(s, 1, g), rec + 8);
    if (s.e.rsi[2]) szest_store_size<2>(at(2), szest_count(s, 2, g), rec + 12);
    if (s.e.rsi[3]) szest_store_size<1>(at(3), szest_count(s, 3, g), rec + 14);
}

// ---- fast path (a), kSzEstStraight: no planes, chunk base and line bytes multiples of 16 --------------------------------
// 16-byte groups of the row of piece g of line l that are 16 bytes of the line as the chunk holds it (szest_fill_row does
// the rest of the row, from byte 16 * this on)
AEC_HD uint32_t szest_straight_groups(const SzLayout &L, const SzChunk &D, uint64_t l, uint32_t g)
{
    const uint64_t take = sz_take(L, D, l), k0 = (uint64_t)g * kEstPiece * L.pixel;
    if (take <= k0) return 0;
    const uint64_t whole = (take - k0) / 16u;
    return whole < 4u * L.pixel ? (uint32_t)whole : 4u * L.pixel;
}
// where group `sub` of them lies in the caller's buffer (16-byte aligned there)
AEC_HD uint64_t szest_straight_at(const SzLayout &L, const SzChunk &D, uint64_t l, uint32_t g, uint32_t sub)
{
    return D.off + l * L.line + (uint64_t)g * kEstPiece * L.pixel + sub * 16u;
}

// ---- fast path (b), kSzEstPlanes4: 4-byte pixels, whole lines per plane, chunk base 16-byte aligned, pps % 4 == 0 --------
// A UNIT (r, g) is the 64 pixels r * pps + 64 g ... of the chunk: loaded once, as 16 quads of four pixels, it is piece g
// of the lines r, lpp + r, 2 lpp + r and 3 lpp + r (lpp = lines per plane) -- the same pixels' bytes 0, 1, 2 and 3.
// Where quad t of a unit is loaded from; fill: it lies behind the line, and the line's last four pixels are loaded instead.
AEC_HD uint64_t szest_quad_at(const SzEstPass &s, const SzChunk &D, uint64_t r, uint32_t g, uint32_t t, bool &fill)
{
    const uint32_t x = kEstPiece * g + 4u * t;
    fill = x >= s.pps;
    return D.off + 4u * (r * s.pps + (fill ? s.pps - 4u : x));
}
// the four pixels of a quad -> word t of the rows of the four planes' pieces
AEC_HD void szest_quad_planes(const SzLayout &L, uint32_t x, uint32_t y, uint32_t z, uint32_t w, bool fill, uint32_t out[4])
{
    if (fill) x = y = z = w = L.repeat ? w : 0u;
    sz_transpose4(x, y, z, w, out);
}

// ---- the per-chunk sum -----------------------------------------------------------------------------------------------------
// The scan lines whose records wavefront j of a chunk sums: those whose first piece is among the chunk's pieces
// [64 j, 64 j + 64).  Every line of the chunk belongs to exactly one of its wavefronts, whatever the chunk's path.
AEC_HD void szest_wave_lines(const SzEstPass &s, const SzChunk &D, uint64_t j, uint64_t &lo, uint64_t &hi)
{
    uint64_t r;
    sz_divmod(64u * j + s.ppl - 1u, s.ppl, lo, r);
    sz_divmod(64u * (j + 1u) + s.ppl - 1u, s.ppl, hi, r);
    lo = lo < D.lines ? lo : D.lines;
    hi = hi < D.lines ? hi : D.lines;
}

// bytes of SZ_BufftoBuffCompress's stream of a chunk whose coded data sets have `bits` bits
AEC_HD uint64_t szest_stream_bytes(uint64_t bits) { return bits ? (bits + 7u) / 8u : 1u; }

}  // namespace aec
