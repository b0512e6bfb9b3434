// sz_chunks_emul.cpp -- the SZIP marshalling of batches of UNEQUAL chunks (libaec_amd/csrc/aec_szmap.h: SzChunk;
// aec_sz.hip: k_sz_chunks_setup, k_sz_marshal_chunks, k_sz_unmarshal_chunks, k_sz_split_chunks, k_sz_merge_chunks,
// k_sz_fill_chunks) on the CPU: the descriptors as the host writes them, the wavefront table as the set-up kernel fills
// it, and every wavefront of the launches lane by lane with the functions the kernels call.  Buffers are addressed as
// the device would see them: `base_low` stands for the low four bits of the caller's buffer address.
// (test infrastructure; built by tests/test_sz_chunks_layout.py.  With -DSZ_CHUNKS_EMUL_MAIN: a stand-alone program
// that runs synthetic batches, for a sanitizer build.)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../libaec_amd/csrc/aec_szmap.h"

using namespace aec;

static int layout(const int *prm, SzLayout *L) { return sz_make_layout(prm[0], prm[1], prm[2], prm[3], 64, L); }

static uint32_t ld32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static void st32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }

// sz_make_chunks: n + 1 descriptors of 80 bytes.  0, or -1 for an invalid SZ_com_t or a chunk without a whole pixel
extern "C" int emul_szc_make(const int *prm, uint32_t base_low, const uint64_t *offsets, const uint64_t *chunk_bytes, uint64_t n,
                             int unmarshal, SzChunk *desc)
{
    static_assert(sizeof(SzChunk) == 80, "the tests read the descriptors as 80-byte records");
    SzLayout L;
    if (layout(prm, &L) != RC_OK) return -1;
    return sz_make_chunks(L, base_low, offsets, chunk_bytes, n, unmarshal != 0, desc) ? 0 : -1;
}

// k_sz_chunks_setup: the byte path's wavefronts, then the plane path's
extern "C" void emul_szc_table(const SzChunk *desc, uint64_t n, uint32_t *table)
{
    const uint64_t nb = desc[n].wave0[kSzBytes], np = desc[n].wave0[kSzPlanes];
    for (uint64_t i = 0; i < nb + np; i++)
        table[i] = i < nb ? (uint32_t)sz_chunk_of_wave(desc, n, kSzBytes, i) : (uint32_t)sz_chunk_of_wave(desc, n, kSzPlanes, i - nb);
}

// the group of lane i (sz_group_at of aec_sz.hip)
struct Group {
    uint64_t first, end;
    int64_t lo;
    bool whole;
};
static bool group_at(uint64_t i, uint64_t total, uint32_t head, Group &g)
{
    g.lo = (int64_t)(i * 16u) - (int64_t)head;
    if (g.lo >= (int64_t)total) return false;
    g.first = g.lo < 0 ? 0u : (uint64_t)g.lo;
    g.end = (uint64_t)(g.lo + 16) < total ? (uint64_t)(g.lo + 16) : total;
    g.whole = g.lo >= 0 && (uint64_t)(g.lo + 16) <= total;
    return true;
}

// split + fill + marshal launches of aec_gpu_sz_compress_chunks_async.  src: the caller's buffer (byte 0 = address
// base_low mod 16), work: the work buffer.  Returns the number of bytes at which the cursor's walk differs from map 1
// applied byte by byte (must be 0); straight_groups: groups moved as one 16-byte load.
extern "C" int64_t emul_szc_marshal(const int *prm, uint32_t base_low, const SzChunk *desc, uint64_t n, const uint32_t *table,
                                    const uint8_t *src, uint8_t *work, uint64_t *straight_groups)
{
    SzLayout L;
    if (layout(prm, &L) != RC_OK) return -1;
    const uint64_t nb = desc[n].wave0[kSzBytes], np = desc[n].wave0[kSzPlanes];
    uint64_t straight = 0;
    for (uint64_t w = 0; w < np; w++) {                                     // k_sz_split_chunks
        const SzChunk &D = desc[table[nb + w]];
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t m = (w - D.wave0[kSzPlanes]) * 64u + lane;
            if (m >= D.pixels / 4u) continue;
            const uint8_t *p = src + D.off + m * 4u * L.word;
            uint32_t piece[8];
            if (L.word == 4) {
                sz_transpose4(ld32(p), ld32(p + 4), ld32(p + 8), ld32(p + 12), piece);
            } else {
                sz_transpose4(ld32(p), ld32(p + 8), ld32(p + 16), ld32(p + 24), piece);
                sz_transpose4(ld32(p + 4), ld32(p + 12), ld32(p + 20), ld32(p + 28), piece + 4);
            }
            for (uint32_t j = 0; j < L.word; j++) st32(work + sz_piece_at(L, D, j, m), piece[j]);
        }
    }
    for (uint64_t w = 0; w < np; w++) {                                     // k_sz_fill_chunks
        const SzChunk &D = desc[table[nb + w]];
        if (D.coder_bytes == D.coded_bytes) continue;
        for (uint32_t lane = 0; lane < 64; lane++) {
            SzInCursor c;
            c.chunk = 0;
            for (c.l = w - D.wave0[kSzPlanes]; c.l < D.lines; c.l += sz_quad_waves(D)) {
                c.take = sz_take(L, D, c.l);
                for (uint64_t k = c.take + 4u * lane; k < L.padded_line; k += 4u * 64u)
                    for (int i = 0; i < 4; i++) {
                        c.k = k + i;
                        work[D.work_off + c.l * L.padded_line + c.k] = sz_in_byte(L, D, src, c);
                    }
            }
        }
    }
    for (uint64_t w = 0; w < nb; w++) {                                     // k_sz_marshal_chunks
        const SzChunk &D = desc[table[w]];
        for (uint32_t lane = 0; lane < 64; lane++) {
            Group g;
            if (!group_at((w - D.wave0[kSzBytes]) * 64u + lane, D.coder_bytes, 0u, g)) continue;
            uint8_t *out = work + D.work_off;
            SzInCursor c;
            sz_in_seek(L, D, g.first, c);
            if (g.whole) {
                const uint64_t at = sz_in_straight(L, D, c);
                if (at != kSzZero && ((base_low + at) & 15u) == 0) {
                    memcpy(out + g.lo, src + at, 16);
                    straight++;
                    continue;
                }
            }
            for (uint64_t o = g.first; o < g.end; o++) {
                out[o] = sz_in_byte(L, D, src, c);
                sz_in_next(L, D, c);
            }
        }
    }
    int64_t differ = 0;
    for (uint64_t i = 0; i < n; i++) {
        const SzChunk &D = desc[i];
        for (uint64_t r = 0; r < D.coder_bytes; r++) {
            const uint64_t l = r / L.padded_line, k = r % L.padded_line, s = sz_src_at(L, D, l, k, sz_take(L, D, l));
            if (work[D.work_off + r] != (s == kSzZero ? 0 : src[s])) differ++;
        }
    }
    if (straight_groups) *straight_groups = straight;
    return differ;
}

// merge + un-marshal launches of aec_gpu_sz_decompress_chunks_async.  Returns the number of bytes written twice (two
// chunks that share a 16-byte line must write disjoint bytes: 0), -1 for an invalid SZ_com_t.
extern "C" int64_t emul_szc_unmarshal(const int *prm, uint32_t base_low, const SzChunk *desc, uint64_t n, const uint32_t *table,
                                      const uint8_t *work, uint8_t *dst, uint64_t dst_bytes, uint64_t *straight_groups)
{
    SzLayout L;
    if (layout(prm, &L) != RC_OK) return -1;
    const uint64_t nb = desc[n].wave0[kSzBytes], np = desc[n].wave0[kSzPlanes];
    std::vector<uint8_t> times(dst_bytes, 0);
    uint64_t straight = 0;
    for (uint64_t w = 0; w < np; w++) {                                     // k_sz_merge_chunks
        const SzChunk &D = desc[table[nb + w]];
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t m = (w - D.wave0[kSzPlanes]) * 64u + lane;
            if (m >= D.pixels / 4u) continue;
            uint32_t piece[8], lo[4], hi[4];
            for (uint32_t j = 0; j < L.word; j++) piece[j] = ld32(work + sz_piece_at(L, D, j, m));
            const uint64_t at = D.off + m * 4u * L.word;
            uint8_t *p = dst + at;
            sz_transpose4(piece[0], piece[1], piece[2], piece[3], lo);
            if (L.word == 4) {
                for (int i = 0; i < 4; i++) st32(p + 4 * i, lo[i]);
            } else {
                sz_transpose4(piece[4], piece[5], piece[6], piece[7], hi);
                for (int i = 0; i < 4; i++) {
                    st32(p + 8 * i, lo[i]);
                    st32(p + 8 * i + 4, hi[i]);
                }
            }
            for (uint64_t o = at; o < at + 4u * L.word; o++) times[o]++;
        }
    }
    for (uint64_t w = 0; w < nb; w++) {                                     // k_sz_unmarshal_chunks
        const SzChunk &D = desc[table[w]];
        for (uint32_t lane = 0; lane < 64; lane++) {
            Group g;
            if (!group_at((w - D.wave0[kSzBytes]) * 64u + lane, D.chunk_bytes, D.head, g)) continue;
            uint8_t *out = dst + D.off;
            uint64_t d = g.first;
            bool moved = false;
            if (g.whole) {
                const uint64_t at = sz_out_straight(L, D, d);
                if (at != kSzZero && (at & 15u) == 0) {
                    memcpy(out + g.lo, work + at, 16);
                    straight++;
                    moved = true;
                }
            }
            if (!moved)
                for (uint64_t o = g.first; o < g.end; o++) out[o] = sz_out_byte(L, D, work, d++);
            for (uint64_t o = g.first; o < g.end; o++) times[D.off + o]++;
        }
    }
    int64_t twice = 0;
    for (uint8_t t : times) twice += t > 1;
    if (straight_groups) *straight_groups = straight;
    return twice;
}

#ifdef SZ_CHUNKS_EMUL_MAIN
// the synthetic batches of tests/test_sz_chunks_layout.py, round trip: chunks -> work -> chunks, behind guard bytes
int main()
{
    static const int sets[4][5] = {{32 | 128, 32, 16, 1000, 2501 * 4}, {32 | 16 | 128, 64, 8, 24, 100 * 8}, {128, 8, 16, 100, 250},
                                   {32 | 128, 24, 32, 500, 1203 * 4}};
    int bad = 0;
    for (const auto &s : sets) {
        const uint64_t unit = s[1] == 32 || s[1] == 64 ? s[1] / 8 : (s[1] > 16 ? 4 : (s[1] > 8 ? 2 : 1));
        const uint64_t line = (uint64_t)s[3] * (s[1] == 32 || s[1] == 64 ? 1 : unit);
        const uint64_t sizes[6] = {unit, (uint64_t)s[4], 16 * line * unit, 3 * unit + unit / 2 + 1, line / 2 / unit * unit + unit,
                                   64 * 16};
        for (uint32_t skew : {0u, 5u}) {
            std::vector<uint64_t> off, len(sizes, sizes + 6);
            uint64_t at = 0;
            for (uint64_t i = 0; i < 6; i++) {
                off.push_back(at);
                at += len[i] + (i % 2 ? 16 - (at + len[i]) % 16 : 0);          // some chunks aligned, some back to back
            }
            std::vector<uint8_t> src(at), back(at, 0xA5);
            for (uint64_t i = 0; i < at; i++) src[i] = (uint8_t)(i * 131u + (i >> 8) * 7u + 1u);
            std::vector<SzChunk> dm(7), du(7);
            if (emul_szc_make(s, skew, off.data(), len.data(), 6, 0, dm.data()) || emul_szc_make(s, skew, off.data(), len.data(), 6, 1, du.data())) {
                printf("set %d bpp: refused\n", s[1]);
                bad++;
                continue;
            }
            std::vector<uint32_t> tm(dm[6].wave0[0] + dm[6].wave0[1]), tu(du[6].wave0[0] + du[6].wave0[1]);
            emul_szc_table(dm.data(), 6, tm.data());
            emul_szc_table(du.data(), 6, tu.data());
            std::vector<uint8_t> work(dm[6].work_off, 0x5A);
            const int64_t differ = emul_szc_marshal(s, skew, dm.data(), 6, tm.data(), src.data(), work.data(), nullptr);
            const int64_t twice = emul_szc_unmarshal(s, skew, du.data(), 6, tu.data(), work.data(), back.data(), at, nullptr);
            uint64_t wrong = 0;
            for (uint64_t i = 0; i < 6; i++)
                for (uint64_t b = 0; b < len[i]; b++) {
                    const bool coded = b < dm[i].coded_bytes;
                    wrong += back[off[i] + b] != (coded ? src[off[i] + b] : 0);
                    back[off[i] + b] = 0xA5;
                }
            for (uint8_t b : back) wrong += b != 0xA5;                           // (nothing outside the chunks is written)
            printf("%d bpp, skew %u: %lld differ, %lld written twice, %llu wrong\n", s[1], skew, (long long)differ, (long long)twice,
                   (unsigned long long)wrong);
            bad += differ != 0 || twice != 0 || wrong != 0;
        }
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
