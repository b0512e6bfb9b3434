// sz_est_emul.cpp -- host harness for libaec_amd/csrc/aec_szest.h: what the kernels of aec_szest.hip do, wavefront by
// wavefront and lane by lane, through the same functions, descriptors and workspace layout -- the three ways a chunk's
// bytes reach the rows of its pieces, est_piece per piece, the per-chunk sum per wavefront and size, the finish.
// Built by tests/test_sz_estimate_emul.py with g++: as a shared object, and with -DSZ_EST_EMUL_MAIN as a stand-alone
// program (for the sanitizers) that reads the cases from a file and prints what the shared object returns.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libaec_amd/csrc/aec_szest.h"

using namespace aec;

namespace {

constexpr int kNotWritten = -100, kMisaligned = -101;

struct Lane {
    bool live;
    uint64_t l;
    uint32_t g;
};

// the piece of lane `lane` of wavefront j of its chunk
Lane lane_piece(const SzEstPass &s, const SzChunk &D, uint64_t j, uint32_t lane)
{
    Lane a{false, 0, 0};
    if (D.planes == kSzEstPlanes4) {
        const uint64_t lpp = D.lines / 4u, q = 16u * j + (lane & 15u);
        if (q >= lpp * s.ppl) return a;
        uint64_t r;
        szest_piece_at(s, q, r, a.g);
        a.l = (lane >> 4) * lpp + r;
    } else {
        const uint64_t p = 64u * j + lane;
        if (p >= D.coder_bytes) return a;
        szest_piece_at(s, p, a.l, a.g);
    }
    a.live = true;
    return a;
}

template <int BYTES>
int pieces(const SzEstPass &s, const SzChunk *d, uint64_t n, const uint8_t *src, uint8_t *ws, bool force_generic)
{
    constexpr uint32_t CPP = 4u * BYTES;
    for (uint64_t w = 0; w < s.waves; w++) {
        SzChunk D = d[sz_chunk_of_wave(d, n, 0, w)];
        const uint32_t path = force_generic ? kSzEstGeneric : D.planes;
        D.planes = path;
        const uint64_t j = w - D.wave0[0];
        static uint32_t rows[64][16 * BYTES];
        memset(rows, 0xEE, sizeof(rows));
        if (path == kSzEstStraight) {
            for (uint32_t ci = 0; ci < 64u * CPP; ci++) {
                const Lane a = lane_piece(s, D, j, ci / CPP);
                if (!a.live || ci % CPP >= szest_straight_groups(s.L, D, a.l, a.g)) continue;
                const uint64_t at = szest_straight_at(s.L, D, a.l, a.g, ci % CPP);
                if (reinterpret_cast<uintptr_t>(src + at) & 15u) return kMisaligned;
                memcpy(reinterpret_cast<uint8_t *>(rows[ci / CPP]) + (ci % CPP) * 16u, src + at, 16);
            }
        } else if (path == kSzEstPlanes4) {
            const uint64_t units = D.lines / 4u * s.ppl;
            for (uint32_t tt = 0; tt < 256u; tt++) {
                const uint32_t u = tt / 16u, t = tt % 16u;
                const uint64_t q = 16u * j + u;
                if (q >= units) continue;
                uint64_t r;
                uint32_t g;
                szest_piece_at(s, q, r, g);
                bool fill;
                const uint64_t at = szest_quad_at(s, D, r, g, t, fill);
                if (reinterpret_cast<uintptr_t>(src + at) & 15u) return kMisaligned;
                uint32_t v[4], out[4];
                memcpy(v, src + at, 16);
                szest_quad_planes(s.L, v[0], v[1], v[2], v[3], fill, out);
                for (uint32_t pl = 0; pl < 4u; pl++) rows[pl * 16u + u][t] = out[pl];
            }
        }
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const Lane a = lane_piece(s, D, j, lane);
            if (!a.live) continue;
            if (path == kSzEstGeneric) szest_fill_row(s.L, D, src, a.l, a.g, 0u, reinterpret_cast<uint8_t *>(rows[lane]));
            if (path == kSzEstStraight)
                szest_fill_row(s.L, D, src, a.l, a.g, 16u * szest_straight_groups(s.L, D, a.l, a.g),
                               reinterpret_cast<uint8_t *>(rows[lane]));
            uint16_t rec[16] = {0};
            est_piece<BYTES>(s.e, rows[lane], szest_prev(s.L, D, src, a.l, a.g), a.g, rec);
            szest_store(s, ws, D.work_off + a.l, a.g, rec);
        }
    }
    return RC_OK;
}

// the per-chunk sums of one pass, a wavefront of the chunk and a size at a time
int sums(const SzEstPass &s, const SzChunk *d, uint64_t n, const uint8_t *ws, uint64_t *chunk_bits)
{
    for (uint64_t w = 0; w < s.waves; w++) {
        const uint64_t c = sz_chunk_of_wave(d, n, 0, w);
        const SzChunk &D = d[c];
        uint64_t lo, hi;
        szest_wave_lines(s, D, w - D.wave0[0], lo, hi);
        for (uint32_t i = 0; i < kEstSizes; i++) {
            if (!((s.e.mask >> i) & 1u)) continue;
            const uint16_t *recs = reinterpret_cast<const uint16_t *>(ws + s.e.rec_off[i]);
            const uint64_t spr = s.e.segs_per_rsi[i];
            for (uint64_t sg = (D.work_off + lo) * spr; sg < (D.work_off + hi) * spr; sg++) {
                const EstSeg g = est_seg(s.e, i, sg);
                uint64_t zmask = 0;
                for (uint32_t l = 0; l < g.nv; l++) {
                    if (recs[g.blk0 + l] == 0xA5A5u) return kNotWritten;
                    if (recs[g.blk0 + l] & kEstZero) zmask |= 1ull << l;
                }
                for (uint32_t l = 0; l < 64u; l++)
                    chunk_bits[c * 4u + i] += est_seg_lane(s.e, g, l, l < g.nv ? recs[g.blk0 + l] : 0u, zmask);
            }
        }
    }
    return RC_OK;
}

}  // namespace

// params = {options_mask, bits_per_pixel}; pps[i] = 0: size i is not asked.  The chunks are sizes[c] bytes at
// src + offsets[c]; the harness copies src to a buffer whose byte 0 is base_low off a 16-byte boundary.  chunk_bits:
// n * 4 entries; paths: n entries, the chunk's path in the first pass.  Returns 0, RC_CONF_ERROR where the call is
// refused, kNotWritten where a record that is summed was not written, kMisaligned where a fast path loads off a boundary.
extern "C" int sz_est_emul(const int *params, const unsigned int *pps, uint32_t base_low, const uint8_t *src, uint64_t src_bytes,
                           const uint64_t *offsets, const uint64_t *sizes, uint64_t n, int force_generic, uint64_t *chunk_bits,
                           uint64_t total_bytes[4], uint32_t *best, uint32_t *passes, uint64_t *pieces_out, uint32_t *paths)
{
    std::vector<uint8_t> room(src_bytes + 32u + 16u, 0x5C);
    uint8_t *base = room.data() + 16u;
    base += (16u - (reinterpret_cast<uintptr_t>(base) & 15u)) % 16u + base_low % 16u;
    if (src_bytes) memcpy(base, src, src_bytes);
    uint32_t mask = 0, done = 0;
    for (uint32_t i = 0; i < kEstSizes; i++) mask |= pps[i] ? 1u << i : 0u;
    if (!mask) return RC_CONF_ERROR;
    for (uint64_t k = 0; k < n * 4u; k++) chunk_bits[k] = ((mask >> (k & 3u)) & 1u) ? 0ull : ~0ull;
    *passes = 0;
    *pieces_out = 0;
    std::vector<SzChunk> d(n + 1);
    for (uint32_t i = 0; i < kEstSizes; i++) {
        if (!((mask >> i) & 1u) || ((done >> i) & 1u)) continue;
        uint32_t m = 0;
        for (uint32_t k = i; k < kEstSizes; k++) m |= pps[k] == pps[i] ? 1u << k : 0u;
        done |= m;
        SzEstPass s;
        if (szest_make_pass(params[0], params[1], pps[i], m, &s) != RC_OK) return RC_CONF_ERROR;
        if (!szest_make_chunks(&s, reinterpret_cast<uintptr_t>(base), offsets, sizes, n, d.data())) return RC_CONF_ERROR;
        if (!*passes)
            for (uint64_t c = 0; c < n; c++) paths[c] = d[c].planes;
        std::vector<uint8_t> ws(s.rec_bytes + 16u, 0xA5);
        int rc;
        switch (s.L.pixel) {
        case 1: rc = pieces<1>(s, d.data(), n, base, ws.data(), force_generic != 0); break;
        case 2: rc = pieces<2>(s, d.data(), n, base, ws.data(), force_generic != 0); break;
        default: rc = pieces<4>(s, d.data(), n, base, ws.data(), force_generic != 0); break;
        }
        if (rc == RC_OK) rc = sums(s, d.data(), n, ws.data(), chunk_bits);
        if (rc != RC_OK) return rc;
        for (uint32_t k = 0; k < 16u; k++)
            if (ws[s.rec_bytes + k] != 0xA5) return kNotWritten;          // nothing behind the records
        ++*passes;
        *pieces_out += s.e.pieces;
    }
    for (uint32_t i = 0; i < kEstSizes; i++) {
        total_bytes[i] = ((mask >> i) & 1u) ? 0ull : ~0ull;
        if ((mask >> i) & 1u)
            for (uint64_t c = 0; c < n; c++) total_bytes[i] += szest_stream_bytes(chunk_bits[c * 4u + i]);
    }
    *best = est_best(total_bytes, mask);
    return RC_OK;
}

#ifdef SZ_EST_EMUL_MAIN
// argv[1]: the cases, one after the other -- int32 options, bits per pixel; uint32 pps[4], base_low, force_generic;
// uint64 n, src_bytes; uint64 offsets[n], sizes[n]; the bytes.  Prints per case "rc passes pieces best | total_bytes |
// chunk_bits".
int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    int cases = 0;
    for (;;) {
        int32_t params[2];
        uint32_t head[6];
        uint64_t counts[2];
        if (fread(params, 4, 2, f) != 2) break;
        if (fread(head, 4, 6, f) != 6 || fread(counts, 8, 2, f) != 2) return 3;
        const uint64_t n = counts[0];
        std::vector<uint64_t> offs(n + 1), sizes(n + 1), bits(n * 4 + 1);
        std::vector<uint32_t> paths(n + 1);
        std::vector<uint8_t> src(counts[1] + 1);
        if (fread(offs.data(), 8, n, f) != n || fread(sizes.data(), 8, n, f) != n || fread(src.data(), 1, counts[1], f) != counts[1])
            return 3;
        uint64_t total[4] = {0, 0, 0, 0}, pieces_out = 0;
        uint32_t best = 0, passes = 0;
        const int rc = sz_est_emul(params, head, head[4], src.data(), counts[1], offs.data(), sizes.data(), n, (int)head[5],
                                   bits.data(), total, &best, &passes, &pieces_out, paths.data());
        printf("%d %u %llu %u |", rc, passes, (unsigned long long)pieces_out, best);
        for (int i = 0; i < 4; i++) printf(" %llu", (unsigned long long)total[i]);
        printf(" |");
        for (uint64_t k = 0; k < n * 4u; k++) printf(" %llu", (unsigned long long)bits[k]);
        printf("\n");
        cases++;
    }
    fclose(f);
    printf("%d cases ok\n", cases);
    return 0;
}
#endif
