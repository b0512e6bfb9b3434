// est_emul.cpp -- host harness for libaec_amd/csrc/aec_est.h: what k_est_blocks does piece by piece and k_est_sum segment
// by segment (libaec_amd/csrc/aec_est.hip), one lane at a time, through the same functions and the same workspace layout.
// Built by tests/test_estimate_emul.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../libaec_amd/csrc/aec_est.h"

using namespace aec;

template <int BYTES>
static void pieces(const EstCfg &e, const uint8_t *in, uint8_t *ws)
{
    const uint64_t last = e.c.total_samples - 1;
    for (uint64_t pi = 0; pi < e.pieces; pi++) {
        uint8_t bytes[kEstPiece * BYTES];
        for (uint32_t i = 0; i < kEstPiece; i++) {
            uint64_t s = pi * kEstPiece + i;
            if (s > last) s = last;                                  // the last sample repeated
            memcpy(bytes + i * BYTES, in + s * BYTES, BYTES);
        }
        uint32_t row[16 * BYTES];
        memcpy(row, bytes, sizeof(row));
        const uint32_t prev = pi ? load_sample_bytes(in + (pi * kEstPiece - 1) * BYTES, BYTES, e.c.flags & F_MSB) : 0u;
        uint16_t rec[16] = {0};
        est_piece<BYTES>(e, row, prev, pi, rec);
        if (e.rsi[0]) memcpy(ws + e.rec_off[0] + pi * 16u, rec, 16);
        if (e.rsi[1]) memcpy(ws + e.rec_off[1] + pi * 8u, rec + 8, 8);
        if (e.rsi[2]) memcpy(ws + e.rec_off[2] + pi * 4u, rec + 12, 4);
        if (e.rsi[3]) memcpy(ws + e.rec_off[3] + pi * 2u, rec + 14, 2);
    }
}

// params = {bits_per_sample, flags}; rsi = four values or null (then rsi_all for all).  Per size i asked for: bits[i]
// (uint32 per block) receives what every block contributes, kind[i] (uint8 per block) 0 = a coded block, 1 = a zero block
// that starts a run, 2 = a zero block inside a run.  Returns make_est_cfg's code.
extern "C" int est_emul(const uint32_t *params, const unsigned int *rsi, uint32_t rsi_all, const uint8_t *in, size_t in_bytes,
                        uint64_t total[4], uint32_t *best, uint32_t *mask, uint32_t *const bits[4], uint8_t *const kind[4])
{
    EstCfg e;
    size_t need = 0;
    const int rc = make_est_cfg(params[0], params[1], rsi, rsi_all, in_bytes, &e, &need);
    if (rc != RC_OK) return rc;
    std::vector<uint8_t> ws(need + 16, 0xA5);
    if (e.pieces) {
        switch (e.c.bytes) {
        case 1: pieces<1>(e, in, ws.data()); break;
        case 2: pieces<2>(e, in, ws.data()); break;
        case 3: pieces<3>(e, in, ws.data()); break;
        default: pieces<4>(e, in, ws.data()); break;
        }
    }
    for (uint32_t i = 0; i < kEstSizes; i++) {
        total[i] = ~0ull;
        if (!((e.mask >> i) & 1u)) continue;
        total[i] = 0;
        const uint16_t *recs = reinterpret_cast<const uint16_t *>(ws.data() + e.rec_off[i]);
        for (uint64_t sg = 0; sg < e.segs[i]; sg++) {
            const EstSeg g = est_seg(e, i, sg);
            uint64_t zmask = 0;
            for (uint32_t l = 0; l < g.nv; l++)
                if (recs[g.blk0 + l] & kEstZero) zmask |= 1ull << l;
            for (uint32_t l = 0; l < 64; l++) {
                const uint32_t rec = l < g.nv ? recs[g.blk0 + l] : 0u;
                const uint32_t b = est_seg_lane(e, g, l, rec, zmask);
                total[i] += b;
                if (l < g.nv) {
                    bits[i][g.blk0 + l] = b;
                    kind[i][g.blk0 + l] = (rec & kEstZero) ? (b ? 1 : 2) : 0;
                }
            }
        }
    }
    *best = est_best(total, e.mask);
    *mask = e.mask;
    return RC_OK;
}
