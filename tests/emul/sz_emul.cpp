// sz_emul.cpp -- the SZIP marshalling of the device (libaec_amd/csrc/aec_szmap.h; aec_sz.hip) on the CPU: the layout,
// the two maps, and the lanes of the kernels -- the 16-byte groups of the byte path walked with the cursor the kernel
// uses, the four pixels of the plane path transposed with the same permutes -- over whole batches of chunks.
// (test infrastructure; built by tests/test_sz_layout.py)
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../libaec_amd/csrc/aec_szmap.h"

using namespace aec;

static int layout(const int *prm, uint64_t chunk_bytes, SzLayout *L)
{
    return sz_make_layout(prm[0], prm[1], prm[2], prm[3], chunk_bytes, L);
}

// out[13]: bps, bs, rsi, flags, word, pixel, repeat, passthrough, line, padded_line, lines, coder_bytes, coded_bytes
extern "C" int emul_sz_layout(const int *prm, uint64_t chunk_bytes, uint64_t *out)
{
    SzLayout L;
    const int rc = layout(prm, chunk_bytes, &L);
    if (rc != RC_OK) return rc;
    const uint64_t v[13] = {L.bps, L.bs, L.rsi, L.flags, L.word, L.pixel, L.repeat, L.passthrough, L.line, L.padded_line,
                            L.lines, L.coder_bytes, L.coded_bytes};
    memcpy(out, v, sizeof v);
    return RC_OK;
}

// k_sz_marshal: every 16-byte group of the run of coder inputs as its lane moves it.  `head` shifts the groups as an
// output that is not 16-byte aligned would (the kernel's own output is aligned: head 0).  Returns the number of bytes at
// which the cursor's walk differs from the map applied byte by byte (must be 0), -1 for an invalid layout.
extern "C" int64_t emul_sz_marshal(const int *prm, uint64_t chunk_bytes, uint64_t n, const uint8_t *src, uint8_t *out,
                                   uint32_t head, uint64_t *straight_groups)
{
    SzLayout L;
    if (layout(prm, chunk_bytes, &L) != RC_OK) return -1;
    const uint64_t total = n * L.coder_bytes;
    int64_t differ = 0;
    uint64_t straight = 0;
    for (int64_t lo = -(int64_t)head; lo < (int64_t)total; lo += 16) {
        const uint64_t first = lo < 0 ? 0 : (uint64_t)lo, end = (uint64_t)(lo + 16) < total ? (uint64_t)(lo + 16) : total;
        SzInCursor c;
        sz_in_seek(L, first, c);
        if (lo >= 0 && (uint64_t)lo + 16 <= total) {
            const uint64_t at = sz_in_straight(L, c);
            if (at != kSzZero) {
                memcpy(out + lo, src + at, 16);
                straight++;
                continue;
            }
        }
        for (uint64_t o = first; o < end; o++) {
            out[o] = sz_in_byte(L, src, c);
            sz_in_next(L, c);
        }
    }
    for (uint64_t o = 0; o < total; o++) {
        const uint64_t s = sz_src_of(L, o % L.coder_bytes);
        const uint8_t want = s == kSzZero ? 0 : src[(o / L.coder_bytes) * chunk_bytes + s];
        if (out[o] != want) differ++;
    }
    if (straight_groups) *straight_groups = straight;
    return differ;
}

extern "C" int64_t emul_sz_unmarshal(const int *prm, uint64_t chunk_bytes, uint64_t n, const uint8_t *coder_out, uint8_t *dst,
                                     uint32_t head, uint64_t *straight_groups)
{
    SzLayout L;
    if (layout(prm, chunk_bytes, &L) != RC_OK) return -1;
    const uint64_t total = n * chunk_bytes;
    uint64_t straight = 0;
    for (int64_t lo = -(int64_t)head; lo < (int64_t)total; lo += 16) {
        const uint64_t first = lo < 0 ? 0 : (uint64_t)lo, end = (uint64_t)(lo + 16) < total ? (uint64_t)(lo + 16) : total;
        uint64_t chunk, d;
        sz_divmod(first, L.chunk_bytes, chunk, d);
        if (lo >= 0 && (uint64_t)lo + 16 <= total) {
            const uint64_t at = sz_out_straight(L, chunk, d);
            if (at != kSzZero) {
                memcpy(dst + lo, coder_out + at, 16);
                straight++;
                continue;
            }
        }
        for (uint64_t o = first; o < end; o++) {
            dst[o] = sz_out_byte(L, coder_out, chunk, d);
            if (++d == L.chunk_bytes) {
                d = 0;
                chunk++;
            }
        }
    }
    if (straight_groups) *straight_groups = straight;
    return 0;
}

static uint32_t ld32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static void st32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }

// k_sz_split + k_sz_fill / k_sz_merge: 1 = done, 0 = the layout does not take the register path, -1 invalid
extern "C" int emul_sz_planes(const int *prm, uint64_t chunk_bytes, uint64_t n, const uint8_t *src, uint8_t *coder_in,
                              uint8_t *back)
{
    SzLayout L;
    if (layout(prm, chunk_bytes, &L) != RC_OK) return -1;
    if (!sz_planes_fast(L)) return 0;
    const uint64_t qpc = L.pixels / 4u;
    for (uint64_t t = 0; t < n * qpc; t++) {                              // k_sz_split
        const uint64_t chunk = t / qpc, m = t % qpc;
        const uint8_t *p = src + chunk * L.chunk_bytes + m * 4u * L.word;
        uint32_t piece[8];
        if (L.word == 4) {
            sz_transpose4(ld32(p), ld32(p + 4), ld32(p + 8), ld32(p + 12), piece);
        } else {
            sz_transpose4(ld32(p), ld32(p + 8), ld32(p + 16), ld32(p + 24), piece);
            sz_transpose4(ld32(p + 4), ld32(p + 12), ld32(p + 20), ld32(p + 28), piece + 4);
        }
        for (uint32_t j = 0; j < L.word; j++) st32(coder_in + chunk * L.coder_bytes + sz_piece_at(L, j, m), piece[j]);
    }
    for (uint64_t row = 0; row < n * L.lines; row++) {                     // k_sz_fill
        SzInCursor c;
        c.chunk = row / L.lines;
        c.l = row % L.lines;
        c.take = sz_take(L, c.l);
        for (c.k = c.take; c.k < L.padded_line; c.k++)
            coder_in[c.chunk * L.coder_bytes + c.l * L.padded_line + c.k] = sz_in_byte(L, src, c);
    }
    for (uint64_t t = 0; t < n * qpc; t++) {                              // k_sz_merge
        const uint64_t chunk = t / qpc, m = t % qpc;
        uint32_t piece[8], lo[4], hi[4];
        for (uint32_t j = 0; j < L.word; j++) piece[j] = ld32(coder_in + chunk * L.coder_bytes + sz_piece_at(L, j, m));
        uint8_t *p = back + chunk * L.chunk_bytes + m * 4u * L.word;
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
    }
    return 1;
}
