// aec_gribcxw.h -- WRITING GRIB2 complex packing, templates 5.2 / 5.3 and 7.2 / 7.3 (include/aec_gpu_grib.h, COMPLEX PACKING,
// the writer's rule): the per-lane arithmetic of aec_gribcxw.hip, which turns the X rooms of aec_grib.h into section 7 streams
// with groups of a fixed power-of-two length G.
//
// A stream is what aec_gribcx.h reads: the extra descriptors, the references, the widths, (no lengths: length_bits = 0), the
// packed values.  Bit positions are 64-bit; bit b is bit 7 - b % 8 of byte b / 8.
//   differences  a lane owns the values of 16 bytes of its field's room, a wavefront a value tile (1 KiB of room).  d_j is
//                X_j (order 0), X_j - X_(j-1) or X_j - 2 X_(j-1) + X_(j-2), exact in an int64_t; cxw_lane_ext gives a lane's
//                smallest and largest d over its COUNTED values (j >= order); the smallest of a field is minsd.
//   groups       G is 16 .. 256 and a tile 256 .. 1024 values, so a group is G / per adjacent lanes of one wavefront:
//                cxw_group makes the reference, the width and the bits of a group from its extremes; CxwTile is what a tile
//                leaves for its field (bits, largest reference, smallest and largest width), cxw_tile_join joins two.
//   tables       the references and the widths are bits_pack over the group tables: cxw_table_string builds a lane's four
//                entries into the string that grib_bits_store (aec_gribbits.h) stores.
//   values       lanes own OUTPUT bytes, 16 of the packed string each: cxw_group_at finds the last group whose first bit is
//                at or before the lane's (a tile's first bit, then a group's inside the tile; groups without a bit share the
//                next one's start and so are never the last), cxw_lane_string walks values and groups from there, recomputes
//                packed_j from the room and fills the lane's 128 bits.  A byte that holds parts of several values is still
//                one lane's, no lane needs another lane's bits, and the string ends in zero bits.
// nbits + order <= 32 (the host refuses anything else), so every s_j = d_j - minsd, reference and width fits 32 bits.
// Memory goes through a policy (Mem: ldx and ld128 at byte offsets from the first byte of the FIELD'S ROOM, st8 and st32 at
// byte offsets from the base of the stream buffer): plain loads and stores in the kernels, checked and counted ones in
// tests/emul/gribcxw_emul.cpp, which runs these functions launch by launch and lane by lane.  No load touches a sample
// behind value n - 1.
#pragma once
#include "aec_gribbits.h"

namespace aec {

constexpr uint32_t kCxwTableLane = 4;                      // groups of a lane of the table kernel (16 bytes of a group table)
constexpr uint32_t kCxwTableTile = 64 * kCxwTableLane;     // ... of a wavefront
constexpr uint32_t kCxwOutLane = 16;                       // bytes of the packed string a lane of the value kernel owns
constexpr uint32_t kCxwOutTile = 64 * kCxwOutLane;         // ... a wavefront

// what the whole batch is written under
struct CxwShape {
    uint32_t order, G, nbits, extra;     // extra: octets of an extra descriptor, 0 for order 0
};

// Descriptor of field i (host-written, n + 1 of them: entry n holds the totals)
struct CxwField {
    uint64_t off;                        // its stream: byte offset from d_complex
    uint64_t n, work_off, room;          // as GribField
    uint64_t vtile0, ttile0, otile0;     // its first value tile, table tile, output tile
    uint64_t group0;                     // its first entry of the group tables
    uint32_t ng, pad;
};

// what the scan over a field's tiles leaves for the lanes of the tables and of the values
struct CxwDyn {
    int64_t minsd;
    uint64_t bits;                       // of the packed string
    uint64_t data_byte;                  // the packed string's first byte, from the stream's first
    uint32_t ref_bits, width_ref, width_bits, pad;
};

// a value tile: the bits of its groups (behind the field scan: the first bit of the tile), its largest reference, its
// smallest and largest width
struct CxwTile {
    uint64_t bits;
    uint32_t max_ref, min_w, max_w, pad;
};

struct CxwGroup { uint32_t ref, width, bits; };

// aec_gpu_grib_cxw: the members of aec_gpu_grib_complex_field in their order, pad, bytes
struct CxwRecord {
    uint32_t desc[11];
    uint32_t pad;
    uint64_t bytes;
};

// the group tables of one field, from its first tile and its first group
struct CxwTables {
    const CxwTile *tile;
    const uint32_t *gref, *gwid, *gbit;  // gbit: a group's first bit from its tile's
};

AEC_HD uint32_t cxw_bitlen(uint32_t v) { return v ? 32u - (uint32_t)__builtin_clz(v) : 0u; }
AEC_HD uint32_t cxw_extra(uint32_t nbits, uint32_t order) { return order ? (nbits + order + 7u) / 8u : 0u; }
AEC_HD uint64_t cxw_head(uint32_t nbits, uint32_t order) { return order ? (uint64_t)(order + 1u) * cxw_extra(nbits, order) : 0u; }
AEC_HD uint64_t cxw_groups(uint64_t n, uint32_t G) { return (n + G - 1u) / G; }
AEC_HD uint64_t cxw_table_bytes(uint64_t ng, uint32_t bits) { return (ng * bits + 7u) / 8u; }
// bytes of the packed string at its longest
AEC_HD uint64_t cxw_string_bound(uint64_t n, uint32_t nbits, uint32_t order) { return (n * (nbits + order) + 7u) / 8u; }
// B_i: no stream is longer (n < 2^35, so nothing here wraps)
AEC_HD uint64_t cxw_bound(uint64_t n, uint32_t nbits, uint32_t order, uint32_t G)
{
    const uint64_t ng = cxw_groups(n, G);
    return cxw_head(nbits, order) + cxw_table_bytes(ng, nbits + order) + cxw_table_bytes(ng, 6u) + cxw_string_bound(n, nbits, order);
}
AEC_HD uint32_t cxw_group_len(const CxwField &F, uint32_t G, uint64_t g)
{
    const uint64_t left = F.n - g * G;
    return left < G ? (uint32_t)left : G;
}

// value j < n of the room, modulo 2^nbits
template <int CONT, class Mem>
AEC_HD uint32_t cxw_x(Mem &m, uint64_t j, uint32_t mask) { return m.ldx((int64_t)(j * CONT), CONT) & mask; }

// the values of a lane: one 16-byte load where all of them are values, one by one where the field ends inside; 0 behind it
template <int CONT, class Mem>
AEC_HD void cxw_lane_x(Mem &m, const GribBitsLane &L, uint32_t nbits, uint32_t (&x)[16 / CONT])
{
    constexpr uint32_t per = 16u / CONT;
    if (L.cnt == per) {
        uint32_t w[4];
        m.ld128((int64_t)(L.j0 * CONT), w);
        grib_bits_take<CONT>(w, nbits, per, x);
        return;
    }
    const uint32_t mask = low_mask32(nbits);
#pragma unroll
    for (uint32_t i = 0; i < per; i++) x[i] = i < L.cnt ? cxw_x<CONT>(m, L.j0 + i, mask) : 0u;
}

// what the first lane of a tile loads: the one or two values in front of value j0 (0 where there is none or the order
// does not ask)
template <int CONT, class Mem>
AEC_HD void cxw_pred(Mem &m, uint64_t j0, uint32_t order, uint32_t nbits, uint32_t *p1, uint32_t *p2)
{
    const uint32_t mask = low_mask32(nbits);
    *p1 = (order >= 1u && j0 >= 1u) ? cxw_x<CONT>(m, j0 - 1u, mask) : 0u;
    *p2 = (order == 2u && j0 >= 2u) ? cxw_x<CONT>(m, j0 - 2u, mask) : 0u;
}

AEC_HD int64_t cxw_d(uint32_t order, uint32_t x, uint32_t x1, uint32_t x2)
{
    return order == 0u ? (int64_t)x : order == 1u ? (int64_t)x - (int64_t)x1 : (int64_t)x - 2 * (int64_t)x1 + (int64_t)x2;
}

// smallest and largest d of the lane's counted values; lo > hi where it has none.  p1, p2: the values in front of j0
template <int PER>
AEC_HD void cxw_lane_ext(const uint32_t (&x)[PER], uint64_t j0, uint32_t cnt, uint32_t order, uint32_t p1, uint32_t p2, int64_t *lo, int64_t *hi)
{
    int64_t a = INT64_MAX, b = INT64_MIN;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)PER; i++) {
        if (i < cnt && j0 + i >= order) {
            const int64_t d = cxw_d(order, x[i], p1, p2);
            a = d < a ? d : a;
            b = d > b ? d : b;
        }
        p2 = p1;
        p1 = x[i];
    }
    *lo = a;
    *hi = b;
}

// a group of len values from the extremes of its counted d
AEC_HD CxwGroup cxw_group(int64_t lo, int64_t hi, int64_t minsd, uint32_t len)
{
    if (lo > hi) return CxwGroup{0u, 0u, 0u};
    const uint32_t width = cxw_bitlen((uint32_t)(hi - lo));
    return CxwGroup{(uint32_t)(lo - minsd), width, len * width};
}

AEC_HD CxwTile cxw_tile_none() { return CxwTile{0u, 0u, 0xFFFFFFFFu, 0u, 0u}; }
AEC_HD CxwTile cxw_tile_of(const CxwGroup &g) { return CxwTile{g.bits, g.ref, g.width, g.width, 0u}; }
AEC_HD CxwTile cxw_tile_join(const CxwTile &a, const CxwTile &b)
{
    return CxwTile{a.bits + b.bits, a.max_ref > b.max_ref ? a.max_ref : b.max_ref, a.min_w < b.min_w ? a.min_w : b.min_w,
                   a.max_w > b.max_w ? a.max_w : b.max_w, 0u};
}

// the record of a field from the join of its tiles (every field has a group)
AEC_HD CxwDyn cxw_dyn(const CxwField &F, const CxwShape &P, const CxwTile &all, int64_t minsd)
{
    CxwDyn Y;
    Y.minsd = P.order ? minsd : 0;
    Y.bits = all.bits;
    Y.ref_bits = cxw_bitlen(all.max_ref);
    Y.width_ref = all.min_w;
    Y.width_bits = cxw_bitlen(all.max_w - all.min_w);
    Y.pad = 0u;
    Y.data_byte = cxw_head(P.nbits, P.order) + cxw_table_bytes(F.ng, Y.ref_bits) + cxw_table_bytes(F.ng, Y.width_bits);
    return Y;
}

AEC_HD CxwRecord cxw_record(const CxwField &F, const CxwShape &P, const CxwDyn &Y)
{
    CxwRecord R;
    R.desc[0] = Y.ref_bits;
    R.desc[1] = F.ng;
    R.desc[2] = Y.width_ref;
    R.desc[3] = Y.width_bits;
    R.desc[4] = P.G;                                          // length_ref
    R.desc[5] = 1u;                                           // length_inc
    R.desc[6] = (uint32_t)(F.n - (uint64_t)(F.ng - 1u) * P.G);  // last_length
    R.desc[7] = 0u;                                           // length_bits: the lengths table is empty
    R.desc[8] = P.order;
    R.desc[9] = P.extra;
    R.desc[10] = 0u;                                          // missing
    R.pad = 0u;
    R.bytes = Y.data_byte + (Y.bits + 7u) / 8u;
    return R;
}

// sign and magnitude in `octets` bytes at byte `at` of the stream buffer; zero is plus zero
template <class Mem>
AEC_HD void cxw_put_sm(Mem &m, uint64_t at, int64_t v, uint32_t octets)
{
    const uint64_t word = (uint64_t)(v < 0 ? -v : v) | (v < 0 ? 1ull << (8u * octets - 1u) : 0ull);
    for (uint32_t b = 0; b < octets; b++) m.st8((int64_t)(at + b), (uint8_t)(word >> (8u * (octets - 1u - b))));
}

// the extra descriptors of a field: ival1, ival2 (order 2), minsd.  One lane of the field scan writes them.
template <int CONT, class Mem>
AEC_HD void cxw_head_bytes(Mem &m, const CxwField &F, const CxwShape &P, const CxwDyn &Y)
{
    if (P.order == 0u) return;
    const uint32_t mask = low_mask32(P.nbits);
    cxw_put_sm(m, F.off, (int64_t)cxw_x<CONT>(m, 0, mask), P.extra);
    if (P.order == 2u) cxw_put_sm(m, F.off + P.extra, F.n > 1u ? (int64_t)cxw_x<CONT>(m, 1, mask) : 0, P.extra);
    cxw_put_sm(m, F.off + (uint64_t)P.order * P.extra, Y.minsd, P.extra);
}

// A lane of the table kernel: entries g0 .. g0 + 4 of a group table (less `sub`) as a string of `bits`-bit integers, bits >= 1;
// *cnt: those of them below ng
AEC_HD void cxw_table_string(const uint32_t *tab, uint32_t sub, uint64_t g0, uint64_t ng, uint32_t bits, uint64_t *hi, uint64_t *lo, uint32_t *cnt)
{
    uint32_t w[4];
    *cnt = g0 >= ng ? 0u : (ng - g0 < kCxwTableLane ? (uint32_t)(ng - g0) : kCxwTableLane);
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) w[i] = i < *cnt ? tab[g0 + i] - sub : 0u;
    grib_bits_of_group<4>(w, bits, *cnt, hi, lo);
}

// The LAST group whose first bit is <= p, for p below the field's bits: such a group has bits of its own.  gpt: the groups
// of a tile.  (The first tile starts at 0 and so does the first group of a tile.)
AEC_HD uint64_t cxw_group_at(const CxwTables &T, uint64_t ng, uint32_t gpt, uint64_t p)
{
    uint64_t lo = 0, hi = (ng + gpt - 1u) / gpt;
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (T.tile[mid].bits <= p) lo = mid;
        else hi = mid;
    }
    const uint64_t base = T.tile[lo].bits, g0 = lo * gpt;
    uint32_t a = 0, b = ng - g0 < gpt ? (uint32_t)(ng - g0) : gpt;
    while (b - a > 1u) {
        const uint32_t mid = a + (b - a) / 2u;
        if (base + T.gbit[g0 + mid] <= p) a = mid;
        else b = mid;
    }
    return g0 + a;
}

// `take` bits (1 .. 32) behind the first `filled` of the 128-bit string hi : lo.  (Both halves are written whatever the place:
// a choice between the two ADDRESSES would put the string into memory.)
AEC_HD void cxw_put(uint64_t &hi, uint64_t &lo, uint32_t filled, uint32_t chunk, uint32_t take)
{
    const uint32_t sh = 128u - filled - take;        // the chunk's last bit from the string's last: 0 .. 127
    const uint64_t c = chunk;
    hi |= sh >= 64u ? c << (sh - 64u) : (sh ? c >> (64u - sh) : 0u);
    lo |= sh >= 64u ? 0u : c << sh;
}

// A lane of the value kernel: the 16 bytes from byte 16 * lane_in_field of the packed string, left aligned in hi : lo and
// zero behind the string's last bit.  Returns the bytes of them the string has (0 .. 16).
template <int CONT, class Mem>
AEC_HD uint32_t cxw_lane_string(Mem &m, const CxwField &F, const CxwShape &P, const CxwDyn &Y, const CxwTables &T, uint64_t lane_in_field,
                                uint64_t *hi, uint64_t *lo)
{
    *hi = *lo = 0u;
    const uint64_t p0 = lane_in_field * (8u * kCxwOutLane);
    if (p0 >= Y.bits) return 0u;
    uint64_t h = 0, l = 0;
    const uint64_t left = (Y.bits - p0 + 7u) / 8u;
    const uint32_t gpt = kGribWaveRoom / CONT / P.G, mask = low_mask32(P.nbits);
    uint64_t g = cxw_group_at(T, F.ng, gpt, p0);
    uint32_t filled = 0;
    for (;;) {
        const uint64_t start = T.tile[g / gpt].bits + T.gbit[g], j0 = g * P.G;
        const uint32_t w = T.gwid[g], ref = T.gref[g], len = cxw_group_len(F, P.G, g);
        const uint32_t rel = (uint32_t)(p0 + filled - start);        // (a group has at most 256 * 32 bits; w >= 1 here)
        uint32_t k = rel / w, skip = rel - k * w;
        uint32_t x1, x2;
        cxw_pred<CONT>(m, j0 + k, P.order, P.nbits, &x1, &x2);
        for (; k < len && filled < 128u; k++) {
            const uint64_t j = j0 + k;
            const uint32_t x = cxw_x<CONT>(m, j, mask);
            const uint32_t packed = j < P.order ? 0u : (uint32_t)(cxw_d(P.order, x, x1, x2) - Y.minsd) - ref;
            x2 = x1;
            x1 = x;
            const uint32_t avail = w - skip, take = avail < 128u - filled ? avail : 128u - filled;
            cxw_put(h, l, filled, (packed & low_mask32(avail)) >> (avail - take), take);
            filled += take;
            skip = 0u;
        }
        if (filled >= 128u || p0 + filled >= Y.bits) break;
        g++;                                                         // (bits follow, so groups do)
        if (T.gwid[g] == 0u) g = cxw_group_at(T, F.ng, gpt, p0 + filled);
    }
    *hi = h;
    *lo = l;
    return left < kCxwOutLane ? (uint32_t)left : kCxwOutLane;
}

// the field that owns tile t of the value tiles (which = 0), the table tiles (1) or the output tiles (2); every field has
// one of each at least
AEC_HD uint64_t cxw_field_of_tile(const CxwField *d, uint64_t n, int which, uint64_t t)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        const uint64_t first = which == 0 ? d[mid].vtile0 : which == 1 ? d[mid].ttile0 : d[mid].otile0;
        if (first <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace aec
