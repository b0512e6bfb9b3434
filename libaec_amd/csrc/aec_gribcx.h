// aec_gribcx.h -- GRIB2 complex packing, templates 5.2 / 5.3 and 7.2 / 7.3 (include/aec_gpu_grib.h, COMPLEX PACKING): the
// per-lane arithmetic of aec_gribcx.hip, which expands section 7 streams into the X rooms of aec_grib.h.
//
// A stream is: the extra descriptors (sign-magnitude), three tables of NG big-endian integers (references, widths, lengths),
// each padded to a byte, then the packed values group after group.  Bit positions are counted from bit 7 of the STREAM's
// first byte and are 64-bit; bit b is bit 7 - b % 8 of byte b / 8.
//   groups   cx_group: a lane a group -- its reference, width and (len, len * width), saturated; cx_sum_add, the saturating
//            sum the two scans over them use: group starts in values and in bits
//   values   cx_lane_values: a lane owns the values of one 16-byte group of its field's room, as in k_grib_quantise; it
//            finds the group of its first value by binary search over the group starts (cx_group_of), walks forward and
//            leaves d_j = ref + packed + minsd per value
//   orders   with d_0 = ival1 (and, order 2, d_1 = ival2 - 2 ival1) spatial differencing is one running sum (order 1) or
//            two nested ones (order 2) over d: Y_j = Y_(j-1) + d_j, X_j = X_(j-1) + Y_j.  A run of L values from a zero
//            state has the aggregate CxAgg (Y and X at its end); cx_combine joins two runs.  All of it modulo 2^64.
// NO WRAP IN THE COUNTS.  A group length above n counts as n + 1, a width above 32 as "every bit the stream has left and one
// more", and both running sums are held at those caps (n + 1 values, 8 * (bytes - head) + 1 bits): the sums stay below 2^40
// whatever the tables hold, a sum that reached its cap says MALFORMED, and saturating addition is associative, so the
// scans may combine in any order.  Every read of the stream is bounded by the stream's own end (cx_read gives 0 for an
// integer that would cross it): no load leaves [off, off + bytes) whatever the bytes contain.
// Memory of the STREAM goes through a policy (Mem: ld8 at byte offsets from the stream's first byte): plain loads in the
// kernels, checked and counted ones in tests/emul/gribcx_emul.cpp, which runs these functions lane by lane.
#pragma once
#include "aec_gribbits.h"

namespace aec {

enum { kCxRange = 1u, kCxMalformed = 2u };       // status bits of a d_cx record
constexpr uint32_t kCxGroupTile = 64;            // groups of a group tile: a wavefront, a lane a group
constexpr uint64_t kCxMaxBytes = 1ull << 35;     // a stream is shorter than this

// Descriptor of field i (host-written, n + 1 of them: entry n holds the totals in vtile0, gtile0 and group0)
struct CxField {
    uint64_t off, bytes;                 // the stream: byte offset from d_complex, complex_bytes_each
    uint64_t n, work_off, room;          // as GribField
    uint64_t vtile0, gtile0, group0;     // its first value tile, first group tile, first entry of the group tables
    uint64_t refs_bit, widths_bit, lengths_bit, data_bit;   // where the three tables and the packed values start
    uint32_t ng, ref_bits, width_ref, width_bits, length_ref, length_inc, last_length, length_bits, order, extra;
};

// what the scan over a field's groups leaves for its value lanes
struct CxDyn {
    uint64_t d0, d1, minsd;              // d_0 = ival1, d_1 = ival2 - 2 ival1, minsd
    uint64_t xlast;                      // X of value n - 1, orders 1 and 2 (the scan over the value tiles writes it)
    uint32_t malformed, pad;
};

struct CxSum { uint64_t v, b; };         // values, bits: saturating
struct CxAgg { uint64_t s, w; };         // Y and X behind a run of values that started from Y = X = 0
struct CxExt { int64_t lo, hi; };        // signed reading of the X seen so far

AEC_HD uint64_t cx_cap_values(const CxField &F) { return F.n + 1u; }
AEC_HD uint64_t cx_cap_bits(const CxField &F) { return 8u * F.bytes - F.data_bit + 1u; }

AEC_HD CxSum cx_sum_add(CxSum a, CxSum c, uint64_t capv, uint64_t capb)
{
    const uint64_t v = a.v + c.v, b = a.b + c.b;         // (each below 2^39)
    return CxSum{v < capv ? v : capv, b < capb ? b : capb};
}

// an integer of w bits at bit p; 0 for w == 0 and for one that would cross the stream's end
template <class Mem>
AEC_HD uint32_t cx_read(Mem &m, uint64_t p, uint32_t w, uint64_t end_bits)
{
    if (w == 0u || p + w > end_bits) return 0u;
    return grib_bits_value_at(m, p, w);
}

// sign and magnitude in `octets` bytes (0 .. 8) at a byte, as a two's complement number; "minus zero" is 0
template <class Mem>
AEC_HD uint64_t cx_read_sm(Mem &m, uint64_t byte, uint32_t octets)
{
    if (octets == 0u) return 0u;
    uint64_t v = 0;
    for (uint32_t b = 0; b < octets; b++) v = (v << 8) | (uint64_t)m.ld8((int64_t)(byte + b));
    const uint64_t sign = 1ull << (8u * octets - 1u), mag = v & (sign - 1u);
    return (v & sign) ? 0u - mag : mag;
}

// group g < ng of a field
struct CxGroup {
    uint32_t ref, width;                 // width 0 where the stream says more than 32
    CxSum s;                             // (len, len * width), saturated
};
template <class Mem>
AEC_HD CxGroup cx_group(Mem &m, const CxField &F, uint64_t g)
{
    const uint64_t end = 8u * F.bytes, capv = cx_cap_values(F), capb = cx_cap_bits(F);
    CxGroup G;
    G.ref = cx_read(m, F.refs_bit + g * F.ref_bits, F.ref_bits, end);
    const uint64_t wide = (uint64_t)F.width_ref + cx_read(m, F.widths_bit + g * F.width_bits, F.width_bits, end);
    const uint64_t stored = cx_read(m, F.lengths_bit + g * F.length_bits, F.length_bits, end);
    const uint64_t len = g + 1u == F.ng ? (uint64_t)F.last_length : (uint64_t)F.length_ref + stored * F.length_inc;     // < 2^41
    G.s.v = len < capv ? len : capv;
    if (wide > 32u) {
        G.width = 0u;
        G.s.b = capb;
    } else {
        G.width = (uint32_t)wide;
        const uint64_t bits = G.s.v * wide;             // < 2^41
        G.s.b = bits < capb ? bits : capb;
    }
    return G;
}

// the record of a field from the totals of its groups
template <class Mem>
AEC_HD CxDyn cx_dyn(Mem &m, const CxField &F, CxSum total)
{
    CxDyn Y{};
    Y.malformed = (total.v != F.n || total.b >= cx_cap_bits(F)) ? 1u : 0u;
    if (F.order >= 1u) {
        const uint64_t ival1 = cx_read_sm(m, 0, F.extra);
        const uint64_t ival2 = F.order == 2u ? cx_read_sm(m, F.extra, F.extra) : 0u;
        Y.minsd = cx_read_sm(m, (uint64_t)F.order * F.extra, F.extra);
        Y.d0 = ival1;
        Y.d1 = ival2 - 2u * ival1;
    }
    return Y;
}

// the group tables of one field: starts in values and in bits (from data_bit), references, widths
struct CxTables {
    const uint64_t *gval, *gbit;
    const uint32_t *gref, *gwid;
};

// the LAST group whose first value is <= j (groups without a value share the next one's start; gval[0] = 0)
AEC_HD uint64_t cx_group_of(const uint64_t *gval, uint64_t ng, uint64_t j)
{
    uint64_t lo = 0, hi = ng;
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (gval[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// d of the values j0 .. j0 + cnt (cnt <= PER, all below n); 0 behind them
template <int PER, class Mem>
AEC_HD void cx_lane_values(Mem &m, const CxField &F, const CxDyn &Y, const CxTables &T, uint64_t j0, uint32_t cnt, uint64_t (&d)[PER])
{
    const uint64_t end = 8u * F.bytes, add = F.order ? Y.minsd : 0u;
    uint64_t g = 0, start = 0, next = ~0ull, bit = 0;
    uint32_t ref = 0, w = 0;
    if (cnt) {
        g = cx_group_of(T.gval, F.ng, j0);
        start = T.gval[g];
        next = g + 1u < F.ng ? T.gval[g + 1u] : ~0ull;
        bit = T.gbit[g];
        ref = T.gref[g];
        w = T.gwid[g];
    }
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)PER; i++) {
        d[i] = 0u;
        if (i >= cnt) continue;
        const uint64_t j = j0 + i;
        while (j >= next) {                             // (at most ng steps: next is ~0 at the last group)
            g++;
            start = next;
            next = g + 1u < F.ng ? T.gval[g + 1u] : ~0ull;
            bit = T.gbit[g];
            ref = T.gref[g];
            w = T.gwid[g];
        }
        const uint64_t v = cx_read(m, F.data_bit + bit + (j - start) * w, w, end);         // (j - start < 2^36, bit < 2^39)
        d[i] = j < F.order ? (j == 0u ? Y.d0 : Y.d1) : (uint64_t)ref + v + add;
    }
}

// a then b, b a run of Lb values.  Also: the state behind Lb values of aggregate b that follow the state a.
AEC_HD CxAgg cx_combine(CxAgg a, CxAgg b, uint64_t Lb) { return CxAgg{a.s + b.s, a.w + Lb * a.s + b.w}; }

template <int PER>
AEC_HD CxAgg cx_lane_agg(const uint64_t (&d)[PER])
{
    uint64_t y = 0, x = 0;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)PER; i++) {
        y += d[i];
        x += y;
    }
    return CxAgg{y, x};
}

// X of a lane's values from the state in front of them, in place of their d
template <int PER>
AEC_HD void cx_lane_x(uint64_t (&d)[PER], uint32_t order, CxAgg in)
{
    uint64_t y = in.s, X = in.w;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)PER; i++) {
        y += d[i];
        X += y;
        d[i] = order == 0u ? d[i] : order == 1u ? y : X;
    }
}

// X of value n - 1 from the state behind `covered` >= n values of which those from n on had d = 0
AEC_HD uint64_t cx_last_x(CxAgg behind, uint32_t order, uint64_t covered, uint64_t n)
{
    return order == 1u ? behind.s : behind.w - (covered - n) * behind.s;
}

AEC_HD CxExt cx_ext_none() { return CxExt{INT64_MAX, INT64_MIN}; }
AEC_HD CxExt cx_ext_join(CxExt a, CxExt b) { return CxExt{a.lo < b.lo ? a.lo : b.lo, a.hi > b.hi ? a.hi : b.hi}; }

// The 16 bytes a lane stores: its cnt values modulo 2^nbits, `last` (X of value n - 1) behind them; e takes the values in.
template <int CONT>
AEC_HD void cx_lane_words(const uint64_t (&x)[16 / CONT], uint32_t cnt, uint64_t last, uint32_t nbits, CxExt *e, uint32_t (&w)[4])
{
    const uint32_t mask = low_mask32(nbits);
    uint32_t c[16 / CONT];
#pragma unroll
    for (uint32_t i = 0; i < 16u / CONT; i++) {
        if (i < cnt) *e = cx_ext_join(*e, CxExt{(int64_t)x[i], (int64_t)x[i]});
        c[i] = (uint32_t)(i < cnt ? x[i] : last) & mask;
    }
    grib_bits_give<CONT>(c, w);
}

AEC_HD uint32_t cx_status(const CxDyn &Y, CxExt e, uint32_t nbits)
{
    const int64_t M = (int64_t)((1ull << nbits) - 1u);
    return (Y.malformed ? (uint32_t)kCxMalformed : 0u) | ((e.lo < 0 || e.hi > M) ? (uint32_t)kCxRange : 0u);
}

// the field that owns tile t of the value tiles (which = 1) or the group tiles (0); every field has one of each at least
AEC_HD uint64_t cx_field_of_tile(const CxField *d, uint64_t n, int which, uint64_t t)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if ((which ? d[mid].vtile0 : d[mid].gtile0) <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// bytes of a table of ng integers of `bits` bits
AEC_HD uint64_t cx_table_bytes(uint64_t ng, uint32_t bits) { return (ng * bits + 7u) / 8u; }

}  // namespace aec
