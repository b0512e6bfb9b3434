// aec_gribbits.h -- GRIB2 simple packing, template 7.0 (include/aec_gpu_grib.h, SIMPLE PACKING): the per-lane arithmetic of
// aec_gribbits.hip between the X rooms of aec_grib.h and big-endian strings of nbits-bit integers at any byte.
//
// Value j of a field is the bits [j * nbits, (j + 1) * nbits) of its stream, bit b of a stream bit 7 - b % 8 of byte b / 8.
// A lane owns one 16-byte group of its field's room, as in k_grib_quantise: per = 16 / 8 / 4 values for containers of
// 1 / 2 / 4 bytes, at most 128 bits of the stream, held left aligned in two 64-bit halves hi : lo ("the string").  Bit
// positions are counted from bit 7 of the first byte of the call's buffer and are 64-bit.
//   rooms -> streams   grib_bits_take (the group's values, taken modulo 2^nbits), grib_bits_join (the string),
//                      grib_bits_store (the bytes the lane owns: those whose FIRST bit is one of its own; the last of
//                      them is filled from the next lane's string, or with zeros behind value n - 1)
//   streams -> rooms   grib_bits_load (the string, by aligned words inside the buffer and bytes at its ends),
//                      grib_bits_split (the values), grib_bits_value_at (value n - 1 by its own bit position, for the
//                      samples that pad the last block)
// per * nbits is a multiple of 8 for containers 1 and 2, so such a lane's string starts and ends on a byte.  A lane of 4
// values ends on half a byte for odd nbits: then the even lanes end, and the odd lanes start, four bits into a byte.  That
// byte is the even lane's; the odd lane's first four bits reach it through a shuffle (the next lane's `head`).
// Memory goes through a policy (Mem: ld8, ld32, st8, st32 at byte offsets from the buffer's base): plain loads and stores
// in the kernels, checked and counted ones in tests/emul/gribbits_emul.cpp, which runs these functions lane by lane.
#pragma once
#include "aec_grib.h"

namespace aec {

// where the values of a lane's group lie
struct GribBitsLane {
    uint64_t j0;        // the group's first sample
    uint32_t cnt;       // its samples that are values (below n): 0 .. per
    uint64_t p0, p1;    // the bits of those values: [p0, p1)
};

AEC_HD GribBitsLane grib_bits_lane(uint64_t wave_in_field, uint32_t lane, uint32_t per, uint64_t n, uint64_t off, uint32_t nbits)
{
    GribBitsLane L;
    L.j0 = (wave_in_field * 64u + lane) * per;
    L.cnt = L.j0 >= n ? 0u : (n - L.j0 < per ? (uint32_t)(n - L.j0) : per);
    L.p0 = off * 8u + L.j0 * nbits;
    L.p1 = L.p0 + (uint64_t)L.cnt * nbits;
    return L;
}

// bytes of the stream of n values
AEC_HD uint64_t grib_bits_bytes(uint64_t n, uint32_t nbits) { return (n * nbits + 7u) / 8u; }

// the group's values from its 16 bytes: modulo 2^nbits, 0 behind the last value
template <int CONT>
AEC_HD void grib_bits_take(const uint32_t (&w)[4], uint32_t nbits, uint32_t cnt, uint32_t (&x)[16 / CONT])
{
    const uint32_t mask = low_mask32(nbits);
#pragma unroll
    for (uint32_t i = 0; i < 16u / CONT; i++) {
        const uint32_t v = CONT == 4 ? w[i * CONT / 4u] : (w[i * CONT / 4u] >> (8u * (i * CONT % 4u))) & (CONT == 1 ? 0xFFu : 0xFFFFu);
        x[i] = i < cnt ? v & mask : 0u;
    }
}

// the reverse: values into the 16 bytes
template <int CONT>
AEC_HD void grib_bits_give(const uint32_t (&x)[16 / CONT], uint32_t (&w)[4])
{
    w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 16u / CONT; i++) w[i * CONT / 4u] |= x[i] << (8u * (i * CONT % 4u));
}

// The string of per values (each below 2^nbits).  Half of them fit 64 bits whatever nbits the container allows, so the
// halves are built in 64-bit registers and meet once.
template <int CONT>
AEC_HD void grib_bits_join(const uint32_t (&x)[16 / CONT], uint32_t nbits, uint64_t *hi, uint64_t *lo)
{
    constexpr uint32_t half = 8u / CONT;
    uint64_t a = 0, b = 0;
#pragma unroll
    for (uint32_t i = 0; i < half; i++) {
        a = (a << nbits) | x[i];
        b = (b << nbits) | x[half + i];
    }
    const uint32_t w = half * nbits;                 // 8 .. 64
    const uint64_t A = a << (64u - w), B = b << (64u - w);
    *hi = A | ((B >> 1) >> (w - 1u));
    *lo = B << (64u - w);
}

template <int CONT>
AEC_HD void grib_bits_split(uint64_t hi, uint64_t lo, uint32_t nbits, uint32_t (&x)[16 / CONT])
{
    constexpr uint32_t half = 8u / CONT;
    const uint32_t w = half * nbits, mask = low_mask32(nbits);
    const uint64_t B = ((hi << (w - 1u)) << 1) | (lo >> (64u - w));
#pragma unroll
    for (uint32_t i = 0; i < half; i++) {
        const uint32_t down = 64u - (i + 1u) * nbits;
        x[i] = (uint32_t)(hi >> down) & mask;
        x[half + i] = (uint32_t)(B >> down) & mask;
    }
}

// what a lane hands to the lane in front of it: the first 32 bits of its string
AEC_HD uint32_t grib_bits_head(uint64_t hi) { return (uint32_t)(hi >> 32); }

// word k (0 .. 4) of a 128-bit string moved back by `back` bytes (0 .. 3), big-endian: what lies in the aligned word
// that holds the bytes 4k - back .. 4k + 3 - back of the string
AEC_HD uint32_t grib_bits_window(const uint32_t (&t)[4], uint32_t k, uint32_t back)
{
    const uint32_t prev = k ? t[k - 1u] : 0u, cur = k < 4u ? t[k] : 0u;
    return back ? (prev << (32u - 8u * back)) | (cur >> (8u * back)) : cur;
}

// The lane's bytes of the stream: [ceil(p0 / 8), ceil(p1 / 8)), every byte whole and once.  next_head: the head of the
// next lane's string, 0 where there is none or it has no value.  mis: the buffer's address modulo 4 -- words are stored
// where their ADDRESS is a multiple of 4 and they lie inside the lane's bytes, single bytes elsewhere.
template <class Mem>
AEC_HD void grib_bits_store(Mem &m, uint64_t hi, uint64_t lo, uint64_t p0, uint64_t p1, uint32_t next_head, uint32_t mis)
{
    if (p1 <= p0) return;
    const uint32_t q = (uint32_t)(p0 & 7u), r = (uint32_t)(p1 & 7u), len = (uint32_t)(p1 - p0);
    if (r) {
        // (only a lane that starts on a byte has a follower inside its last byte: the end of the filled byte is a
        // multiple of 8 bits into the string and never straddles the two halves)
        const uint64_t v = next_head >> (24u + r);
        const uint32_t end = len + 8u - r;
        if (end <= 64u) hi |= v << (64u - end);
        else if (end <= 128u) lo |= v << (128u - end);
    }
    if (q) {                                         // the byte the string starts in is the lane's in front
        const uint32_t d = 8u - q;
        hi = (hi << d) | (lo >> (64u - d));
        lo <<= d;
    }
    const uint64_t bs = (p0 + 7u) >> 3, be = (p1 + 7u) >> 3;
    const uint32_t nb = (uint32_t)(be - bs);         // 0 .. 16
    const uint32_t k0 = (uint32_t)((mis + bs) & 3u);
    const uint32_t t[4] = {(uint32_t)(hi >> 32), (uint32_t)hi, (uint32_t)(lo >> 32), (uint32_t)lo};
    const int64_t first = (int64_t)bs - (int64_t)k0;
#pragma unroll
    for (uint32_t k = 0; k < 5u; k++) {
        const uint32_t w = grib_bits_window(t, k, k0);
        if (4u * k >= k0 && 4u * k + 4u <= k0 + nb) {
            m.st32(first + 4 * (int64_t)k, bswap32(w));
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 4u; b++)
                if (4u * k + b >= k0 && 4u * k + b < k0 + nb) m.st8(first + 4 * (int64_t)k + b, (uint8_t)(w >> (24u - 8u * b)));
        }
    }
}

// The string that starts at bit p0; the bits behind p1 are whatever follows in the buffer.  The words that hold the
// bytes [p0 / 8, ceil(p1 / 8)) are loaded whole where they lie inside [0, simple_bytes), byte by byte where they cross an
// end of it: no load leaves the buffer.  p1 - p0 <= 128, p1 > p0.
template <class Mem>
AEC_HD void grib_bits_load(Mem &m, uint64_t p0, uint64_t p1, uint32_t mis, uint64_t simple_bytes, uint64_t *hi, uint64_t *lo)
{
    const uint64_t b0 = p0 >> 3, b1 = (p1 + 7u) >> 3;
    const uint32_t k0 = (uint32_t)((mis + b0) & 3u), need = k0 + (uint32_t)(b1 - b0);          // <= 3 + 17
    const int64_t first = (int64_t)b0 - (int64_t)k0, size = (int64_t)simple_bytes;
    uint32_t w[5];
#pragma unroll
    for (uint32_t k = 0; k < 5u; k++) {
        w[k] = 0u;
        if (4u * k >= need) continue;
        const int64_t o = first + 4 * (int64_t)k;
        if (o >= 0 && o + 4 <= size) {
            w[k] = bswap32(m.ld32(o));
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 4u; b++)
                if (o + b >= 0 && o + b < size) w[k] |= (uint32_t)m.ld8(o + b) << (24u - 8u * b);
        }
    }
    const uint32_t s = 8u * k0 + (uint32_t)(p0 & 7u);            // 0 .. 31
    uint32_t t[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) t[k] = s ? (w[k] << s) | (w[k + 1u] >> (32u - s)) : w[k];
    *hi = ((uint64_t)t[0] << 32) | t[1];
    *lo = ((uint64_t)t[2] << 32) | t[3];
}

// one value by its bit position: its at most five bytes, one by one
template <class Mem>
AEC_HD uint32_t grib_bits_value_at(Mem &m, uint64_t p, uint32_t nbits)
{
    const uint64_t b0 = p >> 3;
    const uint32_t q = (uint32_t)(p & 7u), bytes = (q + nbits + 7u) >> 3;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 5u; b++) v = (v << 8) | (b < bytes ? (uint64_t)m.ld8((int64_t)(b0 + b)) : 0u);
    return (uint32_t)(v >> (40u - q - nbits)) & low_mask32(nbits);
}

// A lane of the pack: the group's 16 bytes (w) to its string
template <int CONT>
AEC_HD void grib_bits_of_group(const uint32_t (&w)[4], uint32_t nbits, uint32_t cnt, uint64_t *hi, uint64_t *lo)
{
    uint32_t x[16 / CONT];
    grib_bits_take<CONT>(w, nbits, cnt, x);
    grib_bits_join<CONT>(x, nbits, hi, lo);
}

// A lane of the unpack: the 16 bytes of its group.  Samples behind value n - 1 take that value, read at ITS place in the
// stream (it may be another lane's, another wavefront's).
template <int CONT, class Mem>
AEC_HD void grib_bits_group_of(Mem &m, const GribBitsLane &L, uint64_t off, uint64_t n, uint32_t nbits, uint32_t mis,
                               uint64_t simple_bytes, uint32_t (&w)[4])
{
    constexpr uint32_t per = 16u / CONT;
    uint32_t x[per];
    if (L.cnt) {
        uint64_t hi, lo;
        grib_bits_load(m, L.p0, L.p1, mis, simple_bytes, &hi, &lo);
        grib_bits_split<CONT>(hi, lo, nbits, x);
    }
    if (L.cnt < per) {
        const uint32_t last = grib_bits_value_at(m, off * 8u + (n - 1u) * nbits, nbits);
#pragma unroll
        for (uint32_t i = 0; i < per; i++)
            if (i >= L.cnt) x[i] = last;
    }
    grib_bits_give<CONT>(x, w);
}

}  // namespace aec
