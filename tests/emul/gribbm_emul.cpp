// gribbm_emul.cpp -- host harness for libaec_amd/csrc/aec_gribbm.h: what k_grib_bm_build, k_grib_bm_minmax, k_grib_bm_scan,
// k_grib_bm_quantise and k_grib_bm_expand (libaec_amd/csrc/aec_gribbm.hip) do wavefront by wavefront and lane by lane,
// through the same functions and the same descriptors.  Every access goes through a check against the field's elements,
// its bitmap or its room: an access outside is skipped and counted, and the count is what the calls return (0 = none).
// Built by tests/test_grib_bitmap_emul.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../libaec_amd/csrc/aec_gribbm.h"

using namespace aec;

namespace {

struct Batch {
    std::vector<GribField> d;
    std::vector<GribBitmap> b;
    uint64_t tiles = 0;
    int64_t outside = 0;
};

Batch describe(const uint64_t *offsets, const uint64_t *n_points, const uint64_t *bm_offsets, const uint64_t *n_values,
               const uint64_t *work_offsets, const int32_t *D, int have, const GribRecord *params, uint64_t n, uint32_t bs, uint32_t nbits)
{
    Batch B;
    B.d.assign(n + 1, GribField{});
    B.b.assign(n + 1, GribBitmap{});
    for (uint64_t i = 0; i < n; i++) {
        GribField &f = B.d[i];
        f.off = offsets[i];
        f.n = n_values ? n_values[i] : 0;
        f.work_off = work_offsets ? work_offsets[i] : 0;
        f.room = n_values ? grib_room(f.n, bs, grib_container(nbits)) : 0;
        f.given.D = D ? D[i] : params ? params[i].D : 0;
        if (have) {
            f.given.R = params[i].R;
            f.given.E = params[i].E;
            f.given.status = 1;
        }
        B.b[i] = GribBitmap{bm_offsets[i], n_points[i], B.tiles};
        B.tiles += grib_bm_tiles(n_points[i]);
    }
    B.b[n].tile0 = B.tiles;
    return B;
}

// the lane's word, by the bytes grib_bm_lane names
uint32_t word_of(Batch &B, const uint8_t *bitmap, const GribBitmap &bm, const GribBmLane &L)
{
    uint32_t byte[2] = {0, 0};
    for (uint32_t k = 0; k < L.nbytes; k++) {
        if (L.byte0 + k >= grib_bm_bytes(bm.points)) B.outside++;
        else byte[k] = bitmap[bm.bm_off + L.byte0 + k];
    }
    return grib_bm_word(byte[0], byte[1], L.valid);
}

// the inclusive scan over 64 lanes, step by step as the wavefront does it
void wave_scan(uint32_t v[64])
{
    for (uint32_t off = 1; off < 64; off <<= 1) {
        uint32_t next[64];
        for (uint32_t lane = 0; lane < 64; lane++) next[lane] = grib_bm_scan_step(v[lane], lane >= off ? v[lane - off] : 0u, lane, off);
        memcpy(v, next, sizeof(next));
    }
}

template <typename T>
bool value_at(Batch &B, const uint8_t *src, const GribField &F, const GribBitmap &bm, uint64_t point, T *v)
{
    if (point >= bm.points) {
        B.outside++;
        return false;
    }
    memcpy(v, src + F.off + point * sizeof(T), sizeof(T));
    return true;
}

// the counts of every tile; with values the keys of the present points into the extremes
template <typename T, typename K>
void minmax(Batch &B, uint64_t n, const uint8_t *bitmap, const uint8_t *src, uint64_t *extremes, std::vector<uint32_t> &counts)
{
    counts.assign(B.tiles, 0);
    for (uint64_t w = 0; w < B.tiles; w++) {
        const uint64_t field = grib_bm_field_of_tile(B.b.data(), n, w);
        const GribField &F = B.d[field];
        const GribBitmap &bm = B.b[field];
        uint32_t ones[64];
        K kmin = ~(K)0, kmax = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const GribBmLane L = grib_bm_lane(w - bm.tile0, lane, bm.points);
            const uint32_t word = word_of(B, bitmap, bm, L);
            ones[lane] = grib_bm_count(word);
            if (!src) continue;
            for (uint32_t j = 0; j < kGribBmLane; j++) {
                T v;
                if (grib_bm_present(word, j) && value_at(B, src, F, bm, L.p0 + j, &v)) grib_minmax_take<T, K>(&v, 1u, &kmin, &kmax);
            }
        }
        wave_scan(ones);
        counts[w] = ones[63];
        if (!src || ones[63] == 0) continue;
        const uint64_t lo = grib_widen(kmin), hi = grib_widen(kmax);
        if (lo < extremes[2 * field]) extremes[2 * field] = lo;
        if (hi > extremes[2 * field + 1]) extremes[2 * field + 1] = hi;
    }
}

// k_grib_bm_scan: rounds of 64 tiles; returns the ones of every field
void scan(const Batch &B, uint64_t n, const std::vector<uint32_t> &counts, uint64_t *bases, std::vector<uint64_t> &total)
{
    total.assign(n, 0);
    for (uint64_t field = 0; field < n; field++) {
        const uint64_t tile0 = B.b[field].tile0, ntiles = B.b[field + 1].tile0 - tile0;
        uint64_t carry = 0;
        for (uint64_t t0 = 0; t0 < ntiles; t0 += 64) {
            uint32_t c[64], incl[64];
            for (uint32_t lane = 0; lane < 64; lane++) incl[lane] = c[lane] = t0 + lane < ntiles ? counts[tile0 + t0 + lane] : 0u;
            wave_scan(incl);
            for (uint32_t lane = 0; lane < 64; lane++)
                if (t0 + lane < ntiles) bases[tile0 + t0 + lane] = grib_bm_tile_base(carry, incl[lane], c[lane]);
            carry += incl[63];
        }
        total[field] = carry;
    }
}

void store_x(Batch &B, uint8_t *work, const GribField &F, uint32_t cont, uint64_t sample, uint32_t x)
{
    if ((sample + 1) * cont > F.room) B.outside++;
    else memcpy(work + F.work_off + sample * cont, &x, cont);            // (little-endian host)
}

template <typename T>
void quantise(Batch &B, uint64_t n, uint32_t nbits, const uint8_t *bitmap, const uint8_t *src, const uint64_t *bases, uint8_t *work,
              GribRecord *fields)
{
    const uint32_t cont = grib_container(nbits);
    for (uint64_t w = 0; w < B.tiles; w++) {
        const uint64_t field = grib_bm_field_of_tile(B.b.data(), n, w);
        const GribField &F = B.d[field];
        const GribBitmap &bm = B.b[field];
        const GribRecord rec = fields[field];
        const GribQuant q = grib_quant(rec, nbits, F.given.status != 0);
        uint32_t word[64], incl[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            word[lane] = word_of(B, bitmap, bm, grib_bm_lane(w - bm.tile0, lane, bm.points));
            incl[lane] = grib_bm_count(word[lane]);
        }
        wave_scan(incl);
        bool clamped = false;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const GribBmLane L = grib_bm_lane(w - bm.tile0, lane, bm.points);
            const uint64_t r0 = bases[w] + (incl[lane] - grib_bm_count(word[lane]));
            for (uint32_t j = 0; j < kGribBmLane; j++) {
                const uint64_t r = r0 + grib_bm_rank(word[lane], j);
                T v;
                if (!grib_bm_present(word[lane], j) || !grib_bm_kept(r, F.n) || !value_at(B, src, F, bm, L.p0 + j, &v)) continue;
                const uint32_t x = rec.D == 0 ? grib_quantise<0>((double)v, q, &clamped)
                                              : rec.D > 0 ? grib_quantise<1>((double)v, q, &clamped) : grib_quantise<-1>((double)v, q, &clamped);
                store_x(B, work, F, cont, r, x);
                if (grib_bm_pads(r, F.n))
                    for (uint64_t s = F.n; s < F.room / cont; s++) store_x(B, work, F, cont, s, x);
            }
        }
        if (!(rec.status & kGribBad) && clamped) fields[field].status |= kGribClamped;
    }
}

template <typename T>
void expand(Batch &B, uint64_t n, uint32_t nbits, const uint8_t *bitmap, const uint8_t *work, const uint64_t *bases, uint8_t *dst, T missing)
{
    const uint32_t cont = grib_container(nbits);
    for (uint64_t w = 0; w < B.tiles; w++) {
        const uint64_t field = grib_bm_field_of_tile(B.b.data(), n, w);
        const GribField &F = B.d[field];
        const GribBitmap &bm = B.b[field];
        const double R = (double)F.given.R, scale = grib_pow2(F.given.E), p = grib_pow10(F.given.D);
        uint32_t word[64], incl[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            word[lane] = word_of(B, bitmap, bm, grib_bm_lane(w - bm.tile0, lane, bm.points));
            incl[lane] = grib_bm_count(word[lane]);
        }
        wave_scan(incl);
        for (uint32_t lane = 0; lane < 64; lane++) {
            const GribBmLane L = grib_bm_lane(w - bm.tile0, lane, bm.points);
            const uint64_t r0 = bases[w] + (incl[lane] - grib_bm_count(word[lane]));
            for (uint32_t j = 0; j < L.valid; j++) {
                T y = missing;
                if (grib_bm_present(word[lane], j)) {
                    const uint64_t s = grib_bm_sample(r0 + grib_bm_rank(word[lane], j), F.n);
                    uint32_t x = 0;
                    if ((s + 1) * cont > F.room) B.outside++;
                    else memcpy(&x, work + F.work_off + s * cont, cont);
                    y = (T)(F.given.D == 0 ? grib_dequantise<0>(x, R, scale, p)
                                           : F.given.D > 0 ? grib_dequantise<1>(x, R, scale, p) : grib_dequantise<-1>(x, R, scale, p));
                }
                if (L.p0 + j >= bm.points) B.outside++;
                else memcpy(dst + F.off + (L.p0 + j) * sizeof(T), &y, sizeof(T));
            }
        }
    }
}

template <typename T>
void build(Batch &B, uint64_t n, const uint8_t *src, T missing, uint8_t *bitmap, uint64_t *ones_of_field)
{
    const bool is_nan = missing != missing;
    for (uint64_t w = 0; w < B.tiles; w++) {
        const uint64_t field = grib_bm_field_of_tile(B.b.data(), n, w);
        const GribField &F = B.d[field];
        const GribBitmap &bm = B.b[field];
        uint32_t ones[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            const GribBmLane L = grib_bm_lane(w - bm.tile0, lane, bm.points);
            uint32_t word = 0;
            for (uint32_t j = 0; j < L.valid; j++) {
                T v;
                if (value_at(B, src, F, bm, L.p0 + j, &v) && !grib_bm_is_missing(v, missing, is_nan)) word |= 1u << (15u - j);
            }
            for (uint32_t k = 0; k < L.nbytes; k++) {
                if (L.byte0 + k >= grib_bm_bytes(bm.points)) B.outside++;
                else bitmap[bm.bm_off + L.byte0 + k] = (uint8_t)grib_bm_byte(word, k);
            }
            ones[lane] = grib_bm_count(word);
        }
        wave_scan(ones);
        ones_of_field[field] += ones[63];
    }
}

}  // namespace

extern "C" uint32_t gribbm_emul_tile_points(void) { return kGribBmTile; }

extern "C" int64_t gribbm_emul_build(int elem, const uint8_t *src, const uint64_t *offsets, const uint64_t *n_points, double missing,
                                     uint64_t n, uint8_t *bitmap, const uint64_t *bm_offsets, uint64_t *counts)
{
    Batch B = describe(offsets, n_points, bm_offsets, nullptr, nullptr, nullptr, 0, nullptr, n, 8, 8);
    for (uint64_t i = 0; i < n; i++) counts[i] = 0;
    if (elem == 4) build<float>(B, n, src, (float)missing, bitmap, counts);
    else build<double>(B, n, src, missing, bitmap, counts);
    return B.outside;
}

// tmpl = {nbits, options, block size, rsi}.  bases receives the base of every tile, fields the records.
extern "C" int64_t gribbm_emul_pack(const uint32_t *tmpl, int elem, const uint8_t *src, const uint64_t *offsets, const uint64_t *n_points,
                                    const uint64_t *n_values, const uint64_t *work_offsets, const int32_t *D, int have,
                                    const GribRecord *params, uint64_t n, const uint8_t *bitmap, const uint64_t *bm_offsets, uint8_t *work,
                                    GribRecord *fields, uint64_t *bases)
{
    Batch B = describe(offsets, n_points, bm_offsets, n_values, work_offsets, D, have, params, n, tmpl[2], tmpl[0]);
    std::vector<uint64_t> extremes(2 * n), total;
    std::vector<uint32_t> counts;
    for (uint64_t i = 0; i < n; i++) {
        extremes[2 * i] = ~0ull;
        extremes[2 * i + 1] = 0;
    }
    if (elem == 4) minmax<float, uint32_t>(B, n, bitmap, src, extremes.data(), counts);
    else minmax<double, uint64_t>(B, n, bitmap, src, extremes.data(), counts);
    scan(B, n, counts, bases, total);
    for (uint64_t i = 0; i < n; i++) {
        const GribRecord g = B.d[i].given;
        fields[i] = grib_params(extremes[2 * i], extremes[2 * i + 1], g.D, tmpl[0], g.status != 0, g.R, g.E);
        fields[i].status |= grib_bm_mismatch(total[i], B.d[i].n);
    }
    if (elem == 4) quantise<float>(B, n, tmpl[0], bitmap, src, bases, work, fields);
    else quantise<double>(B, n, tmpl[0], bitmap, src, bases, work, fields);
    return B.outside;
}

extern "C" int64_t gribbm_emul_unpack(const uint32_t *tmpl, int elem, const uint8_t *work, const uint64_t *work_offsets,
                                      const uint64_t *n_points, const uint64_t *n_values, const GribRecord *params,
                                      const uint64_t *dst_offsets, uint64_t n, const uint8_t *bitmap, const uint64_t *bm_offsets,
                                      double missing, uint8_t *dst, uint32_t *status, uint64_t *bases)
{
    Batch B = describe(dst_offsets, n_points, bm_offsets, n_values, work_offsets, nullptr, 1, params, n, tmpl[2], tmpl[0]);
    std::vector<uint64_t> total;
    std::vector<uint32_t> counts;
    minmax<float, uint32_t>(B, n, bitmap, nullptr, nullptr, counts);
    scan(B, n, counts, bases, total);
    for (uint64_t i = 0; i < n; i++) status[i] = grib_bm_mismatch(total[i], B.d[i].n);
    if (elem == 4) expand<float>(B, n, tmpl[0], bitmap, work, bases, dst, (float)missing);
    else expand<double>(B, n, tmpl[0], bitmap, work, bases, dst, missing);
    return B.outside;
}
