// grib_emul.cpp -- host harness for libaec_amd/csrc/aec_grib.h: what k_grib_minmax does wavefront by wavefront and lane by
// lane (the table of one field per wavefront, the groups of a lane's four steps, the keys, the reduction into the field's
// two extremes), k_grib_params field by field and k_grib_quantise / k_grib_dequantise group by group (libaec_amd/csrc/
// aec_grib.hip), through the same functions and the same descriptors.  Built by tests/test_grib_emul.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../libaec_amd/csrc/aec_grib.h"

using namespace aec;

// the descriptors as send_fields writes them (n + 1 entries), the wavefronts of the two launches in w
static std::vector<GribField> describe(const uint64_t *offsets, const uint64_t *n_values, const uint64_t *work_offsets,
                                       const int32_t *D, int have, const GribRecord *params, uint64_t n, uint32_t bs, uint32_t nbits,
                                       int elem, bool minmax, uint64_t w[2])
{
    std::vector<GribField> d(n + 1);
    w[0] = w[1] = 0;
    for (uint64_t i = 0; i <= n; i++) {
        GribField &f = d[i];
        f = GribField{};
        f.wave0[0] = w[0];
        f.wave0[1] = w[1];
        if (i == n) break;
        f.off = offsets[i];
        f.n = n_values[i];
        f.work_off = work_offsets[i];
        f.room = grib_room(f.n, bs, grib_container(nbits));
        f.given.D = D ? D[i] : params[i].D;
        if (have) {
            f.given.R = params[i].R;
            f.given.E = params[i].E;
            f.given.status = 1;
        }
        if (minmax) w[0] += grib_minmax_waves(f.n, (uint32_t)elem);
        w[1] += grib_room_waves(f.room);
    }
    return d;
}

template <typename T, typename K>
static void minmax(const std::vector<GribField> &d, uint64_t n, uint64_t waves, const uint8_t *src, uint64_t *extremes)
{
    const uint32_t per = 16u / sizeof(T);
    for (uint64_t w = 0; w < waves; w++) {
        const uint64_t field = grib_field_of_wave(d.data(), n, 0, w);
        const GribField &F = d[field];
        K lane_min[64], lane_max[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            K kmin = ~(K)0, kmax = 0;
            for (uint32_t s = 0; s < 4; s++) {
                uint64_t first;
                uint32_t count;
                grib_minmax_group<T>(w - F.wave0[0], s, lane, F.n, &first, &count);
                T v[per];
                if (count) memcpy(v, src + F.off + first * sizeof(T), count * sizeof(T));
                grib_minmax_take<T, K>(v, count, &kmin, &kmax);
            }
            lane_min[lane] = kmin;
            lane_max[lane] = kmax;
        }
        for (int off = 32; off > 0; off >>= 1)                       // the butterfly of the wave reduction
            for (int lane = 0; lane < 64; lane++) {
                const K a = lane_min[lane ^ off], b = lane_max[lane ^ off];
                if (lane < (lane ^ off)) {
                    lane_min[lane] = lane_min[lane ^ off] = a < lane_min[lane] ? a : lane_min[lane];
                    lane_max[lane] = lane_max[lane ^ off] = b > lane_max[lane] ? b : lane_max[lane];
                }
            }
        const uint64_t lo = grib_widen(lane_min[0]), hi = grib_widen(lane_max[0]);
        if (lo < extremes[2 * field]) extremes[2 * field] = lo;
        if (hi > extremes[2 * field + 1]) extremes[2 * field + 1] = hi;
    }
}

template <typename T>
static void quantise(const std::vector<GribField> &d, uint64_t n, uint64_t waves, uint32_t nbits, const uint8_t *src, uint8_t *work,
                     GribRecord *fields)
{
    const uint32_t cont = grib_container(nbits), per = 16u / cont;
    for (uint64_t w = 0; w < waves; w++) {
        const uint64_t field = grib_field_of_wave(d.data(), n, 1, w);
        const GribField &F = d[field];
        const GribRecord rec = fields[field];
        const bool have = F.given.status != 0;
        const GribQuant q = grib_quant(rec, nbits, have);
        bool clamped = false;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t g = (w - F.wave0[1]) * 64u + lane, lo = g * 16u;
            if (lo >= F.room) continue;
            uint8_t out[16] = {0};
            for (uint32_t i = 0; i < per; i++) {
                T v;
                memcpy(&v, src + F.off + grib_value_of_sample(g * per + i, F.n) * sizeof(T), sizeof(T));
                const uint32_t x = rec.D == 0 ? grib_quantise<0>((double)v, q, &clamped)
                                              : rec.D > 0 ? grib_quantise<1>((double)v, q, &clamped) : grib_quantise<-1>((double)v, q, &clamped);
                memcpy(out + i * cont, &x, cont);                    // (little-endian host)
            }
            for (uint32_t i = 0; i < 16; i++)
                if (lo + i < F.room) work[F.work_off + lo + i] = out[i];
        }
        if (!(rec.status & kGribBad) && clamped) fields[field].status |= kGribClamped;
    }
}

template <typename T>
static void dequantise(const std::vector<GribField> &d, uint64_t n, uint64_t waves, uint32_t nbits, const uint8_t *work, uint8_t *dst)
{
    const uint32_t cont = grib_container(nbits), per = 16u / cont;
    for (uint64_t w = 0; w < waves; w++) {
        const uint64_t field = grib_field_of_wave(d.data(), n, 1, w);
        const GribField &F = d[field];
        const double R = (double)F.given.R, scale = grib_pow2(F.given.E), p = grib_pow10(F.given.D);
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t g = (w - F.wave0[1]) * 64u + lane, j0 = g * per;
            for (uint32_t i = 0; i < per && j0 + i < F.n; i++) {
                uint32_t x = 0;
                memcpy(&x, work + F.work_off + g * 16u + i * cont, cont);
                const T y = (T)(F.given.D == 0 ? grib_dequantise<0>(x, R, scale, p)
                                               : F.given.D > 0 ? grib_dequantise<1>(x, R, scale, p) : grib_dequantise<-1>(x, R, scale, p));
                memcpy(dst + F.off + (j0 + i) * sizeof(T), &y, sizeof(T));
            }
        }
    }
}

// tmpl = {nbits, options, block size, rsi}.  extremes (2 per field) receives the keys of the raw minimum and maximum.
extern "C" int grib_emul_pack(const uint32_t *tmpl, int elem, const uint8_t *src, const uint64_t *offsets, const uint64_t *n_values,
                              const uint64_t *work_offsets, const int32_t *D, int have, const GribRecord *params, uint64_t n,
                              uint8_t *work, GribRecord *fields, uint64_t *extremes)
{
    uint64_t w[2];
    const std::vector<GribField> d = describe(offsets, n_values, work_offsets, D, have, params, n, tmpl[2], tmpl[0], elem, true, w);
    for (uint64_t i = 0; i < n; i++) {
        extremes[2 * i] = ~0ull;
        extremes[2 * i + 1] = 0;
    }
    if (elem == 4) minmax<float, uint32_t>(d, n, w[0], src, extremes);
    else minmax<double, uint64_t>(d, n, w[0], src, extremes);
    for (uint64_t i = 0; i < n; i++) {
        const GribRecord g = d[i].given;
        fields[i] = grib_params(extremes[2 * i], extremes[2 * i + 1], g.D, tmpl[0], g.status != 0, g.R, g.E);
    }
    if (elem == 4) quantise<float>(d, n, w[1], tmpl[0], src, work, fields);
    else quantise<double>(d, n, w[1], tmpl[0], src, work, fields);
    return 0;
}

extern "C" int grib_emul_unpack(const uint32_t *tmpl, int elem, const uint8_t *work, const uint64_t *work_offsets,
                                const uint64_t *n_values, const GribRecord *params, const uint64_t *dst_offsets, uint64_t n,
                                uint8_t *dst)
{
    uint64_t w[2];
    const std::vector<GribField> d = describe(dst_offsets, n_values, work_offsets, nullptr, 1, params, n, tmpl[2], tmpl[0], elem, false, w);
    if (elem == 4) dequantise<float>(d, n, w[1], tmpl[0], work, dst);
    else dequantise<double>(d, n, w[1], tmpl[0], work, dst);
    return 0;
}

// the key mapping alone: keys of n doubles / floats, and back
extern "C" void grib_emul_keys(const double *v, uint64_t n, uint64_t *k64, double *back, uint32_t *k32, uint64_t *widened)
{
    for (uint64_t i = 0; i < n; i++) {
        k64[i] = grib_key(v[i]);
        back[i] = grib_unkey(k64[i]);
        k32[i] = grib_key((float)v[i]);
        widened[i] = grib_widen(k32[i]);
    }
}
