// aec_grib.h -- GRIB2 simple packing around the CCSDS coder (include/aec_gpu_grib.h): the per-lane arithmetic of
// aec_grib.hip and the host arithmetic of its plan.  WMO regulation 92.9.4:  Y * 10^D = R + X * 2^E.
//
// Every quantisation step is ONE correctly rounded IEEE double operation.  hipcc contracts a * b - c into an FMA in
// device code by default (-ffp-contract=fast-honor-pragmas), an FMA rounds once where the contract rounds twice, and HIP's
// __dmul_rn / __dsub_rn are plain operators that fuse just the same after inlining; so every function that does
// arithmetic opens with GRIB_NO_CONTRACT (#pragma clang fp contract(off): its operations do not carry the flag the
// backend needs to fuse them, wherever they are inlined).  g++ for x86-64 has no FMA to contract into unless told
// -mfma; tests/test_grib_emul.py builds with -ffp-contract=off all the same.
// Nothing here calls frexp / ldexp / nextafter: powers of two are built from their bits and a multiplication by one is
// exact, so that g++ and hipcc cannot differ in a library routine either.
// The functions are __host__ __device__: the kernels call them and tests/emul/grib_emul.cpp runs the same functions on
// the CPU, lane by lane.
#pragma once
#include <stdint.h>
#include <string.h>

#include "aec_lane.h"

#if defined(__clang__)
#define GRIB_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GRIB_NO_CONTRACT
#endif

namespace aec {

enum { kGribBad = 1u, kGribConstant = 2u, kGribClamped = 4u };   // status bits of a field record
constexpr int kGribMaxD = 22;                                    // 10^22 is the last power of ten exact in a double
constexpr uint32_t kGribSpan = 4096;     // source bytes a wavefront of k_grib_minmax reduces: 4 loads of 16 bytes a lane
constexpr uint32_t kGribWaveRoom = 1024; // bytes of a field's room a wavefront of k_grib_(de)quantise owns: 16 a lane

// the per-field record on the device (aec_gpu_grib_field)
struct GribRecord {
    float R;
    int32_t E, D;
    uint32_t status;
};

// Descriptor of field i (host-written, n + 1 of them: entry n holds the totals in wave0).
struct GribField {
    uint64_t off;        // byte offset of its values from the call's d_src / d_dst
    uint64_t n;          // values
    uint64_t work_off;   // its room in d_work (a multiple of 16)
    uint64_t room;       // bytes of the room the coder sees: blocks * block_size * container
    uint64_t wave0[2];   // its first wavefront of k_grib_minmax | of k_grib_quantise / k_grib_dequantise
    GribRecord given;    // D; with have_params (status != 0 here) the caller's R and E
};

AEC_HD double grib_pow10(int a)
{
    const double t[kGribMaxD + 1] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                     1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    return t[a < 0 ? -a : a];
}

AEC_HD uint64_t grib_bits(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}
AEC_HD double grib_double(uint64_t b)
{
    double v;
    memcpy(&v, &b, 8);
    return v;
}
AEC_HD uint32_t grib_bits32(float v)
{
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}
AEC_HD float grib_float(uint32_t b)
{
    float v;
    memcpy(&v, &b, 4);
    return v;
}

// 2^e, -1022 <= e <= 1023
AEC_HD double grib_pow2(int e) { return grib_double((uint64_t)(e + 1023) << 52); }

// Order-preserving integer keys: a < b as numbers <=> key(a) < key(b) as unsigned integers, with -0.0 just below +0.0,
// NaNs with the sign bit below -inf and NaNs without it above +inf.  Integer min / max commute, so a reduction over
// keys gives the same bits in whatever order its atomics arrive; a NaN anywhere in a field surfaces as a non-finite
// minimum or maximum.
AEC_HD uint64_t grib_key(double v)
{
    const uint64_t b = grib_bits(v);
    return (b >> 63) ? ~b : b | (1ull << 63);
}
AEC_HD double grib_unkey(uint64_t k) { return grib_double((k >> 63) ? k & ~(1ull << 63) : ~k); }
AEC_HD uint32_t grib_key(float v)
{
    const uint32_t b = grib_bits32(v);
    return (b >> 31) ? ~b : b | (1u << 31);
}
AEC_HD float grib_unkey(uint32_t k) { return grib_float((k >> 31) ? k & ~(1u << 31) : ~k); }
// (float -> double is exact and monotone: a field of floats is reduced over 32-bit keys and only the two winners are
// widened)
AEC_HD uint64_t grib_widen(uint64_t k) { return k; }
AEC_HD uint64_t grib_widen(uint32_t k) { return grib_key((double)grib_unkey(k)); }

// s(y): the value in units of 10^-D
template <int DSIGN>
AEC_HD double grib_scale(double y, double p)
{
    GRIB_NO_CONTRACT
    if (DSIGN > 0) return y * p;
    if (DSIGN < 0) return y / p;
    return y;
}
AEC_HD double grib_scale_any(double y, int D)
{
    const double p = grib_pow10(D);
    return D > 0 ? grib_scale<1>(y, p) : D < 0 ? grib_scale<-1>(y, p) : grib_scale<0>(y, p);
}

// the largest float <= v, |v| <= FLT_MAX (what __double2float_rd gives): the nearest float, one step down where that
// lies above v
AEC_HD float grib_float_below(double v)
{
    const float f = (float)v;
    if ((double)f <= v) return f;
    const uint32_t b = grib_bits32(f);
    if ((b & 0x7FFFFFFFu) == 0) return grib_float(0x80000001u);     // below zero: the smallest negative float
    return grib_float((b >> 31) ? b + 1u : b - 1u);
}

// The parameters of a field from its extremes (keys of the RAW minimum and maximum) and its D; with have, the caller's R
// and E are kept and only the status is found.
AEC_HD GribRecord grib_params(uint64_t kmin, uint64_t kmax, int D, uint32_t nbits, bool have, float R, int32_t E)
{
    GRIB_NO_CONTRACT
    GribRecord r;
    r.R = have ? R : 0.0f;
    r.E = have ? E : 0;
    r.D = D;
    r.status = 0;
    double lo = grib_scale_any(grib_unkey(kmin), D), hi = grib_scale_any(grib_unkey(kmax), D);
    const double flt_max = 3.4028234663852886e38;
    // (written so that a NaN fails the test)
    if (!(lo >= -flt_max && lo <= flt_max && hi >= -flt_max && hi <= flt_max)) {
        r.status = kGribBad;
        return r;
    }
    if (lo == 0.0) lo = 0.0;            // -0.0 -> +0.0: R's bits do not depend on which zero the reduction met
    if (hi == 0.0) hi = 0.0;
    if (lo == hi) r.status |= kGribConstant;
    if (have) return r;
    r.R = grib_float_below(lo);
    if (r.status & kGribConstant) return r;     // E = 0, every X is 0
    const double range = hi - (double)r.R;
    // range = m * 2^e, 0.5 <= m < 1: E = e - nbits puts range * 2^-E into [2^(nbits-1), 2^nbits), one more where that
    // is above M = 2^nbits - 1 (M is exact in a double; one less is never enough).  A subnormal range is below every
    // 2^-127 * M there is.
    const uint64_t b = grib_bits(range);
    const int ex = (int)((b >> 52) & 0x7FFu);
    int e = -127;
    if (ex != 0) {
        const double m = grib_double((b & ~(0x7FFull << 52)) | (1022ull << 52));
        const double M = grib_pow2((int)nbits) - 1.0;
        e = ex - 1022 - (int)nbits + ((m * grib_pow2((int)nbits) > M) ? 1 : 0);
    }
    r.E = e < -127 ? -127 : e > 127 ? 127 : e;       // (held at 127, range * 2^-E exceeds M: the quantiser holds X and says so)
    return r;
}

// what a lane of k_grib_quantise knows of its field
struct GribQuant {
    double R, scale, p, M;       // (double)R, 2^-E, 10^|D|, 2^nbits - 1
    bool zero;                   // a constant field: every X is 0
};
AEC_HD GribQuant grib_quant(const GribRecord &r, uint32_t nbits, bool have)
{
    GRIB_NO_CONTRACT
    GribQuant q;
    q.R = (double)r.R;
    q.scale = grib_pow2(-r.E);
    q.p = grib_pow10(r.D);
    q.M = grib_pow2((int)nbits) - 1.0;
    q.zero = (r.status & kGribConstant) && !have;
    return q;
}

// X of one value: trunc((s(y) - R) * 2^-E + 0.5), ties up.  Held to [0, M]; *clamped is set where that changed it.  For
// the parameters grib_params finds it changes nothing unless E had to be held at 127 (a range beyond 2^127 * M).
template <int DSIGN>
AEC_HD uint32_t grib_quantise(double y, const GribQuant &q, bool *clamped)
{
    GRIB_NO_CONTRACT
    if (q.zero) return 0u;
    const double d = grib_scale<DSIGN>(y, q.p) - q.R;
    const double t = d * q.scale;               // exact: a power of two
    double u = t + 0.5;
    if (!(u >= 0.0)) {                          // (a NaN too: the field's record says so)
        *clamped |= !(u > -1.0);                // trunc of (-1, 0) is 0 all the same
        u = 0.0;
    }
    if (u >= q.M + 1.0) {
        *clamped = true;
        u = q.M;
    }
    return (uint32_t)u;                         // trunc
}

// Y of one X: (X * 2^E + R) in units of 10^-D, then one rounding to the element type by the caller
template <int DSIGN>
AEC_HD double grib_dequantise(uint32_t x, double R, double scale, double p)
{
    GRIB_NO_CONTRACT
    const double v = (double)x * scale + R;     // the product is exact
    if (DSIGN > 0) return v / p;
    if (DSIGN < 0) return v * p;
    return v;
}

// ---- host arithmetic of the layout and the plan --------------------------------------------------------------------------
AEC_HD uint32_t grib_container(uint32_t nbits) { return nbits <= 8 ? 1u : nbits <= 16 ? 2u : 4u; }

// the coder's flags from the template's compression-options octet: preprocessing, the restricted code set and RSI padding
// pass through, AEC_NOT_ENFORCE is added (as the SZIP layer adds it); AEC_DATA_MSB and AEC_DATA_3BYTE say how samples
// lie in memory and never change a stream -- here they lie little-endian in containers of 1, 2 or 4 bytes
AEC_HD uint32_t grib_flags(uint32_t octet) { return (octet & (uint32_t)(F_PREPROCESS | F_RESTRICTED | F_PAD_RSI)) | (uint32_t)F_NOT_ENFORCE; }

// bytes of the room of a field of n values: its whole blocks
AEC_HD uint64_t grib_room(uint64_t n, uint32_t bs, uint32_t container) { return (n + bs - 1) / bs * bs * container; }

AEC_HD uint64_t grib_minmax_waves(uint64_t n, uint32_t elem) { return (n * elem + kGribSpan - 1) / kGribSpan; }
AEC_HD uint64_t grib_room_waves(uint64_t room) { return (room + kGribWaveRoom - 1) / kGribWaveRoom; }

// the field that owns wavefront w of launch `which`: the LAST field whose first wavefront is <= w (fields without a
// wavefront share the next one's).  w must be below d[n].wave0[which].
AEC_HD uint64_t grib_field_of_wave(const GribField *d, uint64_t n, int which, uint64_t w)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (d[mid].wave0[which] <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The elements a lane of k_grib_minmax reduces in one of its four steps: group g = step * 64 + lane of the wavefront's
// span, 16 bytes of the field.  first >= n: nothing.
template <typename T>
AEC_HD void grib_minmax_group(uint64_t wave_in_field, uint32_t step, uint32_t lane, uint64_t n, uint64_t *first, uint32_t *count)
{
    const uint32_t per = 16u / (uint32_t)sizeof(T);
    *first = wave_in_field * (kGribSpan / sizeof(T)) + (uint64_t)(step * 64u + lane) * per;
    *count = *first >= n ? 0u : (n - *first < per ? (uint32_t)(n - *first) : per);
}

// A lane's reduction over elements v[0 .. count) into its running keys
template <typename T, typename K>
AEC_HD void grib_minmax_take(const T *v, uint32_t count, K *kmin, K *kmax)
{
    for (uint32_t i = 0; i < count; i++) {
        const K k = grib_key(v[i]);
        *kmin = k < *kmin ? k : *kmin;
        *kmax = k > *kmax ? k : *kmax;
    }
}

// Sample j of a field's room is value min(j, n - 1): the last block is padded with the last X, as the encoder pads a
// short block by repeating its last sample.
AEC_HD uint64_t grib_value_of_sample(uint64_t j, uint64_t n) { return j < n ? j : n - 1; }

}  // namespace aec
