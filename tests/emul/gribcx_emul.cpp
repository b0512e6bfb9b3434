// gribcx_emul.cpp -- host harness for libaec_amd/csrc/aec_gribcx.h: what the seven kernels of libaec_amd/csrc/aec_gribcx.hip
// do, launch by launch, wavefront by wavefront and lane by lane, through the same functions, the same descriptors and the same
// tables (a wavefront's shuffles are loops over its lanes here).  Every load of a stream goes through a checked policy: one
// outside the field's complex_bytes_each bytes is skipped and counted, and the count is what the call returns (0 = none).
// Every store into the work buffer is counted per byte, so the caller sees one that missed a room, or a byte stored twice.
// Built by tests/test_grib_complex_emul.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../libaec_amd/csrc/aec_gribcx.h"

using namespace aec;

namespace {

struct Mem {
    const uint8_t *p;
    int64_t size;
    int64_t *outside;
    uint32_t ld8(int64_t o) const
    {
        if (o < 0 || o >= size) {
            ++*outside;
            return 0;
        }
        return p[o];
    }
};

struct Batch {
    std::vector<CxField> d;
    std::vector<CxDyn> dyn;
    std::vector<CxSum> gagg;
    std::vector<uint64_t> gval, gbit;
    std::vector<uint32_t> gref, gwid;
    std::vector<CxAgg> vagg;
    std::vector<int64_t> vmin, vmax;
    uint64_t vtiles = 0, gtiles = 0;
    int64_t outside = 0;
};

// (what cx_expand of aec_gribcx.hip writes)
Batch describe(const uint32_t *tmpl, const uint64_t *n_values, const uint32_t *descs, const uint64_t *offsets, const uint64_t *each,
               const uint64_t *work_offsets, uint64_t n)
{
    Batch B;
    B.d.assign(n + 1, CxField{});
    uint64_t vt = 0, gt = 0, g0 = 0;
    for (uint64_t i = 0; i <= n; i++) {
        CxField &f = B.d[i];
        f.vtile0 = vt;
        f.gtile0 = gt;
        f.group0 = g0;
        if (i == n) break;
        const uint32_t *c = descs + 11 * i;       // the members of aec_gpu_grib_complex_field in their order
        f.off = offsets[i];
        f.bytes = each[i];
        f.n = n_values[i];
        f.work_off = work_offsets[i];
        f.room = grib_room(n_values[i], tmpl[2], grib_container(tmpl[0]));
        f.ref_bits = c[0];
        f.ng = c[1];
        f.width_ref = c[2];
        f.width_bits = c[3];
        f.length_ref = c[4];
        f.length_inc = c[5];
        f.last_length = c[6];
        f.length_bits = c[7];
        f.order = c[8];
        f.extra = c[8] ? c[9] : 0u;
        f.refs_bit = 8u * (c[8] ? (uint64_t)(c[8] + 1u) * c[9] : 0u);
        f.widths_bit = f.refs_bit + 8u * cx_table_bytes(f.ng, f.ref_bits);
        f.lengths_bit = f.widths_bit + 8u * cx_table_bytes(f.ng, f.width_bits);
        f.data_bit = f.lengths_bit + 8u * cx_table_bytes(f.ng, f.length_bits);
        vt += grib_room_waves(f.room);
        gt += (f.ng + kCxGroupTile - 1) / kCxGroupTile;
        g0 += f.ng;
    }
    B.vtiles = vt;
    B.gtiles = gt;
    B.dyn.assign(n, CxDyn{});
    B.gagg.assign(gt, CxSum{0, 0});
    B.gval.assign(g0, 0);
    B.gbit.assign(g0, 0);
    B.gref.assign(g0, 0);
    B.gwid.assign(g0, 0);
    B.vagg.assign(vt, CxAgg{0, 0});
    B.vmin.assign(vt, 0);
    B.vmax.assign(vt, 0);
    return B;
}

void groups(Batch &B, uint64_t n, const uint8_t *complex)
{
    for (uint64_t w = 0; w < B.gtiles; w++) {                               // k_cx_groups
        const CxField &F = B.d[cx_field_of_tile(B.d.data(), n, 0, w)];
        Mem m{complex + F.off, (int64_t)F.bytes, &B.outside};
        CxSum run{0, 0};
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t g = (w - F.gtile0) * kCxGroupTile + lane;
            if (g >= F.ng) continue;
            const CxGroup G = cx_group(m, F, g);
            B.gval[F.group0 + g] = run.v;
            B.gbit[F.group0 + g] = run.b;
            B.gref[F.group0 + g] = G.ref;
            B.gwid[F.group0 + g] = G.width;
            run = cx_sum_add(run, G.s, cx_cap_values(F), cx_cap_bits(F));
        }
        B.gagg[w] = run;
    }
    for (uint64_t f = 0; f < n; f++) {                                      // k_cx_group_scan
        const CxField &F = B.d[f];
        CxSum carry{0, 0};
        for (uint64_t t = F.gtile0; t < B.d[f + 1].gtile0; t++) {
            const CxSum total = B.gagg[t];
            B.gagg[t] = carry;
            carry = cx_sum_add(carry, total, cx_cap_values(F), cx_cap_bits(F));
        }
        Mem m{complex + F.off, (int64_t)F.bytes, &B.outside};
        B.dyn[f] = cx_dyn(m, F, carry);
    }
    for (uint64_t w = 0; w < B.gtiles; w++) {                               // k_cx_group_apply
        const CxField &F = B.d[cx_field_of_tile(B.d.data(), n, 0, w)];
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t g = (w - F.gtile0) * kCxGroupTile + lane;
            if (g >= F.ng) continue;
            const CxSum at = cx_sum_add(B.gagg[w], CxSum{B.gval[F.group0 + g], B.gbit[F.group0 + g]}, cx_cap_values(F), cx_cap_bits(F));
            B.gval[F.group0 + g] = at.v;
            B.gbit[F.group0 + g] = at.b;
        }
    }
}

CxTables tables_of(const Batch &B, const CxField &F)
{
    return CxTables{B.gval.data() + F.group0, B.gbit.data() + F.group0, B.gref.data() + F.group0, B.gwid.data() + F.group0};
}

template <int CONT>
void values(Batch &B, uint64_t n, uint32_t nbits, const uint8_t *complex, uint8_t *work, uint32_t *stores)
{
    constexpr uint32_t per = 16u / CONT;
    constexpr uint64_t T = kGribWaveRoom / CONT;
    for (uint64_t w = 0; w < B.vtiles; w++) {                               // k_cx_values
        const uint64_t f = cx_field_of_tile(B.d.data(), n, 1, w);
        const CxField &F = B.d[f];
        if (F.order == 0u) continue;
        Mem m{complex + F.off, (int64_t)F.bytes, &B.outside};
        CxAgg run{0, 0};
        for (uint32_t lane = 0; lane < 64; lane++) {
            const GribBitsLane L = grib_bits_lane(w - F.vtile0, lane, per, F.n, 0, 0);
            uint64_t d[per];
            cx_lane_values<(int)per>(m, F, B.dyn[f], tables_of(B, F), L.j0, L.cnt, d);
            run = cx_combine(run, cx_lane_agg<(int)per>(d), per);
        }
        B.vagg[w] = run;
    }
    for (uint64_t f = 0; f < n; f++) {                                      // k_cx_value_scan
        const CxField &F = B.d[f];
        if (F.order == 0u) continue;
        CxAgg carry{0, 0};
        uint64_t covered = 0;
        for (uint64_t t = F.vtile0; t < B.d[f + 1].vtile0; t++) {
            const CxAgg total = B.vagg[t];
            B.vagg[t] = carry;
            carry = cx_combine(carry, total, T);
            covered += T;
        }
        B.dyn[f].xlast = cx_last_x(carry, F.order, covered, F.n);
    }
    for (uint64_t w = 0; w < B.vtiles; w++) {                               // k_cx_apply
        const uint64_t f = cx_field_of_tile(B.d.data(), n, 1, w);
        const CxField &F = B.d[f];
        const CxDyn &Y = B.dyn[f];
        const CxTables Tb = tables_of(B, F);
        Mem m{complex + F.off, (int64_t)F.bytes, &B.outside};
        const uint64_t in_field = w - F.vtile0;
        CxAgg run{0, 0};
        CxExt e = cx_ext_none();
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t at = (in_field * 64u + lane) * 16u;
            const GribBitsLane L = grib_bits_lane(in_field, lane, per, F.n, 0, 0);
            uint64_t d[per];
            cx_lane_values<(int)per>(m, F, Y, Tb, L.j0, L.cnt, d);
            const CxAgg own = cx_lane_agg<(int)per>(d);
            CxAgg in{0, 0};
            if (F.order) in = cx_combine(B.vagg[w], run, (uint64_t)lane * per);
            run = cx_combine(run, own, per);
            cx_lane_x<(int)per>(d, F.order, in);
            uint64_t last = Y.xlast;
            if (F.order == 0u && L.cnt < per && at < F.room) {
                uint64_t one[1];
                cx_lane_values<1>(m, F, Y, Tb, F.n - 1u, 1u, one);
                last = one[0];
            }
            uint32_t words[4];
            cx_lane_words<CONT>(d, L.cnt, last, nbits, &e, words);
            for (uint32_t i = 0; i < 16; i++) {
                if (at + i >= F.room) continue;
                work[F.work_off + at + i] = (uint8_t)(words[i >> 2] >> (8 * (i & 3)));
                stores[F.work_off + at + i]++;
            }
        }
        B.vmin[w] = e.lo;
        B.vmax[w] = e.hi;
    }
}

}  // namespace

extern "C" uint32_t gribcx_emul_group_tile(void) { return kCxGroupTile; }

// tmpl = {nbits, options, block size, rsi}; descs: 11 uint32_t per field, the members of aec_gpu_grib_complex_field in their
// order; stores: an entry per byte of work; cx: per field x_min, x_max, status.  Returns the accesses that were out of place.
extern "C" int64_t gribcx_emul_expand(const uint32_t *tmpl, const uint64_t *n_values, const uint32_t *descs, uint64_t n, const uint8_t *complex,
                                      const uint64_t *offsets, const uint64_t *each, uint8_t *work, const uint64_t *work_offsets, uint32_t *stores,
                                      int64_t *cx)
{
    Batch B = describe(tmpl, n_values, descs, offsets, each, work_offsets, n);
    groups(B, n, complex);
    const uint32_t cont = grib_container(tmpl[0]);
    if (cont == 1) values<1>(B, n, tmpl[0], complex, work, stores);
    else if (cont == 2) values<2>(B, n, tmpl[0], complex, work, stores);
    else values<4>(B, n, tmpl[0], complex, work, stores);
    for (uint64_t f = 0; f < n; f++) {                                      // k_cx_records
        CxExt e = cx_ext_none();
        for (uint64_t t = B.d[f].vtile0; t < B.d[f + 1].vtile0; t++) e = cx_ext_join(e, CxExt{B.vmin[t], B.vmax[t]});
        cx[3 * f] = e.lo;
        cx[3 * f + 1] = e.hi;
        cx[3 * f + 2] = cx_status(B.dyn[f], e, tmpl[0]);
    }
    return B.outside;
}
