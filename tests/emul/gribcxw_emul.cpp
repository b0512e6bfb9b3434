// gribcxw_emul.cpp -- host harness for libaec_amd/csrc/aec_gribcxw.h: what the six kernels of libaec_amd/csrc/aec_gribcxw.hip
// do, launch by launch, wavefront by wavefront and lane by lane, through the same functions, the same descriptors and the same
// tables (a wavefront's shuffles, butterflies and scans are loops over its lanes here).  Every load of a room and every store
// into the stream buffer goes through a checked policy: a load outside the n values of the field's room, a misaligned load, a
// store outside the field's own range [offset, offset + B), or a word store whose address is no multiple of 4 is skipped and
// counted, and the count is what the call returns (0 = none).  Every store is counted per byte, so the caller sees a byte stored
// twice or not at all.  Built by tests/test_grib_complex_write_emul.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../libaec_amd/csrc/aec_gribcxw.h"

using namespace aec;

namespace {

struct Mem {
    const uint8_t *room;
    int64_t room_bytes;          // n * container: the values, not the padding of the last block
    uint8_t *out;
    int64_t lo, hi;              // the field's range of the stream buffer
    uint32_t mis;                // the buffer's address modulo 4
    uint32_t *stores;
    int64_t *outside;
    uint32_t ldx(int64_t o, uint32_t cont) const
    {
        if (o < 0 || o + (int64_t)cont > room_bytes || o % cont) {
            ++*outside;
            return 0;
        }
        uint32_t v = 0;
        memcpy(&v, room + o, cont);
        return v;
    }
    void ld128(int64_t o, uint32_t (&w)[4]) const
    {
        if (o < 0 || o + 16 > room_bytes || o % 16) {
            ++*outside;
            w[0] = w[1] = w[2] = w[3] = 0;
            return;
        }
        memcpy(w, room + o, 16);
    }
    void st8(int64_t o, uint8_t v) const
    {
        if (o < lo || o >= hi) {
            ++*outside;
            return;
        }
        out[o] = v;
        stores[o]++;
    }
    void st32(int64_t o, uint32_t v) const
    {
        if (o < lo || o + 4 > hi || (o + mis) % 4) {
            ++*outside;
            return;
        }
        memcpy(out + o, &v, 4);
        for (int b = 0; b < 4; b++) stores[o + b]++;
    }
};

struct Batch {
    CxwShape P;
    std::vector<CxwField> d;
    std::vector<uint64_t> bound;
    std::vector<CxwDyn> dyn;
    std::vector<int64_t> minsd, tmin;
    std::vector<CxwTile> tile;
    std::vector<uint32_t> gref, gwid, gbit;
    uint64_t vtiles = 0, ttiles = 0, otiles = 0;
    const uint8_t *work;
    uint8_t *complex;
    uint32_t mis;
    uint32_t *stores;
    int64_t outside = 0;
    Mem mem(const CxwField &F, uint64_t f, uint32_t cont)
    {
        return Mem{work + F.work_off, (int64_t)(F.n * cont), complex, (int64_t)F.off, (int64_t)(F.off + bound[f]), mis, stores, &outside};
    }
};

// (what cxw_write of aec_gribcxw.hip writes)
void describe(Batch &B, const uint32_t *tmpl, const uint64_t *n_values, const uint64_t *offsets, const uint64_t *work_offsets, uint64_t n)
{
    B.d.assign(n + 1, CxwField{});
    B.bound.assign(n, 0);
    uint64_t vt = 0, tt = 0, ot = 0, g0 = 0;
    for (uint64_t i = 0; i <= n; i++) {
        CxwField &f = B.d[i];
        f.vtile0 = vt;
        f.ttile0 = tt;
        f.otile0 = ot;
        f.group0 = g0;
        if (i == n) break;
        f.off = offsets[i];
        f.n = n_values[i];
        f.work_off = work_offsets[i];
        f.room = grib_room(f.n, tmpl[2], grib_container(tmpl[0]));
        f.ng = (uint32_t)cxw_groups(f.n, B.P.G);
        B.bound[i] = cxw_bound(f.n, B.P.nbits, B.P.order, B.P.G);
        vt += grib_room_waves(f.room);
        tt += ((uint64_t)f.ng + kCxwTableTile - 1) / kCxwTableTile;
        ot += (cxw_string_bound(f.n, B.P.nbits, B.P.order) + kCxwOutTile - 1) / kCxwOutTile;
        g0 += f.ng;
    }
    B.vtiles = vt;
    B.ttiles = tt;
    B.otiles = ot;
    B.dyn.assign(n, CxwDyn{});
    B.minsd.assign(n, 0);
    B.tmin.assign(vt, 0);
    B.tile.assign(vt, CxwTile{});
    B.gref.assign(g0, 0);
    B.gwid.assign(g0, 0);
    B.gbit.assign(g0, 0);
}

// the extremes of every lane of a value tile (k_cxw_diff and k_cxw_groups: lane_ext)
template <int CONT>
void tile_ext(Batch &B, uint64_t n, uint64_t w, uint64_t *field, int64_t (&lo)[64], int64_t (&hi)[64])
{
    constexpr uint32_t per = 16u / CONT;
    const uint64_t f = cxw_field_of_tile(B.d.data(), n, 0, w);
    const CxwField &F = B.d[f];
    Mem m = B.mem(F, f, CONT);
    uint32_t prev[per] = {};
    for (uint32_t lane = 0; lane < 64; lane++) {
        const GribBitsLane L = grib_bits_lane(w - F.vtile0, lane, per, F.n, 0, 0);
        uint32_t x[per];
        cxw_lane_x<CONT>(m, L, B.P.nbits, x);
        uint32_t p1 = prev[per - 1], p2 = prev[per - 2];
        if (lane == 0) {
            p1 = p2 = 0;
            if (L.cnt) cxw_pred<CONT>(m, L.j0, B.P.order, B.P.nbits, &p1, &p2);
        }
        cxw_lane_ext<(int)per>(x, L.j0, L.cnt, B.P.order, p1, p2, &lo[lane], &hi[lane]);
        memcpy(prev, x, sizeof(x));
    }
    *field = f;
}

template <int CONT>
void run(Batch &B, uint64_t n, uint8_t *cxw)
{
    constexpr uint32_t per = 16u / CONT;
    const CxwShape &P = B.P;
    int64_t lo[64], hi[64];
    uint64_t f;
    if (P.order) {
        for (uint64_t w = 0; w < B.vtiles; w++) {                           // k_cxw_diff
            tile_ext<CONT>(B, n, w, &f, lo, hi);
            int64_t least = INT64_MAX;
            for (uint32_t lane = 0; lane < 64; lane++) least = lo[lane] < least ? lo[lane] : least;
            B.tmin[w] = least;
        }
        for (f = 0; f < n; f++) {                                           // k_cxw_minsd
            int64_t least = INT64_MAX;
            for (uint64_t t = B.d[f].vtile0; t < B.d[f + 1].vtile0; t++) least = B.tmin[t] < least ? B.tmin[t] : least;
            B.minsd[f] = least == INT64_MAX ? 0 : least;
        }
    }
    for (uint64_t w = 0; w < B.vtiles; w++) {                               // k_cxw_groups
        tile_ext<CONT>(B, n, w, &f, lo, hi);
        const CxwField &F = B.d[f];
        const int64_t minsd = P.order ? B.minsd[f] : 0;
        const uint32_t lanes = P.G / per, gpt = 64u / lanes;
        uint32_t run_bits = 0;
        CxwTile a = cxw_tile_none();
        for (uint32_t q = 0; q < gpt; q++) {
            const uint64_t g = (w - F.vtile0) * gpt + q;
            if (g >= F.ng) break;
            int64_t glo = INT64_MAX, ghi = INT64_MIN;
            for (uint32_t lane = q * lanes; lane < (q + 1) * lanes; lane++) {
                glo = lo[lane] < glo ? lo[lane] : glo;
                ghi = hi[lane] > ghi ? hi[lane] : ghi;
            }
            const CxwGroup G = cxw_group(glo, ghi, minsd, cxw_group_len(F, P.G, g));
            B.gref[F.group0 + g] = G.ref;
            B.gwid[F.group0 + g] = G.width;
            B.gbit[F.group0 + g] = run_bits;
            run_bits += G.bits;
            a = cxw_tile_join(a, cxw_tile_of(G));
        }
        B.tile[w] = a;
    }
    for (f = 0; f < n; f++) {                                               // k_cxw_field
        const CxwField &F = B.d[f];
        uint64_t carry = 0;
        CxwTile all = cxw_tile_none();
        for (uint64_t t = F.vtile0; t < B.d[f + 1].vtile0; t++) {
            const CxwTile a = B.tile[t];
            B.tile[t].bits = carry;
            carry += a.bits;
            all = cxw_tile_join(all, a);
        }
        all.bits = carry;
        const CxwDyn Y = cxw_dyn(F, P, all, P.order ? B.minsd[f] : 0);
        B.dyn[f] = Y;
        const CxwRecord R = cxw_record(F, P, Y);
        memcpy(cxw + 56 * f, &R, 56);
        Mem m = B.mem(F, f, CONT);
        cxw_head_bytes<CONT>(m, F, P, Y);
    }
    for (uint64_t w = 0; w < B.ttiles; w++) {                               // k_cxw_tables
        f = cxw_field_of_tile(B.d.data(), n, 1, w);
        const CxwField &F = B.d[f];
        const CxwDyn &Y = B.dyn[f];
        Mem m = B.mem(F, f, CONT);
        uint64_t at = F.off + cxw_head(P.nbits, P.order);
        for (int which = 0; which < 2; which++) {
            const uint32_t bits = which ? Y.width_bits : Y.ref_bits;
            if (bits) {
                uint64_t shi[64], slo[64];
                uint32_t cnt[64];
                const uint32_t *tab = (which ? B.gwid.data() : B.gref.data()) + F.group0;
                for (uint32_t lane = 0; lane < 64; lane++)
                    cxw_table_string(tab, which ? Y.width_ref : 0u, ((w - F.ttile0) * 64u + lane) * kCxwTableLane, F.ng, bits, &shi[lane], &slo[lane],
                                     &cnt[lane]);
                for (uint32_t lane = 0; lane < 64; lane++) {
                    const uint64_t g0 = ((w - F.ttile0) * 64u + lane) * kCxwTableLane, p0 = at * 8u + g0 * bits;
                    grib_bits_store(m, shi[lane], slo[lane], p0, p0 + (uint64_t)cnt[lane] * bits, lane < 63u ? grib_bits_head(shi[lane + 1]) : 0u,
                                    B.mis);
                }
            }
            at += cxw_table_bytes(F.ng, bits);
        }
    }
    for (uint64_t w = 0; w < B.otiles; w++) {                               // k_cxw_values
        f = cxw_field_of_tile(B.d.data(), n, 2, w);
        const CxwField &F = B.d[f];
        const CxwDyn &Y = B.dyn[f];
        if ((w - F.otile0) * (8u * kCxwOutTile) >= Y.bits) continue;
        Mem m = B.mem(F, f, CONT);
        const CxwTables T{B.tile.data() + F.vtile0, B.gref.data() + F.group0, B.gwid.data() + F.group0, B.gbit.data() + F.group0};
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t lane_in_field = (w - F.otile0) * 64u + lane;
            uint64_t shi, slo;
            const uint32_t nb = cxw_lane_string<CONT>(m, F, P, Y, T, lane_in_field, &shi, &slo);
            const uint64_t p0 = 8u * (F.off + Y.data_byte + lane_in_field * kCxwOutLane);
            grib_bits_store(m, shi, slo, p0, p0 + 8u * nb, 0u, B.mis);
        }
    }
}

}  // namespace

extern "C" uint32_t gribcxw_emul_tiles(uint32_t which) { return which ? kCxwOutTile : kCxwTableTile; }

extern "C" uint64_t gribcxw_emul_bound(uint64_t n, uint32_t nbits, uint32_t order, uint32_t G) { return cxw_bound(n, nbits, order, G); }

// tmpl = {nbits, options, block size, rsi}; work: the rooms; complex: the stream buffer, as if it lay at an address of `mis`
// modulo 4; stores: an entry per byte of it; cxw: 56 bytes per field.  Returns the accesses that were out of place.
extern "C" int64_t gribcxw_emul_write(const uint32_t *tmpl, uint32_t order, uint32_t G, const uint64_t *n_values, uint64_t n, const uint8_t *work,
                                      const uint64_t *work_offsets, uint8_t *complex, uint32_t mis, const uint64_t *offsets, uint32_t *stores,
                                      uint8_t *cxw)
{
    Batch B;
    B.P = CxwShape{order, G, tmpl[0], cxw_extra(tmpl[0], order)};
    B.work = work;
    B.complex = complex;
    B.mis = mis;
    B.stores = stores;
    describe(B, tmpl, n_values, offsets, work_offsets, n);
    const uint32_t cont = grib_container(tmpl[0]);
    if (cont == 1) run<1>(B, n, cxw);
    else if (cont == 2) run<2>(B, n, cxw);
    else run<4>(B, n, cxw);
    return B.outside;
}
