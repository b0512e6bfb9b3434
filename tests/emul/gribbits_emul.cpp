// gribbits_emul.cpp -- host harness for libaec_amd/csrc/aec_gribbits.h: what k_grib_bits_pack and k_grib_bits_unpack
// (libaec_amd/csrc/aec_gribbits.hip) do wavefront by wavefront and lane by lane, through the same functions and the same
// descriptors.  Every access to the stream buffer goes through a checked policy: a store outside the field's S_i bytes, a
// load outside the buffer and a word access whose address is no multiple of 4 are skipped and counted, and the count is what
// the calls return (0 = none).  Every store is counted per byte as well (stores: of the stream buffer, of the work buffer).
// Built by tests/test_grib_simple_emul.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../libaec_amd/csrc/aec_gribbits.h"

using namespace aec;

namespace {

struct Batch {
    std::vector<GribField> d;
    uint64_t waves = 0;
    int64_t outside = 0;
};

Batch describe(const uint32_t *tmpl, const uint64_t *n_values, const uint64_t *work_offsets, const uint64_t *simple_offsets, uint64_t n)
{
    Batch B;
    B.d.assign(n + 1, GribField{});
    for (uint64_t i = 0; i <= n; i++) {
        B.d[i].wave0[1] = B.waves;
        if (i == n) break;
        B.d[i].off = simple_offsets[i];
        B.d[i].n = n_values[i];
        B.d[i].work_off = work_offsets[i];
        B.d[i].room = grib_room(n_values[i], tmpl[2], grib_container(tmpl[0]));
        B.waves += grib_room_waves(B.d[i].room);
    }
    return B;
}

// the stream buffer as a lane sees it: bytes [lo, hi) may be stored (a pack: the field's), bytes [0, size) loaded
struct Mem {
    uint8_t *p;
    int64_t lo, hi, size;
    uint32_t mis;
    uint32_t *stores;
    int64_t *outside;
    uint32_t ld8(int64_t o) const
    {
        if (o < 0 || o >= size) {
            ++*outside;
            return 0;
        }
        return p[o];
    }
    uint32_t ld32(int64_t o) const
    {
        if ((o + (int64_t)mis) & 3) ++*outside;
        uint32_t v = 0;
        for (int b = 0; b < 4; b++) v |= ld8(o + b) << (8 * b);           // (little-endian, as the device)
        return v;
    }
    void st8(int64_t o, uint8_t v) const
    {
        if (o < lo || o >= hi) {
            ++*outside;
            return;
        }
        p[o] = v;
        stores[o]++;
    }
    void st32(int64_t o, uint32_t v) const
    {
        if ((o + (int64_t)mis) & 3) ++*outside;
        for (int b = 0; b < 4; b++) st8(o + b, (uint8_t)(v >> (8 * b)));
    }
};

template <int CONT>
void pack(Batch &B, uint64_t n, uint32_t nbits, const uint8_t *work, uint64_t work_bytes, uint8_t *simple, uint32_t mis, uint32_t *stores)
{
    for (uint64_t w = 0; w < B.waves; w++) {
        const GribField &F = B.d[grib_field_of_wave(B.d.data(), n, 1, w)];
        const uint64_t in_field = w - F.wave0[1];
        GribBitsLane L[64];
        uint64_t hi[64], lo[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            L[lane] = grib_bits_lane(in_field, lane, 16u / CONT, F.n, F.off, nbits);
            hi[lane] = lo[lane] = 0;
            if (!L[lane].cnt) continue;
            const uint64_t at = F.work_off + (in_field * 64u + lane) * 16u;
            if (at + 16u > work_bytes) {
                B.outside++;
                continue;
            }
            uint32_t g[4];
            memcpy(g, work + at, 16);
            grib_bits_of_group<CONT>(g, nbits, L[lane].cnt, &hi[lane], &lo[lane]);
        }
        const int64_t first = (int64_t)F.off;
        Mem m{simple, first, first + (int64_t)grib_bits_bytes(F.n, nbits), 0, mis, stores, &B.outside};
        for (uint32_t lane = 0; lane < 64; lane++)
            grib_bits_store(m, hi[lane], lo[lane], L[lane].p0, L[lane].p1, lane < 63 ? grib_bits_head(hi[lane + 1]) : 0u, mis);
    }
}

template <int CONT>
void unpack(Batch &B, uint64_t n, uint32_t nbits, const uint8_t *simple, uint64_t simple_bytes, uint32_t mis, uint8_t *work, uint32_t *stores)
{
    Mem m{const_cast<uint8_t *>(simple), 0, 0, (int64_t)simple_bytes, mis, nullptr, &B.outside};
    for (uint64_t w = 0; w < B.waves; w++) {
        const GribField &F = B.d[grib_field_of_wave(B.d.data(), n, 1, w)];
        const uint64_t in_field = w - F.wave0[1];
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t at = (in_field * 64u + lane) * 16u;
            if (at >= F.room) continue;
            const GribBitsLane L = grib_bits_lane(in_field, lane, 16u / CONT, F.n, F.off, nbits);
            uint32_t g[4];
            grib_bits_group_of<CONT>(m, L, F.off, F.n, nbits, mis, simple_bytes, g);
            for (uint32_t i = 0; i < 16; i++) {
                if (at + i >= F.room) continue;
                work[F.work_off + at + i] = (uint8_t)(g[i >> 2] >> (8 * (i & 3)));
                stores[F.work_off + at + i]++;
            }
        }
    }
}

}  // namespace

extern "C" uint32_t gribbits_emul_wave_room(void) { return kGribWaveRoom; }

// tmpl = {nbits, options, block size, rsi}.  simple is the buffer's first byte, mis what its address is taken to be modulo 4;
// stores has an entry per byte of it.
extern "C" int64_t gribbits_emul_pack(const uint32_t *tmpl, const uint64_t *n_values, uint64_t n, const uint8_t *work, uint64_t work_bytes,
                                      const uint64_t *work_offsets, uint8_t *simple, const uint64_t *simple_offsets, uint32_t mis,
                                      uint32_t *stores)
{
    Batch B = describe(tmpl, n_values, work_offsets, simple_offsets, n);
    const uint32_t cont = grib_container(tmpl[0]);
    if (cont == 1) pack<1>(B, n, tmpl[0], work, work_bytes, simple, mis, stores);
    else if (cont == 2) pack<2>(B, n, tmpl[0], work, work_bytes, simple, mis, stores);
    else pack<4>(B, n, tmpl[0], work, work_bytes, simple, mis, stores);
    return B.outside;
}

// stores has an entry per byte of work
extern "C" int64_t gribbits_emul_unpack(const uint32_t *tmpl, const uint64_t *n_values, uint64_t n, const uint8_t *simple,
                                        uint64_t simple_bytes, const uint64_t *simple_offsets, uint32_t mis, uint8_t *work,
                                        const uint64_t *work_offsets, uint32_t *stores)
{
    Batch B = describe(tmpl, n_values, work_offsets, simple_offsets, n);
    const uint32_t cont = grib_container(tmpl[0]);
    if (cont == 1) unpack<1>(B, n, tmpl[0], simple, simple_bytes, mis, work, stores);
    else if (cont == 2) unpack<2>(B, n, tmpl[0], simple, simple_bytes, mis, work, stores);
    else unpack<4>(B, n, tmpl[0], simple, simple_bytes, mis, work, stores);
    return B.outside;
}
