// aec_gribbm.h -- GRIB2 section 6 bitmaps around the simple packing of aec_grib.h (include/aec_gpu_grib.h): the per-lane
// arithmetic of aec_gribbm.hip.  A field of N grid points has a bitmap of N bits, point k is bit 7 - k % 8 of byte k / 8
// (most significant bit first, what numpy.packbits writes), 1 = present; section 7 holds the X of the present points only,
// in grid order.
//
// A field owns whole TILES of kGribBmTile grid points, a wavefront owns one tile and a lane kGribBmLane = 16 consecutive
// points of it: two whole bytes of the bitmap, which the lane reads (or writes) as BYTES, so a bitmap may begin on any byte
// and no load reaches past byte ceil(N / 8) - 1; the bytes go into a 16-bit word with the first byte on top, so point j of
// the lane is bit 15 - j of the word, whatever the byte order of the machine.
//   rank of a point   ones in front of it in its field = the tile's base (exclusive sum of the tile counts of the field, 64
//                     bits) + the ones of the lower lanes (a wave scan) + the ones above its bit in the lane's word
//   pack              the X of a present point goes to sample `rank` of the field's room; ranks at or beyond n (the host's
//                     count of present points) are dropped, and the lane that holds rank n - 1 also writes the padding of
//                     the last block (grib_value_of_sample: the last X repeated)
//   unpack            a present point reads sample min(rank, n - 1)
// so no index leaves the room, the bitmap or the N elements whatever the bitmap holds.
// The functions are __host__ __device__: the kernels call them and tests/emul/gribbm_emul.cpp runs the same functions on
// the CPU, wavefront by wavefront and lane by lane.
#pragma once
#include "aec_grib.h"

namespace aec {

enum { kGribMismatch = 8u };             // status bit 3: the bitmap does not hold n ones
constexpr uint32_t kGribBmTile = 1024;   // grid points a wavefront of the bitmap kernels owns
constexpr uint32_t kGribBmLane = kGribBmTile / 64;
static_assert(kGribBmLane == 16, "a lane owns two whole bytes of the bitmap");

// Bitmap descriptor of field i (host-written, n + 1 of them: entry n holds the total in tile0) beside its GribField, whose
// off is the place of the WHOLE grid and whose n is the host's count of present points.
struct GribBitmap {
    uint64_t bm_off;     // byte offset of its bitmap from the call's d_bitmap: any byte
    uint64_t points;     // grid points N
    uint64_t tile0;      // its first tile (= wavefront) of a launch
};

AEC_HD uint64_t grib_bm_tiles(uint64_t points) { return (points + kGribBmTile - 1) / kGribBmTile; }
AEC_HD uint64_t grib_bm_bytes(uint64_t points) { return (points + 7) / 8; }

// the field that owns tile w: the last field whose first tile is <= w.  w must be below b[n].tile0 (every field has a tile).
AEC_HD uint64_t grib_bm_field_of_tile(const GribBitmap *b, uint64_t n, uint64_t w)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (b[mid].tile0 <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

// what a lane owns of its field
struct GribBmLane {
    uint64_t p0;         // its first grid point
    uint32_t valid;      // how many of its 16 points the field has: 0 .. 16
    uint64_t byte0;      // its first byte of the field's bitmap
    uint32_t nbytes;     // how many of its two bytes the bitmap has: 0 .. 2
};
AEC_HD GribBmLane grib_bm_lane(uint64_t tile_in_field, uint32_t lane, uint64_t points)
{
    GribBmLane L;
    L.p0 = tile_in_field * kGribBmTile + (uint64_t)lane * kGribBmLane;
    L.valid = points > L.p0 ? (points - L.p0 < kGribBmLane ? (uint32_t)(points - L.p0) : kGribBmLane) : 0u;
    L.byte0 = L.p0 / 8u;
    L.nbytes = (L.valid + 7u) / 8u;
    return L;
}

// the lane's word from its two bytes (a byte the bitmap does not have is passed as 0): point j is bit 15 - j; bits of
// points the field does not have are cleared, whatever a foreign bitmap holds there
AEC_HD uint32_t grib_bm_word(uint32_t b0, uint32_t b1, uint32_t valid) { return ((b0 << 8) | b1) & ~(0xFFFFu >> valid) & 0xFFFFu; }
AEC_HD uint32_t grib_bm_byte(uint32_t word, uint32_t k) { return (word >> (8u * (1u - k))) & 0xFFu; }      // byte k of the lane, to write
AEC_HD bool grib_bm_present(uint32_t word, uint32_t j) { return (word >> (15u - j)) & 1u; }
AEC_HD uint32_t grib_bm_count(uint32_t word) { return (uint32_t)__builtin_popcount(word); }
// ones of the lane in front of its point j
AEC_HD uint32_t grib_bm_rank(uint32_t word, uint32_t j) { return (uint32_t)__builtin_popcount(word >> (16u - j)); }

// One step of the inclusive wave scan (Hillis-Steele): lane takes the value `lower` of lane - off where there is one.
// After the steps off = 1, 2, .. 32 a lane holds the sum over lanes 0 .. lane.
AEC_HD uint32_t grib_bm_scan_step(uint32_t own, uint32_t lower, uint32_t lane, uint32_t off) { return lane >= off ? own + lower : own; }

// the base of a tile from the round's carry (the ones of the field's tiles in front of the round, 64 bits) and the
// inclusive scan over the round's 64 tile counts
AEC_HD uint64_t grib_bm_tile_base(uint64_t carry, uint32_t inclusive, uint32_t count) { return carry + (inclusive - count); }

// pack: rank r of the field (tile base + ones in front within the tile) is sample r of the room if the host counted it
AEC_HD bool grib_bm_kept(uint64_t r, uint64_t n) { return r < n; }
// ... and its writer also writes samples n .. room_samples - 1, the padding of the last block
AEC_HD bool grib_bm_pads(uint64_t r, uint64_t n) { return r + 1 == n; }
// unpack: the sample a present point of rank r reads
AEC_HD uint64_t grib_bm_sample(uint64_t r, uint64_t n) { return grib_value_of_sample(r, n); }

// a point is missing iff its value == the missing value (IEEE: either zero matches a zero); under a NaN iff it is a NaN
template <typename T>
AEC_HD bool grib_bm_is_missing(T v, T missing, bool missing_is_nan) { return missing_is_nan ? v != v : v == missing; }

// the record of a field after the scan: grib_params of the present points' extremes, plus bit 3 where the bitmap's ones
// are not the host's count
AEC_HD uint32_t grib_bm_mismatch(uint64_t ones, uint64_t n) { return ones == n ? 0u : (uint32_t)kGribMismatch; }

}  // namespace aec
