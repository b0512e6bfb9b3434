// aec_chunks.h -- a batch of UNEQUAL chunks as one launch set (aec_gpu_encode_chunks_async): the chunk descriptors
// and the arithmetic of the segmented three-phase scan that gives every segment its start bit and carried k.
//
// The chunks are numbered 0 .. n-1 and their segments are numbered through, chunk after chunk ("concatenated
// numbering"); an empty chunk (no whole sample) has no segment.  The scan runs over tiles of kScanChunk segments of
// that numbering with the operator of the single-stream scan (bits add, k clamps compose) RESTARTED at every chunk's
// first segment:
//   phase 1  per tile: the tile's aggregate, and for every chunk that has segments in the tile their bits added to the
//            chunk's total;
//   phase 2  one workgroup: the chunks' byte-aligned bases from the totals (an empty chunk takes one zero byte), and
//            the exclusive scan of the tile aggregates = what the chunk that is open at a tile's start has
//            accumulated in front of the tile (the tile carry);
//   phase 3  per tile: start bit and carried k of every segment (k counted from 0 at the chunk start), the RSI table
//            entries, and the zeroing of the output words two waves of the pack kernel share.
// The functions are __host__ __device__: the kernels (aec_enc.hip k_chunks_*) are loops over them with a workgroup
// scan in between, and tests/emul/chunks_emul.cpp runs the same functions tile by tile on the CPU.
#pragma once
#include <stdint.h>

#include "aec_lane.h"

namespace aec {

// Descriptor of chunk i (host-written, n + 1 of them: entry n holds the totals).  Everything but in_off and samples
// is a prefix sum over the chunks in front.
struct ChunkDesc {
    uint64_t in_off;    // byte offset of the chunk in d_in (multiple of 16)
    uint64_t samples;   // whole samples of the chunk
    uint64_t blk0;      // its first block in the per-block summaries
    uint64_t seg0;      // its first segment in the concatenated numbering
    uint64_t rsi0;      // its first entry in the RSI table (a chunk has rsi_count + 1 entries)
    uint64_t wave0;     // its first wavefront (a chunk has ceil(segs / segs_per_wave) of them)
};

// blocks, segments and RSIs of a chunk of `samples` samples (make_cfg's arithmetic)
struct ChunkCounts {
    uint64_t blocks, segs, rsis;
};
AEC_HD ChunkCounts chunk_counts(uint64_t samples, uint32_t bs, uint32_t rsi, uint32_t segs_per_rsi)
{
    ChunkCounts r;
    r.blocks = (samples + bs - 1) / bs;
    r.rsis = (r.blocks + rsi - 1) / rsi;
    r.segs = (r.blocks / rsi) * segs_per_rsi + (r.blocks % rsi + 63) / 64;
    return r;
}

// the chunk that owns element x of a prefix-summed field (seg0 or wave0): the LAST chunk whose first element is <= x
// -- empty chunks in front of it share its value, chunks behind it start later.  x must be below the total.
template <class Field>
AEC_HD uint64_t chunk_owner(const ChunkDesc *d, uint64_t n, uint64_t x, Field field)
{
    uint64_t lo = 0, hi = n;            // invariant: field(d[lo]) <= x < field(d[hi])
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (field(d[mid]) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
AEC_HD uint64_t chunk_of_seg(const ChunkDesc *d, uint64_t n, uint64_t s)
{
    return chunk_owner(d, n, s, [](const ChunkDesc &e) { return e.seg0; });
}
AEC_HD uint64_t chunk_of_wave(const ChunkDesc *d, uint64_t n, uint64_t w)
{
    return chunk_owner(d, n, w, [](const ChunkDesc &e) { return e.wave0; });
}

// bytes a chunk's stream occupies: zero-padded to a byte; the empty stream is one zero byte
AEC_HD uint64_t chunk_stream_bytes(uint64_t bits) { return bits ? (bits + 7) / 8 : 1; }

// ---- the scan's value and operator ---------------------------------------------------------------------------
struct CkVal {
    uint64_t bits;
    uint32_t cl;      // k clamp, lo | hi << 8
    uint32_t head;    // a chunk starts inside the range: bits and cl count from the last such start
};
AEC_HD CkVal ck_identity()
{
    const KClamp id = kclamp_identity();
    return CkVal{0, id.lo | (id.hi << 8), 0u};
}
AEC_HD CkVal ck_then(CkVal a, CkVal b)
{
    if (b.head) return b;
    const KClamp t = kclamp_then(KClamp{a.cl & 0xFFu, (a.cl >> 8) & 0xFFu}, KClamp{b.cl & 0xFFu, (b.cl >> 8) & 0xFFu});
    return CkVal{a.bits + b.bits, t.lo | (t.hi << 8), a.head};
}

// Cursor of a thread that walks consecutive segments: the chunk of the segment it stands on
struct CkCursor {
    uint64_t chunk, seg_end;     // seg_end = first segment behind the chunk
};
AEC_HD CkCursor ck_cursor(const ChunkDesc *d, uint64_t n, uint64_t s)
{
    const uint64_t c = chunk_of_seg(d, n, s);
    return CkCursor{c, d[c + 1].seg0};
}
AEC_HD void ck_advance(const ChunkDesc *d, uint64_t n, uint64_t s, CkCursor &cur)
{
    while (s >= cur.seg_end && cur.chunk + 1 < n) {     // (empty chunks are stepped over)
        cur.chunk++;
        cur.seg_end = d[cur.chunk + 1].seg0;
    }
}
// segment s as the scan sees it
AEC_HD CkVal ck_item(const ChunkDesc *d, const CkCursor &cur, uint64_t s, uint32_t bits, uint32_t clamp)
{
    return CkVal{bits, clamp, s == d[cur.chunk].seg0 ? 1u : 0u};
}

// ---- phase 1: a thread's consecutive segments [s0, s1) of a tile that ends at tile_end ----------------------------
// aggregate of the segments (the input of the workgroup scan)
AEC_HD CkVal ck_reduce_items(const ChunkDesc *d, uint64_t n, const uint32_t *seg_bits, const uint16_t *seg_clamp,
                             uint64_t s0, uint64_t s1)
{
    CkVal acc = ck_identity();
    if (s0 >= s1) return acc;
    CkCursor cur = ck_cursor(d, n, s0);
    for (uint64_t s = s0; s < s1; s++) {
        ck_advance(d, n, s, cur);
        acc = ck_then(acc, ck_item(d, cur, s, seg_bits[s], seg_clamp[s]));
    }
    return acc;
}
// ... and with the thread's exclusive prefix INSIDE the tile (run), the contribution of the tile to every chunk that
// ends its stay in the tile at one of these segments: add(chunk, bits) -- on the device a vector atomic
template <class Add>
AEC_HD void ck_flush_totals(const ChunkDesc *d, uint64_t n, const uint32_t *seg_bits, const uint16_t *seg_clamp,
                            uint64_t s0, uint64_t s1, uint64_t tile_end, CkVal run, Add add)
{
    if (s0 >= s1) return;
    CkCursor cur = ck_cursor(d, n, s0);
    for (uint64_t s = s0; s < s1; s++) {
        ck_advance(d, n, s, cur);
        run = ck_then(run, ck_item(d, cur, s, seg_bits[s], seg_clamp[s]));
        if (s + 1 == cur.seg_end || s + 1 == tile_end) add(cur.chunk, run.bits);
    }
}

// ---- phase 2 ---------------------------------------------------------------------------------------------------
// bases: run_bytes = bytes of the streams in front of chunk i; returns the bytes behind it
AEC_HD uint64_t ck_base(uint64_t run_bytes, uint64_t bits, uint64_t *base_bits)
{
    *base_bits = run_bytes * 8;
    return run_bytes + chunk_stream_bytes(bits);
}

// ---- phase 3: what segment s receives -----------------------------------------------------------------------------
struct CkSeg {
    uint64_t start;        // absolute start bit
    uint32_t kin;          // k carried into the segment (0 at the chunk start)
    uint32_t first_rsi;    // 1: the segment opens an RSI, whose table entry is rsi_entry
    uint64_t rsi_entry;
    uint32_t last;         // 1: the chunk ends with this segment, at bit `end` (table entry rsi_entry_end)
    uint64_t end, rsi_entry_end;
    uint32_t wave_first;   // 1: a wavefront of the pack kernel starts with this segment
};
// run = the scan's exclusive prefix of s (tile carry included); item = segment s
AEC_HD CkSeg ck_segment(const ChunkDesc *d, const CkCursor &cur, uint64_t s, CkVal run, CkVal item, uint64_t base_bits,
                        uint32_t segs_per_rsi, uint32_t segs_per_wave)
{
    const CkVal excl = item.head ? ck_identity() : run;
    const uint64_t local = s - d[cur.chunk].seg0;
    CkSeg r;
    r.start = base_bits + excl.bits;
    r.kin = kclamp_apply(KClamp{excl.cl & 0xFFu, (excl.cl >> 8) & 0xFFu}, 0u);
    r.first_rsi = local % segs_per_rsi == 0 ? 1u : 0u;
    r.rsi_entry = d[cur.chunk].rsi0 + local / segs_per_rsi;
    r.last = s + 1 == cur.seg_end ? 1u : 0u;
    r.end = r.start + item.bits;
    r.rsi_entry_end = d[cur.chunk + 1].rsi0 - 1;
    r.wave_first = local % segs_per_wave == 0 ? 1u : 0u;
    return r;
}

}  // namespace aec
