// aec_dchunks.h -- a batch of UNEQUAL chunks decoded as one launch (aec_gpu_decode_chunks_async): the chunk descriptors
// and the arithmetic that turns an item of the launch into its chunk, its RSI, its table entry and its place in the
// output.
//
// The chunks are numbered 0 .. n-1; chunk i announces rsis_i RSIs (the last of them last_blocks_i blocks, the others
// c.rsi), and the RSIs are numbered through, chunk after chunk: these are the ITEMS of the decode launch.  The offset
// table has rsis_i + 1 entries per chunk (the layout aec_gpu_encode_chunks_async writes), so item r of chunk i starts at
// entry r + i.  Every chunk has a room of its own in the output, at a 16-byte aligned offset: block b of the chunk lands
// at out_off_i + b * block bytes, which is what the store paths of the decode kernels take as "blocks counted from one
// 16-byte aligned base" -- per chunk instead of per launch.
//
// How an item finds its chunk: a table of one uint32_t per item (item_chunk[r], written by k_dchunks_setup with
// dchunk_of_item below).  4 bytes per item against the rsi * block bytes an item writes (8 bytes at the very least:
// 8-bit samples, blocks of 8, rsi 1; 1 KiB for the 8-bit shape of rsi 128); a search over the chunks' item prefix per
// item would cost no memory but log2(n) dependent loads in front of every lane's first stream load, and a full record
// per item (chunk, RSI, entry, blocks, position: 32 bytes) four times an 8-byte RSI.
// The functions are __host__ __device__: the kernels (aec_dec.hip) call them and tests/emul/dchunks_emul.cpp runs the same
// functions on the CPU.
#pragma once
#include <stdint.h>

#include "aec_lane.h"

namespace aec {

// Descriptor of chunk i (host-written, n + 1 of them: entry n holds the totals).
struct DChunkDesc {
    uint64_t in_off, in_bytes;   // the chunk's stream: in_bytes bytes at byte in_off of d_in (bare streams only)
    uint64_t out_off;            // byte offset of its room in d_out (multiple of 16)
    uint64_t item0;              // its first item = the sum of the RSI counts in front; its first table entry: item0 + i
    uint32_t rsis;               // RSIs announced
    uint32_t last_blocks;        // blocks of the last of them (1 .. c.rsi; 0 for a chunk without a sample)
};

// samples, blocks and RSIs of a chunk that decodes to out_bytes bytes (make_cfg's arithmetic; a trailing fraction of a
// sample is ignored, the last block is decoded whole)
struct DChunkCounts {
    uint64_t samples, blocks, rsis;
    uint32_t last_blocks;
};
AEC_HD DChunkCounts dchunk_counts(uint64_t out_bytes, uint32_t bytes, uint32_t bs, uint32_t rsi)
{
    DChunkCounts r;
    r.samples = out_bytes / bytes;
    r.blocks = (r.samples + bs - 1) / bs;
    r.rsis = (r.blocks + rsi - 1) / rsi;
    r.last_blocks = r.blocks ? (uint32_t)(r.blocks - (r.rsis - 1) * rsi) : 0u;
    return r;
}

// room of a chunk in a PACKED output (aec_gpu_decode_chunks_plan, Codec.decode_chunks, the libaec ABI): its whole
// blocks, rounded up to the alignment of the next room
AEC_HD uint64_t dchunk_room(uint64_t blocks, uint64_t blk_bytes) { return (blocks * blk_bytes + 15u) & ~(uint64_t)15u; }

// the chunk that owns item r: the LAST chunk whose first item is <= r -- chunks without an item in front of it share
// its item0, chunks behind it start later.  r must be below d[n].item0.
AEC_HD uint64_t dchunk_of_item(const DChunkDesc *d, uint64_t n, uint64_t r)
{
    uint64_t lo = 0, hi = n;            // invariant: d[lo].item0 <= r < d[hi].item0
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (d[mid].item0 <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}

// what the index pass found for a chunk -- or, with the caller's table, what the chunk announces -- in the form of an
// index record: whole RSIs and the blocks of a trailing short one
AEC_HD void dchunk_announced(const DChunkDesc &e, uint32_t rsi, uint64_t *whole, uint64_t *tail)
{
    const bool full = e.rsis != 0u && e.last_blocks == rsi;
    *whole = e.rsis ? (full ? e.rsis : e.rsis - 1u) : 0u;
    *tail = (e.rsis && !full) ? e.last_blocks : 0u;
}

// Item r of the launch, chunk `chunk` (= item_chunk[r])
struct DItem {
    uint64_t chunk;
    uint64_t rin;        // the RSI within the chunk
    uint64_t entry;      // index of its start bit in the offset table
    uint32_t nb;         // blocks to decode
    uint64_t out_pos;    // byte offset in d_out of its first block
};
// whole / tail: the chunk's record (n_rsi, tail_blocks).  An item decodes what the record holds for it, and never more
// than the chunk announces: nothing is written outside the chunk's room whatever a stream pretends.
AEC_HD DItem dchunk_item(const DChunkDesc *d, uint64_t chunk, uint64_t r, uint32_t rsi, uint64_t blk_bytes, uint64_t whole,
                         uint64_t tail)
{
    const DChunkDesc &e = d[chunk];
    DItem it;
    it.chunk = chunk;
    it.rin = r - e.item0;
    it.entry = r + chunk;
    const uint32_t found = it.rin < whole ? rsi : (it.rin == whole ? (uint32_t)(tail < rsi ? tail : rsi) : 0u);
    const uint32_t room = it.rin + 1u < e.rsis ? rsi : (it.rin + 1u == e.rsis ? e.last_blocks : 0u);
    it.nb = found < room ? found : room;
    it.out_pos = e.out_off + it.rin * rsi * blk_bytes;
    return it;
}

}  // namespace aec
