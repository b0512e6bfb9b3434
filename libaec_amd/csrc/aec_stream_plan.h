// aec_stream_plan.h -- the arithmetic of one streaming decode batch (aec_abi.cpp: decode_run), host only.
//
// decode_run is four parts: PLAN (what part of the resident stream the batch indexes, how many RSIs it may bring,
// how large its buffers are), the launches and their one synchronisation, the VERDICT over the two result records
// (what is good, what is an error now, what is deferred to the next call and where the walker resumes) and the
// ADVANCE of the stream's position.  The three pure parts are here -- no HIP, no globals -- so that tests/emul/
// abi_emul.cpp can run them on a machine without a GPU (tests/test_stream_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/aec_gpu.h"
#include "aec_cfg.h"

namespace aec {

constexpr size_t kMinBatchOut = (size_t)4 << 20;     // output a decode batch may produce beyond the room offered
constexpr size_t kPipeOut = (size_t)64 << 20;        // decode: output per batch where batches are pipelined (plan_batch)
constexpr size_t kPipeMin = kPipeOut + kPipeOut / 2; // ... which takes a caller that offers at least this much room

// bytes one RSI can occupy at most in the stream (every block uncompressed)
inline uint64_t worst_rsi_bytes(const Cfg &c)
{
    return ((uint64_t)c.rsi * (c.id_len + (uint64_t)c.bs * c.bps) + c.bps + 7) / 8 + 1;
}

// What the index pass is told about the coded RSIs: a look-ahead of 1.5 means (the window tables are sized from it) --
// except for RSIs of uncompressed blocks, where the pass is told the mean itself so that it leaves out the schemes that
// look for reference samples (aec_cfg.h: index_incompressible), and a look-ahead that happens to fall into that
// band is moved beyond it.
inline uint64_t index_hint_of(const Cfg &c, uint64_t mean)
{
    if (index_incompressible(c, mean)) return mean;
    const uint64_t h = mean + mean / 2;
    return index_incompressible(c, h) ? (uint64_t)c.rsi * (c.id_len + (uint64_t)c.bs * c.bps) + 65 : h;
}

// Where a decoding stream stands: d_in holds stream bytes [base, base + d_len); all *_bit values are absolute stream bits
struct StreamPos {
    uint64_t base = 0;             // multiple of 16
    size_t d_len = 0;
    uint64_t rsi_start_bit = 0;    // start of the RSI being decoded
    uint64_t rsi_bits_seen = 0;    // average coded RSI of the previous batch (0 = none yet)
    uint64_t walk_bit = 0;         // coded-data-set boundary where the index walker resumes
    uint32_t walk_blocks = 0;      // blocks of that RSI in front of walk_bit
    uint64_t delivered = 0;        // samples of that RSI already handed out
    size_t walked_len = 0;         // d_len at the last index pass (anything beyond it is new)
    uint64_t span_mul = 1;         // widening of the batch's input span (coded data sets beyond the encoder's bound)
    bool span_wide = false;        // pipelined batches: the tight span did not hold once, the worst case from now on
    bool more = false;             // the last batch stopped at its RSI bound: decodable input remains
};

// ---- plan ---------------------------------------------------------------------------------------------------------------
struct BatchPlan {
    uint64_t walk_rel = 0, rsi_rel = 0;   // the walker's resume point and the current RSI's start, in bits from d_in
    size_t skip = 0;                      // bytes of the current RSI already handed out
    uint64_t hint = 0;                    // average coded RSI the index pass is to expect, in bits (0: unknown)
    bool pipe = false;                    // batches of kPipeOut, copies beside the next batch's kernels
    uint64_t max_rsi = 0;                 // RSIs the batch may bring
    size_t in_bytes = 0;                  // the front of the resident stream the batch is given
    bool piece = false;                   // ... which is the tight span: the index pass is told that it sees a piece
    size_t off_bytes = 0, out_bytes = 0, seg_bytes = 0;   // buffers to ensure: RSI starts, output, segment starts (0: none)
};

// Look-ahead of the speculative index = a small multiple of the average coded RSI: measured on the previous batch of
// this stream, else estimated from the room the caller offers for output (whole-buffer callers offer the decoded size).
inline uint64_t plan_hint(const Cfg &c, const StreamPos &p, size_t room)
{
    const size_t rsi_bytes = (size_t)c.rsi * c.bs * c.bytes, skip = (size_t)p.delivered * c.bytes;
    if (p.rsi_bits_seen || room < rsi_bytes) return p.rsi_bits_seen;
    const uint64_t expect = (room + skip + rsi_bytes - 1) / rsi_bytes;
    return ((uint64_t)p.d_len * 8 - (p.rsi_start_bit - p.base * 8)) / expect;
}

// room: the caller's avail_out; windowed: aec_gpu_index_is_windowed for the stream behind the current RSI's start with a
// look-ahead of 1.5 plan_hint (asked only when room >= kPipeMin)
inline BatchPlan plan_batch(const Cfg &c, const StreamPos &p, size_t room, bool windowed)
{
    BatchPlan b;
    const size_t blk_bytes = (size_t)c.bs * c.bytes, rsi_bytes = (size_t)c.rsi * blk_bytes;
    b.walk_rel = p.walk_bit - p.base * 8;
    b.rsi_rel = p.rsi_start_bit - p.base * 8;
    b.skip = (size_t)p.delivered * c.bytes;
    b.hint = plan_hint(c, p, room);
    // Large outputs of streams whose index pass is cheap per call (the window tables): batches of kPipeOut, the copy
    // of one batch to the caller's buffer on a side stream beside the index pass and the decode of the next one (one
    // batch for everything was upload, index, decode, copy one behind the other: 21 GB/s for 256 MiB of config 2
    // against 42 for the encoder).  The trunk index pays too much per call for that (spans, burn-in): one batch.
    b.pipe = room >= kPipeMin && windowed;
    // bound of the batch: the room offered (at least kMinBatchOut), and no more than the input can hold
    const size_t out_room = (b.pipe ? kPipeOut : (room > kMinBatchOut ? room : kMinBatchOut)) + b.skip;
    b.max_rsi = out_room / rsi_bytes + 2;
    const uint64_t min_rsi_bits = (uint64_t)c.segs_per_rsi * (c.id_len + 2) + ((c.flags & F_PREPROCESS) ? c.bps : 0);
    const uint64_t avail_bits = (uint64_t)p.d_len * 8 - b.rsi_rel;
    if (b.max_rsi > avail_bits / min_rsi_bits + 2) b.max_rsi = avail_bits / min_rsi_bits + 2;
    // the part of the resident stream this batch can need
    // (worst_rsi_bytes is what an ENCODER makes of an RSI at most; the format allows longer ones: should the
    // walker run out of input inside the span while more is resident, the next batch looks further)
    uint64_t span = b.walk_rel / 8 + b.max_rsi * worst_rsi_bytes(c) * p.span_mul + 64;
    // (pipelined batches: the tables are built over the whole span, so the worst case -- five times the input a
    // batch of compressible data needs -- would have every batch index most of what is left.  The span is what the
    // batch's RSIs need on average plus the index pass's look-ahead; the pass is told that it sees a piece
    // (aec_gpu_set_index_piece) and stops in front of the RSIs its tables cannot resolve at the end of it -- the next
    // batch's -- instead of walking them serially.)
    if (b.pipe && b.hint && p.span_mul == 1 && !p.span_wide) {
        const uint64_t tight = b.walk_rel / 8 + (b.max_rsi * b.hint + 8 * b.hint) / 8 + 65536;
        if (tight < span && tight < p.d_len) {
            span = tight;
            b.piece = true;
        }
    }
    b.in_bytes = span < p.d_len ? (size_t)span : p.d_len;
    b.off_bytes = (size_t)(b.max_rsi + 2) * 8;
    b.out_bytes = (size_t)b.max_rsi * rsi_bytes + blk_bytes + 64;
    // RSIs of eight segments and more: the index pass also leaves the segment starts, and the decoder takes a lane per
    // segment instead of one per RSI (include/aec_gpu.h: aec_gpu_index_segments_async)
    b.seg_bytes = c.segs_per_rsi >= 8 ? (size_t)(b.max_rsi + 2) * c.segs_per_rsi * 8 : 0;
    return b;
}

// ---- verdict ------------------------------------------------------------------------------------------------------------
struct BatchVerdict {
    size_t total = 0;                     // good output of the batch in bytes, from the start of its first RSI
    uint32_t part = 0;                    // samples released from the coded data set the input ends in
    bool corrupt = false;                 // AEC_DATA_ERROR, once the samples in front of the error are handed out
    bool more_behind = false;             // an error lies behind what this call was asked for: the next call meets it
    uint64_t good_rsi = 0, tail_blocks = 0;          // whole RSIs and blocks of the next one that are good
    uint64_t res_rsi = 0, res_tail = 0, res_end = 0; // where the walker resumes: RSIs and blocks in front of bit res_end
    bool fetch_off = false;               // res_end is entry good_rsi of the batch's RSI starts: the caller fetches it
};

// idx, dec: the records of the index pass and of the decoder; skip as in the plan; want_out: the room THIS call offered
inline BatchVerdict judge_batch(const Cfg &c, const aec_gpu_dec_result &idx, const aec_gpu_dec_result &dec, size_t skip,
                                size_t want_out)
{
    BatchVerdict v;
    // What is good: all of it, or -- when the decoder met a corrupt coded data set the walker could
    // not see (a second-extension code beyond the table, reference decode.c:589-616) -- the RSIs in
    // front of the first bad one; the reference delivers every sample preceding the error as well.
    v.good_rsi = idx.n_rsi;
    v.tail_blocks = idx.tail_blocks;
    v.corrupt = idx.status == DEC_DATA_ERROR;
    if (dec.status != DEC_OK) {
        v.corrupt = true;
        if (dec.bad_rsi <= v.good_rsi) {
            // (the decode record's tail_blocks: the lowest failing block of the batch -- the blocks of its RSI in
            // front of it are decoded and good)
            const uint64_t bad_block = dec.tail_blocks;
            v.good_rsi = dec.bad_rsi;
            v.tail_blocks = (bad_block != ~0ull && bad_block / c.rsi == v.good_rsi) ? bad_block % c.rsi : 0;
        }
    }
    // samples released from the coded data set the input ends in (reference decode.c:423-460)
    v.part = (!v.corrupt && idx.pad == 1) ? (dec.pad & 0x7FFFFFFFu) : 0u;   // (bit 31: slow path ran)
    const uint64_t blocks = v.good_rsi * c.rsi + v.tail_blocks;
    v.total = (size_t)blocks * c.bs * c.bytes + (size_t)v.part * c.bytes;
    // A coded data set that cannot be accepted -- a zero run overrunning its RSI (found by the walker), a
    // second-extension code beyond the table (found by the decoder) -- BEHIND everything this call was asked for is
    // not this call's error: the reference stops when the output is full (decode.c:797-831) and only meets it
    // when it is asked for more, as the next call here will.  The walk then resumes at the coded data set the walker
    // stopped at, or at the start of the RSI the decoder gave up.
    v.res_rsi = idx.n_rsi;
    v.res_tail = idx.tail_blocks;
    v.res_end = idx.end_bit;
    // (a call that offers NO room defers what the walker found -- the reference's m_zero_block only refuses a run when
    // avail_out holds it, decode.c:542-544 -- but not a second-extension code beyond the table, which the reference
    // reports whatever the room, decode.c:589-616)
    if (v.corrupt && v.total >= skip + want_out && (want_out || dec.status == DEC_OK)) {
        v.corrupt = false;
        v.more_behind = true;                               // (the next call that offers room meets the error)
        if (dec.status != DEC_OK) {
            v.fetch_off = true;
            v.res_rsi = v.good_rsi;
            v.res_tail = 0;                                 // (the walker starts the RSI again; its good blocks are `delivered`)
        }
    }
    return v;
}

// ---- advance ------------------------------------------------------------------------------------------------------------
// The walker resumes behind the last complete coded data set.  v: the verdict, res_end complete; idx: the index pass's
// record; tail_start: entry max_rsi of the batch's RSI starts (the start of the trailing partial RSI).  Returns how many
// bytes at the front of the resident stream are consumed and dropped (0: none); p.base and p.d_len say so already, the
// caller moves the p.d_len bytes behind them to the front of d_in.
inline size_t advance_stream(const Cfg &c, StreamPos &p, const BatchPlan &b, const BatchVerdict &v,
                             const aec_gpu_dec_result &idx, uint64_t tail_start)
{
    const uint64_t base_bits = p.base * 8;
    if (v.res_rsi) p.rsi_bits_seen = (v.res_end - b.rsi_rel) / (v.res_rsi + (v.res_tail ? 1 : 0));
    p.walk_bit = base_bits + v.res_end;
    p.walk_blocks = (uint32_t)v.res_tail;
    if (v.res_tail) {
        p.rsi_start_bit = base_bits + tail_start;
        p.delivered = v.res_tail * c.bs + v.part;
    } else {
        p.rsi_start_bit = p.walk_bit;
        p.delivered = v.fetch_off ? v.tail_blocks * c.bs : v.part;
    }
    p.walked_len = b.in_bytes;
    // (the walker ran out of input inside the span although more is resident: first the worst case instead of the
    // tight span of the pipelined batches, then wider and wider)
    if (idx.pad == 1 && b.in_bytes < p.d_len) {
        if (b.piece && !p.span_wide) p.span_wide = true;
        else p.span_mul = p.span_mul < (1u << 20) ? p.span_mul * 4 : p.span_mul;
    } else {
        p.span_mul = 1;
    }
    // stopped at the bound with input left: the caller's next call (or this one, if it still has
    // room) goes on from here
    p.more = idx.n_rsi >= b.max_rsi || b.in_bytes < p.d_len || v.more_behind;

    // drop the consumed front of the resident stream once it is the larger part (the copy must not overlap)
    const uint64_t keep_from = (p.rsi_start_bit / 8 - p.base) & ~(uint64_t)15;
    const size_t rem = p.d_len - (size_t)keep_from;
    if (keep_from < rem || keep_from < 4096) return 0;
    p.base += keep_from;
    p.d_len = rem;
    p.walked_len = p.walked_len > keep_from ? p.walked_len - (size_t)keep_from : 0;
    return (size_t)keep_from;
}

}  // namespace aec
