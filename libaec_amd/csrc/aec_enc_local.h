// aec_enc_local.h -- the encoder route that codes every block ONCE (aec_enc.hip k_encode_local / k_encode_redo / k_place):
// the arithmetic the three kernels share with the host and with tests/emul/enc_local_emul.cpp.
//
// A wavefront owns a run of consecutive segments (segs_per_wave of them).  k_encode_local analyses each segment and
// emits it straight away, from the block in the lane's registers, into the wavefront's own SLOT of a workspace area:
// the run's bit string from bit 0 of the slot on, words in native order (bit p of the string is bit 31 - p % 32 of
// word p / 32).  Two things it cannot know then:
//   where the run starts in the stream  -- the scan tells; k_place copies the slot to its place, shifted by the start
//                                          bit's position inside a 32-bit word;
//   the k carried into the run          -- it GUESSES (local_guess); a block's coded length never depends on the carried k
//                                          (the plateau of assess_split_with), only its content, so the layout of the
//                                          slot is right whatever the guess; per segment it leaves the k it used and the
//                                          own clamp of the segment's first k-updating block, and k_encode_redo codes
//                                          the segments from the first to the last miss of a run again with the scan's
//                                          k, where local_missed says a block got another k than the true one.
// No wavefront waits for another one anywhere: a slot has one writer, the stream words two runs share are zeroed by the
// scan and taken by atomic OR (the rules of k_pack's copy-out).
#pragma once
#include <stdint.h>

#include "aec_lane.h"

namespace aec {

// ---- slot geometry -----------------------------------------------------------------------------------------------------
// worst case of one coded block (make_geom's bound: no option is longer) and of a segment: 64 blocks, or all the blocks
// of an RSI shorter than that
AEC_HD uint32_t local_block_bits(uint32_t id_len, uint32_t bs, uint32_t bps) { return id_len + bs * bps + 2u + bps; }
AEC_HD uint32_t local_seg_bits(uint32_t id_len, uint32_t bs, uint32_t bps, uint32_t rsi)
{
    return (rsi < 64u ? rsi : 64u) * local_block_bits(id_len, bs, bps);
}
// words between the slots of two wavefronts: segs_per_wave worst-case segments, rounded up to 128 bytes
AEC_HD uint32_t local_slot_words(uint32_t id_len, uint32_t bs, uint32_t bps, uint32_t rsi, uint32_t segs_per_wave)
{
    const uint32_t bits = segs_per_wave * local_seg_bits(id_len, bs, bps, rsi);
    return ((bits + 31u) / 32u + 31u) & ~31u;
}

// ---- the guess and the test for a miss ---------------------------------------------------------------------------------
// What a segment leaves for the test: the k carried into it as the kernel had it, and the own clamp (lo | hi << 8) of
// its first block that updates k.  A segment without such a block (zero blocks, zero-run continuations, id_len 1)
// reads no k at all: kLocalNoClamp, which maps every k to 0.
static const uint32_t kLocalNoClamp = 0u;
static const uint32_t kLocalGuessRule = 0xFFFFFFFFu;     // `fixed` of local_guess: no forced value

// the k assumed in front of a run whose first k-updating block has the plateau [lo, hi]: its lower end (a count on
// 64 MiB of the bench generator's 16-bit data gave 3.8 % of the runs missing with lo and 4.5 % with hi; what the misses
// cost on the device is in profiles/r11)
AEC_HD uint32_t local_guess(uint32_t first_clamp, uint32_t fixed)
{
    if (fixed != kLocalGuessRule) return fixed > 31u ? 31u : fixed;
    return first_clamp & 0xFFu;
}

AEC_HD uint32_t local_clamp1(uint32_t first_clamp, uint32_t k)
{
    return kclamp_apply(KClamp{first_clamp & 0xFFu, (first_clamp >> 8) & 0xFFu}, k);
}
// Some block of the segment got another k than the true carry gives it.  Exact both ways: the first k-updating block's k
// is one clamp of the carried k, every later block's k follows from that block's k alone, and the blocks in front of
// it read none.
AEC_HD bool local_missed(uint32_t first_clamp, uint32_t k_used, uint32_t k_true)
{
    return local_clamp1(first_clamp, k_used) != local_clamp1(first_clamp, k_true);
}

// ---- coding a run again ----------------------------------------------------------------------------------------------------
// `missed`: bit i = segment i of the run missed (not 0).  Only the segments from the first to the last miss are coded
// again: as a rule the first k-updating block behind a miss has a plateau of one k and the carry is the true one from
// there on.  The scan has the positions by then; the bits in front of the first segment and behind the last one are in
// the slot, in the words the range shares with them.
struct LocalRedo {
    uint32_t first, end;      // segments [first, end) of the run
};
AEC_HD LocalRedo local_redo_range(uint64_t missed)
{
    LocalRedo r;
    r.first = 0;
    while (!((missed >> r.first) & 1u)) r.first++;
    r.end = 64;
    while (!((missed >> (r.end - 1u)) & 1u)) r.end--;
    return r;
}
// the open word in front of a segment that starts at bit `pos` of the slot: the bits of `word` (slot word pos / 32)
// that belong to the segments in front
AEC_HD uint32_t local_redo_head(uint32_t word, uint32_t pos)
{
    return (pos & 31u) ? word & ~(0xFFFFFFFFu >> (pos & 31u)) : 0u;
}
// the last word of the range, which ends `tail` (1..31) bits into it: the new bits and, behind them, what the slot held
AEC_HD uint32_t local_redo_tail(uint32_t fresh, uint32_t old, uint32_t tail)
{
    return fresh | (old & (0xFFFFFFFFu >> tail));
}

// ---- placement -----------------------------------------------------------------------------------------------------------
// A run of `bits` > 0 bits that starts at stream bit `start`: the stream words it touches and which of them it shares.
struct LocalSpan {
    uint64_t word0;       // first stream word
    uint32_t lead;        // start & 31
    uint32_t nwords;      // stream words touched
    uint32_t nslot;       // slot words that hold bits of the run (the words behind them are stale)
    bool head_shared;     // word0 also holds bits in front of the run
    bool tail_shared;     // the last word also holds bits behind the run (or the stream's zero padding)
};
AEC_HD LocalSpan local_span(uint64_t start, uint64_t bits)
{
    LocalSpan s;
    s.word0 = start >> 5;
    s.lead = (uint32_t)(start & 31u);
    s.nwords = (uint32_t)((s.lead + bits + 31u) >> 5);
    s.nslot = (uint32_t)((bits + 31u) >> 5);
    s.head_shared = s.lead != 0;
    s.tail_shared = ((s.lead + bits) & 31u) != 0;
    return s;
}
// stream word j of the span (native order) from slot words j - 1 and j (0 where there is none)
AEC_HD uint32_t local_word(const LocalSpan &s, uint32_t before, uint32_t at)
{
    return s.lead ? (before << (32u - s.lead)) | (at >> s.lead) : at;
}
// the word goes in by atomic OR (into a word the scan zeroed) and not by a plain store
AEC_HD bool local_word_shared(const LocalSpan &s, uint32_t j)
{
    return (j == 0 && s.head_shared) || (j + 1 == s.nwords && s.tail_shared);
}

}  // namespace aec
