// aec_bsmall.h -- the every-bit index scheme (aec_small.h) over a BATCH of bare streams (aec_idx.hip: launch_index_chunks;
// DESIGN.md §2 "small streams, a batch of them"): which streams of a batch of unequal chunks the scheme takes, how their
// per-bit tables share one set of launches, and what one table entry of each launch computes.  The per-bit arithmetic is
// that of aec_small.h, called as it is; this header adds the places: a stream's SLOT in the tables, its chain, its
// verdict.  The functions are __host__ __device__: the kernels call them and tests/emul/bsmall_emul.cpp runs the same
// functions on the CPU.
//
// Slots.  A stream of nbits bits has nbits + 1 table entries (entry q: the bit q behind the stream's first; entry nbits:
// "the input ends here").  Its slot is those entries rounded up to kBsUnit = 1024, the width of the widest kernel's
// workgroup (kSmRsiWg), so that every workgroup of every kernel lies inside ONE stream: what a workgroup stages in LDS,
// and the bound it walks to, are one stream's.  How a workgroup finds its stream: a table of one uint32_t (slot number)
// per 1024 entries, written by the host with the slots -- the reasoning of aec_dchunks.h for item_chunk: 4 bytes per 1024
// entries of 8 .. 12 bytes each against log2(n) dependent loads in front of every lane's first read.
// Positions in the tables are relative to the stream's first bit; the parse reads the shared buffer at absolute bits
// with the stream's OWN end bound, so no bit of a neighbour that begins on the next byte is ever taken for its own.
//
// Rounds.  The tables cost 8 bytes per entry (12 where c.rsi > kBsHopRsi: the hops), so the batch is cut into rounds of
// whole streams, in the order of the chunks, whose slots fit round_bits entries; the rounds use the same tables one
// after the other, their launches are enqueued at once.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "aec_dchunks.h"
#include "aec_small.h"

namespace aec {

constexpr uint32_t kBsUnit = 1024;                 // entries a slot is a multiple of (= kSmRsiWg)
constexpr uint64_t kBsMinBits = 64;                // streams the scheme takes: at least ...
constexpr uint64_t kBsMaxBits = 1ull << 24;        // ... and at most this many bits (= kSmMaxBits: no pieces here)
constexpr uint32_t kBsMaxRsi = 256;                // ... with RSIs of at most this many blocks (no hops of hops here)
constexpr uint32_t kBsHopRsi = 16;                 // RSIs of more blocks walk through the table of hops
constexpr uint64_t kBsRoundBits = 1ull << 24;      // default budget of a round, in table entries
constexpr uint64_t kBsMinRoundBits = 4096;
// Where the scheme runs when the caller leaves it to the plan (BS_PLANNED), by measurement (MI355X,
// profiles/r18/bench_index_chunks.txt; tests/bench_index_chunks.py, --sweep for the first two groups of rows).
// What the rows say: the serial walk costs what its LONGEST stream costs, however many streams there are -- a wavefront
// per stream, 0.4 (8-bit samples in blocks of 8) to 0.58 us (16-bit in blocks of 16) per block:
//     16 chunks of 4 to 128 KiB, 8 / 8 / 128      walk  6.4 ms   (longest: 16 384 blocks)      every bit 0.53 ms
//     1024 such chunks                            walk  6.5 ms   (the same longest stream)     every bit 17.6 ms
//     64 x 1 MiB                                  walk 51.5 ms                                 every bit 16.3 ms
// and the every-bit scheme what ALL the bits it takes cost, 0.085 to 0.096 ns per bit (24.5 MiB of stream: 17.6 ms; the
// supposition of 2 to 3 ms for them did not hold), and 0.05 to 0.1 ms per round beside that:
//     1024 chunks, 16-bit, in 6 / 9 / 17 / 33 rounds:   9.3 / 10.0 / 12.2 / 16.5 ms
// So the scheme pays where FEW streams are long -- 16 chunks: 12 times faster, 64 x 1 MiB: 3 times -- and never where
// hundreds are about as long as the longest (256 equal chunks, 32 to 4096 blocks each: 1.1 to 3.5 times the walk's time;
// below 128 blocks 2.7 times and more).  The plan therefore weighs the two times against each other, in these terms:
constexpr uint32_t kBsB0 = 128;                    // a stream of fewer blocks is never taken (256 chunks of 64 blocks: 3.1 .. 3.5 x the walk)
constexpr uint32_t kBsR = 16;                      // rounds at the most (64 x 1 MiB of 8-bit data make 13; 33 rounds cost 1.25 .. 1.8 x 13 / 6)
constexpr uint64_t kBsWalkNsPerBlock = 400;        // the walk: ns per block of the longest stream it is left with (the lower figure)
constexpr uint64_t kBsBitsPerNs = 10;              // the every-bit scheme: 0.1 ns per bit taken (the higher figure, rounded up) ...
constexpr uint64_t kBsRoundNs = 100000;            // ... per round ...
constexpr uint64_t kBsFixedNs = 100000;            // ... and per pass (slots and unit table sent, flags cleared)

enum : int { BS_PLANNED = 0, BS_SERIAL = 1, BS_EVERY_BIT = 2 };

// A taken stream's place (host-written, uploaded with the unit table).
struct BsSlot {
    uint64_t in_off;     // the stream's first byte in d_in
    uint32_t chunk;      // its number in the batch
    uint32_t t0;         // first entry of its slot in the round's tables (a multiple of kBsUnit)
    uint32_t nbits;      // its bits
    uint32_t len;        // entries of its slot (a multiple of kBsUnit, > nbits)
    uint32_t s0;         // first entry of its chain in the round's chain area
    uint32_t scap;       // capacity of the chain: 4^levels
    uint32_t levels;     // doubling rounds it needs
    uint32_t rsis;       // RSIs the chunk announces
};
struct BsRound {
    uint64_t slot0, nslots;   // its slots: slot0 .. slot0 + nslots - 1 of the batch's
    uint64_t unit0;           // its first entry in the unit table
    uint32_t entries;         // table entries (a multiple of kBsUnit)
    uint32_t chain;           // chain entries
    uint32_t levels;          // the most doubling rounds of a stream in it
    uint32_t pad;
};

AEC_HD uint64_t bs_round_bits(uint64_t asked)
{
    if (asked == 0 || asked > kBsRoundBits) return kBsRoundBits;
    return asked < kBsMinRoundBits ? kBsMinRoundBits : asked;
}
AEC_HD uint32_t bs_slot_len(uint64_t nbits) { return (uint32_t)((nbits + 1u + kBsUnit - 1u) & ~(uint64_t)(kBsUnit - 1u)); }

// rounds of the doubling a stream needs: its chain holds the starts the chunk announces and the one behind them --
// or, where the chunk announces more than the stream has bits for, what the bits can hold at most (aec_idx.hip: small_plan)
AEC_HD uint32_t bs_levels(const Cfg &c, uint64_t nbits, uint64_t rsis)
{
    const uint64_t min_rsi_bits = (uint64_t)c.segs_per_rsi * (c.id_len + 2u) + ((c.flags & F_PREPROCESS) ? c.bps : 0u);
    uint64_t most = nbits / min_rsi_bits + 2u;
    if (most > rsis + 1u) most = rsis + 1u;
    uint32_t levels = 0;
    while ((1ull << (2u * levels)) < most) levels++;
    return levels;
}

// the scheme's LIMITS: what it can take at all (a slot must fit a round)
AEC_HD bool bs_within(const Cfg &c, uint64_t in_bytes, uint64_t round_bits)
{
    const uint64_t nbits = in_bytes * 8u;
    return in_bytes < (1ull << 32) && nbits >= kBsMinBits && nbits <= kBsMaxBits && c.rsi <= kBsMaxRsi && bs_slot_len(nbits) <= round_bits;
}

struct BsPlan {
    uint64_t taken, rounds, units;      // streams taken, rounds, entries of the unit table (all rounds)
    uint64_t table_bits, chain;         // entries of the largest round's tables / of the largest chain area
    uint64_t min_blocks;                // the block threshold the plan settled on
    uint64_t bits, walk_blocks;         // bits of the streams taken; blocks of the longest stream left to the walker
    size_t o_slots, o_units, o_flags, o_e, o_ja, o_hop, o_sidx, bytes;      // the workspace
};

// One pass over the chunks: the streams with at least min_blocks blocks within the limits, packed into rounds in the
// order of the chunks.  slots / rounds / units: written where not null (the counts of a pass without them size them).
inline void bs_pack(const Cfg &c, uint64_t round_bits, const uint64_t *in_offsets, const uint64_t *in_bytes_each, const uint64_t *out_bytes,
                    uint64_t n, uint64_t min_blocks, BsPlan *p, BsSlot *slots, BsRound *rounds, uint32_t *units)
{
    uint64_t taken = 0, nrounds = 0, nunits = 0, most_entries = 0, most_chain = 0, bits = 0, walk_blocks = 0;
    BsRound cur{};
    auto close = [&]() {
        if (!cur.nslots) return;
        if (rounds) rounds[nrounds] = cur;
        nrounds++;
        if (cur.entries > most_entries) most_entries = cur.entries;
        if (cur.chain > most_chain) most_chain = cur.chain;
    };
    for (uint64_t i = 0; i < n; i++) {
        const DChunkCounts k = dchunk_counts(out_bytes[i], c.bytes, c.bs, c.rsi);
        if (k.blocks < min_blocks || !bs_within(c, in_bytes_each[i], round_bits)) {
            if (k.blocks > walk_blocks) walk_blocks = k.blocks;
            continue;
        }
        const uint32_t nbits = (uint32_t)(in_bytes_each[i] * 8u), len = bs_slot_len(nbits);
        const uint32_t levels = bs_levels(c, nbits, k.rsis), scap = 1u << (2u * levels);
        if ((uint64_t)cur.entries + len > round_bits || (uint64_t)cur.chain + scap > 0xFFFFFFFFull) {
            close();
            cur = BsRound{taken, 0, nunits, 0u, 0u, 0u, 0u};
        }
        if (slots)
            slots[taken] = BsSlot{in_offsets ? in_offsets[i] : 0u, (uint32_t)i, cur.entries, nbits, len, cur.chain, scap, levels, (uint32_t)k.rsis};
        if (units)
            for (uint32_t u = 0; u < len / kBsUnit; u++) units[nunits + u] = (uint32_t)taken;
        nunits += len / kBsUnit;
        bits += nbits;
        cur.entries += len;
        cur.chain += scap;
        cur.nslots++;
        if (levels > cur.levels) cur.levels = levels;
        taken++;
    }
    close();
    p->taken = taken;
    p->rounds = nrounds;
    p->units = nunits;
    p->table_bits = most_entries;
    p->chain = most_chain;
    p->min_blocks = min_blocks;
    p->bits = bits;
    p->walk_blocks = walk_blocks;
}

// what the plan expects a pass to take, in ns (the constants above)
inline uint64_t bs_cost_ns(const BsPlan &p)
{
    return (p.taken ? kBsFixedNs + p.rounds * kBsRoundNs + p.bits / kBsBitsPerNs : 0u) + p.walk_blocks * kBsWalkNsPerBlock;
}

// The plan of a batch: how = BS_SERIAL takes none, BS_EVERY_BIT every stream within the limits.  BS_PLANNED takes the
// streams within the limits that announce at least T blocks, for the T among kBsB0, 4 kBsB0, 16 kBsB0, ... whose pass is
// expected to be the shortest (bs_cost_ns: the every-bit scheme's time for the bits taken and the walk's for the longest
// stream left) among those of at most kBsR rounds -- and none where no such pass is expected to beat the walk alone.
// O(n) per T, at most 64 of them, deterministic.
inline void bs_plan(const Cfg &c, int how, uint64_t round_bits_asked, const uint64_t *in_bytes_each, const uint64_t *out_bytes, uint64_t n,
                    BsPlan *p)
{
    const uint64_t round_bits = bs_round_bits(round_bits_asked);
    *p = BsPlan{};
    if (how == BS_EVERY_BIT) {
        bs_pack(c, round_bits, nullptr, in_bytes_each, out_bytes, n, 0, p, nullptr, nullptr, nullptr);
    } else if (how == BS_PLANNED) {
        uint64_t most_blocks = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t blocks = dchunk_counts(out_bytes[i], c.bytes, c.bs, c.rsi).blocks;
            if (blocks > most_blocks) most_blocks = blocks;
        }
        uint64_t best_t = 0, best_ns = most_blocks * kBsWalkNsPerBlock;          // (the walk alone)
        // (a walk as short as one round of the scheme is not weighed at all: the passes over the chunks are host time in
        // front of every call -- 4000 chunks below 4 KiB: 0.03 ms on a call of 0.33 ms)
        for (uint64_t t = kBsB0; best_ns > kBsFixedNs + kBsRoundNs && t <= most_blocks && t; t *= 4u) {
            BsPlan q{};
            bs_pack(c, round_bits, nullptr, in_bytes_each, out_bytes, n, t, &q, nullptr, nullptr, nullptr);
            if (q.taken && q.rounds <= kBsR && bs_cost_ns(q) < best_ns) {
                best_ns = bs_cost_ns(q);
                best_t = t;
            }
        }
        if (best_t) bs_pack(c, round_bits, nullptr, in_bytes_each, out_bytes, n, best_t, p, nullptr, nullptr, nullptr);
    }
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    p->o_flags = o;  o = up(o + (size_t)(n ? n : 1) * 4);
    p->o_slots = o;  o = up(o + (size_t)p->taken * sizeof(BsSlot));
    p->o_units = o;  o = up(o + (size_t)p->units * 4);
    p->o_e = o;      o = up(o + (size_t)p->table_bits * 4);     // both parses of an entry; the second table of the doubling
    p->o_ja = o;     o = up(o + (size_t)p->table_bits * 4);
    p->o_hop = o;
    if (c.rsi > kBsHopRsi) o = up(o + (size_t)p->table_bits * 4);
    p->o_sidx = o;   o = up(o + (size_t)p->chain * 4);
    p->bytes = o;
}

// ---- what one table entry of each launch computes (q: the entry within the slot) -----------------------------------------
AEC_HD TrStream bs_stream(const uint32_t *words, uint64_t nwords, const BsSlot &sl)
{
    return TrStream{words, nwords, 8u * sl.in_off + sl.nbits};
}

// step 1: both parses of the coded data set that would begin at bit q of the stream
AEC_HD void bs_parse_entry(const Cfg &c, const uint32_t *words, uint64_t nwords, const BsSlot &sl, uint32_t q, uint16_t *e0, uint16_t *e1)
{
    uint16_t a = 0, b = 0;
    if (q < sl.nbits) sm_parse(bs_stream(words, nwords, sl), c, 8u * sl.in_off + q, a, b);
    e0[sl.t0 + q] = a;
    e1[sl.t0 + q] = b;
}

// AEC_PAD_RSI: a stream begins on a byte, so the RSIs behind the first begin on multiples of 8 of its own bits
AEC_HD uint32_t bs_pad(const Cfg &c) { return (c.flags & F_PAD_RSI) ? 1u : 0u; }

// the chain starts empty but for the stream's first bit; entry i of it and every sl.len-th behind it are this lane's
AEC_HD void bs_chain_init(const BsSlot &sl, uint32_t q, uint32_t *sidx)
{
    for (uint32_t i = q; i < sl.scap; i += sl.len) sidx[sl.s0 + i] = i ? kSmNone : 0u;
}

// step 3, round k, for the streams that still double
AEC_HD void bs_double_entry(const BsSlot &sl, uint32_t k, uint32_t q, const uint32_t *j, uint32_t *jn, uint32_t *sidx)
{
    if (k >= sl.levels) return;
    const uint32_t quarter = 1u << (2u * k);
    for (uint32_t i = q; i < quarter; i += sl.len) sm_double_starts(j + sl.t0, sidx + sl.s0, i, quarter, sl.scap);
    if (k + 1u < sl.levels && q <= sl.nbits) jn[sl.t0 + q] = sm_double_table(j + sl.t0, q);
}

// step 4: the verdict on a stream from its chain.  m: starts on the chain (the first entry of sidx that is kSmNone, scap
// where there is none).  Delivered is what the serial walker would write (aec_idx.hip: k_index, the streams branch):
//  * the chain reaches the start of RSI `rsis`: all announced RSIs are there, the record ends on that start;
//  * it ends earlier: the RSI it ends in is walked as the walker walks it, and only "the input ends inside a coded data
//    set" -- a stream shorter than announced, a short last RSI -- is this scheme's to report.  Anything else (a coded
//    data set that does not parse, a run that does not fit, a chain without an end) leaves the stream alone.
struct BsVerdict {
    uint32_t delivered;
    uint64_t nout;                      // table entries to write: the chain's first nout starts
    uint64_t n_rsi, tail_blocks, end_bit;
};
template <class Fetch>
AEC_HD BsVerdict bs_finish(const Cfg &c, const Fetch &f, const BsSlot &sl, const uint32_t *sidx, uint32_t m)
{
    BsVerdict v{};
    const uint64_t start = 8u * sl.in_off, end = start + sl.nbits;
    const uint32_t *s = sidx + sl.s0;
    if (m == 0u) return v;
    if (m > sl.rsis) {
        v.delivered = 1u;
        v.nout = sl.rsis;
        v.n_rsi = sl.rsis;
        v.tail_blocks = 0;
        v.end_bit = start + s[sl.rsis];
        return v;
    }
    if (m >= sl.scap) return v;
    const uint64_t pos0 = start + s[m - 1u];
    BitReaderT<Fetch> br;
    br.init(f, end, pos0);
    uint32_t b = 0, st = DEC_OK;
    uint64_t good = pos0;
    while (b < c.rsi) {
        uint32_t nblk = 1;
        st = skip_cds(br, c, (b == 0u && (c.flags & F_PREPROCESS)) ? 1u : 0u, b, nblk);
        if (st != DEC_OK) break;
        good = br.pos;
        b += nblk;
    }
    if (st != DEC_NEED_INPUT) return v;
    v.delivered = 1u;
    v.nout = m;
    v.n_rsi = m - 1u;
    v.tail_blocks = b;
    v.end_bit = good;
    return v;
}

}  // namespace aec
