// bsmall_emul.cpp -- the every-bit index scheme over a BATCH of bare streams (libaec_amd/csrc/aec_bsmall.h; aec_idx.hip:
// launch_index_chunks) on the CPU: the plan, the slots and rounds, and per round what the launches compute entry by
// entry -- the parses, the hops, the walk of one RSI from every bit, the doubling round by round for the streams that
// still need it, the verdict -- with the functions the kernels call.
// (test infrastructure; built by tests/test_bsmall_emul.py)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../libaec_amd/csrc/aec_cfg.h"
#include "../../libaec_amd/csrc/aec_bsmall.h"

using namespace aec;

extern "C" uint32_t emul_bsmall_slot_len(uint64_t nbits) { return bs_slot_len(nbits); }
extern "C" uint64_t emul_bsmall_round_bits(uint64_t asked) { return bs_round_bits(asked); }
extern "C" int emul_bsmall_within(const uint32_t *prm, uint64_t in_bytes, uint64_t round_bits)
{
    Cfg c;
    if (make_cfg(prm[0], prm[1], prm[2], prm[3], 0, false, &c) != RC_OK) return -1;
    return bs_within(c, in_bytes, bs_round_bits(round_bits)) ? 1 : 0;
}
extern "C" uint32_t emul_bsmall_consts(int which) { return which == 0 ? kBsB0 : kBsR; }

// plan_out[6]: taken, rounds, table_bits, workspace bytes, block threshold, unit-table entries
extern "C" int emul_bsmall_plan(const uint32_t *prm, int how, uint64_t round_bits, const uint64_t *in_bytes, const uint64_t *out_bytes,
                                uint64_t n, uint64_t *plan_out)
{
    Cfg c;
    if (make_cfg(prm[0], prm[1], prm[2], prm[3], 0, false, &c) != RC_OK) return -1;
    BsPlan p;
    bs_plan(c, how, round_bits, in_bytes, out_bytes, n, &p);
    plan_out[0] = p.taken;
    plan_out[1] = p.rounds;
    plan_out[2] = p.table_bits;
    plan_out[3] = p.bytes;
    plan_out[4] = p.min_blocks;
    plan_out[5] = p.units;
    return 0;
}

// The pass over buf (nbytes; streams of in_bytes[i] bytes at in_off[i], announcing out_bytes[i] bytes of samples).
// table: the RSI table (sum of rsis_i + 1 entries; only what a delivered stream owns is written);
// rec[4 i ..]: delivered, n_rsi, tail_blocks, end_bit of stream i (delivered 0: left to the serial walker);
// slots_out[4 k ..] (optional): chunk, t0, len, levels of taken stream k;  plan_out as above.
extern "C" int emul_bsmall(const uint32_t *prm, const uint8_t *buf, size_t nbytes, const uint64_t *in_off, const uint64_t *in_bytes,
                           const uint64_t *out_bytes, uint64_t n, int how, uint64_t round_bits, uint64_t *table, uint64_t *rec,
                           uint64_t *slots_out, uint64_t *plan_out)
{
    Cfg c;
    if (make_cfg(prm[0], prm[1], prm[2], prm[3], 0, false, &c) != RC_OK) return -1;
    std::vector<uint8_t> in(nbytes + 64, 0);
    memcpy(in.data(), buf, nbytes);
    const uint32_t *words = reinterpret_cast<const uint32_t *>(in.data());
    const uint64_t nwords = (nbytes + 3) / 4;

    BsPlan p;
    bs_plan(c, how, round_bits, in_bytes, out_bytes, n, &p);
    emul_bsmall_plan(prm, how, round_bits, in_bytes, out_bytes, n, plan_out);
    for (uint64_t i = 0; i < 4 * n; i++) rec[i] = 0;
    if (!p.taken) return 0;
    std::vector<BsSlot> slots(p.taken);
    std::vector<BsRound> rounds(p.rounds);
    std::vector<uint32_t> units(p.units);
    BsPlan again;
    bs_pack(c, bs_round_bits(round_bits), in_off, in_bytes, out_bytes, n, p.min_blocks, &again, slots.data(), rounds.data(), units.data());
    if (again.taken != p.taken || again.rounds != p.rounds || again.units != p.units) return -2;
    std::vector<uint64_t> item0(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) item0[i + 1] = item0[i] + dchunk_counts(out_bytes[i], c.bytes, c.bs, c.rsi).rsis;

    // the round's tables, as the workspace lays them out: filled with a pattern between rounds so that nothing a round
    // reads can be what the round before left
    std::vector<uint16_t> e(2 * p.table_bits);
    std::vector<uint32_t> ja(p.table_bits), hop(p.table_bits), sidx(p.chain);
    const bool hops = c.rsi > kBsHopRsi;
    for (uint64_t r = 0; r < p.rounds; r++) {
        const BsRound &rd = rounds[r];
        if (rd.entries % kBsUnit || rd.entries > bs_round_bits(round_bits)) return -3;
        std::fill(e.begin(), e.end(), (uint16_t)0xA5A5);
        std::fill(ja.begin(), ja.end(), 0x5A5A5A5Au);
        std::fill(hop.begin(), hop.end(), 0x5A5A5A5Au);
        std::fill(sidx.begin(), sidx.end(), 0x5A5A5A5Au);
        uint16_t *e0 = e.data(), *e1 = e.data() + p.table_bits;
        const uint32_t *un = units.data() + rd.unit0;
        auto slot_of = [&](uint32_t at) -> const BsSlot & { return slots[un[at / kBsUnit]]; };
        for (uint32_t at = 0; at < rd.entries; at++) {
            const BsSlot &sl = slot_of(at);
            if (at < sl.t0 || at - sl.t0 >= sl.len || sl.t0 % kBsUnit || sl.len % kBsUnit || sl.len <= sl.nbits) return -4;
            if (at - sl.t0 <= sl.nbits) bs_parse_entry(c, words, nwords, sl, at - sl.t0, e0, e1);
        }
        if (hops)
            for (uint32_t at = 0; at < rd.entries; at++) {
                const BsSlot &sl = slot_of(at);
                const uint16_t *s0 = e0 + sl.t0;
                if (at - sl.t0 <= sl.nbits) hop[at] = sm_hop(c, [&](uint32_t q) { return (uint32_t)s0[q]; }, at - sl.t0, sl.nbits);
            }
        for (uint32_t at = 0; at < rd.entries; at++) {
            const BsSlot &sl = slot_of(at);
            const uint32_t q = at - sl.t0;
            const uint16_t *s0 = e0 + sl.t0, *s1 = e1 + sl.t0;
            const uint32_t *sh = hop.data() + sl.t0;
            bs_chain_init(sl, q, sidx.data());
            if (q > sl.nbits) continue;
            ja[at] = sm_rsi(c, [&](uint32_t x) { return (uint32_t)s0[x]; }, [&](uint32_t x) { return (uint32_t)s1[x]; },
                            [&](uint32_t x) { return sh[x]; }, hops, [&](uint32_t) { return 0u; }, false, q, sl.nbits, 0u, bs_pad(c));
        }
        // (from here the parses are dead: the second table of the doubling lies over them)
        uint32_t *over = reinterpret_cast<uint32_t *>(e.data());
        for (uint32_t k = 0; k < rd.levels; k++)
            for (uint32_t at = 0; at < rd.entries; at++) {
                const BsSlot &sl = slot_of(at);
                bs_double_entry(sl, k, at - sl.t0, (k & 1u) ? over : ja.data(), (k & 1u) ? ja.data() : over, sidx.data());
            }
        for (uint64_t k = 0; k < rd.nslots; k++) {
            const BsSlot &sl = slots[rd.slot0 + k];
            uint32_t m = 0;
            while (m < sl.scap && sidx[sl.s0 + m] != kSmNone) m++;
            const BsVerdict v = bs_finish(c, MemFetch{words, nwords}, sl, sidx.data(), m);
            uint64_t *out = rec + 4 * sl.chunk;
            out[0] = v.delivered;
            if (!v.delivered) continue;
            if (v.nout > (uint64_t)sl.rsis + 1u) return -5;
            out[1] = v.n_rsi;
            out[2] = v.tail_blocks;
            out[3] = v.end_bit;
            for (uint64_t i = 0; i < v.nout; i++) table[item0[sl.chunk] + sl.chunk + i] = 8u * sl.in_off + sidx[sl.s0 + i];
        }
    }
    if (slots_out)
        for (uint64_t k = 0; k < p.taken; k++) {
            slots_out[4 * k] = slots[k].chunk;
            slots_out[4 * k + 1] = slots[k].t0;
            slots_out[4 * k + 2] = slots[k].len;
            slots_out[4 * k + 3] = slots[k].levels;
        }
    return 0;
}
