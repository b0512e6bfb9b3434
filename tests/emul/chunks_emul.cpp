// chunks_emul.cpp -- the segmented three-phase scan of a batch of unequal chunks (libaec_amd/csrc/aec_chunks.h;
// aec_enc.hip: k_chunks_reduce / k_chunks_bases / k_chunks_apply) on the CPU: the same per-thread functions over the same
// tiles of kTile segments and the same 256 threads of 8 items, with the workgroup scan between them replaced by a loop
// over the threads in order.
// (test infrastructure; built by tests/test_encode_chunks_scan.py)
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../libaec_amd/csrc/aec_chunks.h"

using namespace aec;

namespace {
constexpr uint64_t kThreads = 256, kItems = 8, kTile = kThreads * kItems;

struct ThreadSpan {
    uint64_t s0, s1;
};
ThreadSpan span_of(uint64_t tile, uint64_t t, uint64_t nseg)
{
    const uint64_t tile0 = tile * kTile, tile_end = tile0 + kTile < nseg ? tile0 + kTile : nseg;
    uint64_t s0 = tile0 + t * kItems, s1 = s0 + kItems;
    if (s0 > tile_end) s0 = tile_end;
    if (s1 > tile_end) s1 = tile_end;
    return ThreadSpan{s0, s1};
}
// exclusive prefixes of the threads' aggregates and their total: what block_excl_scan_ck returns
CkVal excl_scan(const std::vector<CkVal> &agg, std::vector<CkVal> &excl)
{
    CkVal run = ck_identity();
    excl.resize(agg.size());
    for (size_t t = 0; t < agg.size(); t++) {
        excl[t] = run;
        run = ck_then(run, agg[t]);
    }
    return run;
}
}  // namespace

// samples[n]: whole samples per chunk; seg_bits / seg_clamp: one entry per segment of the concatenated numbering.
// Out: chunk_base[n], chunk_bits[n], seg_start / seg_kin per segment, rsi_table (sum of rsi_count + 1 entries),
// wave_chunk (one entry per wave), zeroed[]: 1 for every 32-bit output word below cap_words that phase 3 clears,
// empty_byte[n]: the byte phase 2 clears for an empty chunk (~0 for the others).  Returns the segments, -1 on misuse.
extern "C" long long emul_chunks(uint32_t bs, uint32_t rsi, uint32_t spw, const uint64_t *samples, uint64_t n,
                                 const uint32_t *seg_bits, const uint16_t *seg_clamp, uint64_t nseg_given,
                                 uint64_t *chunk_base, uint64_t *chunk_bits, uint64_t *seg_start, uint8_t *seg_kin,
                                 uint64_t *rsi_table, uint64_t n_entries, uint32_t *wave_chunk, uint64_t n_waves,
                                 uint8_t *zeroed, uint64_t cap_words, uint64_t *empty_byte, uint64_t *total_bytes)
{
    const uint32_t segs_per_rsi = (rsi + 63) / 64;
    std::vector<ChunkDesc> d(n + 1);
    uint64_t blocks = 0, segs = 0, entries = 0, waves = 0;
    for (uint64_t i = 0; i < n; i++) {
        const ChunkCounts k = chunk_counts(samples[i], bs, rsi, segs_per_rsi);
        d[i] = ChunkDesc{16 * i, samples[i], blocks, segs, entries, waves};
        blocks += k.blocks;
        segs += k.segs;
        entries += k.rsis + 1;
        waves += (k.segs + spw - 1) / spw;
    }
    d[n] = ChunkDesc{0, 0, blocks, segs, entries, waves};
    if (segs != nseg_given || entries != n_entries || waves != n_waves) return -1;
    const uint64_t nseg = segs, ntiles = (nseg + kTile - 1) / kTile;

    // set-up: the per-wave table, the totals cleared
    for (uint64_t w = 0; w < waves; w++) wave_chunk[w] = (uint32_t)chunk_of_wave(d.data(), n, w);
    for (uint64_t i = 0; i < n; i++) chunk_bits[i] = 0;

    // phase 1
    std::vector<CkVal> tiles(ntiles), agg(kThreads), excl;
    for (uint64_t tile = 0; tile < ntiles; tile++) {
        const uint64_t tile_end = (tile + 1) * kTile < nseg ? (tile + 1) * kTile : nseg;
        for (uint64_t t = 0; t < kThreads; t++) {
            const ThreadSpan sp = span_of(tile, t, nseg);
            agg[t] = ck_reduce_items(d.data(), n, seg_bits, seg_clamp, sp.s0, sp.s1);
        }
        tiles[tile] = excl_scan(agg, excl);
        for (uint64_t t = 0; t < kThreads; t++) {
            const ThreadSpan sp = span_of(tile, t, nseg);
            ck_flush_totals(d.data(), n, seg_bits, seg_clamp, sp.s0, sp.s1, tile_end, excl[t],
                            [&](uint64_t chunk, uint64_t bits) { chunk_bits[chunk] += bits; });
        }
    }
    // phase 2
    uint64_t run_bytes = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t before = run_bytes;
        run_bytes = ck_base(run_bytes, chunk_bits[i], &chunk_base[i]);
        empty_byte[i] = ~0ull;
        if (d[i + 1].seg0 == d[i].seg0) {
            empty_byte[i] = before;
            rsi_table[d[i].rsi0] = chunk_base[i];
        }
    }
    *total_bytes = run_bytes;
    {
        CkVal run = ck_identity();
        for (uint64_t tile = 0; tile < ntiles; tile++) {
            const CkVal cur = tiles[tile];
            tiles[tile] = run;
            run = ck_then(run, cur);
        }
    }
    // phase 3
    for (uint64_t tile = 0; tile < ntiles; tile++) {
        for (uint64_t t = 0; t < kThreads; t++) {
            const ThreadSpan sp = span_of(tile, t, nseg);
            agg[t] = ck_reduce_items(d.data(), n, seg_bits, seg_clamp, sp.s0, sp.s1);
        }
        excl_scan(agg, excl);
        for (uint64_t t = 0; t < kThreads; t++) {
            const ThreadSpan sp = span_of(tile, t, nseg);
            if (sp.s0 >= sp.s1) continue;
            CkVal run = ck_then(tiles[tile], excl[t]);
            CkCursor cur = ck_cursor(d.data(), n, sp.s0);
            for (uint64_t s = sp.s0; s < sp.s1; s++) {
                ck_advance(d.data(), n, s, cur);
                const CkVal item = ck_item(d.data(), cur, s, seg_bits[s], seg_clamp[s]);
                const CkSeg g = ck_segment(d.data(), cur, s, run, item, chunk_base[cur.chunk], segs_per_rsi, spw);
                seg_start[s] = g.start;
                seg_kin[s] = (uint8_t)g.kin;
                if (g.first_rsi) rsi_table[g.rsi_entry] = g.start;
                if (g.wave_first && (g.start >> 5) < cap_words) zeroed[g.start >> 5] = 1;
                if (g.last) {
                    rsi_table[g.rsi_entry_end] = g.end;
                    for (uint64_t w = g.end >> 5; w <= (g.end >> 5) + 1; w++)
                        if (w < cap_words) zeroed[w] = 1;
                }
                run = ck_then(run, item);
            }
        }
    }
    return (long long)nseg;
}

#ifdef CHUNKS_EMUL_MAIN
// a stand-alone run for the host sanitizers: g++ -fsanitize=address,undefined -DCHUNKS_EMUL_MAIN chunks_emul.cpp
int main()
{
    const uint32_t bs = 8, rsi = 128, spw = 4;
    std::vector<uint64_t> samples;
    uint64_t x = 12345;
    auto rnd = [&]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(x >> 33); };
    for (int i = 0; i < 700; i++) samples.push_back(i % 7 == 3 ? 0 : rnd() % 200000);
    samples.push_back((uint64_t)bs * 64 * 4100);
    const uint64_t n = samples.size();
    uint64_t nseg = 0, entries = 0, waves = 0;
    for (uint64_t s : samples) {
        const ChunkCounts k = chunk_counts(s, bs, rsi, (rsi + 63) / 64);
        nseg += k.segs; entries += k.rsis + 1; waves += (k.segs + spw - 1) / spw;
    }
    std::vector<uint32_t> bits(nseg);
    std::vector<uint16_t> cl(nseg);
    for (uint64_t s = 0; s < nseg; s++) {
        bits[s] = rnd() % 40000;
        const uint32_t lo = rnd() % 14, hi = lo + rnd() % (14 - lo);
        cl[s] = (uint16_t)(rnd() % 3 ? (lo | hi << 8) : (0 | 31 << 8));
    }
    std::vector<uint64_t> base(n), cbits(n), start(nseg), table(entries), empty(n);
    std::vector<uint8_t> kin(nseg);
    std::vector<uint32_t> wc(waves);
    uint64_t total = 0;
    const uint64_t cap_words = 1 << 20;
    std::vector<uint8_t> zeroed(cap_words);
    const long long r = emul_chunks(bs, rsi, spw, samples.data(), n, bits.data(), cl.data(), nseg, base.data(), cbits.data(),
                                    start.data(), kin.data(), table.data(), entries, wc.data(), waves, zeroed.data(), cap_words,
                                    empty.data(), &total);
    printf("segments %lld, %llu bytes\n", r, (unsigned long long)total);
    return r == (long long)nseg ? 0 : 1;
}
#endif
