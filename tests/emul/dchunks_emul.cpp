// dchunks_emul.cpp -- the item table of a batch of unequal chunks decoded as one launch (libaec_amd/csrc/aec_dchunks.h;
// aec_dec.hip: k_dchunks_setup and the CHUNKS variants of the decode kernels) on the CPU: the descriptors as the host
// entry point writes them, the chunk of every item as the set-up kernel finds it, and every item as a lane of the decode
// kernels derives it.
// (test infrastructure; built by tests/test_decode_chunks_items.py)
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../libaec_amd/csrc/aec_dchunks.h"

using namespace aec;

// out_bytes / out_off [n]: what every chunk decodes to and where its room begins; whole / tail [n] (or null: what the
// chunks announce): the chunks' records.  Out, per item: its chunk, RSI within the chunk, table entry, blocks, byte
// offset of its first block; per chunk: the record made of what it announces.  Returns the items, -1 on misuse.
extern "C" long long emul_dchunks(uint32_t bytes, uint32_t bs, uint32_t rsi, const uint64_t *out_bytes, const uint64_t *out_off,
                                  uint64_t n, const uint64_t *whole, const uint64_t *tail, uint64_t items_given,
                                  uint32_t *item_chunk, uint64_t *item_rin, uint64_t *item_entry, uint32_t *item_nb,
                                  uint64_t *item_pos, uint64_t *ann_whole, uint64_t *ann_tail)
{
    const uint64_t blk_bytes = (uint64_t)bs * bytes;
    std::vector<DChunkDesc> d(n + 1);
    uint64_t items = 0;
    for (uint64_t i = 0; i < n; i++) {
        const DChunkCounts k = dchunk_counts(out_bytes[i], bytes, bs, rsi);
        d[i] = DChunkDesc{0, 0, out_off[i], items, (uint32_t)k.rsis, k.last_blocks};
        items += k.rsis;
    }
    d[n] = DChunkDesc{0, 0, 0, items, 0u, 0u};
    if (items != items_given) return -1;
    for (uint64_t i = 0; i < n; i++) dchunk_announced(d[i], rsi, &ann_whole[i], &ann_tail[i]);
    // set-up: a thread per item
    for (uint64_t r = 0; r < items; r++) item_chunk[r] = (uint32_t)dchunk_of_item(d.data(), n, r);
    // decode: a lane (or a wavefront) per item
    for (uint64_t r = 0; r < items; r++) {
        const uint64_t c = item_chunk[r];
        const DItem it = dchunk_item(d.data(), c, r, rsi, blk_bytes, whole ? whole[c] : ann_whole[c], tail ? tail[c] : ann_tail[c]);
        item_rin[r] = it.rin;
        item_entry[r] = it.entry;
        item_nb[r] = it.nb;
        item_pos[r] = it.out_pos;
    }
    return (long long)items;
}

#ifdef DCHUNKS_EMUL_MAIN
// a stand-alone run for the host sanitizers: g++ -fsanitize=address,undefined -DDCHUNKS_EMUL_MAIN dchunks_emul.cpp
// argv[1]: a text file of lists -- "bytes bs rsi n" and then n lines "out_bytes out_off" each -- as the test writes it;
// prints the items of every list and checks that the items of a chunk tile its room.
int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    unsigned bytes, bs, rsi;
    unsigned long long n;
    int bad = 0;
    while (fscanf(f, "%u %u %u %llu", &bytes, &bs, &rsi, &n) == 4) {
        std::vector<uint64_t> ob(n), oo(n), aw(n), at(n);
        uint64_t items = 0;
        for (uint64_t i = 0; i < n; i++) {
            unsigned long long a, b;
            if (fscanf(f, "%llu %llu", &a, &b) != 2) return 2;
            ob[i] = a;
            oo[i] = b;
            items += dchunk_counts(a, bytes, bs, rsi).rsis;
        }
        std::vector<uint32_t> ic(items), nb(items);
        std::vector<uint64_t> rin(items), entry(items), pos(items);
        const long long got = emul_dchunks(bytes, bs, rsi, ob.data(), oo.data(), n, nullptr, nullptr, items, ic.data(), rin.data(),
                                           entry.data(), nb.data(), pos.data(), aw.data(), at.data());
        if (got != (long long)items) bad = 1;
        uint64_t r = 0;
        for (uint64_t i = 0; i < n; i++) {                       // the items of chunk i, one behind the other in its room
            uint64_t at_byte = oo[i];
            for (; r < items && ic[r] == i; r++) {
                if (pos[r] != at_byte || entry[r] != r + i) bad = 1;
                at_byte += (uint64_t)nb[r] * bs * bytes;
            }
            if (at_byte != oo[i] + dchunk_counts(ob[i], bytes, bs, rsi).blocks * bs * bytes) bad = 1;
        }
        if (r != items) bad = 1;
        printf("items %lld\n", got);
    }
    fclose(f);
    return bad;
}
#endif
