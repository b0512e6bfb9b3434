// enc_local_emul.cpp -- the encoder route that codes every block once (libaec_amd/csrc/aec_enc_local.h; aec_enc.hip:
// k_encode_local / k_encode_redo / k_place) on the CPU, on blocks that are only a length, an own clamp (or none) and bits
// that depend on the block and on the k it is coded with: the guess, the carry inside a run, the test for a miss, the
// slots and the placement are the header's functions, the scan between them is a plain loop.
// (test infrastructure; built by tests/test_enc_local_emul.py, and with -DENC_LOCAL_EMUL_MAIN as a program of its own)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../libaec_amd/csrc/aec_cfg.h"
#include "../../libaec_amd/csrc/aec_enc_local.h"

using namespace aec;

namespace {
// bit i of block b coded with k
inline uint32_t block_bit(uint64_t b, uint32_t k, uint32_t i)
{
    uint64_t x = (b + 1) * 0x9E3779B97F4A7C15ull ^ (uint64_t)(k + 1) * 0xC2B2AE3D27D4EB4Full ^ (uint64_t)(i + 1) * 0x165667B19E3779F9ull;
    x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
    return (uint32_t)(x & 1u);
}
inline void put_bit(std::vector<uint32_t> &w, uint64_t pos, uint32_t bit)
{
    if (bit) w[pos >> 5] |= 0x80000000u >> (pos & 31u);
}
const uint32_t kNone = 255;      // lo of a block that neither reads nor updates k
}  // namespace

// Blocks [seg_blk0[s], seg_blk0[s + 1]) form segment s; block b has len[b] bits and the own clamp [lo[b], hi[b]]
// (lo[b] == 255: none).  Runs of segs_per_wave segments.  Returns 0, or a code that says which property failed; out[]
// receives counts: [0] runs that missed, [1] runs, [2] words taken by atomic OR.
extern "C" int emul_enc_local(uint64_t nseg, const uint64_t *seg_blk0, const uint32_t *len, const uint8_t *lo, const uint8_t *hi,
                              uint32_t segs_per_wave, uint32_t k_in, uint32_t guess_fixed, uint32_t start_bit,
                              uint32_t slot_words, uint64_t *out)
{
    const uint64_t nwaves = (nseg + segs_per_wave - 1) / segs_per_wave;
    std::vector<uint32_t> image(nwaves * slot_words, 0xDEADBEEFu);          // stale words everywhere
    std::vector<uint32_t> seg_bits(nseg), seg_first(nseg), seg_kused(nseg), seg_kin(nseg);
    std::vector<uint16_t> seg_clamp(nseg);
    std::vector<uint64_t> seg_start(nseg + 1);
    const uint64_t nblk = seg_blk0[nseg];
    std::vector<uint32_t> k_guess(nblk, 0), k_true(nblk, 0);

    // One run into its slot.  redo: as k_encode_redo does it -- only the segments from the first to the last miss, at the
    // positions the scan gave, the open words at both ends of the range merged with what the slot holds.
    auto code_run = [&](uint64_t wv, bool redo) -> int {
        const uint64_t run0 = wv * segs_per_wave, run1 = run0 + segs_per_wave < nseg ? run0 + segs_per_wave : nseg;
        uint64_t s0 = run0, s1 = run1;
        std::vector<uint32_t> slot(slot_words, 0u);
        uint64_t pos = 0;
        if (redo) {
            uint64_t missed = 0;
            for (uint64_t s = run0; s < run1; s++)
                if (local_missed(seg_first[s], seg_kused[s], seg_kin[s])) missed |= 1ull << (s - run0);
            const LocalRedo range = local_redo_range(missed);
            s0 = run0 + range.first;
            s1 = run0 + range.end;
            pos = seg_start[s0] - seg_start[run0];
            slot[pos >> 5] = local_redo_head(image[wv * slot_words + (pos >> 5)], (uint32_t)pos);
        }
        const uint64_t pos0 = pos;
        uint32_t k = k_in;
        bool have_k = wv == 0;
        for (uint64_t s = s0; s < s1; s++) {
            uint32_t first = kLocalNoClamp, tot = 0;
            bool found = false;
            KClamp cl = kclamp_identity();
            for (uint64_t b = seg_blk0[s]; b < seg_blk0[s + 1]; b++) {
                tot += len[b];
                if (lo[b] == kNone) continue;
                if (!found) first = lo[b] | ((uint32_t)hi[b] << 8);
                found = true;
                cl = kclamp_then(cl, KClamp{lo[b], hi[b]});
            }
            uint32_t kin;
            if (redo) {
                kin = seg_kin[s];
            } else {
                if (!have_k && found) {
                    k = local_guess(first, guess_fixed);
                    have_k = true;
                }
                kin = k;
                seg_bits[s] = tot;
                seg_clamp[s] = (uint16_t)(cl.lo | (cl.hi << 8));
                seg_first[s] = first;
                seg_kused[s] = kin;
                k = kclamp_apply(cl, k);
            }
            uint32_t kb = kin;
            for (uint64_t b = seg_blk0[s]; b < seg_blk0[s + 1]; b++) {
                if (lo[b] != kNone) kb = kclamp_apply(KClamp{lo[b], hi[b]}, kb);
                const uint32_t kk = lo[b] == kNone ? 0u : kb;
                if (!redo) k_guess[b] = kk;
                if (pos + len[b] > (uint64_t)slot_words * 32u) return 10;          // the slot holds its run
                for (uint32_t i = 0; i < len[b]; i++) put_bit(slot, pos + i, block_bit(b, kk, i));
                pos += len[b];
            }
        }
        if (pos == pos0) return 0;
        for (uint64_t w = pos0 >> 5; w < (pos + 31) / 32; w++) {                                // (the rest stays stale)
            uint32_t v = slot[w];
            if (redo && s1 < run1 && (pos & 31u) && w == (pos >> 5)) v = local_redo_tail(v, image[wv * slot_words + w], pos & 31u);
            image[wv * slot_words + w] = v;
        }
        return 0;
    };
    for (uint64_t wv = 0; wv < nwaves; wv++)
        if (int rc = code_run(wv, false)) return rc;

    // the scan, and the true k of every block
    {
        uint64_t bit = start_bit;
        uint32_t k = k_in;
        for (uint64_t s = 0; s < nseg; s++) {
            seg_start[s] = bit;
            seg_kin[s] = k;
            uint32_t kb = k;
            for (uint64_t b = seg_blk0[s]; b < seg_blk0[s + 1]; b++) {
                if (lo[b] != kNone) kb = kclamp_apply(KClamp{lo[b], hi[b]}, kb);
                k_true[b] = lo[b] == kNone ? 0u : kb;
            }
            bit += seg_bits[s];
            k = kclamp_apply(KClamp{seg_clamp[s] & 0xFFu, (uint32_t)(seg_clamp[s] >> 8)}, k);
            if (k != kb && seg_blk0[s + 1] > seg_blk0[s]) {
                bool any = false;
                for (uint64_t b = seg_blk0[s]; b < seg_blk0[s + 1]; b++) any = any || lo[b] != kNone;
                if (any) return 11;                                                  // the clamp of a segment is its blocks'
            }
        }
        seg_start[nseg] = bit;
    }
    const uint64_t total = seg_start[nseg] - start_bit;

    // the test for a miss is exact, run by run
    uint64_t missed_runs = 0;
    for (uint64_t wv = 0; wv < nwaves; wv++) {
        const uint64_t s0 = wv * segs_per_wave, s1 = s0 + segs_per_wave < nseg ? s0 + segs_per_wave : nseg;
        bool fires = false, differs = false;
        for (uint64_t s = s0; s < s1; s++) {
            fires = fires || local_missed(seg_first[s], seg_kused[s], seg_kin[s]);
            for (uint64_t b = seg_blk0[s]; b < seg_blk0[s + 1]; b++) differs = differs || k_guess[b] != k_true[b];
        }
        if (fires && !differs) return 20;       // false positive
        if (!fires && differs) return 21;       // false negative
        if (fires) {
            missed_runs++;
            if (int rc = code_run(wv, true)) return rc;
        }
    }

    // placement: the words the scan zeroes, then every run
    const uint64_t nout = ((uint64_t)start_bit + total + 31) / 32 + 2;
    std::vector<uint32_t> stream(nout, 0xA5A5A5A5u);
    std::vector<uint8_t> zeroed(nout, 0), stored(nout, 0), ored(nout, 0);
    for (uint64_t s = 0; s < nseg; s += segs_per_wave) zeroed[seg_start[s] >> 5] = 1;
    zeroed[seg_start[nseg] >> 5] = zeroed[(seg_start[nseg] >> 5) + 1] = 1;
    for (uint64_t w = 0; w < nout; w++)
        if (zeroed[w]) stream[w] = 0;
    for (uint64_t wv = 0; wv < nwaves; wv++) {
        const uint64_t s0 = wv * segs_per_wave, s1 = s0 + segs_per_wave < nseg ? s0 + segs_per_wave : nseg;
        if (seg_start[s1] == seg_start[s0]) continue;
        const LocalSpan sp = local_span(seg_start[s0], seg_start[s1] - seg_start[s0]);
        const uint32_t *slot = &image[wv * slot_words];
        for (uint32_t j = 0; j < sp.nwords; j++) {
            const uint32_t before = j ? slot[j - 1] : 0u, at = j < sp.nslot ? slot[j] : 0u;
            const uint32_t v = local_word(sp, before, at);
            if (sp.word0 + j >= nout) return 30;
            if (local_word_shared(sp, j)) {
                if (!zeroed[sp.word0 + j]) return 31;                                // OR into a word nobody zeroed
                stream[sp.word0 + j] |= v;
                ored[sp.word0 + j] = 1;
            } else {
                if (stored[sp.word0 + j] || ored[sp.word0 + j]) return 32;           // a second writer
                stream[sp.word0 + j] = v;
                stored[sp.word0 + j] = 1;
            }
        }
    }
    uint64_t nor = 0;
    for (uint64_t w = 0; w < nout; w++) {
        nor += ored[w];
        if (stored[w] && ored[w]) return 33;
        if (w < ((uint64_t)start_bit + total + 31) / 32 && !stored[w] && !ored[w]) return 34;   // a word of the stream nobody wrote
    }
    // the stream is the blocks' bits with their true k, one after the other
    uint64_t pos = start_bit;
    for (uint64_t b = 0; b < nblk; b++)
        for (uint32_t i = 0; i < len[b]; i++, pos++)
            if (((stream[pos >> 5] >> (31u - (pos & 31u))) & 1u) != block_bit(b, k_true[b], i)) return 40;
    for (; pos < (nout - 1) * 32; pos++)                                             // zero behind the end, up to the padding word
        if (((pos >> 5) <= (seg_start[nseg] >> 5) + 1) && ((stream[pos >> 5] >> (31u - (pos & 31u))) & 1u)) return 41;
    out[0] = missed_runs;
    out[1] = nwaves;
    out[2] = nor;
    return 0;
}

// slot geometry of a shape: [0] bits of a segment's share, [1] words between two slots
extern "C" void emul_local_geometry(uint32_t id_len, uint32_t bs, uint32_t bps, uint32_t rsi, uint32_t segs_per_wave,
                                    uint32_t *out)
{
    out[0] = local_seg_bits(id_len, bs, bps, rsi);
    out[1] = local_slot_words(id_len, bs, bps, rsi, segs_per_wave);
}

// How often a guess rule misses on real samples: unsigned samples of at most 16 bits with the preprocessor, every block
// through the library's own option selection (aec_lane.h choose_option).  out: [0] runs with a predecessor, [1] of those
// the runs whose first k-updating block has a plateau of more than one k, [2] [3] [4] runs in which some block takes
// another k than the true carry gives with the guess lo / hi / (lo + hi) / 2, [5] blocks that update k, [6] of those
// with a plateau of more than one k.
extern "C" int emul_miss_rates(const uint8_t *data, uint64_t nbytes, uint32_t bps, uint32_t bs, uint32_t rsi,
                               uint32_t segs_per_wave, uint64_t *out)
{
    Cfg c;
    if (make_cfg(bps, bs, rsi, F_PREPROCESS, nbytes, true, &c) != RC_OK || bps > 16 || bs > 64) return 1;
    const uint64_t nblk = c.total_samples / bs;
    std::vector<uint8_t> lo(nblk), hi(nblk);
    auto sample = [&](uint64_t i) { return c.bytes == 1 ? (uint32_t)data[i] : (uint32_t)data[2 * i] | ((uint32_t)data[2 * i + 1] << 8); };
    for (uint64_t b = 0; b < nblk; b++) {
        uint32_t d[64], any = 0;
        const uint32_t ref = b % rsi == 0 ? 1u : 0u;
        for (uint32_t i = 0; i < bs; i++) {
            const uint64_t at = b * bs + i;
            d[i] = (ref && i == 0) ? 0u : pp_unsigned(sample(at - 1), sample(at), c.xmax);
            any |= d[i];
        }
        lo[b] = 255;
        hi[b] = 0;
        if (any && c.id_len > 1) {
            const BlockChoice ch = choose_option<0, false>(d, c, ref);
            lo[b] = (uint8_t)ch.klo;
            hi[b] = (uint8_t)ch.khi;
        }
    }
    for (int i = 0; i < 7; i++) out[i] = 0;
    const uint64_t run_blocks = (uint64_t)segs_per_wave * (rsi < 64 ? rsi : 64);
    uint32_t k = 0;
    for (uint64_t b0 = 0; b0 < nblk; b0 += run_blocks) {
        const uint64_t b1 = b0 + run_blocks < nblk ? b0 + run_blocks : nblk;
        uint32_t g[3] = {0, 0, 0};
        bool have = false, miss[3] = {false, false, false};
        for (uint64_t b = b0; b < b1; b++) {
            if (lo[b] == 255) continue;
            out[5]++;
            out[6] += lo[b] != hi[b];
            if (!have) {
                have = true;
                if (b0) out[1] += lo[b] != hi[b];
                g[0] = lo[b]; g[1] = hi[b]; g[2] = (lo[b] + hi[b]) / 2u;
            }
            const KClamp own{lo[b], hi[b]};
            k = kclamp_apply(own, k);
            for (int r = 0; r < 3; r++) {
                g[r] = kclamp_apply(own, g[r]);
                miss[r] = miss[r] || g[r] != k;
            }
        }
        if (b0) {
            out[0]++;
            for (int r = 0; r < 3; r++) out[2 + r] += miss[r];
        }
    }
    return 0;
}

#ifdef ENC_LOCAL_EMUL_MAIN
// a few random inputs, for a run under the sanitizers (tests/test_enc_local_emul.py builds and runs it)
int main()
{
    uint64_t state = 12345;
    auto rnd = [&](uint32_t n) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((state >> 33) % n);
    };
    for (int it = 0; it < 200; it++) {
        const uint32_t spw = 1u << rnd(4), nseg = 1 + rnd(70), maxlen = 1 + rnd(3) * 20;
        std::vector<uint64_t> blk0(nseg + 1, 0);
        std::vector<uint32_t> len;
        std::vector<uint8_t> lo, hi;
        for (uint32_t s = 0; s < nseg; s++) {
            const uint32_t nb = 1 + rnd(it % 3 ? 6 : 64);
            for (uint32_t b = 0; b < nb; b++) {
                const bool none = rnd(3) == 0;
                const uint32_t a = rnd(14), w = rnd(3) ? 0 : rnd(4);
                len.push_back(none && rnd(2) ? 0 : 1 + rnd(maxlen));
                lo.push_back(none ? 255 : a);
                hi.push_back(none ? 0 : a + w);
            }
            if (len[blk0[s]] == 0) len[blk0[s]] = 1;                 // a segment's first block always emits
            blk0[s + 1] = len.size();
        }
        uint64_t out[3];
        const uint32_t slot_words = (spw * 64 * (maxlen + 1) / 32 + 32) & ~31u;
        const int rc = emul_enc_local(nseg, blk0.data(), len.data(), lo.data(), hi.data(), spw, rnd(14),
                                      rnd(2) ? kLocalGuessRule : rnd(40), rnd(8), slot_words, out);
        if (rc) {
            std::printf("case %d failed: %d\n", it, rc);
            return 1;
        }
    }
    std::printf("enc_local_emul ok\n");
    return 0;
}
#endif
