// CPU harness for the small-block emitter on sample pairs (libaec_amd/csrc/aec_lane.h: pairs_eligible,
// emit_small_pairs): every block it takes must leave, bit for bit, what emit_block leaves at the same bit position
// of a zeroed image -- the words around the block included.  Checks itself; a non-zero return names the property:
//   1  an eligible block's image differs from emit_block's        2  the image is touched outside its words
//   3  a directed case did not land on the side of the eligibility test it was built for
//   4  a sweep that can meet both sides of the eligibility test saw only one
// Build: g++ -O2 -std=c++17 -shared -fPIC tests/emul/emit_pairs_emul.cpp   (-DEMIT_PAIRS_EMUL_MAIN: a program)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../libaec_amd/csrc/aec_lane.h"

using namespace aec;

namespace {

struct HostSink {
    uint32_t *w;
    void or_word(uint32_t i, uint32_t v) { w[i] |= v; }
};

constexpr uint32_t kWords = 160;       // emit_block of 16 codes of up to 256 bits, a header, 31 bits of lead: < 4200 bits
constexpr uint32_t kMaxT = 250;        // longest fundamental sequence a block of the sweeps holds

struct Stats {
    uint64_t blocks, eligible, refused;
};

struct Rng {
    uint64_t s;
    uint32_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    uint32_t below(uint32_t n) { return next() % n; }
};

Cfg make_cfg(uint32_t id_len, uint32_t bs)
{
    Cfg c{};
    c.id_len = id_len;
    c.bps = id_len == 3 ? 8u : 16u;
    c.bs = bs;
    c.kmax = (1u << id_len) - 3u;
    c.bytes = c.bps / 8u;
    c.flags = F_PREPROCESS;
    return c;
}

// coded length of the block in the option given, as the analysis hands it to the emitters
uint32_t coded_len(const Cfg &c, uint32_t bs, const uint32_t *d, uint32_t opt, uint32_t k_or_fs, uint32_t ref)
{
    uint32_t len = c.id_len + ref * c.bps;
    if (opt == OPT_SPLIT) {
        for (uint32_t i = ref; i < bs; i++) len += (d[i] >> k_or_fs) + 1u + k_or_fs;
    } else if (opt == OPT_SE) {
        len += 1u;
        for (uint32_t i = 0; i < bs; i += 2) {
            const uint32_t s = d[i] + d[i + 1];
            len += s * (s + 1u) / 2u + d[i + 1] + 1u;
        }
    } else {
        len += 1u + k_or_fs + 1u;
    }
    return len;
}

// 0: same image (or not eligible), else the property that failed
template <int BS>
int check_block(const Cfg &c, const uint32_t *d, uint32_t opt, uint32_t k_or_fs, uint32_t ref, uint32_t ref_sample,
                uint32_t pos, Stats &st, int want_eligible = -1)
{
    uint32_t a[kWords], b[kWords];
    memset(a, 0, sizeof a);
    memset(b, 0, sizeof b);
    const uint32_t len = coded_len(c, BS, d, opt, k_or_fs, ref);
    uint32_t ubits = 0, fbits = 0;
    const bool ok = pairs_eligible(c, BS, opt, k_or_fs, ref, len, ubits, fbits);
    st.blocks++;
    if (want_eligible >= 0 && (int)ok != want_eligible) return 3;
    uint32_t w[BS / 2];
    for (int j = 0; j < BS / 2; j++) w[j] = d[2 * j] | (d[2 * j + 1] << 16);
    HostSink sb{b};
    // (a lane that is not eligible runs the same text with live = false and must leave the image alone)
    emit_small_pairs<BS>(sb, pos, w, c, opt, k_or_fs, ref, ref_sample, ubits, fbits, ok);
    if (!ok) {
        st.refused++;
        for (uint32_t i = 0; i < kWords; i++)
            if (b[i]) return 2;
        return 0;
    }
    st.eligible++;
    HostSink sa{a};
    BitWriter<HostSink> bw(sa, pos);
    emit_block<BS>(bw, d, c, opt, k_or_fs, ref, ref_sample);
    if (memcmp(a, b, sizeof a)) return 1;
    // nothing in front of the block's first bit, nothing behind its last
    const uint32_t end = pos + len;
    for (uint32_t i = 0; i < kWords; i++) {
        uint32_t mask = 0xFFFFFFFFu;                    // bits of word i that belong to the block
        if (32u * i + 32u <= pos || 32u * i >= end) mask = 0;
        else {
            if (32u * i < pos) mask &= 0xFFFFFFFFu >> (pos - 32u * i);
            if (32u * i + 32u > end) mask &= ~(0xFFFFFFFFu >> (end - 32u * i));
        }
        if (b[i] & ~mask) return 2;
    }
    return 0;
}

// a split block whose fundamental sequences add up to `ubits` and whose fields are random
// (false: the sample range has no such block)
template <int BS>
bool split_block(Rng &r, const Cfg &c, uint32_t k, uint32_t ref, uint32_t ubits, uint32_t *d)
{
    const uint32_t n = BS - ref;
    uint32_t t[BS] = {};
    const uint32_t tmax = (low_mask32(c.bps) >> k) < 62u ? (low_mask32(c.bps) >> k) : 62u;
    if (ubits < n || ubits > n * (tmax + 1u)) return false;
    uint32_t left = ubits - n;                          // every code has its closing 1
    while (left) {
        const uint32_t i = ref + r.below(n);
        if (t[i] < tmax) { t[i]++; left--; }
    }
    for (uint32_t i = 0; i < (uint32_t)BS; i++) d[i] = (t[i] << k) | (r.next() & low_mask32(k));
    if (ref) d[0] = 0;
    return true;
}

template <int BS>
int sweep(uint32_t id_len, uint64_t per_combination, uint64_t seed, Stats &total)
{
    const Cfg c = make_cfg(id_len, BS);
    const uint32_t full = low_mask32(c.bps);
    Rng r{seed * 977u + id_len * 31u + BS};
    uint32_t d[BS];
    for (uint32_t ref = 0; ref < 2; ref++) {
        const uint32_t ref_sample = r.next() & full;
        // ---- split, k = 0 .. kmax; second extension (k = kmax + 1 here); zero-run codes (kmax + 2)
        for (uint32_t k = 0; k <= c.kmax + 2; k++) {
            const uint32_t opt = k <= c.kmax ? OPT_SPLIT : (k == c.kmax + 1 ? OPT_SE : OPT_ZERO);
            Stats st{};
            for (uint64_t it = 0; it < per_combination; it++) {
                const uint32_t pos = (uint32_t)(it & 31u) + 32u * (uint32_t)((it >> 5) & 3u);      // every lead, four words
                uint32_t arg = k;
                if (opt == OPT_SPLIT) {
                    // codes of a few bits, now and then a long one, so that blocks fall on both sides of 64 bits
                    const uint32_t scale = 1u + r.below(4);
                    for (uint32_t i = 0; i < (uint32_t)BS; i++) {
                        uint32_t t = r.below(scale + 1u);
                        if (r.below(16) == 0) t += r.below(kMaxT - 8u);
                        if (t > (full >> k)) t = full >> k;
                        d[i] = (t << k) | (r.next() & low_mask32(k));
                    }
                } else if (opt == OPT_SE) {
                    const uint32_t hi = 1u + r.below(4);
                    for (uint32_t i = 0; i < (uint32_t)BS; i++) d[i] = r.below(hi + 1u) + (r.below(24) == 0 ? r.below(12) : 0u);
                } else {
                    for (uint32_t i = 0; i < (uint32_t)BS; i++) d[i] = 0;
                    arg = r.below(4) ? r.below(65) : 60u + r.below(30);      // the run's code: fs zeros and a 1
                }
                if (ref) d[0] = 0;
                const int rc = check_block<BS>(c, d, opt, arg, ref, ref_sample, pos, st);
                if (rc) return rc;
            }
            const bool fields_fit = opt != OPT_SPLIT || (BS - ref) * k <= 64u;      // (else no block is eligible)
            // (both sides for every option; for split wherever the sample range has codes long enough: 8-bit samples
            // at k = 5 have codes of at most 8 bits)
            const bool can_miss = opt != OPT_SPLIT || !fields_fit || (full >> k) >= 64u;
            if ((fields_fit && !st.eligible) || (can_miss && !st.refused)) return 4;
            total.blocks += st.blocks; total.eligible += st.eligible; total.refused += st.refused;
        }
    }
    return 0;
}

// every block of 8 residuals out of {0, 1, 2, 3}: split with every k, second extension; the lead moves with the block
int exhaustive8(uint32_t id_len, Stats &total)
{
    const Cfg c = make_cfg(id_len, 8);
    uint32_t d[8];
    for (uint32_t ref = 0; ref < 2; ref++)
        for (uint32_t k = 0; k <= c.kmax + 1; k++)
            for (uint32_t code = 0; code < 65536u; code++) {
                for (uint32_t i = 0; i < 8; i++) d[i] = (code >> (2 * i)) & 3u;
                if (ref) d[0] = 0;
                const uint32_t opt = k <= c.kmax ? OPT_SPLIT : OPT_SE;
                // (codes of at most four bits: a split block is eligible wherever its fields fit)
                const int want = opt == OPT_SPLIT ? ((8u - ref) * k <= 64u ? 1 : 0) : -1;
                const int rc = check_block<8>(c, d, opt, k, ref, 0x5Au & low_mask32(c.bps), (code + k) & 31u, total, want);
                if (rc) return rc;
            }
    return 0;
}

// the borders of the eligibility test, at every lead
template <int BS>
int directed(uint32_t id_len, Stats &total)
{
    const Cfg c = make_cfg(id_len, BS);
    Rng r{id_len * 131u + BS};
    uint32_t d[BS];
    for (uint32_t lead = 0; lead < 32; lead++)
        for (uint32_t ref = 0; ref < 2; ref++) {
            const uint32_t n = BS - ref, head = c.id_len + ref * c.bps, ref_sample = r.next() & low_mask32(c.bps);
            for (uint32_t k = 0; k <= c.kmax; k++) {
                // unary regions of exactly 63, 64 and 65 bits (never eligible: the header needs room in the same 64 bits),
                // and header + unary region of exactly 63, 64 (eligible where the fields fit) and 65 bits
                for (uint32_t ubits = 63; ubits <= 65; ubits++) {
                    int rc = 0;
                    if (split_block<BS>(r, c, k, ref, ubits, d))
                        rc = check_block<BS>(c, d, OPT_SPLIT, k, ref, ref_sample, lead, total, 0);
                    if (rc) return rc;
                    if (!split_block<BS>(r, c, k, ref, ubits - head, d)) continue;
                    rc = check_block<BS>(c, d, OPT_SPLIT, k, ref, ref_sample, lead, total, ubits <= 64 && n * k <= 64 ? 1 : 0);
                    if (rc) return rc;
                }
                // a field region of exactly 64 bits, and the next k, whose fields do not fit
                if (n * k == 64u || (n * k > 64u && n * (k - 1u) <= 64u)) {
                    if (!split_block<BS>(r, c, k, ref, n + r.below(8), d)) return 3;
                    const int rc = check_block<BS>(c, d, OPT_SPLIT, k, ref, ref_sample, lead, total, n * k == 64u ? 1 : 0);
                    if (rc) return rc;
                }
                // 128 bits that end on a word border: header + unary region 64 bits, fields 64 bits
                if (n * k == 64u && lead == 0) {
                    if (!split_block<BS>(r, c, k, ref, 64u - head, d)) return 3;
                    for (uint32_t word = 0; word < 3; word++) {
                        const int rc = check_block<BS>(c, d, OPT_SPLIT, k, ref, ref_sample, 32u * word, total, 1);
                        if (rc) return rc;
                    }
                }
            }
            // zero-run codes at the border: header + fs + 1 of 64 and of 65 bits
            for (uint32_t i = 0; i < (uint32_t)BS; i++) d[i] = 0;
            for (uint32_t over = 0; over < 2; over++) {
                const uint32_t fs = 64u + over - (head + 1u) - 1u;
                const int rc = check_block<BS>(c, d, OPT_ZERO, fs, ref, ref_sample, lead, total, over ? 0 : 1);
                if (rc) return rc;
            }
        }
    return 0;
}

}  // namespace

// out: blocks checked, eligible, not eligible
extern "C" int emul_emit_pairs(uint64_t per_combination, uint64_t seed, uint64_t *out)
{
    Stats st{};
    int rc = 0;
    for (uint32_t id_len = 3; id_len <= 4 && !rc; id_len++) {
        rc = sweep<8>(id_len, per_combination, seed, st);
        if (!rc) rc = sweep<16>(id_len, per_combination, seed, st);
        if (!rc) rc = directed<8>(id_len, st);
        if (!rc) rc = directed<16>(id_len, st);
    }
    out[0] = st.blocks; out[1] = st.eligible; out[2] = st.refused;
    return rc;
}

extern "C" int emul_emit_pairs_exhaustive(uint64_t *out)
{
    Stats st{};
    int rc = exhaustive8(3, st);
    if (!rc) rc = exhaustive8(4, st);
    out[0] = st.blocks; out[1] = st.eligible; out[2] = st.refused;
    return rc;
}

#ifdef EMIT_PAIRS_EMUL_MAIN
int main()
{
    uint64_t a[3], b[3];
    const int r1 = emul_emit_pairs(100000, 1, a), r2 = emul_emit_pairs_exhaustive(b);
    if (r1 || r2) {
        printf("emit_pairs_emul FAILED: sweep %d exhaustive %d\n", r1, r2);
        return 1;
    }
    printf("emit_pairs_emul ok: %llu blocks (%llu eligible), exhaustive %llu\n", (unsigned long long)a[0],
           (unsigned long long)a[1], (unsigned long long)b[0]);
    return 0;
}
#endif
