// aec_enc_pack.inc -- the body of k_pack and k_pack_chunks (aec_enc.hip), included inside both kernels.
// A wavefront packs segments [AEC_WAVE_INDEX * segs_per_wave, + segs_per_wave) of the input that c describes, clipped at
// c.total_segs.  It reads the names c, in, meta, seg_start, seg_kin, out_words, cap_words, segs_per_wave, obuf_words,
// fast_ok: k_pack's parameters; in k_pack_chunks the chunk's own counts, input and array bases, formed by its prologue.
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (scalar: segment geometry and addresses then run on the SALU)
    const uint32_t bs = BS ? (uint32_t)BS : c.bs;
    const uint32_t stride = Rows<BS, BYTES>::stride_words(bs);
    const uint32_t per_wave = 64u * stride + obuf_words;
    uint32_t *rows = smem + (size_t)wave * per_wave;
    uint32_t *obuf = rows + 64u * stride;
    const bool pp = c.flags & F_PREPROCESS, msb = c.flags & F_MSB;

    const uint64_t gwave = AEC_WAVE_INDEX;
    uint64_t sg = gwave * segs_per_wave;
    uint64_t sg_end = sg + segs_per_wave;
    if (sg_end > c.total_segs) sg_end = c.total_segs;

    Feeder<BS, BYTES> feeder;
    feeder.init(c, fast_ok);
    Seg gnext = seg_geom(c, sg < sg_end ? sg : 0);
    if (sg < sg_end) {
        if (Feeder<BS, BYTES>::DIRECT) feeder.prefetch_direct(c, in, gnext, lane);
        else feeder.prefetch(c, in, gnext, lane);
    }
    uint32_t pending = 0;        // open tail word of the previous segment (stream bit order)
    bool first_seg = true, carried_shared = false;
    // the image buffer starts out zero and every word is zeroed again when it is copied out
    for (uint32_t w = lane; w < obuf_words; w += kWave) obuf[w] = 0u;

    // what a segment needs from HBM besides its samples
    struct SegIn {
        uint32_t m, kin, ref_sample;
        uint64_t start;
    };
    auto seg_in = [&](const Seg &g, uint64_t sgi) {
        SegIn r;
        r.m = lane < g.nv ? meta[g.blk0 + lane] : meta_pack(0, OPT_ZCONT, 0, 0);
        r.kin = seg_kin[sgi];
        r.start = seg_start[sgi];
        r.ref_sample = 0;
        if (pp && g.b0 == 0 && lane == 0)
            r.ref_sample = load_sample_bytes(in + g.samp0 * c.bytes, c.bytes, msb) & low_mask32(c.bps);
        return r;
    };
    // emission of one segment from its rows and copy-out of the image
    auto do_segment = [&](const Seg &g, const uint32_t *seg_rows, const SegIn &si, uint64_t sgi, const uint32_t *direct) {
        const uint32_t lead = (uint32_t)(si.start & 31u);
        uint32_t total;
        emit_segment<BS, BYTES>(c, g, seg_rows, stride, obuf, lane, si.m, si.kin, lead, si.ref_sample, pending, total, direct);
        const uint32_t nwords = (lead + total + 31u) >> 5;

        // Copy the image out.  Only a word this wave does not own alone needs an atomic: the first
        // word of the wave's first segment (shared with the previous wave) and the open tail word of
        // its last segment.  An open tail in between is carried to the next segment in `pending`.
        const uint64_t gw = si.start >> 5;
        const uint32_t tail = (lead + total) & 31u;
        const bool last_seg = sgi + 1 == sg_end;
        const bool carry_tail = tail != 0 && !last_seg && nwords > 0;
        // word 0 also holds bits of another wave only in the wave's first segment, or when a one-word
        // segment carried that word along
        const bool left_shared = first_seg ? lead != 0 : carried_shared;
        const uint32_t tail_word = carry_tail ? obuf[nwords - 1] : 0u;   // uniform: every lane reads the same word
        for (uint32_t w = lane; w < nwords; w += kWave) {
            const uint32_t v = obuf[w];
            obuf[w] = 0u;
            const uint64_t idx = gw + w;
            const bool is_tail = w == nwords - 1 && tail != 0;
            if (idx < cap_words && !(is_tail && carry_tail)) {
                const bool shared = (w == 0 && left_shared) || is_tail;
                const uint32_t sv = bswap32(v);
                if (!shared)
                    out_words[idx] = sv;                 // (zero words too: nothing clears the buffer)
                else if (v != 0)
                    __hip_atomic_fetch_or(&out_words[idx], sv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        pending = tail_word;
        carried_shared = carry_tail && nwords == 1 && left_shared;
        first_seg = false;
        wave_lds_fence();
    };

    if (Feeder<BS, BYTES>::DIRECT) {
        // small blocks: lane = block from the load on, nothing goes through the rows (Feeder::DIRECT)
        for (; sg < sg_end; sg++) {
            const auto cur = feeder.pre_direct;
            const Seg g = gnext;
            const SegIn si = seg_in(g, sg);
            if (sg + 1 < sg_end) gnext = seg_next(c, gnext);
            feeder.prefetch_direct(c, in, gnext, lane);   // the next segment's loads fly during this one
            if (feeder.direct_ok(c, g)) {
                uint32_t w[BS ? BS / 2 : 1];
                direct_finish<(Feeder<BS, BYTES>::DIRECT ? BS : 8), (Feeder<BS, BYTES>::DIRECT ? BYTES : 1)>(c, g, cur, lane, w);
                do_segment(g, rows, si, sg, w);
            } else {
                feeder.feed_now(c, in, g, rows, stride, lane);
                do_segment(g, rows, si, sg, nullptr);
            }
        }
        return;
    }
    for (; sg < sg_end; sg++) {
        const auto cur = feeder.pre;
        const Seg g = gnext;
        // everything this segment needs from HBM is requested before the first wait (requesting the
        // summaries a segment ahead as well was tried: no gain, two registers too many)
        const SegIn si = seg_in(g, sg);
        if (sg + 1 < sg_end) gnext = seg_next(c, gnext);
        feeder.prefetch(c, in, gnext, lane);      // next segment's loads fly during this one
        feeder.feed(c, in, g, cur, rows, stride, lane);
        do_segment(g, rows, si, sg, nullptr);
    }
