// aec_enc_analyze.inc -- the body of k_analyze and k_analyze_chunks (aec_enc.hip), included inside both kernels.
// A wavefront analyses segments [AEC_WAVE_INDEX * segs_per_wave, + segs_per_wave) of the input that c describes, clipped
// at c.total_segs.  It reads the names c, in, meta, seg_bits, seg_clamp, segs_per_wave, fast_ok: k_analyze's parameters;
// in k_analyze_chunks the chunk's own counts, input and array bases, formed by its prologue.  (Text shared by inclusion
// and not through a function: as a function it moved the registers of the existing kernels, DESIGN.md section 4.)
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (scalar: segment geometry and addresses then run on the SALU)
    const uint32_t bs = BS ? (uint32_t)BS : c.bs;
    const uint32_t stride = Rows<BS, BYTES>::stride_words(bs);
    uint32_t *rows = smem + (size_t)wave * 64u * stride;

    const uint64_t gwave = AEC_WAVE_INDEX;
    uint64_t sg = gwave * segs_per_wave;
    uint64_t sg_end = sg + segs_per_wave;
    if (sg_end > c.total_segs) sg_end = c.total_segs;

    Feeder<BS, BYTES> feeder;
    feeder.init(c, fast_ok);
    Seg g = seg_geom(c, sg < sg_end ? sg : 0);
    if (Feeder<BS, BYTES>::DIRECT) {
        // small blocks: lane = block from the load on, nothing goes through the rows (Feeder::DIRECT)
        if (sg < sg_end) feeder.prefetch_direct(c, in, g, lane);
        for (; sg < sg_end; sg++) {
            const auto cur = feeder.pre_direct;
            const Seg gcur = g;
            if (sg + 1 < sg_end) g = seg_next(c, g);
            feeder.prefetch_direct(c, in, g, lane);       // the next segment's loads fly during this one
            if (feeder.direct_ok(c, gcur)) {
                uint32_t w[BS ? BS / 2 : 1];
                direct_finish<(Feeder<BS, BYTES>::DIRECT ? BS : 8), (Feeder<BS, BYTES>::DIRECT ? BYTES : 1)>(c, gcur, cur, lane, w);
                analyze_body<BS, BYTES>(c, gcur, rows, stride, lane, sg, meta, seg_bits, seg_clamp, w);
            } else {
                feeder.feed_now(c, in, gcur, rows, stride, lane);
                analyze_body<BS, BYTES>(c, gcur, rows, stride, lane, sg, meta, seg_bits, seg_clamp);
            }
        }
        return;
    }
    if (sg < sg_end) feeder.prefetch(c, in, g, lane);
    for (; sg < sg_end; sg++) {
        const auto cur = feeder.pre;
        const Seg gcur = g;
        if (sg + 1 < sg_end) g = seg_next(c, g);
        feeder.prefetch(c, in, g, lane);          // next segment's loads fly during this one
        feeder.feed(c, in, gcur, cur, rows, stride, lane);
        analyze_body<BS, BYTES>(c, gcur, rows, stride, lane, sg, meta, seg_bits, seg_clamp);
    }
