// aec_gpu.hip -- device-resident batch API (include/aec_gpu.h): context, workspace, enqueue.
// No reference counterpart; this is the host-side seam between the libaec ABI front-end
// (aec_abi.cpp) / GPU-resident callers and the kernels in aec_enc.hip / aec_dec.hip.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "../../include/aec_gpu.h"
#include "aec_cfg.h"
#include <cstdio>
#include <cstdlib>

#include "aec_chunks.h"
#include "aec_dchunks.h"
#include "aec_bsmall.h"
#include "aec_devbuf.h"
#include "aec_est.h"
#include "aec_kernels.h"

using namespace aec;

struct aec_gpu_ctx {
    int device = 0;
    bool profiling = false;    // record PhaseEvents around the kernels of the next calls
    // One event set per call, in a ring, so that a caller can time every launch of a loop without
    // synchronising inside it; aec_gpu_phase_ms() averages over the sets recorded since profiling
    // was switched on (the last kProfRing of them).
    static constexpr unsigned kProfRing = 32;
    PhaseEvents ev[kProfRing] = {};
    unsigned enc_calls = 0, dec_calls = 0;
    // an emit-only call continues the set its plan call opened (its "scan" then spans the host's
    // plan exchange between the two calls)
    const PhaseEvents *enc_events(uint32_t phases)
    {
        if (!profiling) return nullptr;
        if ((phases & ENC_PLAN) || enc_calls == 0) enc_calls++;
        return &ev[(enc_calls - 1) % kProfRing];
    }
    const PhaseEvents *dec_events() { return profiling ? &ev[dec_calls++ % kProfRing] : nullptr; }
    SegEntry *seg_table = nullptr;   // where the next encode / emit calls also leave the segment table (or null)
    uint64_t idx_hint = 0;     // caller's estimate of the coded RSI size in bits (0 = derive from max_rsi)
    uint64_t idx_used_hint = 0;  // ... and what the last index pass worked with (sizes the rings of the decode behind it)
    bool seg_filled = false;   // the last index pass with a segment-start table filled it (it ran over the trunk tables)
    uint64_t idx_stop_near = 0;  // the next index pass is a piece of a longer stream (aec_gpu_set_index_piece)
    int chunks_index = BS_PLANNED;   // how the bare chunk index passes run (aec_gpu_set_chunks_index) ...
    uint64_t chunks_round_bits = 0;  // ... and the budget of a round of the every-bit scheme (0: the default)

    // Device memory, grown on demand (aec_devbuf.h: replace) and kept between calls:
    DevBuf ws;             // workspace of the two-pass encoder (plan / emit: per-block summaries, segment scan)
    DevBuf idx_ws;         // speculative index tables (aec_idx.hip)
    DevBuf dec_ws;         // workspace of the segment-wise decode of bare streams (aec_dec.hip: launch_decode_bare)
    DevBuf range_ws;       // whole blocks of a range decode whose window does not start on an RSI / end on a block
    DevBuf chunks_d;       // the chunk calls: the descriptors and the per-wave / per-item table
    DevBuf sz_d;           // the SZIP chunk calls (aec_sz.hip): their descriptors and per-wave table, which must outlive
                           // the coder call in between (that call re-sends into chunks_d and may free it to grow it)
    // ... of which aec_gpu_held_bytes counts, aec_gpu_trim frees and aec_gpu_destroy releases these: a new one goes here
    // (pointers into the context itself, which is never copied)
    DevBuf *const held[6] = {&ws, &idx_ws, &dec_ws, &range_ws, &chunks_d, &sz_d};
    DevBuf carry;          // device record: what precedes this context's shard (emit_planned); a ShardCarry, never trimmed
    // the pinned buffers the chunk calls write their descriptors to -- kChunkStages, taken in turn, each guarded by the
    // event of its last transfer (stage_descriptors / send_descriptors); never trimmed
    static constexpr unsigned kChunkStages = 2;
    struct ChunkStage {
        DevBuf h{true};
        hipEvent_t ev = nullptr;
    } stage[kChunkStages];
    unsigned chunks_calls = 0;
};
static_assert(sizeof(aec_gpu_seg_entry) == sizeof(SegEntry), "segment table layout");

static_assert(sizeof(aec_gpu_enc_result) == sizeof(EncResult), "result layout");
static_assert(sizeof(aec_gpu_dec_result) == sizeof(DecResult), "result layout");
static_assert(sizeof(aec_gpu_estimate) == sizeof(EstResult) && AEC_GPU_ESTIMATE_SIZES == kEstSizes, "result layout");

static int cfg_from(const aec_gpu_params *p, size_t in_bytes, bool enc, Cfg *c)
{
    return make_cfg(p->bits_per_sample, p->block_size, p->rsi, p->flags, in_bytes, enc, c);
}

extern "C" {

int aec_gpu_create(aec_gpu_ctx **out)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return RC_MEM_ERROR;
    aec_gpu_ctx *ctx = new (std::nothrow) aec_gpu_ctx;
    if (!ctx) return RC_MEM_ERROR;
    ctx->device = dev;
    *out = ctx;
    return RC_OK;
}

void aec_gpu_destroy(aec_gpu_ctx *ctx)
{
    if (!ctx) return;
    for (DevBuf *b : ctx->held) b->release();
    ctx->carry.release();
    for (auto &s : ctx->stage) {
        s.h.release();
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
    for (auto &set : ctx->ev)
        for (auto &e : set.ev)
            if (e) (void)hipEventDestroy(e);
    delete ctx;
}

int aec_gpu_check_params(const aec_gpu_params *p, int for_encode)
{
    Cfg c;
    return cfg_from(p, 0, for_encode != 0, &c);
}

size_t aec_gpu_encode_bound(const aec_gpu_params *p, size_t in_bytes)
{
    Cfg c;
    if (cfg_from(p, in_bytes, true, &c) != RC_OK) return 0;
    return (max_encoded_bytes(c) + 15 + 16) & ~(size_t)15;
}

uint64_t aec_gpu_rsi_count(const aec_gpu_params *p, size_t in_bytes)
{
    Cfg c;
    if (cfg_from(p, in_bytes, true, &c) != RC_OK) return 0;
    return c.rsi_count;
}

uint64_t aec_gpu_block_count(const aec_gpu_params *p, size_t in_bytes)
{
    Cfg c;
    if (cfg_from(p, in_bytes, true, &c) != RC_OK) return 0;
    return c.total_blocks;
}

// reserves the workspace of the two-pass encoder for c (exactly what it needs) and points ws into it
// (whole: for a plain whole encode, which may code every block once and then needs that route's area: aec_enc_local.h)
static int reserve_two_pass(aec_gpu_ctx *ctx, const Cfg &c, EncWorkspace *ws, bool whole = false)
{
    size_t o[6], local = 0;
    const size_t need = enc_workspace_bytes(c, &o[0], &o[1], &o[2], &o[3], &o[4], &o[5], whole ? &local : nullptr);
    if (!ctx->ws.replace(need, need)) {
        // no room for the route's area: the analyze / scan / pack kernels, which need an eighth of the input
        if (!local) return RC_MEM_ERROR;
        (void)hipGetLastError();
        return reserve_two_pass(ctx, c, ws, false);
    }
    uint8_t *base = static_cast<uint8_t *>(ctx->ws.p);
    *ws = EncWorkspace{};
    ws->meta = reinterpret_cast<uint32_t *>(base + o[0]);
    ws->seg_bits = reinterpret_cast<uint32_t *>(base + o[1]);
    ws->seg_clamp = reinterpret_cast<uint16_t *>(base + o[2]);
    ws->seg_start = reinterpret_cast<uint64_t *>(base + o[3]);
    ws->seg_kin = base + o[4];
    ws->partials = reinterpret_cast<ScanPartial *>(base + o[5]);
    if (local) ws->local = base + local;
    return RC_OK;
}

// the one condition every enqueueing call closes on: no launch of this call has failed
static int launched() { return hipGetLastError() == hipSuccess ? RC_OK : RC_MEM_ERROR; }

// the public records, tables and chunk records are the kernels' own (the static_asserts above and below)
static EncResult *rec(aec_gpu_enc_result *r) { return reinterpret_cast<EncResult *>(r); }
static const EncResult *rec(const aec_gpu_enc_result *r) { return reinterpret_cast<const EncResult *>(r); }
static DecResult *rec(aec_gpu_dec_result *r) { return reinterpret_cast<DecResult *>(r); }
static const DecResult *rec(const aec_gpu_dec_result *r) { return reinterpret_cast<const DecResult *>(r); }
static const SegEntry *segs(const aec_gpu_seg_entry *t) { return reinterpret_cast<const SegEntry *>(t); }
static BatchChunk *chunk_recs(aec_gpu_batch_chunk *c) { return reinterpret_cast<BatchChunk *>(c); }

int aec_gpu_reserve(aec_gpu_ctx *ctx, const aec_gpu_params *p, size_t in_bytes)
{
    Cfg c;
    const int rc = cfg_from(p, in_bytes, true, &c);
    if (rc != RC_OK) return rc;
    // what aec_gpu_encode_async needs; the (much larger) workspace of the plan / emit pair is
    // allocated by the first plan call
    EncWorkspace ws;
    return reserve_two_pass(ctx, c, &ws, true);
}

static int encode_phases(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                         void *d_out, size_t out_cap, unsigned int start_bit, unsigned int k_in,
                         uint64_t *d_rsi_bit_offsets, aec_gpu_enc_result *d_result, void *stream, uint32_t phases,
                         const ShardCarry *d_carry = nullptr)
{
    Cfg c;
    int rc = cfg_from(p, in_bytes, true, &c);
    if (rc != RC_OK) return rc;
    if (start_bit > 7 || k_in > 31) return RC_CONF_ERROR;
    if ((phases & ENC_EMIT) && ((reinterpret_cast<uintptr_t>(d_out) & 15u) || (out_cap & 15u) || out_cap < 16))
        return RC_CONF_ERROR;
    EncWorkspace ws;
    rc = reserve_two_pass(ctx, c, &ws, phases == ENC_ALL && !d_carry);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();   // only launch errors of THIS call are reported below
    launch_encode(c, static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(d_out), out_cap, start_bit,
                  k_in, ws, d_rsi_bit_offsets, rec(d_result), static_cast<hipStream_t>(stream), ctx->enc_events(phases),
                  phases, ctx->seg_table, d_carry);
    return launched();
}

int aec_gpu_encode_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                         void *d_out, size_t out_cap, unsigned int start_bit, unsigned int k_in,
                         uint64_t *d_rsi_bit_offsets, aec_gpu_enc_result *d_result, void *stream)
{
    return encode_phases(ctx, p, d_in, in_bytes, d_out, out_cap, start_bit, k_in, d_rsi_bit_offsets, d_result,
                         stream, ENC_ALL);
}

int aec_gpu_encode_plan_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                              aec_gpu_enc_result *d_result, void *stream)
{
    return encode_phases(ctx, p, d_in, in_bytes, nullptr, 0, 0, 0, nullptr, d_result, stream, ENC_PLAN);
}

int aec_gpu_encode_emit_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                              void *d_out, size_t out_cap, unsigned int start_bit, unsigned int k_in,
                              uint64_t *d_rsi_bit_offsets, aec_gpu_enc_result *d_result, void *stream)
{
    return encode_phases(ctx, p, d_in, in_bytes, d_out, out_cap, start_bit, k_in, d_rsi_bit_offsets, d_result,
                         stream, ENC_EMIT);
}

int aec_gpu_encode_emit_planned_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                                      void *d_out, size_t out_cap, const aec_gpu_enc_result *d_plans,
                                      unsigned int rank, uint64_t *d_rsi_bit_offsets, aec_gpu_enc_result *d_result,
                                      void *stream)
{
    if (!d_plans || rank >= 64) return RC_CONF_ERROR;
    if (!ctx->carry.replace(sizeof(ShardCarry), sizeof(ShardCarry))) return RC_MEM_ERROR;
    ShardCarry *carry = static_cast<ShardCarry *>(ctx->carry.p);
    launch_shard_carry(rec(d_plans), rank, carry, static_cast<hipStream_t>(stream));
    return encode_phases(ctx, p, d_in, in_bytes, d_out, out_cap, 0, 0, d_rsi_bit_offsets, d_result, stream,
                         ENC_EMIT, carry);
}

int aec_gpu_stitch_async(const void *d_gathered, size_t slot_bytes, const aec_gpu_enc_result *d_plans,
                         unsigned int world, void *d_stream, size_t stream_cap, uint64_t *d_total_bytes,
                         void *stream)
{
    if (!d_gathered || !d_plans || !d_stream || world == 0 || world > 64 || (slot_bytes & 15u) ||
        (reinterpret_cast<uintptr_t>(d_gathered) & 15u) || (reinterpret_cast<uintptr_t>(d_stream) & 15u))
        return RC_CONF_ERROR;
    (void)hipGetLastError();
    launch_stitch(static_cast<const uint8_t *>(d_gathered), slot_bytes, rec(d_plans), world, static_cast<uint8_t *>(d_stream),
                  stream_cap, d_total_bytes, static_cast<hipStream_t>(stream));
    return launched();
}

int aec_gpu_decode_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                         const uint64_t *d_rsi_bit_offsets, uint64_t n_rsi, uint64_t total_blocks,
                         void *d_out, aec_gpu_dec_result *d_result, void *stream)
{
    Cfg c;
    const int rc = cfg_from(p, 0, false, &c);
    if (rc != RC_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_in) & 3u) return RC_CONF_ERROR;
    if (n_rsi && (total_blocks > n_rsi * c.rsi || total_blocks <= (n_rsi - 1) * c.rsi)) return RC_CONF_ERROR;
    (void)hipGetLastError();
    if (!launch_decode(c, static_cast<const uint8_t *>(d_in), in_bytes, d_rsi_bit_offsets, n_rsi, total_blocks,
                       static_cast<uint8_t *>(d_out), rec(d_result), static_cast<hipStream_t>(stream), ctx->dec_events()))
        return RC_MEM_ERROR;
    return launched();
}

int aec_gpu_decode_range_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                               const uint64_t *d_rsi_bit_offsets, uint64_t n_offsets, uint64_t pos, uint64_t size,
                               void *d_out, aec_gpu_dec_result *d_result, void *stream)
{
    Cfg c;
    const int rc = cfg_from(p, 0, false, &c);
    if (rc != RC_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_in) & 3u) return RC_CONF_ERROR;
    const uint64_t blk_bytes = (uint64_t)c.bs * c.bytes, rsi_bytes = blk_bytes * c.rsi;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    DecResult *res = rec(d_result);
    (void)hipGetLastError();
    if (size == 0) {
        if (!launch_decode_range(c, static_cast<const uint8_t *>(d_in), in_bytes, d_rsi_bit_offsets, 0, false, 0, nullptr,
                                 res, st))
            return RC_MEM_ERROR;
        return launched();
    }
    if (pos + size < pos) return RC_CONF_ERROR;
    // the RSIs the window needs, and its blocks from the first of them on: the last RSI ends behind the block that
    // holds the window's last byte
    const uint64_t r0 = pos / rsi_bytes, r1 = (pos + size - 1) / rsi_bytes;
    if (r1 >= n_offsets) return RC_CONF_ERROR;
    const uint64_t n_rsi = r1 - r0 + 1, first = r0 * rsi_bytes;
    const uint64_t total_blocks = (pos + size - first + blk_bytes - 1) / blk_bytes;
    // Whole blocks from the window's first RSI on land where the window's bytes go when the window starts on that
    // RSI and ends on a block; else they go to the context's workspace and the window is copied out of it.
    uint8_t *out = static_cast<uint8_t *>(d_out);
    const bool direct = pos == first && size % blk_bytes == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
    if (!direct) {
        const size_t need = (size_t)(total_blocks * blk_bytes);
        if (!ctx->range_ws.replace(need, (need + need / 4 + 255) & ~(size_t)255)) return RC_MEM_ERROR;
        out = static_cast<uint8_t *>(ctx->range_ws.p);
    }
    if (!launch_decode_range(c, static_cast<const uint8_t *>(d_in), in_bytes, d_rsi_bit_offsets + r0, n_rsi,
                             r1 + 1 < n_offsets, total_blocks, out, res, st, ctx->dec_events()))
        return RC_MEM_ERROR;
    if (!direct && hipMemcpyAsync(d_out, out + (pos - first), (size_t)size, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return RC_MEM_ERROR;
    return launched();
}

uint64_t aec_gpu_segment_count(const aec_gpu_params *p, size_t in_bytes)
{
    Cfg c;
    if (cfg_from(p, in_bytes, true, &c) != RC_OK) return 0;
    return c.total_segs;
}

void aec_gpu_set_segment_table(aec_gpu_ctx *ctx, aec_gpu_seg_entry *d_table)
{
    ctx->seg_table = reinterpret_cast<SegEntry *>(d_table);
}

int aec_gpu_decode_segments_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                                  const aec_gpu_seg_entry *d_seg_table, uint64_t n_seg, uint64_t total_blocks,
                                  void *d_out, aec_gpu_dec_result *d_result, void *stream)
{
    Cfg c;
    const int rc = cfg_from(p, 0, false, &c);
    if (rc != RC_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_in) & 3u) return RC_CONF_ERROR;
    // n_seg must be the segment count of total_blocks
    const uint64_t full = total_blocks / c.rsi, rem = total_blocks % c.rsi;
    if (n_seg != full * c.segs_per_rsi + (rem + 63) / 64) return RC_CONF_ERROR;
    (void)hipGetLastError();
    if (!launch_decode_segments(c, static_cast<const uint8_t *>(d_in), in_bytes, segs(d_seg_table), n_seg, total_blocks,
                                static_cast<uint8_t *>(d_out), rec(d_result), static_cast<hipStream_t>(stream),
                                ctx->dec_events()))
        return RC_MEM_ERROR;
    return launched();
}

static int index_common(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                        uint64_t start_bit, uint32_t start_block, uint64_t rsi_start_bit,
                        uint64_t *d_rsi_bit_offsets, uint64_t max_rsi, aec_gpu_dec_result *d_result, void *stream,
                        uint32_t tail_slot, uint64_t *d_seg_bits = nullptr)
{
    Cfg c;
    const int rc = cfg_from(p, 0, false, &c);
    if (rc != RC_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_in) & 3u) return RC_CONF_ERROR;
    if (start_block >= c.rsi || (start_block && rsi_start_bit > start_bit)) return RC_CONF_ERROR;
    (void)hipGetLastError();
    // Table workspace of the trunk index, sized from the average coded RSI: the caller's hint, else input
    // bits / expected RSIs.  A failed allocation only means the serial walk.
    const uint64_t in_bits = (uint64_t)in_bytes * 8;
    const uint64_t hint = ctx->idx_hint ? ctx->idx_hint
                          : ((max_rsi && in_bits > start_bit) ? (in_bits - start_bit) / max_rsi : 0);
    const size_t need = index_workspace_bytes(c, in_bytes, start_bit, hint);
    if (!ctx->idx_ws.replace(need, need + need / 16)) {
        // (the every-bit scheme's tables are the largest by far for what they serve -- up to 270 MB for a 2 MiB
        // stream: without them before the serial walk)
        const size_t less = index_workspace_bytes_large(c, in_bytes, start_bit, hint);
        if (less && less < need) (void)ctx->idx_ws.replace(less, less);
    }
    ctx->idx_used_hint = hint;
    if (d_seg_bits && !decode_bare_supported(c)) d_seg_bits = nullptr;
    if (d_seg_bits && hipMemsetAsync(d_seg_bits, 0xFF, (size_t)(max_rsi + 1) * c.segs_per_rsi * 8, static_cast<hipStream_t>(stream)) != hipSuccess)
        return RC_MEM_ERROR;
    ctx->seg_filled = launch_index(c, static_cast<const uint8_t *>(d_in), in_bytes, start_bit, d_rsi_bit_offsets, max_rsi,
                                   rec(d_result), static_cast<hipStream_t>(stream), ctx->idx_ws.p,
                                   ctx->idx_ws.cap, hint, start_block, rsi_start_bit, tail_slot, d_seg_bits, ctx->idx_stop_near);
    ctx->idx_stop_near = 0;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess && getenv("AEC_ABI_TRACE"))
        fprintf(stderr, "aec_gpu_index_async: %s (in_bytes %zu start %llu max_rsi %llu hint %llu ws %zu)\n",
                hipGetErrorString(e), in_bytes, (unsigned long long)start_bit, (unsigned long long)max_rsi,
                (unsigned long long)hint, ctx->idx_ws.cap);
    return e == hipSuccess ? RC_OK : RC_MEM_ERROR;
}

int aec_gpu_index_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                        uint64_t start_bit, uint64_t *d_rsi_bit_offsets, uint64_t max_rsi,
                        aec_gpu_dec_result *d_result, void *stream)
{
    return index_common(ctx, p, d_in, in_bytes, start_bit, 0u, start_bit, d_rsi_bit_offsets, max_rsi, d_result,
                        stream, 0u);
}

int aec_gpu_index_resume_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                               uint64_t start_bit, unsigned int start_block, uint64_t rsi_start_bit,
                               uint64_t *d_rsi_bit_offsets, uint64_t max_rsi, aec_gpu_dec_result *d_result,
                               void *stream)
{
    return index_common(ctx, p, d_in, in_bytes, start_bit, start_block, rsi_start_bit, d_rsi_bit_offsets, max_rsi,
                        d_result, stream, 1u);
}

int aec_gpu_decode_indexed_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                                 const uint64_t *d_rsi_bit_offsets, uint64_t max_rsi,
                                 const aec_gpu_dec_result *d_index_result, void *d_out,
                                 aec_gpu_dec_result *d_result, void *stream)
{
    Cfg c;
    const int rc = cfg_from(p, 0, false, &c);
    if (rc != RC_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(d_in) & 3u) || !d_index_result || d_index_result == d_result)
        return RC_CONF_ERROR;
    (void)hipGetLastError();
    if (!launch_decode(c, static_cast<const uint8_t *>(d_in), in_bytes, d_rsi_bit_offsets, max_rsi,
                       max_rsi * c.rsi, static_cast<uint8_t *>(d_out), rec(d_result), static_cast<hipStream_t>(stream),
                       ctx->dec_events(), rec(d_index_result)))
        return RC_MEM_ERROR;
    launch_decode_partial(c, static_cast<const uint8_t *>(d_in), in_bytes, rec(d_index_result),
                          static_cast<uint8_t *>(d_out), rec(d_result), static_cast<hipStream_t>(stream));
    return launched();
}

unsigned int aec_gpu_segments_per_rsi(const aec_gpu_params *p)
{
    Cfg c;
    return cfg_from(p, 0, false, &c) == RC_OK ? c.segs_per_rsi : 0u;
}

int aec_gpu_index_segments_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                                 uint64_t start_bit, unsigned int start_block, uint64_t rsi_start_bit,
                                 uint64_t *d_rsi_bit_offsets, uint64_t *d_seg_bits, uint64_t max_rsi,
                                 aec_gpu_dec_result *d_result, void *stream)
{
    return index_common(ctx, p, d_in, in_bytes, start_bit, start_block, start_block ? rsi_start_bit : start_bit,
                        d_rsi_bit_offsets, max_rsi, d_result, stream, 1u, d_seg_bits);
}

int aec_gpu_decode_bare_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                              const uint64_t *d_rsi_bit_offsets, const uint64_t *d_seg_bits, uint64_t max_rsi,
                              uint64_t total_blocks, const aec_gpu_dec_result *d_index_result, void *d_out,
                              aec_gpu_dec_result *d_result, void *stream)
{
    Cfg c;
    const int rc = cfg_from(p, 0, false, &c);
    if (rc != RC_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(d_in) & 3u) || d_index_result == d_result) return RC_CONF_ERROR;
    (void)hipGetLastError();
    // (segment starts the last index pass of this context did not fill are no use: every RSI by one lane then)
    const bool seg = d_seg_bits && ctx->seg_filled && decode_bare_supported(c);
    if (seg) {
        const size_t need = decode_bare_workspace_bytes(c, max_rsi);
        (void)ctx->dec_ws.replace(need, need + need / 8);      // (a failure: every RSI by one lane)
    }
    const DecResult *idx = rec(d_index_result);
    if (!launch_decode_bare(c, static_cast<const uint8_t *>(d_in), in_bytes, d_rsi_bit_offsets, seg ? d_seg_bits : nullptr,
                            max_rsi, idx ? max_rsi * c.rsi : total_blocks, static_cast<uint8_t *>(d_out),
                            rec(d_result), static_cast<hipStream_t>(stream), ctx->dec_events(),
                            idx, ctx->dec_ws.p, ctx->dec_ws.cap, ctx->idx_used_hint / c.rsi))
        return RC_MEM_ERROR;
    if (idx)
        launch_decode_partial(c, static_cast<const uint8_t *>(d_in), in_bytes, idx, static_cast<uint8_t *>(d_out),
                              rec(d_result), static_cast<hipStream_t>(stream));
    return launched();
}

void aec_gpu_set_index_hint(aec_gpu_ctx *ctx, uint64_t rsi_bits) { ctx->idx_hint = rsi_bits; }
void aec_gpu_set_index_piece(aec_gpu_ctx *ctx, uint64_t stop_near_bits) { ctx->idx_stop_near = stop_near_bits; }
void aec_gpu_set_chunks_index(aec_gpu_ctx *ctx, int how, uint64_t round_bits)
{
    ctx->chunks_index = (how == AEC_GPU_CHUNKS_INDEX_SERIAL || how == AEC_GPU_CHUNKS_INDEX_EVERY_BIT) ? how : AEC_GPU_CHUNKS_INDEX_PLANNED;
    ctx->chunks_round_bits = round_bits;
}

int aec_gpu_index_is_windowed(const aec_gpu_params *p, size_t in_bytes, uint64_t rsi_bits)
{
    Cfg c;
    return cfg_from(p, 0, false, &c) == RC_OK && index_is_windowed(c, in_bytes, rsi_bits) ? 1 : 0;
}

int aec_gpu_index_scheme(const aec_gpu_params *p, size_t in_bytes, uint64_t rsi_bits, unsigned int start_block)
{
    Cfg c;
    if (cfg_from(p, 0, false, &c) != RC_OK) return 0;
    return index_scheme(c, in_bytes, rsi_bits, start_block);
}

int aec_gpu_index_plan(const aec_gpu_params *p, size_t in_bytes, uint64_t rsi_bits, unsigned int start_block,
                       int want_segments, int piece, size_t ws_bytes, int schemes[AEC_GPU_INDEX_STAGES], size_t *ws_asked,
                       size_t *ws_large, size_t *ws_used)
{
    static_assert(AEC_GPU_INDEX_STAGES == kIdxMaxStages, "aec_gpu.h and aec_kernels.h disagree");
    Cfg c;
    if (!schemes || !ws_asked || !ws_large || !ws_used || cfg_from(p, 0, false, &c) != RC_OK) return -1;
    *ws_asked = index_workspace_bytes(c, in_bytes, 0, rsi_bits);
    *ws_large = index_workspace_bytes_large(c, in_bytes, 0, rsi_bits);
    return index_plan(c, in_bytes, rsi_bits, start_block, want_segments != 0, piece != 0, ws_bytes, schemes, ws_used);
}

void aec_gpu_trim(aec_gpu_ctx *ctx, size_t keep_bytes)
{
    for (DevBuf *b : ctx->held)
        if (b->cap > keep_bytes) b->release();
}

size_t aec_gpu_held_bytes(const aec_gpu_ctx *ctx)
{
    size_t sum = 0;
    if (ctx)
        for (const DevBuf *b : ctx->held) sum += b->cap;
    return sum;
}

// ---- the coded size under block sizes 8, 16, 32 and 64 in one pass (aec_est.h, aec_est.hip) -----------------------------
int aec_gpu_estimate_plan(const aec_gpu_params *p, const unsigned int *rsi, size_t in_bytes,
                          struct aec_gpu_estimate_plan *plan)
{
    if (!p || !plan) return 0;
    EstCfg e;
    size_t need = 0;
    if (make_est_cfg(p->bits_per_sample, p->flags, rsi, p->rsi, in_bytes, &e, &need) != RC_OK) return 0;
    plan->evaluated = e.mask;
    plan->pad = 0;
    plan->workspace_bytes = need;
    return 1;
}

int aec_gpu_estimate_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                           const unsigned int *rsi, aec_gpu_estimate *d_estimate, void *stream)
{
    if (!ctx || !p || !d_estimate) return RC_CONF_ERROR;
    EstCfg e;
    size_t need = 0;
    const int rc = make_est_cfg(p->bits_per_sample, p->flags, rsi, p->rsi, in_bytes, &e, &need);
    if (rc != RC_OK) return rc;
    if (e.pieces && (!d_in || (reinterpret_cast<uintptr_t>(d_in) & 15u))) return RC_CONF_ERROR;
    // the records of all four sizes come out of the encoder's workspace: no encode of this context is under way
    if (!ctx->ws.replace(need, need)) return RC_MEM_ERROR;
    (void)hipGetLastError();
    launch_estimate(e, static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(ctx->ws.p),
                    reinterpret_cast<EstResult *>(d_estimate), static_cast<hipStream_t>(stream));
    return launched();
}

int aec_gpu_index_batch_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                              const uint64_t *d_chunk_offsets, uint64_t n_chunks, uint64_t rsi_per_chunk,
                              uint64_t *d_rsi_bit_offsets, aec_gpu_dec_result *d_results, void *stream)
{
    (void)ctx;
    Cfg c;
    const int rc = cfg_from(p, 0, false, &c);
    if (rc != RC_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(d_in) & 15u) || rsi_per_chunk == 0) return RC_CONF_ERROR;
    (void)hipGetLastError();
    launch_index_batch(c, static_cast<const uint8_t *>(d_in), in_bytes, d_chunk_offsets, n_chunks, rsi_per_chunk,
                       d_rsi_bit_offsets, rec(d_results), static_cast<hipStream_t>(stream));
    return launched();
}

int aec_gpu_batch_uses_tables(aec_gpu_ctx *ctx, const aec_gpu_params *p, size_t in_bytes, uint64_t n_chunks,
                              uint64_t rsi_per_chunk)
{
    Cfg c;
    if (cfg_from(p, 0, false, &c) != RC_OK || n_chunks == 0 || rsi_per_chunk == 0) return 0;
    const size_t mean = in_bytes / n_chunks;
    const uint64_t hint = ctx->idx_hint ? ctx->idx_hint : (uint64_t)mean * 8 / rsi_per_chunk;
    return mean >= ((size_t)16 << 10) && index_batch_workspace_bytes(c, in_bytes, n_chunks, mean * 2 + 65536, hint) != 0;
}

int aec_gpu_decode_batch_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                               const uint64_t *d_chunk_offsets, uint64_t n_chunks, uint64_t rsi_per_chunk,
                               uint64_t *d_rsi_bit_offsets, void *d_out, aec_gpu_dec_result *d_results,
                               aec_gpu_dec_result *d_result, void *stream)
{
    Cfg c;
    const int rc = cfg_from(p, 0, false, &c);
    if (rc != RC_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(d_in) & 15u) || rsi_per_chunk == 0 || rsi_per_chunk > 0xFFFFFFFFull)
        return RC_CONF_ERROR;
    if (n_chunks == 0) return RC_OK;
    (void)hipGetLastError();
    // Streams long enough for the window tables (low-entropy data, tens of KiB and more per stream): ONE
    // speculation launch for the whole buffer, then every stream's wavefront hops over the tables.  The largest
    // stream is not known here: the mean, with room to spare, sizes the hop lists.
    const size_t mean = in_bytes / n_chunks, max_chunk = mean * 2 + 65536;
    const uint64_t hint = ctx->idx_hint ? ctx->idx_hint : (uint64_t)mean * 8 / rsi_per_chunk;
    size_t need = mean >= ((size_t)16 << 10) ? index_batch_workspace_bytes(c, in_bytes, n_chunks, max_chunk, hint) : 0;
    (void)ctx->idx_ws.replace(need, need + need / 16);         // (a failure: the serial walk per stream)
    launch_index_batch(c, static_cast<const uint8_t *>(d_in), in_bytes, d_chunk_offsets, n_chunks, rsi_per_chunk,
                       d_rsi_bit_offsets, rec(d_results), static_cast<hipStream_t>(stream),
                       need ? ctx->idx_ws.p : nullptr, ctx->idx_ws.cap, max_chunk, hint);
    if (!launch_decode(c, static_cast<const uint8_t *>(d_in), in_bytes, d_rsi_bit_offsets, n_chunks * rsi_per_chunk,
                       n_chunks * rsi_per_chunk * c.rsi, static_cast<uint8_t *>(d_out), rec(d_result),
                       static_cast<hipStream_t>(stream), ctx->dec_events(), nullptr, rec(d_results), (uint32_t)rsi_per_chunk))
        return RC_MEM_ERROR;
    return launched();
}

int aec_gpu_encode_batch_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in,
                               const uint64_t *chunk_offsets_host, uint64_t n_chunks, void *d_out, size_t slot_bytes,
                               aec_gpu_enc_result *d_results, void *stream)
{
    if (!chunk_offsets_host || (slot_bytes & 15u) || (reinterpret_cast<uintptr_t>(d_out) & 15u)) return RC_CONF_ERROR;
    // every chunk is a stream of its own (k = 0, bit 0 of its slot): the chunks go through the encoder
    // kernels one after the other on `stream`, sharing the context's workspace; nothing comes back to the host
    for (uint64_t i = 0; i < n_chunks; i++) {
        const uint64_t lo = chunk_offsets_host[i], hi = chunk_offsets_host[i + 1];
        if (hi < lo || (lo & 15u)) return RC_CONF_ERROR;
        const int rc = encode_phases(ctx, p, static_cast<const uint8_t *>(d_in) + lo, (size_t)(hi - lo),
                                     static_cast<uint8_t *>(d_out) + i * slot_bytes, slot_bytes, 0, 0, nullptr,
                                     d_results + i, stream, ENC_ALL);
        if (rc != RC_OK) return rc;
    }
    return RC_OK;
}

int aec_gpu_encode_uniform_batch_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t chunk_bytes,
                                       uint64_t n_chunks, void *d_out, size_t out_cap, aec_gpu_batch_chunk *d_chunks,
                                       aec_gpu_enc_result *d_result, void *stream)
{
    static_assert(sizeof(aec_gpu_batch_chunk) == sizeof(BatchChunk), "public mirror of BatchChunk");
    if (!n_chunks || !chunk_bytes || (reinterpret_cast<uintptr_t>(d_out) & 15u) || (out_cap & 15u) || out_cap < 16)
        return RC_CONF_ERROR;
    Cfg one, c;
    int rc = cfg_from(p, chunk_bytes, true, &one);
    if (rc != RC_OK) return rc;
    const size_t rsi_bytes = (size_t)one.rsi * one.bs * one.bytes;
    if (chunk_bytes % rsi_bytes) return RC_CONF_ERROR;                       // whole RSIs only
    rc = cfg_from(p, chunk_bytes * n_chunks, true, &c);
    if (rc != RC_OK) return rc;
    if (!batch_uniform_ok(c, one.total_segs)) return RC_CONF_ERROR;          // (aec_gpu_uniform_batch_ok says so beforehand)
    EncWorkspace ws;
    rc = reserve_two_pass(ctx, c, &ws);
    if (rc != RC_OK) return rc;
    (void)hipGetLastError();
    launch_encode_uniform_batch(c, static_cast<const uint8_t *>(d_in), one.total_segs, static_cast<uint8_t *>(d_out),
                                out_cap, ws, chunk_recs(d_chunks), rec(d_result), static_cast<hipStream_t>(stream));
    return launched();
}

int aec_gpu_uniform_batch_ok(const aec_gpu_params *p, size_t chunk_bytes, uint64_t n_chunks)
{
    Cfg one, c;
    if (!n_chunks || !chunk_bytes || cfg_from(p, chunk_bytes, true, &one) != RC_OK) return 0;
    if (chunk_bytes % ((size_t)one.rsi * one.bs * one.bytes)) return 0;
    if (cfg_from(p, chunk_bytes * n_chunks, true, &c) != RC_OK) return 0;
    return batch_uniform_ok(c, one.total_segs) ? 1 : 0;
}

// ---- the descriptors of the chunk calls: host to device ------------------------------------------------------------------
// Both chunk calls write their descriptors to a pinned buffer of the context and send it to chunks_d in stream order.  The
// pinned buffers are taken in turn, whichever of the two calls comes (a context's calls are enqueued on one stream, so the
// copy waits for the kernels in front); the event of a buffer's last transfer says when that transfer has left it.
// Step 1: the pinned buffer whose turn it is, with room for h_need bytes and free to write.  null: no memory.
static aec_gpu_ctx::ChunkStage *stage_descriptors(aec_gpu_ctx *ctx, size_t h_need)
{
    aec_gpu_ctx::ChunkStage &s = ctx->stage[ctx->chunks_calls++ % aec_gpu_ctx::kChunkStages];
    if (!s.ev && hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) {
        s.ev = nullptr;
        (void)hipGetLastError();
        return nullptr;
    }
    if (s.h.p && hipEventSynchronize(s.ev) != hipSuccess) return nullptr;
    return s.h.replace(h_need, h_need + h_need / 4 + 4096) ? &s : nullptr;
}

// Step 2, once the descriptors are written: h_need bytes of the buffer to chunks_d (the SZIP layer: to sz_d), which has
// room for d_need bytes (descriptors and the table behind them).  Growing it synchronises the device -- no kernel still
// reads it -- hence after the host's work and before the copy.  Returns the buffer, null where there is no memory or the
// copy failed.
static uint8_t *send_descriptors(DevBuf &d, aec_gpu_ctx::ChunkStage *s, size_t h_need, size_t d_need, hipStream_t st)
{
    if (!d.replace(d_need, ctx_desc_room(d_need))) return nullptr;
    (void)hipGetLastError();   // only errors of THIS call are reported by it
    if (hipMemcpyAsync(d.p, s->h.p, h_need, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipEventRecord(s->ev, st) != hipSuccess)
        return nullptr;
    return static_cast<uint8_t *>(d.p);
}

// the same two steps for aec_sz.hip, which does not see the context (aec_kernels.h)
extern "C++" {
void *aec::ctx_sz_stage(aec_gpu_ctx *ctx, size_t h_need, void **h)
{
    aec_gpu_ctx::ChunkStage *s = stage_descriptors(ctx, h_need);
    if (s) *h = s->h.p;
    return s;
}

uint8_t *aec::ctx_sz_send(aec_gpu_ctx *ctx, void *stage, size_t h_need, size_t d_need, hipStream_t st)
{
    return send_descriptors(ctx->sz_d, static_cast<aec_gpu_ctx::ChunkStage *>(stage), h_need, d_need, st);
}
}  // extern "C++"

// ---- a batch of unequal chunks as one launch set (aec_chunks.h) -------------------------------------------------------
namespace {
struct ChunksShape {
    Cfg c;                  // the parameters with the sums of the chunks' samples, blocks, segments and RSIs
    uint64_t waves, entries;
    uint32_t spw;
    size_t out_bound, ws_bytes, desc_bytes, table_bytes;
};
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// host arithmetic of a batch; with desc (n + 1 entries) the descriptors are written too.  false = refused.
bool chunks_shape(const aec_gpu_params *p, const uint64_t *offsets, const uint64_t *bytes, uint64_t n, ChunksShape *sh,
                  ChunkDesc *desc)
{
    Cfg &c = sh->c;
    if (cfg_from(p, 0, true, &c) != RC_OK || (n && !bytes) || n > 0x7FFFFFFFull) return false;
    const uint64_t cds_bits = c.id_len + (uint64_t)c.bs * c.bps + 2;            // (max_encoded_bytes)
    uint64_t samples = 0, blocks = 0, segs = 0, entries = 0, bound = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t smp = bytes[i] / c.bytes;                                  // a fraction of a sample is ignored
        const ChunkCounts k = chunk_counts(smp, c.bs, c.rsi, c.segs_per_rsi);
        if (desc) desc[i] = ChunkDesc{offsets[i], smp, blocks, segs, entries, 0};
        samples += smp;
        blocks += k.blocks;
        segs += k.segs;
        entries += k.rsis + 1;
        const uint64_t most = (k.blocks * cds_bits + 7) / 8;
        bound += most ? most : 1;
        if (bound >> 48 || blocks >> 48) return false;
    }
    c.total_samples = samples;
    c.total_blocks = blocks;
    c.total_segs = segs;
    c.rsi_count = entries - n;
    sh->spw = chunks_segs_per_wave(c);
    uint64_t waves = 0;
    for (uint64_t i = 0; i < n; i++) {
        const ChunkCounts k = chunk_counts(bytes[i] / c.bytes, c.bs, c.rsi, c.segs_per_rsi);
        if (desc) desc[i].wave0 = waves;
        waves += (k.segs + sh->spw - 1) / sh->spw;
    }
    if (waves > 0x7FFFFFFFull) return false;
    if (desc) desc[n] = ChunkDesc{0, 0, blocks, segs, entries, waves};
    sh->waves = waves;
    sh->entries = entries;
    sh->out_bound = (size_t)((bound + 15) & ~(uint64_t)15) + 16;
    size_t o[6];
    sh->desc_bytes = up256((size_t)(n + 1) * sizeof(ChunkDesc));
    sh->table_bytes = up256((size_t)(waves ? waves : 1) * 4);
    sh->ws_bytes = enc_workspace_bytes(c, &o[0], &o[1], &o[2], &o[3], &o[4], &o[5]) + sh->desc_bytes + sh->table_bytes;
    return true;
}
}  // namespace

int aec_gpu_encode_chunks_plan(const aec_gpu_params *p, const uint64_t *chunk_bytes, uint64_t n_chunks,
                               aec_gpu_chunks_plan *plan)
{
    ChunksShape sh;
    if (!p || !plan || !chunks_shape(p, nullptr, chunk_bytes, n_chunks, &sh, nullptr)) return 0;
    plan->out_bound = sh.out_bound;
    plan->rsi_entries = sh.entries;
    plan->workspace_bytes = sh.ws_bytes;
    plan->waves = sh.waves;
    return 1;
}

int aec_gpu_encode_chunks_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, const uint64_t *chunk_offsets,
                                const uint64_t *chunk_bytes, uint64_t n_chunks, void *d_out, size_t out_cap,
                                aec_gpu_batch_chunk *d_chunks, uint64_t *d_rsi_bit_offsets, aec_gpu_enc_result *d_result,
                                void *stream)
{
    const int prc = aec_gpu_check_params(p, 1);
    if (prc != RC_OK) return RC_CONF_ERROR;
    if (n_chunks == 0) return RC_OK;
    if (!chunk_offsets || !chunk_bytes || !d_chunks || !d_result || (reinterpret_cast<uintptr_t>(d_out) & 15u) ||
        (out_cap & 15u) || out_cap < 16)
        return RC_CONF_ERROR;
    for (uint64_t i = 0; i < n_chunks; i++)
        if (chunk_offsets[i] & 15u) return RC_CONF_ERROR;
    const hipStream_t st = static_cast<hipStream_t>(stream);

    const size_t h_need = (size_t)(n_chunks + 1) * sizeof(ChunkDesc);
    aec_gpu_ctx::ChunkStage *stage = stage_descriptors(ctx, h_need);
    if (!stage) return RC_MEM_ERROR;
    ChunksShape sh;
    if (!chunks_shape(p, chunk_offsets, chunk_bytes, n_chunks, &sh, static_cast<ChunkDesc *>(stage->h.p))) return RC_CONF_ERROR;
    EncWorkspace ws;
    const int rc = reserve_two_pass(ctx, sh.c, &ws);
    if (rc != RC_OK) return rc;
    uint8_t *cd = send_descriptors(ctx->chunks_d, stage, h_need, sh.desc_bytes + sh.table_bytes, st);
    if (!cd) return RC_MEM_ERROR;
    const ChunksLaunch k{reinterpret_cast<const ChunkDesc *>(cd), reinterpret_cast<uint32_t *>(cd + sh.desc_bytes), n_chunks,
                         sh.waves, sh.spw};
    launch_encode_chunks(sh.c, static_cast<const uint8_t *>(d_in), k, static_cast<uint8_t *>(d_out), out_cap, ws,
                         chunk_recs(d_chunks), d_rsi_bit_offsets, rec(d_result), st);
    return launched();
}

// ---- a batch of unequal chunks decoded as one launch (aec_dchunks.h) ----------------------------------------------------
namespace {
struct DChunksShape {
    Cfg c;
    uint64_t items, entries, blocks;
    size_t out_bytes, desc_bytes, table_bytes;
};
// The most items a launch addresses: k_decode_wave takes a workgroup of two wavefronts per two items and a grid has at
// most 2^31 - 1 workgroups; the item table holds 32-bit chunk numbers, so as many chunks at most.
constexpr uint64_t kDChunksMaxItems = 0x7FFFFFFFull;

// host arithmetic of a batch; with desc (n + 1 entries) the descriptors are written too (packed rooms where out_offsets
// is NULL).  false = refused.
bool dchunks_shape(const aec_gpu_params *p, const uint64_t *in_offsets, const uint64_t *in_bytes_each,
                   const uint64_t *out_offsets, const uint64_t *out_bytes, uint64_t n, DChunksShape *sh, DChunkDesc *desc)
{
    Cfg &c = sh->c;
    if (cfg_from(p, 0, false, &c) != RC_OK || (n && !out_bytes) || n > kDChunksMaxItems) return false;
    const uint64_t blk_bytes = (uint64_t)c.bs * c.bytes;
    uint64_t items = 0, blocks = 0, packed = 0;
    for (uint64_t i = 0; i < n; i++) {
        const DChunkCounts k = dchunk_counts(out_bytes[i], c.bytes, c.bs, c.rsi);
        if (k.rsis > kDChunksMaxItems) return false;
        if (desc)
            desc[i] = DChunkDesc{in_offsets ? in_offsets[i] : 0, in_bytes_each ? in_bytes_each[i] : 0,
                                 out_offsets ? out_offsets[i] : packed, items, (uint32_t)k.rsis, k.last_blocks};
        items += k.rsis;
        blocks += k.blocks;
        packed += dchunk_room(k.blocks, blk_bytes);
        if (items > kDChunksMaxItems || packed >> 48) return false;
    }
    if (desc) desc[n] = DChunkDesc{0, 0, packed, items, 0u, 0u};
    sh->items = items;
    sh->entries = items + n;
    sh->blocks = blocks;
    sh->out_bytes = (size_t)packed;
    sh->desc_bytes = up256((size_t)(n + 1) * sizeof(DChunkDesc));
    sh->table_bytes = up256((size_t)(items ? items : 1) * 4);
    return true;
}
}  // namespace

int aec_gpu_decode_chunks_plan(const aec_gpu_params *p, const uint64_t *out_bytes, uint64_t n_chunks,
                               aec_gpu_dchunks_plan *plan)
{
    DChunksShape sh;
    if (!p || !plan || !dchunks_shape(p, nullptr, nullptr, nullptr, out_bytes, n_chunks, &sh, nullptr)) return 0;
    plan->items = sh.items;
    plan->rsi_entries = sh.entries;
    plan->out_bytes = sh.out_bytes;
    plan->workspace_bytes = sh.desc_bytes + sh.table_bytes;
    return 1;
}

// ---- the index pass of a batch of bare chunks (aec_bsmall.h; aec_idx.hip: launch_index_chunks) ----------------------------
namespace {
// What the pass of a batch needs beyond the chunk descriptors: the plan, its rounds, and -- behind the descriptors in the
// pinned buffer -- the slots and the unit table as they lie in the workspace from plan.o_slots on.
struct BareIndex {
    BsPlan plan{};
    std::vector<BsRound> rounds;
    size_t h_bytes = 0;
};
bool bare_index_plan(const Cfg &c, int how, uint64_t round_bits, const uint64_t *in_bytes_each, const uint64_t *out_bytes, uint64_t n,
                     BareIndex *b)
{
    // (the plan of a batch whose longest chunk the walker is through in the time of one round of the every-bit scheme takes
    // none -- bs_plan says so after a pass over the chunks that divides; here from the largest out_bytes alone: thousands
    // of small chunks are a call of a third of a millisecond, and the host's passes come in front of it)
    if (how == BS_PLANNED) {
        uint64_t most = 0;
        for (uint64_t i = 0; i < n; i++) most = out_bytes[i] > most ? out_bytes[i] : most;
        if ((most / c.bytes + c.bs - 1) / c.bs * kBsWalkNsPerBlock <= kBsFixedNs + kBsRoundNs) how = BS_SERIAL;
    }
    bs_plan(c, how, round_bits, in_bytes_each, out_bytes, n, &b->plan);
    b->h_bytes = b->plan.taken ? b->plan.o_e - b->plan.o_slots : 0;
    try {
        b->rounds.resize(b->plan.rounds);
    } catch (...) {
        return false;
    }
    return true;
}
// Writes slots and unit table to h (h_bytes of the pinned buffer), makes room in the context's index-table buffer and
// enqueues their copy.  The workspace, or null: no memory, or a plan that takes none -- the serial walk alone then.
uint8_t *bare_index_send(aec_gpu_ctx *ctx, const Cfg &c, const uint64_t *in_offsets, const uint64_t *in_bytes_each, const uint64_t *out_bytes,
                         uint64_t n, BareIndex *b, uint8_t *h, hipStream_t st)
{
    const BsPlan &pl = b->plan;
    if (!pl.taken) return nullptr;
    BsPlan again{};
    bs_pack(c, bs_round_bits(ctx->chunks_round_bits), in_offsets, in_bytes_each, out_bytes, n, pl.min_blocks, &again,
            reinterpret_cast<BsSlot *>(h), b->rounds.data(), reinterpret_cast<uint32_t *>(h + (pl.o_units - pl.o_slots)));
    if (!ctx->idx_ws.replace(pl.bytes, pl.bytes)) {
        (void)hipGetLastError();
        return nullptr;
    }
    uint8_t *ws = static_cast<uint8_t *>(ctx->idx_ws.p);
    if (hipMemcpyAsync(ws + pl.o_slots, h, b->h_bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return ws;
}
}  // namespace

int aec_gpu_index_chunks_plan(const aec_gpu_params *p, int how, uint64_t round_bits, const uint64_t *in_bytes_each,
                              const uint64_t *out_bytes, uint64_t n_chunks, aec_gpu_ichunks_plan *plan)
{
    DChunksShape sh;
    if (!p || !plan || (n_chunks && !in_bytes_each) || !dchunks_shape(p, nullptr, nullptr, nullptr, out_bytes, n_chunks, &sh, nullptr))
        return 0;
    BsPlan b;
    bs_plan(sh.c, how, round_bits, in_bytes_each, out_bytes, n_chunks, &b);
    plan->taken = b.taken;
    plan->rounds = b.rounds;
    plan->table_bits = b.table_bits;
    plan->rsi_entries = sh.entries;
    plan->workspace_bytes = b.taken ? b.bytes : 0;
    return 1;
}

int aec_gpu_index_chunks_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                               const uint64_t *in_offsets, const uint64_t *in_bytes_each, const uint64_t *out_bytes,
                               uint64_t n_chunks, uint64_t *d_rsi_bit_offsets, aec_gpu_dec_result *d_results,
                               uint32_t *d_how, void *stream)
{
    if (aec_gpu_check_params(p, 0) != RC_OK) return RC_CONF_ERROR;
    if (n_chunks == 0) return RC_OK;
    if (!out_bytes || !d_rsi_bit_offsets || !d_results || (reinterpret_cast<uintptr_t>(d_in) & 3u) || !in_offsets || !in_bytes_each)
        return RC_CONF_ERROR;
    for (uint64_t i = 0; i < n_chunks; i++)
        if (in_offsets[i] > in_bytes || in_bytes_each[i] > in_bytes - in_offsets[i]) return RC_CONF_ERROR;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    Cfg c;
    if (cfg_from(p, 0, false, &c) != RC_OK) return RC_CONF_ERROR;
    BareIndex bi;
    if (!bare_index_plan(c, ctx->chunks_index, ctx->chunks_round_bits, in_bytes_each, out_bytes, n_chunks, &bi)) return RC_MEM_ERROR;
    const size_t h_desc = ((size_t)(n_chunks + 1) * sizeof(DChunkDesc) + 15) & ~(size_t)15;
    aec_gpu_ctx::ChunkStage *stage = stage_descriptors(ctx, h_desc + bi.h_bytes);
    if (!stage) return RC_MEM_ERROR;
    DChunksShape sh;
    if (!dchunks_shape(p, in_offsets, in_bytes_each, nullptr, out_bytes, n_chunks, &sh, static_cast<DChunkDesc *>(stage->h.p)))
        return RC_CONF_ERROR;
    uint8_t *ws = bare_index_send(ctx, sh.c, in_offsets, in_bytes_each, out_bytes, n_chunks, &bi, static_cast<uint8_t *>(stage->h.p) + h_desc, st);
    uint8_t *cd = send_descriptors(ctx->chunks_d, stage, h_desc, sh.desc_bytes, st);
    if (!cd) return RC_MEM_ERROR;
    launch_index_chunks(sh.c, static_cast<const uint8_t *>(d_in), in_bytes, reinterpret_cast<const DChunkDesc *>(cd), n_chunks,
                        d_rsi_bit_offsets, rec(d_results), st, &bi.plan, bi.rounds.data(), ws, d_how);
    return launched();
}

int aec_gpu_decode_chunks_async(aec_gpu_ctx *ctx, const aec_gpu_params *p, const void *d_in, size_t in_bytes,
                                const uint64_t *in_offsets, const uint64_t *in_bytes_each, const uint64_t *out_offsets,
                                const uint64_t *out_bytes, uint64_t n_chunks, uint64_t *d_rsi_bit_offsets, int have_table,
                                void *d_out, aec_gpu_dec_result *d_results, aec_gpu_dec_result *d_result, void *stream)
{
    if (aec_gpu_check_params(p, 0) != RC_OK) return RC_CONF_ERROR;
    if (n_chunks == 0) return RC_OK;
    if (!out_offsets || !out_bytes || !d_rsi_bit_offsets || !d_results || !d_result || (reinterpret_cast<uintptr_t>(d_in) & 3u) ||
        (!have_table && (!in_offsets || !in_bytes_each)))
        return RC_CONF_ERROR;
    for (uint64_t i = 0; i < n_chunks; i++) {
        if (out_offsets[i] & 15u) return RC_CONF_ERROR;
        if (!have_table && (in_offsets[i] > in_bytes || in_bytes_each[i] > in_bytes - in_offsets[i])) return RC_CONF_ERROR;
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);

    BareIndex bi;
    if (!have_table) {
        Cfg c;
        if (cfg_from(p, 0, false, &c) != RC_OK) return RC_CONF_ERROR;
        if (!bare_index_plan(c, ctx->chunks_index, ctx->chunks_round_bits, in_bytes_each, out_bytes, n_chunks, &bi)) return RC_MEM_ERROR;
    }
    const size_t h_need = (size_t)(n_chunks + 1) * sizeof(DChunkDesc), h_desc = (h_need + 15) & ~(size_t)15;
    aec_gpu_ctx::ChunkStage *stage = stage_descriptors(ctx, h_desc + bi.h_bytes);
    if (!stage) return RC_MEM_ERROR;
    DChunksShape sh;
    if (!dchunks_shape(p, in_offsets, in_bytes_each, out_offsets, out_bytes, n_chunks, &sh, static_cast<DChunkDesc *>(stage->h.p)))
        return RC_CONF_ERROR;
    uint8_t *iws = have_table ? nullptr
                              : bare_index_send(ctx, sh.c, in_offsets, in_bytes_each, out_bytes, n_chunks, &bi,
                                                static_cast<uint8_t *>(stage->h.p) + h_desc, st);
    uint8_t *cd = send_descriptors(ctx->chunks_d, stage, h_need, sh.desc_bytes + sh.table_bytes, st);
    if (!cd) return RC_MEM_ERROR;
    const DChunkDesc *d_desc = reinterpret_cast<const DChunkDesc *>(cd);
    uint32_t *d_item_chunk = reinterpret_cast<uint32_t *>(cd + sh.desc_bytes);
    DecResult *records = rec(d_results);
    launch_dchunks_setup(sh.c, d_desc, n_chunks, sh.items, d_item_chunk, have_table ? records : nullptr, st);
    if (!have_table)
        launch_index_chunks(sh.c, static_cast<const uint8_t *>(d_in), in_bytes, d_desc, n_chunks, d_rsi_bit_offsets, records, st,
                            &bi.plan, bi.rounds.data(), iws, nullptr);
    // (bits per coded data set, from what the chunks announce: sizes the rings of the lane kernel)
    const uint64_t avg = sh.blocks ? (uint64_t)in_bytes * 8 / sh.blocks : 0;
    if (!launch_decode_chunks(sh.c, static_cast<const uint8_t *>(d_in), in_bytes, d_rsi_bit_offsets, d_desc, d_item_chunk,
                              sh.items, avg, static_cast<uint8_t *>(d_out), records, rec(d_result), st,
                              ctx->dec_events()))
        return RC_MEM_ERROR;
    return launched();
}

int aec_gpu_profile(aec_gpu_ctx *ctx, int enable)
{
    if (enable) {
        for (auto &set : ctx->ev)
            for (auto &e : set.ev)
                if (!e && hipEventCreate(&e) != hipSuccess) return RC_MEM_ERROR;
        ctx->enc_calls = ctx->dec_calls = 0;
    }
    ctx->profiling = enable != 0;
    return RC_OK;
}

int aec_gpu_phase_ms(aec_gpu_ctx *ctx, float *ms /*[5]: analyze, scan, clear, pack, decode*/)
{
    static const int pair[5][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {5, 6}};
    for (int i = 0; i < 5; i++) {
        const unsigned calls = i < 4 ? ctx->enc_calls : ctx->dec_calls;
        const unsigned sets = calls < aec_gpu_ctx::kProfRing ? calls : aec_gpu_ctx::kProfRing;
        double sum = 0;
        unsigned got = 0;
        for (unsigned s = 0; s < sets; s++) {
            hipEvent_t a = ctx->ev[s].ev[pair[i][0]], b = ctx->ev[s].ev[pair[i][1]];
            if (!a || !b || hipEventSynchronize(b) != hipSuccess) continue;
            float t = 0;
            if (hipEventElapsedTime(&t, a, b) == hipSuccess) { sum += t; got++; }
        }
        ms[i] = got ? static_cast<float>(sum / got) : -1.0f;
    }
    return RC_OK;
}

}  // extern "C"
