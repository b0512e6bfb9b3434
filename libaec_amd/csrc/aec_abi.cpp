// aec_abi.cpp -- the libaec C ABI (include/libaec.h) on top of the device-resident batch API.
//
// This is the host-side stream layer the reference implements as two resumable finite state
// machines (reference src/encode.c:467-518, 661-754, 909-963 and src/decode.c:342-400,
// 797-854).  Its contract is kept -- any chunking of input and output, cumulative
// total_in/total_out, AEC_FLUSH semantics, the same return codes -- but the states are replaced
// by staging and batching:
//
//   encode  input is collected on the host until it is worth a launch (a batch threshold, AEC_FLUSH,
//           or a call that brings no new input while whole RSIs wait); every whole RSI staged is then
//           coded in ONE batch on the GPU with the bit position and k carried between batches.  Cost
//           is linear in the input for any chunking (a caller feeding one sample per call pays a
//           vector append per call, not a launch).
//   decode  the compressed stream is kept RESIDENT ON THE DEVICE: only new bytes are uploaded, the
//           index walker resumes at the coded data set where it stopped (position + blocks of the
//           current RSI), the decoder takes its item counts from the walker's record on the device,
//           and one host synchronisation returns both records and the first output bytes.  A batch
//           is bounded by the room the caller offers (at least kMinBatchOut), so memory is
//           O(offered output + undecoded input), never O(decoded size of everything staged).
//
// The mechanisms every entry point shares are each stated once: a stream's device belongings (Kit: obtain_kit /
// give_kit), the hand-out of what a batch produced (hand_out), the copy to the caller beside the next batch (SideCopy),
// many chunks through pinned staging (stage_up / stage_down).  The kit's device buffers are DevBufs (aec_devbuf.h, shared
// with the context in aec_gpu.hip), grown by ensure(), which keeps their contents.  The arithmetic of a decode batch -- its
// bounds, the verdict over its result records, the advance of the stream's position -- is pure and lives in
// aec_stream_plan.h.
//
// There is no CPU codec in here: without a working HIP device every call fails with AEC_MEM_ERROR.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <mutex>
#include <new>
#include <chrono>
#include <thread>
#include <vector>

#include "../../include/aec_gpu.h"
#include "../../include/libaec.h"
#include "aec_cfg.h"
#include "aec_devbuf.h"
#include "aec_pool.h"
#include "aec_stream_plan.h"
#include "aec_tune.h"

using namespace aec;

namespace {

// AEC_ABI_TRACE=1 in the environment (the one variable the product library reads): say on stderr where a
// device-side failure was detected, and one line per decode batch (span, hint, what the walker brought back)
bool trace_on()
{
    static const bool trace = getenv("AEC_ABI_TRACE") != nullptr;
    return trace;
}
int fail_at(int code, int line)
{
    if (trace_on()) fprintf(stderr, "libaec (MI355X): error %d raised at aec_abi.cpp:%d (last HIP error: %s)\n", code, line,
                       hipGetErrorString(hipPeekAtLastError()));
    return code;
}
#define AEC_FAIL(code) fail_at((code), __LINE__)

// batching thresholds (kMinBatchOut and kPipeOut, which bound a decode batch: aec_stream_plan.h)
constexpr size_t kEncBatchBytes = (size_t)1 << 20;   // staged input that is worth a launch without AEC_FLUSH
constexpr size_t kEncDirectMin = (size_t)64 << 10;   // whole RSIs offered in one call: coded from the caller's buffer
constexpr size_t kDecTinyCall = 8;                   // a call that brings at most this many bytes is a trickle ...
constexpr size_t kDecTrickle = 4096;                 // ... collected on the host up to this many before a launch
constexpr size_t kDecDirectMin = 4096;               // input of at least this size goes straight to the device
constexpr size_t kBacklogMax = (size_t)64 << 20;     // undecoded input held on the device before more is accepted
constexpr size_t kBounce = (size_t)256 << 10;        // pinned bounce buffer: first output bytes ride with the records
constexpr size_t kAsyncMin = (size_t)1 << 20;        // pipelined decode batches: the smallest copy-out that is worth the side stream
constexpr size_t kRangeRsis = 2048;                  // aec_decode_range: RSIs per batch at least (below)

// The copy of a decode batch's output to the caller's buffer on a side stream, beside the kernels of the next batch,
// which write the other of the kit's two output buffers.  The stream and the events are created on demand and stay
// with the kit; which buffer is next and which copies are in flight is the business of one call.
struct SideCopy {
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};     // ev[i]: the last copy out of output buffer i has finished
    unsigned sel = 0;                          // which output buffer the next batch writes
    bool pending[2] = {false, false};          // a copy out of buffer i is in flight: waited for before the call returns

    bool event(unsigned i) { return ev[i] || hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess; }
    // work on `main` is about to write buffer `sel`: the copy that read it two batches ago must have finished first
    bool claim(hipStream_t main) { return !pending[sel] || hipStreamWaitEvent(main, ev[sel], 0) == hipSuccess; }
    // n bytes of buffer `sel` to the host.  beside: on the side stream, the next batch's kernels (the other buffer) run
    // beside it; where the stream or the event is not to be had, and for every other copy, the call blocks
    bool copy_out(void *dst, const void *d_src, size_t n, bool beside)
    {
        if (beside && (stream || hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess) && event(sel)) {
            if (hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                hipEventRecord(ev[sel], stream) != hipSuccess)
                return false;
            pending[sel] = true;
            sel ^= 1u;
            return true;
        }
        if (beside) (void)hipGetLastError();
        return hipMemcpy(dst, d_src, n, hipMemcpyDeviceToHost) == hipSuccess;
    }
    // all copies have arrived: the buffers they write are the caller's again (on every way out of a call)
    bool done()
    {
        if (!pending[0] && !pending[1]) return true;
        pending[0] = pending[1] = false;
        return hipStreamSynchronize(stream) == hipSuccess;
    }
};

// Device-side belongings of a stream.  Callers like the HDF5 SZIP filter run one
// aec_buffer_encode / aec_buffer_decode per chunk, i.e. an init / end cycle per megabyte: creating
// a HIP stream, a pinned result record and four device buffers each time (and freeing them, which
// synchronises the device) costs more than coding the chunk.  So *_end parks them in a small
// process-wide pool and *_init takes them from there.  Buffers above kKeepBytes are released
// first; the pool is never torn down at exit (the driver reclaims it with the process -- calling
// into HIP from static destructors is not safe).
struct Kit {
    int device = -1;
    aec_gpu_ctx *ctx = nullptr;
    hipStream_t stream = nullptr;
    DevBuf d_in, d_out, d_off, d_res, d_seg;   // (d_seg: segment starts beside the RSI starts, long RSIs only)
    DevBuf d_out2;                 // decoder: second output buffer (batches alternate while copies are in flight)
    SideCopy side;                 // decoder: the copy-out of a batch, beside the kernels of the next one
    uint8_t *h_res = nullptr;      // pinned: 256 bytes of records, then kBounce bytes of bounce buffer
    uint8_t *h_stage = nullptr;    // pinned staging of the batch entry points (many chunks, one transfer)
    size_t h_stage_cap = 0;

    DevBuf &out_buf() { return side.sel ? d_out2 : d_out; }   // the output buffer the next batch writes
};

}  // namespace

// A stream: its kit, where its decoder stands (aec_stream_plan.h), and what the host holds for it
struct internal_state : Kit, StreamPos {
    bool encoder = false;
    aec_gpu_params prm{};
    Cfg cfg{};                     // derived values (sizes are per batch, not used from here)

    std::vector<uint8_t> stage;    // encoder: input not yet coded; decoder: input not yet on the device
    size_t stage_pos = 0;          // encoder: first staged byte still to be coded
    std::vector<uint8_t> outq;     // produced bytes not yet delivered
    size_t outq_pos = 0;

    // encoder carry (reference state->k, state->bits / *state->cds)
    uint32_t k = 0;
    uint32_t part_bits = 0;        // bits used in the open byte, 0..7
    uint8_t part_byte = 0;
    bool any_bits = false;         // at least one stream bit produced
    bool finished = false;         // final byte queued
    int flush = AEC_NO_FLUSH;      // last flush argument
    bool flushed = false;          // reference state->flushed

    bool launched = false;         // decoder: at least one batch has run
    int sticky_error = AEC_OK;

    // RSI offset tables (include/libaec.h: aec_*_enable_offsets): absolute stream bits, kept only when enabled
    bool offsets_on = false;
    std::vector<uint64_t> offs;
    uint64_t enc_bits = 0;         // encoder: stream bits produced by the batches so far
    bool took_input = false;       // encoder: an aec_encode call has taken input; decoder: aec_decode has run
};

namespace {

// at most kPoolMax parked kits, none holding a buffer above kKeepBytes, all of them together at most kPoolBytes
constexpr size_t kPoolMax = 8, kKeepBytes = (size_t)256 << 20, kPoolBytes = (size_t)1 << 30;
constexpr size_t kStageKeep = (size_t)96 << 20, kStagePiece = (size_t)64 << 20, kPoolPinned = (size_t)192 << 20;
std::mutex g_pool_mu;
std::vector<Kit> *g_pool = nullptr;      // heap object on purpose: no destructor at exit

void destroy_kit(Kit &k)
{
    k.d_in.release();
    k.d_out.release();
    k.d_off.release();
    k.d_res.release();
    k.d_seg.release();
    k.d_out2.release();
    if (k.side.stream) (void)hipStreamDestroy(k.side.stream);
    for (hipEvent_t &e : k.side.ev)
        if (e) (void)hipEventDestroy(e);
    if (k.h_res) (void)hipHostFree(k.h_res);
    if (k.h_stage) (void)hipHostFree(k.h_stage);
    if (k.stream) (void)hipStreamDestroy(k.stream);
    if (k.ctx) aec_gpu_destroy(k.ctx);
    k = Kit{};
}

bool take_kit(int device, Kit *out)
{
    std::lock_guard<std::mutex> lock(g_pool_mu);
    if (!g_pool) return false;
    for (size_t i = 0; i < g_pool->size(); i++)
        if ((*g_pool)[i].device == device) {
            *out = (*g_pool)[i];
            g_pool->erase(g_pool->begin() + (ptrdiff_t)i);
            return true;
        }
    return false;
}

// A kit for the current device: from the pool, else freshly created.  false: no usable HIP device or no memory (the
// product has no CPU path); what there is of the kit goes back through give_kit all the same.
bool obtain_kit(Kit &k)
{
    if (hipGetDevice(&k.device) != hipSuccess) return false;
    if (take_kit(k.device, &k)) return true;          // (parked with the index hint and the output buffers' turn reset)
    return aec_gpu_create(&k.ctx) == RC_OK && hipStreamCreate(&k.stream) == hipSuccess &&
           hipHostMalloc(reinterpret_cast<void **>(&k.h_res), 256 + kBounce, hipHostMallocDefault) == hipSuccess &&
           k.d_res.ensure(256);
}

size_t kit_bytes(const Kit &k)
{
    return k.d_in.cap + k.d_out.cap + k.d_off.cap + k.d_res.cap + k.d_seg.cap + k.d_out2.cap + aec_gpu_held_bytes(k.ctx);
}

void park_kit(Kit &k)
{
    // an error return may have left copies or kernels of this stream object enqueued: nothing of it may still
    // run when the next owner writes the buffers
    if (hipStreamSynchronize(k.stream) != hipSuccess || (k.side.stream && hipStreamSynchronize(k.side.stream) != hipSuccess)) {
        (void)hipGetLastError();
        destroy_kit(k);
        return;
    }
    for (DevBuf *b : {&k.d_in, &k.d_out, &k.d_off, &k.d_seg, &k.d_out2})
        if (b->cap > kKeepBytes) b->release();
    if (k.h_stage_cap > kStageKeep) {
        (void)hipHostFree(k.h_stage);
        k.h_stage = nullptr;
        k.h_stage_cap = 0;
    }
    aec_gpu_trim(k.ctx, kKeepBytes);
    aec_gpu_set_index_hint(k.ctx, 0);
    k.side.sel = 0;
    k.side.pending[0] = k.side.pending[1] = false;
    {
        std::lock_guard<std::mutex> lock(g_pool_mu);
        if (!g_pool) g_pool = new (std::nothrow) std::vector<Kit>();
        size_t held = kit_bytes(k), pinned = k.h_stage_cap;
        if (g_pool)
            for (const Kit &o : *g_pool) {
                held += kit_bytes(o);
                pinned += o.h_stage_cap;
            }
        if (pinned > kPoolPinned && k.h_stage) {     // page-locked host memory of all parked kits together is bounded too
            (void)hipHostFree(k.h_stage);
            k.h_stage = nullptr;
            k.h_stage_cap = 0;
        }
        if (g_pool && g_pool->size() < kPoolMax && held <= kPoolBytes) {
            g_pool->push_back(k);
            k = Kit{};
            return;
        }
    }
    destroy_kit(k);
}

// A kit goes back: parked if it is complete, else destroyed
void give_kit(Kit &k)
{
    if (k.ctx && k.stream && k.h_res && k.d_res.p) park_kit(k);
    else destroy_kit(k);
}

void free_state(internal_state *s)
{
    if (!s) return;
    give_kit(*s);
    delete s;
}

int init_common(struct aec_stream *strm, bool enc)
{
    aec_gpu_params prm{strm->bits_per_sample, strm->block_size, strm->rsi, strm->flags};
    Cfg c;
    const int rc = make_cfg(prm.bits_per_sample, prm.block_size, prm.rsi, prm.flags, 0, enc, &c);
    if (rc != RC_OK) return AEC_FAIL(rc);
    internal_state *s = new (std::nothrow) internal_state();
    if (!s) return AEC_FAIL(AEC_MEM_ERROR);
    s->encoder = enc;
    s->prm = prm;
    s->cfg = c;
    if (!obtain_kit(*s)) {
        free_state(s);
        return AEC_FAIL(AEC_MEM_ERROR);   // no usable HIP device: the product has no CPU path
    }
    strm->state = s;
    strm->total_in = 0;         // reference encode.c:897-898, decode.c:785-786
    strm->total_out = 0;
    return AEC_OK;
}

inline size_t drain(struct aec_stream *strm, internal_state *s, size_t granule)
{
    size_t n = s->outq.size() - s->outq_pos;
    if (n == 0) return 0;
    if (n > strm->avail_out) n = strm->avail_out;
    n -= n % granule;
    if (n) {
        memcpy(strm->next_out, s->outq.data() + s->outq_pos, n);
        strm->next_out += n;
        strm->avail_out -= n;
        s->outq_pos += n;
    }
    if (s->outq_pos == s->outq.size()) {
        s->outq.clear();
        s->outq_pos = 0;
    }
    return n;
}

// Hand out what a batch produced: `count` fresh bytes at d_bytes on the device (in the output buffer whose turn it is),
// the first `spec` of which are already in the bounce buffer -- they rode with the result record.  As much as fits goes
// straight into the caller's buffer, in whole granules (next_out / avail_out advance), the remainder is queued; the last
// `hold` bytes are queued whatever the room.  beside: a large rest of the direct part may go on the side stream.
int hand_out(internal_state *s, struct aec_stream *strm, const uint8_t *d_bytes, size_t count, size_t hold, size_t spec,
             size_t granule, bool beside)
{
    const uint8_t *bounce = s->h_res + 256;
    size_t direct = count - hold < strm->avail_out ? count - hold : strm->avail_out;
    direct -= direct % granule;
    if (direct) {
        const size_t from_bounce = direct < spec ? direct : spec, rest = direct - from_bounce;
        memcpy(strm->next_out, bounce, from_bounce);
        if (rest && !s->side.copy_out(strm->next_out + from_bounce, d_bytes + from_bounce, rest, beside && rest >= kAsyncMin))
            return AEC_FAIL(AEC_MEM_ERROR);
        strm->next_out += direct;
        strm->avail_out -= direct;
    }
    if (count > direct) {
        const size_t rest = count - direct, at = s->outq.size();
        s->outq.resize(at + rest);
        size_t done = 0;
        if (direct < spec) {
            done = spec - direct < rest ? spec - direct : rest;
            memcpy(s->outq.data() + at, bounce + direct, done);
        }
        if (rest > done &&
            hipMemcpy(s->outq.data() + at + done, d_bytes + direct + done, rest - done, hipMemcpyDeviceToHost) != hipSuccess)
            return AEC_FAIL(AEC_MEM_ERROR);
    }
    return AEC_OK;
}

// Code `nbytes` of input (whole samples) as one GPU batch; append produced whole bytes to the queue
// and keep the open byte / k as carry.  Nothing is queued when this runs, so finished bytes go
// straight into the caller's buffer as far as it has room: the first kBounce of them ride with the
// result record (one synchronisation), only what does not fit -- and the open byte -- is queued.
int encode_batch(internal_state *s, const uint8_t *data, size_t nbytes, struct aec_stream *strm)
{
    if (nbytes == 0) return AEC_OK;
    const size_t cap = aec_gpu_encode_bound(&s->prm, nbytes);
    if (!s->d_in.ensure(nbytes + 16) || !s->d_out.ensure(cap)) return AEC_FAIL(AEC_MEM_ERROR);
    // (offsets enabled: the batch's RSI starts, relative to bit 0 of its first byte -- the open byte's bits included)
    const uint64_t n_rsi = s->offsets_on ? aec_gpu_rsi_count(&s->prm, nbytes) : 0;
    uint64_t *d_tbl = nullptr;
    if (s->offsets_on) {
        if (!s->d_off.ensure((n_rsi + 1) * 8)) return AEC_FAIL(AEC_MEM_ERROR);
        d_tbl = static_cast<uint64_t *>(s->d_off.p);
    }
    if (hipMemcpyAsync(s->d_in.p, data, nbytes, hipMemcpyHostToDevice, s->stream) != hipSuccess)
        return AEC_FAIL(AEC_MEM_ERROR);
    const int rc = aec_gpu_encode_async(s->ctx, &s->prm, s->d_in.p, nbytes, s->d_out.p, cap, s->part_bits,
                                        s->k, d_tbl, static_cast<aec_gpu_enc_result *>(s->d_res.p),
                                        s->stream);
    if (rc != RC_OK) return AEC_FAIL(rc);
    const uint8_t *d_bytes = static_cast<const uint8_t *>(s->d_out.p);
    const size_t spec = cap < kBounce ? cap : kBounce;          // speculative: the size is not known yet
    if (hipMemcpyAsync(s->h_res, s->d_res.p, sizeof(aec_gpu_enc_result), hipMemcpyDeviceToHost, s->stream) !=
            hipSuccess ||
        hipMemcpyAsync(s->h_res + 256, d_bytes, spec, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
        hipStreamSynchronize(s->stream) != hipSuccess)
        return AEC_FAIL(AEC_MEM_ERROR);
    const aec_gpu_enc_result res = *reinterpret_cast<aec_gpu_enc_result *>(s->h_res);
    if (res.overflow) return AEC_FAIL(AEC_MEM_ERROR);   // cannot happen: cap is the worst case
    if (n_rsi) {
        const size_t at = s->offs.size();
        s->offs.resize(at + n_rsi);
        if (hipMemcpy(s->offs.data() + at, d_tbl, n_rsi * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return AEC_FAIL(AEC_MEM_ERROR);
        const uint64_t origin = s->enc_bits - s->part_bits;     // stream bit of the batch's first byte
        for (size_t i = at; i < at + n_rsi; i++) s->offs[i] += origin;
    }
    s->enc_bits += res.total_bits;
    const uint64_t bits = (uint64_t)s->part_bits + res.total_bits;
    const size_t whole = (size_t)(bits / 8), nb = (size_t)((bits + 7) / 8);
    // bytes [0, whole) are finished, byte `whole` (if nb > whole) is the new open byte: queued in any case
    uint8_t *out0 = strm->next_out;
    const size_t at = s->outq.size();
    const int hrc = hand_out(s, strm, d_bytes, nb, nb - whole, spec, 1, false);
    if (hrc != AEC_OK) return hrc;
    const size_t direct = (size_t)(strm->next_out - out0);
    // the byte the batch started in carries the bits of the previous batch
    if (direct) out0[0] |= s->part_byte;
    else if (nb) s->outq[at] |= s->part_byte;
    s->part_bits = (uint32_t)(bits % 8);
    s->part_byte = s->part_bits ? s->outq[at + whole - direct] : 0;
    s->outq.resize(at + whole - direct);
    s->k = res.k_out;
    if (res.total_bits) s->any_bits = true;
    return AEC_OK;
}

// ---- decoder ------------------------------------------------------------------------------------

// Append `n` bytes at `src` (host) to the device-resident stream.
int upload(internal_state *s, const uint8_t *src, size_t n)
{
    if (n == 0) return AEC_OK;
    if (!s->d_in.ensure(s->d_len + n + 32, s->d_len)) return AEC_FAIL(AEC_MEM_ERROR);
    if (hipMemcpyAsync(static_cast<uint8_t *>(s->d_in.p) + s->d_len, src, n, hipMemcpyHostToDevice, s->stream) !=
        hipSuccess)
        return AEC_FAIL(AEC_MEM_ERROR);
    s->d_len += n;
    return AEC_OK;
}

// One batch: index from where the walker stopped, decode what it found, hand out / queue the samples.  What the batch
// takes and brings (plan_batch), what its records mean (judge_batch) and where the stream stands after it
// (advance_stream) is aec_stream_plan.h's; here are the buffers, the launches, the one synchronisation and the copies.
int decode_run(internal_state *s, struct aec_stream *strm)
{
    const Cfg &c = s->cfg;
    if (!s->stage.empty()) {
        const int rc = upload(s, s->stage.data(), s->stage.size());
        if (rc != AEC_OK) return rc;
        // (the copy out of this pageable vector has been staged by the runtime when the call returns,
        // and the batch below is waited for in any case)
        s->stage.clear();
    }
    s->launched = true;
    s->more = false;
    if (s->d_len == 0) return AEC_OK;
    const size_t rsi_bytes = (size_t)c.rsi * c.bs * c.bytes;
    const uint64_t base_bits = s->base * 8;
    const size_t want_out = strm->avail_out;              // (what the caller asks of THIS call)
    const uint64_t ahead = plan_hint(c, *s, want_out);
    const bool windowed = want_out >= kPipeMin &&
                          aec_gpu_index_is_windowed(&s->prm, s->d_len - (size_t)((s->rsi_start_bit - base_bits) / 8),
                                                    ahead + ahead / 2) != 0;
    const BatchPlan b = plan_batch(c, *s, want_out, windowed);
    if (!s->d_off.ensure(b.off_bytes) || !s->out_buf().ensure(b.out_bytes)) return AEC_FAIL(AEC_MEM_ERROR);
    DevBuf &obuf = s->out_buf();
    if (!s->side.claim(s->stream)) return AEC_FAIL(AEC_MEM_ERROR);
    // (without the table of segment starts -- no memory for it -- a lane per RSI)
    uint64_t *d_seg = nullptr;
    if (b.seg_bytes && s->d_seg.ensure(b.seg_bytes)) d_seg = static_cast<uint64_t *>(s->d_seg.p);

    aec_gpu_dec_result *d_idx = static_cast<aec_gpu_dec_result *>(s->d_res.p), *d_dec = d_idx + 1;
    uint64_t *d_off = static_cast<uint64_t *>(s->d_off.p);
    aec_gpu_set_index_hint(s->ctx, index_hint_of(c, b.hint));
    if (b.piece) aec_gpu_set_index_piece(s->ctx, 6 * b.hint + 8192);
    int rc = d_seg ? aec_gpu_index_segments_async(s->ctx, &s->prm, s->d_in.p, b.in_bytes, b.walk_rel, s->walk_blocks, b.rsi_rel,
                                                  d_off, d_seg, b.max_rsi, d_idx, s->stream)
                   : aec_gpu_index_resume_async(s->ctx, &s->prm, s->d_in.p, b.in_bytes, b.walk_rel, s->walk_blocks, b.rsi_rel,
                                                d_off, b.max_rsi, d_idx, s->stream);
    if (rc != RC_OK) return AEC_FAIL(rc);
    rc = d_seg ? aec_gpu_decode_bare_async(s->ctx, &s->prm, s->d_in.p, b.in_bytes, d_off, d_seg, b.max_rsi, 0, d_idx,
                                           obuf.p, d_dec, s->stream)
               : aec_gpu_decode_indexed_async(s->ctx, &s->prm, s->d_in.p, b.in_bytes, d_off, b.max_rsi, d_idx, obuf.p,
                                              d_dec, s->stream);
    if (rc != RC_OK) return AEC_FAIL(rc);
    // records, the start of the trailing partial RSI, and the first output bytes: one synchronisation
    const uint8_t *d_bytes = static_cast<const uint8_t *>(obuf.p) + b.skip;
    size_t spec = b.max_rsi * rsi_bytes - b.skip;
    if (spec > kBounce) spec = kBounce;
    const auto t_enq = std::chrono::steady_clock::now();                // (AEC_ABI_TRACE: where a batch's time goes)
    if (hipMemcpyAsync(s->h_res, d_idx, 2 * sizeof(aec_gpu_dec_result), hipMemcpyDeviceToHost, s->stream) !=
            hipSuccess ||
        hipMemcpyAsync(s->h_res + 128, d_off + b.max_rsi, 8, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
        hipMemcpyAsync(s->h_res + 256, d_bytes, spec, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
        hipStreamSynchronize(s->stream) != hipSuccess)
        return AEC_FAIL(AEC_MEM_ERROR);
    if (trace_on()) {
        static thread_local std::chrono::steady_clock::time_point t_prev = t_enq;
        const auto t_done = std::chrono::steady_clock::now();
        fprintf(stderr, "libaec (MI355X): decode batch: %.3f ms since the batch in front was through, of which %.3f ms "
                "waiting for this one's kernels after the last launch\n",
                std::chrono::duration<double, std::milli>(t_done - t_prev).count(),
                std::chrono::duration<double, std::milli>(t_done - t_enq).count());
        t_prev = t_done;
    }
    const aec_gpu_dec_result idx = reinterpret_cast<aec_gpu_dec_result *>(s->h_res)[0];
    const aec_gpu_dec_result dec = reinterpret_cast<aec_gpu_dec_result *>(s->h_res)[1];
    if (trace_on())
        fprintf(stderr, "libaec (MI355X): decode batch: pipelined %d, room for %llu RSIs, span %zu of %zu resident bytes (from byte %llu), "
                "hint %llu bits per RSI -> %llu RSIs + %llu blocks, walker status %u pad %u\n", (int)b.pipe, (unsigned long long)b.max_rsi,
                b.in_bytes, s->d_len, (unsigned long long)(b.walk_rel / 8), (unsigned long long)b.hint, (unsigned long long)idx.n_rsi,
                (unsigned long long)idx.tail_blocks, idx.status, idx.pad);
    uint64_t tail_start = 0;
    memcpy(&tail_start, s->h_res + 128, 8);

    // the samples in front of an error are delivered before it is reported
    BatchVerdict v = judge_batch(c, idx, dec, b.skip, want_out);
    if (v.total > b.skip) {
        const int hrc = hand_out(s, strm, d_bytes, v.total - b.skip, 0, spec, c.bytes, b.pipe);
        if (hrc != AEC_OK) return hrc;
    }
    // (a decoder's error deferred to the next call: the walk resumes at the start of the RSI the decoder gave up)
    if (v.fetch_off && hipMemcpy(&v.res_end, d_off + v.good_rsi, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return AEC_FAIL(AEC_MEM_ERROR);
    if (v.corrupt) {
        if (trace_on())
            fprintf(stderr, "libaec (MI355X): AEC_DATA_ERROR: walker status %u after %llu RSIs + %llu blocks (bit %llu), "
                    "decoder status %u at RSI %llu\n", idx.status, (unsigned long long)idx.n_rsi,
                    (unsigned long long)idx.tail_blocks, (unsigned long long)idx.end_bit, dec.status,
                    (unsigned long long)dec.bad_rsi);
        return AEC_DATA_ERROR;
    }
    // offsets enabled: the RSIs of the batch whose first coded data set is decoded -- the whole ones, and the one it
    // ends in -- in absolute bits; the first of them may be the one the batch in front ended in (counted once)
    if (s->offsets_on && (v.res_rsi || v.res_tail)) {
        std::vector<uint64_t> got(v.res_rsi + (v.res_tail ? 1 : 0));
        if (v.res_rsi && hipMemcpy(got.data(), d_off, v.res_rsi * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return AEC_FAIL(AEC_MEM_ERROR);
        if (v.res_tail) got[v.res_rsi] = tail_start;
        for (const uint64_t o : got)
            if (s->offs.empty() || base_bits + o > s->offs.back()) s->offs.push_back(base_bits + o);
    }
    // the stream's new position; the consumed front of the resident stream goes (the copy must not overlap:
    // advance_stream drops the front only once it is the larger part)
    StreamPos next = *s;
    const size_t drop = advance_stream(c, next, b, v, idx, tail_start);
    if (drop && next.d_len && hipMemcpyAsync(s->d_in.p, static_cast<uint8_t *>(s->d_in.p) + drop, next.d_len,
                                             hipMemcpyDeviceToDevice, s->stream) != hipSuccess)
        return AEC_FAIL(AEC_MEM_ERROR);
    static_cast<StreamPos &>(*s) = next;
    return AEC_OK;
}

int encode_call(struct aec_stream *strm, int flush)
{
    internal_state *s = strm->state;
    const size_t bytes = s->cfg.bytes;
    const size_t rsi_bytes = (size_t)s->cfg.rsi * s->cfg.bs * bytes;
    s->flush = flush;
    if (strm->avail_in) s->took_input = true;
    strm->total_in += strm->avail_in;     // reference encode.c:919-920
    strm->total_out += strm->avail_out;
    const bool brought = strm->avail_in >= bytes;
    int rc = AEC_OK;

    for (;;) {
        drain(strm, s, 1);
        if (!s->outq.empty()) break;      // output full
        if (s->finished) {
            s->flushed = true;            // reference encode.c:689-694
            break;
        }
        // only whole samples are ever consumed (reference encode.c:673-674)
        const size_t take = strm->avail_in - strm->avail_in % bytes;
        size_t staged = s->stage.size() - s->stage_pos;
        if (staged == 0 && take >= rsi_bytes && (take >= kEncDirectMin || flush == AEC_FLUSH)) {
            // whole RSIs offered and nothing staged: code them from the caller's buffer
            const size_t direct = take / rsi_bytes * rsi_bytes;
            rc = encode_batch(s, strm->next_in, direct, strm);
            strm->next_in += direct;
            strm->avail_in -= direct;
            if (rc != AEC_OK) break;
            continue;
        }
        if (take) {
            if (s->stage_pos && s->stage_pos == s->stage.size()) {
                s->stage.clear();
                s->stage_pos = 0;
            }
            s->stage.insert(s->stage.end(), strm->next_in, strm->next_in + take);
            strm->next_in += take;
            strm->avail_in -= take;
            staged += take;
        }
        const size_t whole = staged / rsi_bytes * rsi_bytes;
        // A launch is worth it for a batch of some size, is due on AEC_FLUSH, and is what a caller asks
        // for who comes back without new input while whole RSIs wait (the reference would have coded
        // them by now: tests/check_aec.c encode_decode_small collects its output that way).
        if (whole && (flush == AEC_FLUSH || whole >= kEncBatchBytes || !brought)) {
            rc = encode_batch(s, s->stage.data() + s->stage_pos, whole, strm);
            s->stage_pos += whole;
            if (s->stage_pos == s->stage.size()) {
                s->stage.clear();
                s->stage_pos = 0;
            } else if (s->stage_pos >= s->stage.size() - s->stage_pos) {
                s->stage.erase(s->stage.begin(), s->stage.begin() + (ptrdiff_t)s->stage_pos);
                s->stage_pos = 0;
            }
            if (rc != AEC_OK) break;
            continue;
        }
        if (flush == AEC_FLUSH) {
            // last, short RSI (reference encode.c:676-684), then the final byte (686-695)
            rc = encode_batch(s, s->stage.data() + s->stage_pos, staged, strm);
            s->stage.clear();
            s->stage_pos = 0;
            if (rc != AEC_OK) break;
            if (s->part_bits || !s->any_bits) s->outq.push_back(s->part_byte);
            s->part_bits = 0;
            s->part_byte = 0;
            s->finished = true;
            continue;
        }
        break;                            // need more input
    }
    strm->total_in -= strm->avail_in;     // reference encode.c:933-934
    strm->total_out -= strm->avail_out;
    return rc;
}

int decode_call(struct aec_stream *strm, int flush)
{
    internal_state *s = strm->state;
    const size_t bytes = s->cfg.bytes;
    s->took_input = true;
    strm->total_in += strm->avail_in;     // reference decode.c:811-812
    strm->total_out += strm->avail_out;
    int rc = s->sticky_error;
    const size_t brought = strm->avail_in;

    while (rc == AEC_OK) {
        drain(strm, s, bytes);
        if (!s->outq.empty()) break;      // output full (or less than one sample of room)
        // Accept input while the undecoded backlog on the device is moderate; large pieces go straight
        // to the device, trickles are collected on the host first.
        // (a caller that offers more room than that may bring as much input: the stream of a one-shot decode goes up
        // whole and is indexed in one pass -- in pieces of 64 MiB a 180 MB stream of the reference's sample shape paid
        // the fixed phases of the trunk index three times, 71 ms instead of 48 for 256 MiB)
        // (as much input as that output can take at most -- incompressible data is longer coded than decoded, and a
        // stream cut at the size of its output had its last few per cent indexed and decoded as a second batch, with
        // an average coded RSI for the first that was too low to tell what kind of stream it is)
        const size_t rsi_out = (size_t)s->cfg.rsi * s->cfg.bs * bytes;
        const size_t in_for_out = (size_t)((strm->avail_out / rsi_out + 2) * worst_rsi_bytes(s->cfg));
        const size_t backlog_max = strm->avail_out >= kBacklogMax ? (in_for_out > strm->avail_out ? in_for_out : strm->avail_out)
                                                                  : kBacklogMax;
        if (strm->avail_in && s->d_len - (size_t)((s->walk_bit / 8) - s->base) < backlog_max) {
            size_t n = strm->avail_in < backlog_max ? strm->avail_in : backlog_max;
            if (n >= kDecDirectMin && s->stage.empty()) {
                rc = upload(s, strm->next_in, n);
                // (the staging buffer for a one-shot caller's whole stream could not be allocated: in pieces of the
                // ordinary backlog, as before round 4 -- only then AEC_MEM_ERROR.  A stream that goes up whole and then
                // finds no memory for its output or its index workspace is NOT retried here: decode_run reports it, or
                // the index pass falls back to a smaller workspace / the serial walk: aec_gpu.hip index_common)
                if (rc == AEC_MEM_ERROR && n > kBacklogMax) {
                    (void)hipGetLastError();
                    n = kBacklogMax;
                    rc = upload(s, strm->next_in, n);
                }
                if (rc != AEC_OK) break;
            } else {
                s->stage.insert(s->stage.end(), strm->next_in, strm->next_in + n);
            }
            strm->next_in += n;
            strm->avail_in -= n;
        }
        const bool pending = !s->stage.empty() || s->d_len > s->walked_len || s->more;
        if (!pending) break;
        // When to run a batch: always -- a caller may take "output not full" to mean that everything
        // the input allows has come out -- except for a caller that trickles input in a few bytes per
        // call (at most kDecTinyCall new bytes, fewer than kDecTrickle waiting, AEC_NO_FLUSH, not the
        // first call): those bytes are collected until a call brings nothing new, which is how such
        // callers ask for the rest (reference src/aec.c:191-221, tests/check_aec.c:138-166), so that a
        // byte-at-a-time caller costs a vector append per call instead of a launch.
        const bool trickle = brought && brought <= kDecTinyCall && flush != AEC_FLUSH && s->launched && !s->more &&
                             s->d_len <= s->walked_len && s->stage.size() < kDecTrickle;
        if (trickle) break;
        const size_t out_before = strm->avail_out, q_before = s->outq.size();
        const uint64_t walk_before = s->walk_bit, span_before = s->span_mul;
        const bool wide_before = s->span_wide;
        rc = decode_run(s, strm);
        if (rc == AEC_DATA_ERROR) s->sticky_error = rc;
        if (rc != AEC_OK) break;
        const bool progressed = out_before != strm->avail_out || q_before != s->outq.size() ||
                                walk_before != s->walk_bit || s->span_mul > span_before ||
                                s->span_wide != wide_before;                               // (a wider span is tried at once)
        if (!progressed) break;           // what is here needs more input before anything else comes out
    }
    // (copies to the caller's buffer that run on the side stream: the buffer is the caller's again on return)
    if (!s->side.done() && rc == AEC_OK) rc = AEC_FAIL(AEC_MEM_ERROR);
    if (rc == AEC_DATA_ERROR) drain(strm, s, bytes);   // the samples in front of the error are delivered
    if (rc != AEC_OK) return rc;          // reference decode.c:818-819 (totals left as they are)
    if (strm->avail_out > 0 && strm->avail_out < bytes) return AEC_FAIL(AEC_MEM_ERROR);   // decode.c:821-823
    strm->total_in -= strm->avail_in;     // reference decode.c:827-828
    strm->total_out -= strm->avail_out;
    return AEC_OK;
}

// ---- many independent streams per call (include/libaec.h: aec_buffer_*_batch) -------------------------
struct BatchKit {
    Kit k;
    const bool ok;
    BatchKit() : ok(obtain_kit(k)) {}
    ~BatchKit() { give_kit(k); }
};

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// pinned staging buffer of a kit, at least n bytes (false: not to be had -- the callers copy chunk by chunk then)
bool stage_ensure(Kit &k, size_t n)
{
    if (n <= k.h_stage_cap) return true;
    if (k.h_stage) (void)hipHostFree(k.h_stage);
    k.h_stage = nullptr;
    k.h_stage_cap = 0;
    if (hipHostMalloc(reinterpret_cast<void **>(&k.h_stage), n, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    k.h_stage_cap = n;
    return true;
}

// many host-to-host copies (caller's buffers <-> pinned staging), on a few threads when there is enough to copy
struct CopyJob {
    void *dst;
    const void *src;
    size_t n;
};
thread_local bool t_in_part = false;          // this thread is one of run_parts' workers: no threads of its own

// Waiting for a kit's stream, or for an event on it, inside the batch paths.  With several host threads each waiting on
// a stream of its own, hipStreamSynchronize was measured to return up to 9 ms late now and then (2.4 ms batches taking
// 10); polling the stream does not.  The poll yields for the first few dozen microseconds -- a small batch is through by
// then -- and then sleeps between two looks (round 6: a part thread burnt a core for the whole of its batch; the timer's
// slack, ~60 us, is a few per cent of the milliseconds such a batch takes).
template <class Query>
hipError_t poll(Query query)
{
    for (unsigned spins = 0;; spins++) {
        const hipError_t e = query();
        if (e != hipErrorNotReady) return e;
        if (spins < 256u) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(25));
    }
}
hipError_t batch_sync(hipStream_t st)
{
    return t_in_part ? poll([st] { return hipStreamQuery(st); }) : hipStreamSynchronize(st);
}
hipError_t batch_sync(hipEvent_t ev)
{
    return t_in_part ? poll([ev] { return hipEventQuery(ev); }) : hipEventSynchronize(ev);
}

void copy_all(const std::vector<CopyJob> &jobs)
{
    size_t total = 0;
    for (const CopyJob &j : jobs) total += j.n;
    const unsigned hw = std::thread::hardware_concurrency();
    unsigned nt = total >= ((size_t)8 << 20) && !t_in_part ? (hw >= 8 ? 4u : (hw >= 2 ? 2u : 1u)) : 1u;
    if (nt > jobs.size()) nt = (unsigned)jobs.size();
    auto work = [&](unsigned t) {
        for (size_t i = t; i < jobs.size(); i += nt)
            if (jobs[i].n) memcpy(jobs[i].dst, jobs[i].src, jobs[i].n);
    };
    if (nt <= 1) {
        work(0);
        return;
    }
    // (the pool's threads, kept between calls -- round 5; until then a thread per share was created and joined per call)
    WorkerPool::run(nt, [&](size_t t) { work((unsigned)t); });
}

// Many chunks from the callers' buffers into k.d_in.  Chunk i is len(i) bytes at src[i] and goes to byte at(i) of
// d_in; at(i + 1) - at(i) is the room it has there (at(n): the end of the last one).  cap != 0: through the pinned
// staging buffer in pieces of as many whole chunks as cap bytes hold -- the host's copies on a few threads, ONE
// transfer per piece, each waiting until the piece in front has left the buffer; cap == 0: chunk by chunk, straight
// from the callers' buffers.  zero: the room behind every chunk is zeroed.  each(i) runs once chunk i is on its way
// (launches on k.stream that read it); anything but AEC_OK from it ends the transfer and is returned.
template <class At, class Len, class Each>
int stage_up(Kit &k, size_t n, const void *const *src, At at, Len len, size_t cap, bool zero, Each each)
{
    uint8_t *d_in = static_cast<uint8_t *>(k.d_in.p);
    if (!cap) {
        if (zero && hipMemsetAsync(d_in + at(0), 0, at(n) - at(0), k.stream) != hipSuccess) return AEC_FAIL(AEC_MEM_ERROR);
        for (size_t i = 0; i < n; i++) {
            if (len(i) && hipMemcpyAsync(d_in + at(i), src[i], len(i), hipMemcpyHostToDevice, k.stream) != hipSuccess)
                return AEC_FAIL(AEC_MEM_ERROR);
            const int rc = each(i);
            if (rc != AEC_OK) return rc;
        }
        return AEC_OK;
    }
    std::vector<CopyJob> jobs;
    for (size_t i = 0, j; i < n; i = j) {
        for (j = i; j < n && at(j + 1) - at(i) <= cap;) j++;
        if (j == i) return AEC_FAIL(AEC_MEM_ERROR);                               // (cannot happen: a chunk fits)
        if (i && batch_sync(k.stream) != hipSuccess) return AEC_FAIL(AEC_MEM_ERROR);   // staging is free again
        jobs.clear();
        for (size_t q = i; q < j; q++) {
            uint8_t *h = k.h_stage + (at(q) - at(i));
            jobs.push_back(CopyJob{h, src[q], len(q)});
            if (zero) memset(h + len(q), 0, at(q + 1) - at(q) - len(q));
        }
        copy_all(jobs);
        if (hipMemcpyAsync(d_in + at(i), k.h_stage, at(j) - at(i), hipMemcpyHostToDevice, k.stream) != hipSuccess)
            return AEC_FAIL(AEC_MEM_ERROR);
        for (size_t q = i; q < j; q++) {
            const int rc = each(q);
            if (rc != AEC_OK) return rc;
        }
    }
    return AEC_OK;
}
inline int no_launch(size_t) { return AEC_OK; }

// What a batch left in k.d_out to the callers' buffers, then the end of the batch is waited for.  Chunk i occupies
// ext(i) bytes at byte pos(i) of d_out; done(i, &st) says how many of them the caller gets (dst_len[i]) and with what
// status (status[i]; the last one that is not AEC_OK is returned).  cap != 0: through the pinned staging buffer in
// pieces of as many whole chunks as cap bytes hold (one that alone is larger goes directly) -- ONE transfer per piece,
// then copies to the callers' buffers on a few threads.  twice: the buffer has two halves of cap bytes and k.side.ev
// its two events; the transfer of piece p + 1 runs beside the host's copies of piece p (every chunk fits then).
// cap == 0: chunk by chunk, straight into the callers' buffers.
template <class Pos, class Ext, class Done>
int stage_down(Kit &k, size_t n, void *const *dst, size_t *dst_len, int *status, Pos pos, Ext ext, size_t cap, bool twice,
               Done done)
{
    const uint8_t *d_out = static_cast<const uint8_t *>(k.d_out.p);
    auto cut = [&](size_t i) {                       // the end of the piece that begins with chunk i (i: it does not fit)
        size_t j = i;
        while (cap && j < n && pos(j) + ext(j) - pos(i) <= cap) j++;
        return j;
    };
    auto fetch = [&](size_t i, size_t j, unsigned half) {        // the transfer of chunks [i, j) into a half of the buffer
        return hipMemcpyAsync(k.h_stage + half * cap, d_out + pos(i), pos(j - 1) + ext(j - 1) - pos(i), hipMemcpyDeviceToHost,
                              k.stream) == hipSuccess &&
               (!twice || hipEventRecord(k.side.ev[half], k.stream) == hipSuccess);
    };
    int worst = AEC_OK;
    std::vector<CopyJob> jobs;
    size_t j = cut(0);
    if (twice && !fetch(0, j, 0)) return AEC_FAIL(AEC_MEM_ERROR);
    for (size_t i = 0, piece = 0; i < n; piece++) {
        const unsigned half = twice ? piece & 1u : 0u;
        const bool staged = j > i;
        size_t next = 0;
        if (staged && twice) {                       // the next piece sets out, this one has to be here
            next = cut(j);
            if ((next > j && !fetch(j, next, half ^ 1u)) || batch_sync(k.side.ev[half]) != hipSuccess)
                return AEC_FAIL(AEC_MEM_ERROR);
        } else if (staged) {
            if (!fetch(i, j, 0) || batch_sync(k.stream) != hipSuccess) return AEC_FAIL(AEC_MEM_ERROR);
        } else {
            j = i + 1;
        }
        jobs.clear();
        for (size_t q = i; q < j; q++) {
            int st = AEC_OK;
            const size_t bytes = done(q, &st);
            if (staged) jobs.push_back(CopyJob{dst[q], k.h_stage + half * cap + (pos(q) - pos(i)), bytes});
            else if (bytes && hipMemcpyAsync(dst[q], d_out + pos(q), bytes, hipMemcpyDeviceToHost, k.stream) != hipSuccess)
                return AEC_FAIL(AEC_MEM_ERROR);
            dst_len[q] = bytes;
            if (status) status[q] = st;
            if (st != AEC_OK) worst = st;
        }
        copy_all(jobs);
        i = j;
        j = twice ? next : cut(i);
    }
    if (batch_sync(k.stream) != hipSuccess) return AEC_FAIL(AEC_MEM_ERROR);
    return worst;
}

// A large batch as several parts side by side: every part is a batch of its own on its own kit (HIP stream,
// context, buffers), driven by its own host thread -- the uploads of one part run beside the kernels and the
// downloads of the others, and the launch sequences of many small chunks (5 launches per coded chunk, ~3 us of
// host time each) are issued from several threads.  part(lo, hi) handles chunks [lo, hi) and returns what the
// batch call would return for them; the call returns the hard error of a part if there is one, else the
// status of the last chunk that has one (as one batch does).
template <class Part>
int run_parts(size_t n, size_t total_bytes, Part part)
{
    const unsigned hw = std::thread::hardware_concurrency();
    size_t parts = total_bytes / ((size_t)4 << 20);
    // (at most 4: with 8, every part's synchronisation spinning on a core, the same batch took 9 ms instead of 2.4
    // on the 16 cores of the test machine)
    if (parts > 4) parts = 4;
    if (hw && parts > hw / 4) parts = hw / 4;
    if (parts > n / 4) parts = n / 4;
    if (parts <= 1 || t_in_part) return part((size_t)0, n);
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return AEC_FAIL(AEC_MEM_ERROR);
    std::vector<int> rcs(parts, AEC_OK);
    // (the threads are kept between calls: aec_pool.h)
    WorkerPool::run(parts, [&](size_t t) {
        (void)hipSetDevice(device);
        const bool outer = !t_in_part;
        t_in_part = true;
        try { rcs[t] = part(n * t / parts, n * (t + 1) / parts); }
        catch (const std::bad_alloc &) { rcs[t] = AEC_MEM_ERROR; }
        catch (...) { rcs[t] = AEC_MEM_ERROR; }
        if (outer) t_in_part = false;
    });
    int rc = AEC_OK;
    for (size_t t = 0; t < parts; t++)
        if (rcs[t] != AEC_OK) rc = rcs[t];
    for (size_t t = 0; t < parts; t++)
        if (rcs[t] == AEC_MEM_ERROR || rcs[t] == AEC_CONF_ERROR) rc = rcs[t];
    return rc;
}

// (AEC_ABI_TRACE) the way a decode batch takes: "chunks" (small chunks of unequal RSI counts: one walker launch and ONE
// decode launch over packed output, aec_gpu_decode_chunks_async), "batch" (small chunks of equal RSI counts), "grouped"
// (large low-entropy chunks over window tables, group by group) or "loop" (large chunks, one after the other)
void trace_decode_batch(const char *path, size_t n, size_t bytes)
{
    if (trace_on()) fprintf(stderr, "libaec (MI355X): decode batch: %zu chunks, %zu bytes on the device, path %s\n", n, bytes, path);
}

int decode_batch(const struct aec_stream *prm, size_t n, const void *const *src, const size_t *src_len,
                 void *const *dst, size_t *dst_len, int *status)
{
    aec_gpu_params gp{prm->bits_per_sample, prm->block_size, prm->rsi, prm->flags};
    Cfg c;
    int rc = make_cfg(gp.bits_per_sample, gp.block_size, gp.rsi, gp.flags, 0, false, &c);
    if (rc != RC_OK) return AEC_FAIL(rc);
    if (n == 0) return AEC_OK;
    BatchKit bk;
    if (!bk.ok) return AEC_FAIL(AEC_MEM_ERROR);
    Kit &k = bk.k;                         // (from the pool: parked with its index hint reset)
    const size_t blk_bytes = (size_t)c.bs * c.bytes, rsi_bytes = (size_t)c.rsi * blk_bytes;
    // geometry: every stream gets room for the RSIs of the largest one
    uint64_t rpc = 1;
    std::vector<uint64_t> off(n + 1);
    size_t total_in = 0;
    bool unequal = false;                  // the chunks' RSI counts differ
    for (size_t i = 0; i < n; i++) {
        off[i] = total_in;
        total_in += up16(src_len[i]) + 16;
        const uint64_t r = (dst_len[i] + rsi_bytes - 1) / rsi_bytes;
        if (i && r != (dst_len[0] + rsi_bytes - 1) / rsi_bytes) unequal = true;
        if (r > rpc) rpc = r;
    }
    off[n] = total_in;
    const bool large = total_in / n >= ((size_t)32 << 10) || n < 64;
    // Small chunks of unequal RSI counts: every chunk gets the room its own blocks need -- packed output, a table of
    // its own RSIs, a launch of the RSIs there are -- instead of the largest chunk's (aec_gpu_decode_chunks_async)
    // (streams of 16 KiB and more that the equal-stride batch would index over window tables stay with it: the serial
    // walk of such a stream is what the tables are there to avoid)
    const bool packed = !large && unequal && !aec_gpu_batch_uses_tables(k.ctx, &gp, total_in, n, rpc);
    std::vector<uint64_t> slot_at, out_want, in_len, item0;
    size_t packed_out = 0;
    uint64_t packed_entries = 0;
    if (packed) {
        slot_at.resize(n);
        out_want.resize(n);
        in_len.resize(n);
        item0.resize(n + 1);
        for (size_t i = 0; i < n; i++) {
            const uint64_t blocks = ((uint64_t)dst_len[i] / c.bytes + c.bs - 1) / c.bs;
            slot_at[i] = packed_out;
            out_want[i] = dst_len[i];
            in_len[i] = src_len[i];
            item0[i] = packed_entries - i;
            packed_out += up16((size_t)blocks * blk_bytes);
            packed_entries += (blocks + c.rsi - 1) / c.rsi + 1;
        }
        item0[n] = packed_entries - n;
    }
    // the index walker takes [off[i], off[i+1]) as stream i: the padding behind a stream is zeroed (zero
    // bits never complete a coded data set), the streams go up straight from the caller's buffers
    // (chunk offsets twice: the n + 1 absolute ones, and -- for the table path, which takes the batch in groups --
    // relative to the group a chunk belongs to, every group with a closing entry of its own: n + G entries for G <= n
    // groups, so the region holds 3 n + 4)
    const size_t o_choff = up16(packed ? (size_t)packed_entries * 8 : (size_t)n * rpc * 8),
                 o_res = o_choff + up16((3 * n + 4) * 8), o_one = o_res + up16(n * 40);
    if (!k.d_in.ensure(total_in + 32) || !k.d_out.ensure((packed ? packed_out : (size_t)n * rpc * rsi_bytes) + 64) ||
        !k.d_off.ensure(o_one + 64))
        return AEC_FAIL(AEC_MEM_ERROR);
    uint8_t *meta = static_cast<uint8_t *>(k.d_off.p);
    // (assembled in pinned memory and ONE transfer where there are a few of them and staging is to be had)
    const auto at_in = [&](size_t i) { return (size_t)off[i]; };
    const bool stage_in = n >= 4 && total_in <= kStagePiece && stage_ensure(k, total_in);
    rc = stage_up(k, n, src, at_in, [&](size_t i) { return src_len[i]; }, stage_in ? total_in : 0, true, no_launch);
    if (rc != AEC_OK) return rc;
    if (hipMemcpyAsync(meta + o_choff, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, k.stream) != hipSuccess)
        return AEC_FAIL(AEC_MEM_ERROR);
    // Small chunks: one wavefront walks each stream, all streams at once (aec_gpu_decode_batch_async).
    // Large chunks would each keep ONE wavefront busy for tens of milliseconds that way; they go through
    // the speculative index one after the other instead (all CUs per chunk), still without returning to
    // the host in between.
    aec_gpu_dec_result *d_results = reinterpret_cast<aec_gpu_dec_result *>(meta + o_res);
    aec_gpu_dec_result *d_one = reinterpret_cast<aec_gpu_dec_result *>(meta + o_one);
    // Large low-entropy chunks: groups of about 12 MiB of streams, each group ONE table launch + one wavefront
    // per stream + one decode launch (aec_gpu_decode_batch_async)
    constexpr size_t kGroupBytes = (size_t)12 << 20;
    bool grouped = false;
    if (large && n >= 2) {
        size_t probe_n = n, probe_bytes = total_in;
        if (total_in > kGroupBytes) {
            probe_n = (size_t)((uint64_t)n * kGroupBytes / total_in);
            if (probe_n < 1) probe_n = 1;
            probe_bytes = total_in / n * probe_n;
        }
        grouped = aec_gpu_batch_uses_tables(k.ctx, &gp, probe_bytes, probe_n, rpc) != 0;
    }
    if (packed) {
        trace_decode_batch("chunks", n, total_in);
        rc = aec_gpu_decode_chunks_async(k.ctx, &gp, k.d_in.p, total_in, off.data(), in_len.data(), slot_at.data(), out_want.data(),
                                         n, reinterpret_cast<uint64_t *>(meta), 0, k.d_out.p, d_results, d_one, k.stream);
        if (rc != RC_OK) return AEC_FAIL(rc);
    } else if (grouped) {
        trace_decode_batch("grouped", n, total_in);
        std::vector<uint64_t> rel;
        std::vector<size_t> first;                      // first chunk of every group, index of its offsets in rel
        std::vector<size_t> at;
        for (size_t i = 0; i < n;) {
            size_t j = i;
            while (j < n && (j == i || off[j + 1] - off[i] <= kGroupBytes)) j++;
            first.push_back(i);
            at.push_back(rel.size());
            for (size_t q = i; q <= j; q++) rel.push_back(off[q] - off[i]);
            i = j;
        }
        first.push_back(n);
        if (n + 1 + rel.size() > 3 * n + 4) return AEC_FAIL(AEC_MEM_ERROR);          // (cannot happen: rel holds n + G <= 2 n)
        uint64_t *d_rel = reinterpret_cast<uint64_t *>(meta + o_choff) + (n + 1);
        if (hipMemcpyAsync(d_rel, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, k.stream) != hipSuccess)
            return AEC_FAIL(AEC_MEM_ERROR);
        for (size_t gi = 0; gi + 1 < first.size() && rc == RC_OK; gi++) {
            const size_t i0 = first[gi], i1 = first[gi + 1];
            rc = aec_gpu_decode_batch_async(k.ctx, &gp, static_cast<const uint8_t *>(k.d_in.p) + off[i0], off[i1] - off[i0],
                                            d_rel + at[gi], i1 - i0, rpc, reinterpret_cast<uint64_t *>(meta) + i0 * rpc,
                                            static_cast<uint8_t *>(k.d_out.p) + i0 * rpc * rsi_bytes, d_results + i0, d_one,
                                            k.stream);
        }
        if (rc != RC_OK) return AEC_FAIL(rc);
        // (decoder-side errors are in the chunks' own records; the overall record belongs to the last group only)
        if (hipMemsetAsync(d_one, 0, sizeof(aec_gpu_dec_result), k.stream) != hipSuccess) return AEC_FAIL(AEC_MEM_ERROR);
    } else if (!large) {
        trace_decode_batch("batch", n, total_in);
        rc = aec_gpu_decode_batch_async(k.ctx, &gp, k.d_in.p, total_in, reinterpret_cast<uint64_t *>(meta + o_choff), n,
                                        rpc, reinterpret_cast<uint64_t *>(meta), k.d_out.p, d_results, d_one, k.stream);
        if (rc != RC_OK) return AEC_FAIL(rc);
    } else {
        trace_decode_batch("loop", n, total_in);
        // (per chunk: its own decode record behind the index records; the overall record is folded on the host)
        // (the per-chunk decode records live behind the stream's own record in d_res, which stays with the kit)
        if (!k.d_res.ensure(256 + n * sizeof(aec_gpu_dec_result) + 64)) return AEC_FAIL(AEC_MEM_ERROR);
        aec_gpu_dec_result *d_dec = reinterpret_cast<aec_gpu_dec_result *>(static_cast<uint8_t *>(k.d_res.p) + 256);
        for (size_t i = 0; i < n && rc == RC_OK; i++) {
            uint64_t *offs = reinterpret_cast<uint64_t *>(meta) + i * rpc;
            const uint8_t *in_i = static_cast<const uint8_t *>(k.d_in.p) + off[i];
            aec_gpu_set_index_hint(k.ctx, rpc ? (uint64_t)src_len[i] * 8 / rpc : 0);
            rc = aec_gpu_index_async(k.ctx, &gp, in_i, src_len[i], 0, offs, rpc, d_results + i, k.stream);
            if (rc == RC_OK)
                rc = aec_gpu_decode_indexed_async(k.ctx, &gp, in_i, src_len[i], offs, rpc, d_results + i,
                                                  static_cast<uint8_t *>(k.d_out.p) + i * rpc * rsi_bytes, d_dec + i,
                                                  k.stream);
        }
        std::vector<aec_gpu_dec_result> dec(n);
        if (rc != RC_OK || hipMemcpyAsync(dec.data(), d_dec, n * sizeof(aec_gpu_dec_result), hipMemcpyDeviceToHost,
                                          k.stream) != hipSuccess ||
            hipMemsetAsync(d_one, 0, sizeof(aec_gpu_dec_result), k.stream) != hipSuccess ||
            batch_sync(k.stream) != hipSuccess) {
            return AEC_FAIL(rc != RC_OK ? rc : AEC_MEM_ERROR);
        }
        // fold the per-chunk decode status into the per-chunk index records on the host below
        std::vector<aec_gpu_dec_result> idx(n);
        if (hipMemcpy(idx.data(), d_results, n * sizeof(aec_gpu_dec_result), hipMemcpyDeviceToHost) != hipSuccess)
            return AEC_FAIL(AEC_MEM_ERROR);
        for (size_t i = 0; i < n; i++)
            if (dec[i].status != DEC_OK) idx[i].status = DEC_DATA_ERROR;
        if (hipMemcpy(d_results, idx.data(), n * sizeof(aec_gpu_dec_result), hipMemcpyHostToDevice) != hipSuccess)
            return AEC_FAIL(AEC_MEM_ERROR);
    }
    std::vector<aec_gpu_dec_result> res(n + 1);
    if (hipMemcpyAsync(res.data(), meta + o_res, n * sizeof(aec_gpu_dec_result), hipMemcpyDeviceToHost, k.stream) != hipSuccess ||
        hipMemcpyAsync(&res[n], meta + o_one, sizeof(aec_gpu_dec_result), hipMemcpyDeviceToHost, k.stream) != hipSuccess ||
        batch_sync(k.stream) != hipSuccess)
        return AEC_FAIL(AEC_MEM_ERROR);
    // the outputs: through pinned staging in pieces of whole slots (one transfer per piece, then copies to the
    // callers' buffers on a few threads), or chunk by chunk where there is no staging to be had
    // (pieces of about 4 MiB through the two halves of the staging buffer: the transfer of piece p + 1 runs beside the
    // host's copies of piece p -- one transfer of a whole part and then its copies were the two largest items of a
    // batch of 64 x 1 MiB behind the index kernels)
    const auto finish = [&](size_t i, int *st, bool bad_item) {
        const uint64_t blocks = res[i].n_rsi * c.rsi + res[i].tail_blocks;
        size_t produced = (size_t)blocks * blk_bytes;
        if (produced > dst_len[i]) produced = dst_len[i] - dst_len[i] % c.bytes;
        if (res[i].status == DEC_DATA_ERROR || bad_item) *st = AEC_DATA_ERROR;
        return produced;
    };
    if (packed) {
        // (the packed slots in pieces of whole slots through the staging buffer; the item the overall record names
        // belongs to the last chunk whose first item is not behind it)
        size_t bad = n;
        if (res[n].status != DEC_OK)
            bad = (size_t)(std::upper_bound(item0.begin(), item0.end(), res[n].bad_rsi) - item0.begin()) - 1;
        const bool staged = n >= 4 && stage_ensure(k, packed_out < kStagePiece ? (packed_out ? packed_out : 16) : kStagePiece);
        return stage_down(k, n, dst, dst_len, status, [&](size_t i) { return (size_t)slot_at[i]; },
                          [&](size_t i) { return (size_t)((i + 1 < n ? slot_at[i + 1] : packed_out) - slot_at[i]); },
                          staged ? k.h_stage_cap : 0, false, [&](size_t i, int *st) { return finish(i, st, i == bad); });
    }
    const size_t slot_out = (size_t)rpc * rsi_bytes;
    constexpr size_t kOutPiece = (size_t)4 << 20;
    const size_t per_piece = !slot_out ? 0 : (slot_out <= kOutPiece ? kOutPiece / slot_out : (slot_out <= kStagePiece / 2 ? 1 : 0));
    const size_t npieces = per_piece ? (n + per_piece - 1) / per_piece : 0;
    const bool staged = n >= 4 && per_piece && stage_ensure(k, (npieces > 1 ? 2 : 1) * (n < per_piece ? n : per_piece) * slot_out) &&
                        k.side.event(0) && k.side.event(1);
    return stage_down(k, n, dst, dst_len, status, [&](size_t i) { return i * slot_out; }, [&](size_t) { return slot_out; },
                      staged ? per_piece * slot_out : 0, staged, [&](size_t i, int *st) {
        return finish(i, st, !grouped && res[n].status != DEC_OK && res[n].bad_rsi / rpc == i);
    });
}

// (AEC_ABI_TRACE) the way an encode batch takes: "uniform" (equal chunks of whole RSIs, one launch set), "chunks" (any
// other batch of two and more, one launch set) or "loop" (chunk after chunk)
void trace_encode_batch(const char *path, size_t n, size_t bytes)
{
    if (trace_on()) fprintf(stderr, "libaec (MI355X): encode batch: %zu chunks, %zu bytes on the device, path %s\n", n, bytes, path);
}

int encode_batch_host(const struct aec_stream *prm, size_t n, const void *const *src, const size_t *src_len,
                      void *const *dst, size_t *dst_len, int *status)
{
    aec_gpu_params gp{prm->bits_per_sample, prm->block_size, prm->rsi, prm->flags};
    Cfg c;
    int rc = make_cfg(gp.bits_per_sample, gp.block_size, gp.rsi, gp.flags, 0, true, &c);
    if (rc != RC_OK) return AEC_FAIL(rc);
    if (n == 0) return AEC_OK;
    BatchKit bk;
    if (!bk.ok) return AEC_FAIL(AEC_MEM_ERROR);
    Kit &k = bk.k;
    std::vector<uint64_t> off(n + 1);
    size_t total_in = 0, largest = 0;
    for (size_t i = 0; i < n; i++) {
        off[i] = total_in;
        const size_t whole = src_len[i] - src_len[i] % c.bytes;          // only whole samples are coded
        total_in += up16(whole) + 16;
        if (whole > largest) largest = whole;
    }
    off[n] = total_in;
    // Equal chunks of whole RSIs (what HDF5 hands the SZIP filter): ONE launch set for all of them, the streams
    // back to back on the device, one transfer each way (aec_gpu_encode_uniform_batch_async)
    {
        bool equal = n >= 2 && src_len[0] && src_len[0] % c.bytes == 0;
        for (size_t i = 1; i < n && equal; i++) equal = src_len[i] == src_len[0];
        const size_t len = src_len[0];
        if (equal && aec_gpu_uniform_batch_ok(&gp, len, n)) {
            trace_encode_batch("uniform", n, n * len);
            const size_t bound = up16(aec_gpu_encode_bound(&gp, len)), cap = n * bound;
            const size_t o_rec = up16(n * sizeof(aec_gpu_batch_chunk));
            if (!k.d_in.ensure(n * len + 32) || !k.d_out.ensure(cap) || !k.d_off.ensure(o_rec + 64))
                return AEC_FAIL(AEC_MEM_ERROR);
            aec_gpu_batch_chunk *d_chunks = static_cast<aec_gpu_batch_chunk *>(k.d_off.p);
            aec_gpu_enc_result *d_one = reinterpret_cast<aec_gpu_enc_result *>(static_cast<uint8_t *>(k.d_off.p) + o_rec);
            // up: through pinned staging in pieces (host copies on a few threads, one transfer per piece)
            const size_t per_up = len <= kStagePiece ? kStagePiece / len : 0;
            // (also large chunks: copies from and to pageable memory issued by several threads at once were measured
            // erratic -- 2.4 or 9 ms for the same 64 MiB -- while pinned transfers plus plain memcpy are steady)
            const size_t up_bytes = (n < per_up ? n : per_up) * len;
            const size_t cap_up = per_up && stage_ensure(k, up_bytes) ? up_bytes : 0;
            rc = stage_up(k, n, src, [&](size_t i) { return i * len; }, [&](size_t) { return len; }, cap_up, false, no_launch);
            if (rc != AEC_OK) return rc;
            rc = aec_gpu_encode_uniform_batch_async(k.ctx, &gp, k.d_in.p, len, n, k.d_out.p, cap, d_chunks, d_one, k.stream);
            if (rc != RC_OK) return AEC_FAIL(rc);

            std::vector<aec_gpu_batch_chunk> rec(n);
            aec_gpu_enc_result one{};
            if (hipMemcpyAsync(rec.data(), d_chunks, n * sizeof(aec_gpu_batch_chunk), hipMemcpyDeviceToHost, k.stream) != hipSuccess ||
                hipMemcpyAsync(&one, d_one, sizeof(one), hipMemcpyDeviceToHost, k.stream) != hipSuccess ||
                batch_sync(k.stream) != hipSuccess)
                return AEC_FAIL(AEC_MEM_ERROR);
            if (one.overflow) return AEC_FAIL(AEC_MEM_ERROR);                     // (cannot happen: cap is the sum of the bounds)

            // down: the packed streams in pieces of whole streams through the staging buffer
            const size_t total = (size_t)(one.total_bits / 8);
            const bool staged = stage_ensure(k, total < kStagePiece ? (total ? total : 16) : kStagePiece);
            const auto ext = [&](size_t i) { return (size_t)((rec[i].bits + 7) / 8); };
            return stage_down(k, n, dst, dst_len, status, [&](size_t i) { return (size_t)(rec[i].base_bits / 8); }, ext,
                              staged ? k.h_stage_cap : 0, false, [&](size_t i, int *st) {
                if (ext(i) <= dst_len[i]) return ext(i);
                *st = AEC_STREAM_ERROR;                                                     // as aec_buffer_encode: a prefix
                return dst_len[i];
            });
        }
    }
    const auto whole = [&](size_t i) { return src_len[i] - src_len[i] % c.bytes; };
    const bool stage_in = n >= 16 && largest <= ((size_t)256 << 10) && stage_ensure(k, total_in < kStagePiece ? total_in : kStagePiece);
    // Any other batch of two chunks and more: still ONE launch set (aec_gpu_encode_chunks_async) -- the chunks at their
    // 16-byte aligned off[i] on the device, the streams back to back, one transfer each way
    aec_gpu_chunks_plan plan;
    std::vector<uint64_t> lens(n);
    for (size_t i = 0; i < n; i++) lens[i] = whole(i);
    if (n >= 2 && aec_gpu_encode_chunks_plan(&gp, lens.data(), n, &plan)) {
        trace_encode_batch("chunks", n, total_in);
        const size_t o_rec = up16(n * sizeof(aec_gpu_batch_chunk));
        if (!k.d_in.ensure(total_in + 32) || !k.d_out.ensure(plan.out_bound) || !k.d_off.ensure(o_rec + 64))
            return AEC_FAIL(AEC_MEM_ERROR);
        aec_gpu_batch_chunk *d_chunks = static_cast<aec_gpu_batch_chunk *>(k.d_off.p);
        aec_gpu_enc_result *d_one = reinterpret_cast<aec_gpu_enc_result *>(static_cast<uint8_t *>(k.d_off.p) + o_rec);
        rc = stage_up(k, n, src, [&](size_t i) { return (size_t)off[i]; }, whole, stage_in ? k.h_stage_cap : 0, false, no_launch);
        if (rc != AEC_OK) return rc;
        rc = aec_gpu_encode_chunks_async(k.ctx, &gp, k.d_in.p, off.data(), lens.data(), n, k.d_out.p, plan.out_bound, d_chunks,
                                         nullptr, d_one, k.stream);
        if (rc != RC_OK) return AEC_FAIL(rc);
        std::vector<aec_gpu_batch_chunk> rec(n);
        aec_gpu_enc_result one{};
        if (hipMemcpyAsync(rec.data(), d_chunks, n * sizeof(aec_gpu_batch_chunk), hipMemcpyDeviceToHost, k.stream) != hipSuccess ||
            hipMemcpyAsync(&one, d_one, sizeof(one), hipMemcpyDeviceToHost, k.stream) != hipSuccess ||
            batch_sync(k.stream) != hipSuccess)
            return AEC_FAIL(AEC_MEM_ERROR);
        if (one.overflow) return AEC_FAIL(AEC_MEM_ERROR);                         // (cannot happen: cap is the plan's bound)
        const size_t total = (size_t)(one.total_bits / 8);
        const bool staged = stage_ensure(k, total < kStagePiece ? (total ? total : 16) : kStagePiece);
        const auto ext = [&](size_t i) { return rec[i].bits ? (size_t)((rec[i].bits + 7) / 8) : (size_t)1; };   // an empty stream is one zero byte
        return stage_down(k, n, dst, dst_len, status, [&](size_t i) { return (size_t)(rec[i].base_bits / 8); }, ext,
                          staged ? k.h_stage_cap : 0, false, [&](size_t i, int *st) {
            if (ext(i) <= dst_len[i]) return ext(i);
            *st = AEC_STREAM_ERROR;                                                         // as aec_buffer_encode: a prefix
            return dst_len[i];
        });
    }
    trace_encode_batch("loop", n, total_in);
    const size_t slot = aec_gpu_encode_bound(&gp, largest);
    if (!k.d_in.ensure(total_in + 32) || !k.d_out.ensure(n * slot) || !k.d_off.ensure(n * sizeof(aec_gpu_enc_result) + 64))
        return AEC_FAIL(AEC_MEM_ERROR);
    // chunk i = [off[i], off[i] + whole samples): the padding between chunks is not input.  Small chunks go up
    // together through pinned staging (one transfer per piece); large ones straight from the callers' buffers, upload
    // and coding alternating so that the kernels of one chunk run while the host stages the next one's copy.
    aec_gpu_enc_result *d_res = static_cast<aec_gpu_enc_result *>(k.d_off.p);
    if (aec_gpu_reserve(k.ctx, &gp, largest) != RC_OK) return AEC_FAIL(AEC_MEM_ERROR);
    rc = stage_up(k, n, src, [&](size_t i) { return (size_t)off[i]; }, whole, stage_in ? k.h_stage_cap : 0, false, [&](size_t i) {
        const uint64_t pair[2] = {off[i], off[i] + whole(i)};
        const int erc = aec_gpu_encode_batch_async(k.ctx, &gp, k.d_in.p, pair, 1, static_cast<uint8_t *>(k.d_out.p) + i * slot, slot,
                                                   d_res + i, k.stream);
        return erc == RC_OK ? AEC_OK : AEC_FAIL(erc);
    });
    if (rc != AEC_OK) return rc;
    std::vector<aec_gpu_enc_result> res(n);
    if (hipMemcpyAsync(res.data(), d_res, n * sizeof(aec_gpu_enc_result), hipMemcpyDeviceToHost, k.stream) != hipSuccess ||
        batch_sync(k.stream) != hipSuccess)
        return AEC_FAIL(AEC_MEM_ERROR);
    // many small streams: whole slots through pinned staging, piece by piece (a transfer per piece beats a copy
    // call per stream even though a slot is the worst case of its stream)
    const size_t per_piece = slot <= kStagePiece ? kStagePiece / slot : 0;
    const bool stage_out = n >= 16 && slot <= ((size_t)512 << 10) && per_piece &&
                           stage_ensure(k, (n < per_piece ? n : per_piece) * slot);
    return stage_down(k, n, dst, dst_len, status, [&](size_t i) { return i * slot; }, [&](size_t) { return slot; },
                      stage_out ? per_piece * slot : 0, false, [&](size_t i, int *st) {
        size_t bytes = (size_t)((res[i].total_bits + 7) / 8);
        if (bytes == 0) bytes = 1;                                           // an empty stream is one zero byte
        if (res[i].overflow) *st = AEC_MEM_ERROR;
        else if (bytes > dst_len[i]) { *st = AEC_STREAM_ERROR; bytes = dst_len[i]; }   // as aec_buffer_encode: a prefix
        return bytes;
    });
}

// ---- random access (include/libaec.h: aec_decode_range) -----------------------------------------------
// The window's RSIs in batches of whole RSIs, kPipeOut of output each: per batch, the stream bytes from its first RSI's
// start to the next table entry behind its last one go up with the batch's rebased table, aec_gpu_decode_range_async
// decodes its blocks in place (from an RSI start to a block end), and the window's part of them goes to the caller's
// buffer -- a small one with the result record (one synchronisation), a large one on the side stream beside the next
// batch's kernels (the two output buffers alternate, as in decode_run).  No index pass: the table says where RSIs start.
int decode_range_call(struct aec_stream *strm, const size_t *offs, size_t n, size_t pos, size_t size)
{
    internal_state *s = strm->state;
    if (!s || s->encoder) return AEC_FAIL(AEC_STREAM_ERROR);
    if (size == 0) return AEC_OK;
    if (s->took_input) return AEC_FAIL(AEC_STREAM_ERROR);
    const Cfg &c = s->cfg;
    const size_t blk_bytes = (size_t)c.bs * c.bytes, rsi_bytes = (size_t)c.rsi * blk_bytes;
    if (!offs || pos / rsi_bytes >= n) return AEC_FAIL(AEC_DATA_ERROR);
    if (strm->avail_out < size) return AEC_FAIL(AEC_MEM_ERROR);
    if (pos + size < pos) return AEC_FAIL(AEC_DATA_ERROR);
    const size_t r0 = pos / rsi_bytes, r1 = (pos + size - 1) / rsi_bytes;
    if (r1 >= n) return AEC_FAIL(AEC_DATA_ERROR);       // (the table ends in front of the window: the stream does too)
    // the entries the window reads, and the one behind it: strictly increasing, inside the input
    const uint64_t in_bits = (uint64_t)strm->avail_in * 8;
    const size_t last = r1 + 1 < n ? r1 + 1 : n - 1;
    for (size_t i = r0; i <= last; i++)
        if (offs[i] >= in_bits || (i > r0 && offs[i] <= offs[i - 1])) return AEC_FAIL(AEC_DATA_ERROR);

    // (at least kRangeRsis RSIs per batch: long RSIs -- 512 KiB of 32-bit output each -- are a wavefront each, and a
    // batch of fewer than the chip holds at once leaves it part idle: k_decode_wave<32, 4> takes 244 VGPRs, 8 waves per
    // CU, 2048 on 256 CUs, and one launch of them takes ~3.1 ms whether it has 512 RSIs or 2048 (profiles/r07: config 3,
    // 1 GiB: 29.7 GB/s with batches of 512 RSIs, 34.6 with 1024, 39.2 with 2048))
    const size_t per = kPipeOut / rsi_bytes > kRangeRsis ? kPipeOut / rsi_bytes : kRangeRsis;
    aec_gpu_dec_result *d_dec = static_cast<aec_gpu_dec_result *>(s->d_res.p);
    uint8_t *bounce = s->h_res + 256;
    int rc = AEC_OK;
    std::vector<uint64_t> tbl;
    for (size_t ra = r0; ra <= r1 && rc == AEC_OK; ra += per) {
        const size_t rb = ra + per - 1 < r1 ? ra + per - 1 : r1;
        const bool next = rb + 1 < n;
        const uint64_t first = (uint64_t)ra * rsi_bytes;
        const uint64_t lo = pos > first ? pos : first;
        const uint64_t hi = pos + size < (uint64_t)(rb + 1) * rsi_bytes ? pos + size : (uint64_t)(rb + 1) * rsi_bytes;
        const uint64_t dev_size = (hi + blk_bytes - 1) / blk_bytes * blk_bytes - first;
        // stream bytes of the batch: from its first RSI's word to a little behind the next entry (or the input's end)
        const size_t from = (size_t)(offs[ra] / 8) & ~(size_t)3;
        size_t to = next ? (size_t)(offs[rb + 1] / 8) + 8 : strm->avail_in;
        if (to > strm->avail_in) to = strm->avail_in;
        const size_t in_bytes = to - from;
        tbl.resize(rb - ra + 1 + (next ? 1 : 0));
        for (size_t i = 0; i < tbl.size(); i++) tbl[i] = offs[ra + i] - (uint64_t)from * 8;
        DevBuf &obuf = s->out_buf();
        if (!s->d_in.ensure(in_bytes + 32) || !s->d_off.ensure(tbl.size() * 8) || !obuf.ensure(dev_size + 64) ||
            !s->side.claim(s->stream)) {
            rc = AEC_FAIL(AEC_MEM_ERROR);
            break;
        }
        if (hipMemcpyAsync(s->d_in.p, strm->next_in + from, in_bytes, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
            hipMemcpyAsync(s->d_off.p, tbl.data(), tbl.size() * 8, hipMemcpyHostToDevice, s->stream) != hipSuccess) {
            rc = AEC_FAIL(AEC_MEM_ERROR);
            break;
        }
        const int grc = aec_gpu_decode_range_async(s->ctx, &s->prm, s->d_in.p, in_bytes, static_cast<const uint64_t *>(s->d_off.p),
                                                   tbl.size(), 0, dev_size, obuf.p, d_dec, s->stream);
        if (grc != RC_OK) {
            rc = AEC_FAIL(grc == RC_MEM_ERROR ? AEC_MEM_ERROR : AEC_DATA_ERROR);
            break;
        }
        const uint8_t *d_bytes = static_cast<const uint8_t *>(obuf.p) + (lo - first);
        const size_t len = (size_t)(hi - lo);
        const bool small = len <= kBounce;
        if (hipMemcpyAsync(s->h_res, d_dec, sizeof(aec_gpu_dec_result), hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
            (small && hipMemcpyAsync(bounce, d_bytes, len, hipMemcpyDeviceToHost, s->stream) != hipSuccess) ||
            hipStreamSynchronize(s->stream) != hipSuccess) {
            rc = AEC_FAIL(AEC_MEM_ERROR);
            break;
        }
        const aec_gpu_dec_result dec = *reinterpret_cast<const aec_gpu_dec_result *>(s->h_res);
        if (dec.status != DEC_OK) {
            if (trace_on())
                fprintf(stderr, "libaec (MI355X): aec_decode_range: status %u at RSI %llu of the table\n", dec.status,
                        (unsigned long long)(ra + dec.bad_rsi));
            rc = AEC_DATA_ERROR;
            break;
        }
        uint8_t *dst = strm->next_out + (lo - pos);
        if (small) {
            memcpy(dst, bounce, len);
            continue;
        }
        if (!s->side.copy_out(dst, d_bytes, len, true)) rc = AEC_FAIL(AEC_MEM_ERROR);
    }
    // (nothing of ours may still write the caller's buffer on return)
    if (!s->side.done() && rc == AEC_OK) rc = AEC_FAIL(AEC_MEM_ERROR);
    if (rc != AEC_OK) return rc;
    strm->next_out += size;
    strm->avail_out -= size;
    strm->total_out += size;
    return AEC_OK;
}

}  // namespace

extern "C" {

int aec_buffer_decode_batch(const struct aec_stream *params, size_t n, const void *const *src, const size_t *src_len,
                            void *const *dst, size_t *dst_len, int *status)
{
    try {
        size_t total = 0;
        for (size_t i = 0; i < n; i++) total += dst_len[i];
        return run_parts(n, total, [&](size_t lo, size_t hi) {
            return decode_batch(params, hi - lo, src + lo, src_len + lo, dst + lo, dst_len + lo, status ? status + lo : nullptr);
        });
    } catch (const std::bad_alloc &) { return AEC_MEM_ERROR; }
}

int aec_buffer_encode_batch(const struct aec_stream *params, size_t n, const void *const *src, const size_t *src_len,
                            void *const *dst, size_t *dst_len, int *status)
{
    try {
        size_t total = 0;
        for (size_t i = 0; i < n; i++) total += src_len[i];
        return run_parts(n, total, [&](size_t lo, size_t hi) {
            return encode_batch_host(params, hi - lo, src + lo, src_len + lo, dst + lo, dst_len + lo, status ? status + lo : nullptr);
        });
    } catch (const std::bad_alloc &) { return AEC_MEM_ERROR; }
}

int aec_encode_init(struct aec_stream *strm)
{
    try { return init_common(strm, true); } catch (const std::bad_alloc &) { return AEC_MEM_ERROR; }
}
int aec_decode_init(struct aec_stream *strm)
{
    try { return init_common(strm, false); } catch (const std::bad_alloc &) { return AEC_MEM_ERROR; }
}

int aec_encode(struct aec_stream *strm, int flush)
{
    try {
        return encode_call(strm, flush);
    } catch (const std::bad_alloc &) {
        strm->total_in -= strm->avail_in;      // (added on entry, as on every other way out)
        strm->total_out -= strm->avail_out;
        return AEC_MEM_ERROR;
    }
}

int aec_encode_end(struct aec_stream *strm)
{
    internal_state *s = strm->state;
    int status = AEC_OK;
    if (s->flush == AEC_FLUSH && !s->flushed) status = AEC_STREAM_ERROR;   // reference encode.c:944-945
    free_state(s);
    strm->state = nullptr;
    return status;
}

int aec_buffer_encode(struct aec_stream *strm)
{
    int status = aec_encode_init(strm);
    if (status != AEC_OK) return status;
    status = aec_encode(strm, AEC_FLUSH);
    if (status != AEC_OK) {
        free_state(strm->state);
        strm->state = nullptr;
        return status;
    }
    return aec_encode_end(strm);
}

int aec_decode(struct aec_stream *strm, int flush)
{
    try {
        return decode_call(strm, flush);   // (flush is ignored by the reference, decode.c:797; here it only
                                           // says that the caller is not trickling input in)
    } catch (const std::bad_alloc &) {
        (void)strm->state->side.done();        // (nothing of ours may still write the caller's buffer)
        strm->total_in -= strm->avail_in;      // (added on entry, as on every other way out)
        strm->total_out -= strm->avail_out;
        return AEC_MEM_ERROR;
    }
}

int aec_decode_end(struct aec_stream *strm)
{
    free_state(strm->state);
    strm->state = nullptr;
    return AEC_OK;
}

int aec_encode_enable_offsets(struct aec_stream *strm)
{
    internal_state *s = strm->state;
    if (!s || !s->encoder || s->took_input) return AEC_RSI_OFFSETS_ERROR;
    s->offsets_on = true;
    return AEC_OK;
}

int aec_decode_enable_offsets(struct aec_stream *strm)
{
    internal_state *s = strm->state;
    if (!s || s->encoder || s->took_input) return AEC_RSI_OFFSETS_ERROR;
    s->offsets_on = true;
    return AEC_OK;
}

static int count_offsets(struct aec_stream *strm, bool encoder, size_t *count)
{
    internal_state *s = strm->state;
    if (!s || s->encoder != encoder || !s->offsets_on) {
        if (count) *count = 0;
        return AEC_RSI_OFFSETS_ERROR;
    }
    if (!count) return AEC_MEM_ERROR;
    *count = s->offs.size();
    return AEC_OK;
}

static int get_offsets(struct aec_stream *strm, bool encoder, size_t *offsets, size_t count)
{
    internal_state *s = strm->state;
    if (!s || s->encoder != encoder || !s->offsets_on) return AEC_RSI_OFFSETS_ERROR;
    if (count < s->offs.size() || (!offsets && !s->offs.empty())) return AEC_MEM_ERROR;
    for (size_t i = 0; i < s->offs.size(); i++) offsets[i] = (size_t)s->offs[i];
    return AEC_OK;
}

int aec_encode_count_offsets(struct aec_stream *strm, size_t *rsi_offsets_count)
{
    return count_offsets(strm, true, rsi_offsets_count);
}
int aec_encode_get_offsets(struct aec_stream *strm, size_t *rsi_offsets, size_t rsi_offsets_count)
{
    return get_offsets(strm, true, rsi_offsets, rsi_offsets_count);
}
int aec_decode_count_offsets(struct aec_stream *strm, size_t *rsi_offsets_count)
{
    return count_offsets(strm, false, rsi_offsets_count);
}
int aec_decode_get_offsets(struct aec_stream *strm, size_t *rsi_offsets, size_t rsi_offsets_count)
{
    return get_offsets(strm, false, rsi_offsets, rsi_offsets_count);
}

int aec_buffer_seek(struct aec_stream *strm, size_t offset)
{
    internal_state *s = strm->state;
    if (!s || s->encoder || s->took_input) return AEC_STREAM_ERROR;
    if (offset / 8 >= strm->avail_in) return AEC_MEM_ERROR;     // (the bit lies beyond the input)
    strm->next_in += offset / 8;
    strm->avail_in -= offset / 8;
    s->walk_bit = s->rsi_start_bit = offset % 8;             // (the first RSI starts at that bit of the byte)
    return AEC_OK;
}

int aec_decode_range(struct aec_stream *strm, const size_t *rsi_offsets, size_t rsi_offsets_count, size_t pos,
                     size_t size)
{
    try {
        return decode_range_call(strm, rsi_offsets, rsi_offsets_count, pos, size);
    } catch (const std::bad_alloc &) {
        (void)strm->state->side.done();        // (nothing of ours may still write the caller's buffer)
        return AEC_MEM_ERROR;
    }
}

int aec_buffer_decode(struct aec_stream *strm)
{
    int status = aec_decode_init(strm);
    if (status != AEC_OK) return status;
    status = aec_decode(strm, AEC_FLUSH);
    aec_decode_end(strm);
    return status;
}

}  // extern "C"
