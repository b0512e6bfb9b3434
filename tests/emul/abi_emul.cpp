// abi_emul.cpp -- the three pure parts of a streaming decode batch (libaec_amd/csrc/aec_stream_plan.h: plan_batch,
// judge_batch, advance_stream) over arrays of 64-bit values, for tests/test_stream_plan.py.  Host only, no HIP.
//
//   cfg   bits per sample, block size, rsi, flags
//   pos   base, d_len, rsi_start_bit, rsi_bits_seen, walk_bit, walk_blocks, delivered, walked_len, span_mul, span_wide, more
//   rec   n_rsi, tail_blocks, end_bit, status, pad, bad_rsi                    (an aec_gpu_dec_result)
//   plan  walk_rel, rsi_rel, skip, hint, pipe, max_rsi, in_bytes, piece, off_bytes, out_bytes, seg_bytes
//   verd  total, part, corrupt, more_behind, good_rsi, tail_blocks, res_rsi, res_tail, res_end, fetch_off
#include <stdint.h>

#include "../../libaec_amd/csrc/aec_stream_plan.h"

using namespace aec;

namespace {

bool cfg_of(const uint64_t *cfg, Cfg *c)
{
    return make_cfg((uint32_t)cfg[0], (uint32_t)cfg[1], (uint32_t)cfg[2], (uint32_t)cfg[3], 0, false, c) == RC_OK;
}
StreamPos pos_of(const uint64_t *v)
{
    StreamPos p;
    p.base = v[0]; p.d_len = (size_t)v[1]; p.rsi_start_bit = v[2]; p.rsi_bits_seen = v[3]; p.walk_bit = v[4];
    p.walk_blocks = (uint32_t)v[5]; p.delivered = v[6]; p.walked_len = (size_t)v[7]; p.span_mul = v[8];
    p.span_wide = v[9] != 0; p.more = v[10] != 0;
    return p;
}
void pos_to(const StreamPos &p, uint64_t *v)
{
    const uint64_t out[11] = {p.base, p.d_len, p.rsi_start_bit, p.rsi_bits_seen, p.walk_bit, p.walk_blocks, p.delivered,
                              p.walked_len, p.span_mul, p.span_wide, p.more};
    for (int i = 0; i < 11; i++) v[i] = out[i];
}
aec_gpu_dec_result rec_of(const uint64_t *v)
{
    return aec_gpu_dec_result{v[0], v[1], v[2], (uint32_t)v[3], (uint32_t)v[4], v[5]};
}
BatchPlan plan_of(const uint64_t *v)
{
    BatchPlan b;
    b.walk_rel = v[0]; b.rsi_rel = v[1]; b.skip = (size_t)v[2]; b.hint = v[3]; b.pipe = v[4] != 0; b.max_rsi = v[5];
    b.in_bytes = (size_t)v[6]; b.piece = v[7] != 0; b.off_bytes = (size_t)v[8]; b.out_bytes = (size_t)v[9];
    b.seg_bytes = (size_t)v[10];
    return b;
}
BatchVerdict verdict_of(const uint64_t *v)
{
    BatchVerdict r;
    r.total = (size_t)v[0]; r.part = (uint32_t)v[1]; r.corrupt = v[2] != 0; r.more_behind = v[3] != 0; r.good_rsi = v[4];
    r.tail_blocks = v[5]; r.res_rsi = v[6]; r.res_tail = v[7]; r.res_end = v[8]; r.fetch_off = v[9] != 0;
    return r;
}

}  // namespace

extern "C" {

void emul_constants(uint64_t *out)
{
    out[0] = kMinBatchOut;
    out[1] = kPipeOut;
    out[2] = kPipeMin;
}

uint64_t emul_worst_rsi_bytes(const uint64_t *cfg)
{
    Cfg c;
    return cfg_of(cfg, &c) ? worst_rsi_bytes(c) : 0;
}

int emul_plan(const uint64_t *cfg, const uint64_t *pos, uint64_t room, int windowed, uint64_t *plan)
{
    Cfg c;
    if (!cfg_of(cfg, &c)) return -1;
    const BatchPlan b = plan_batch(c, pos_of(pos), (size_t)room, windowed != 0);
    const uint64_t out[11] = {b.walk_rel, b.rsi_rel, b.skip, b.hint, b.pipe, b.max_rsi, b.in_bytes, b.piece, b.off_bytes,
                              b.out_bytes, b.seg_bytes};
    for (int i = 0; i < 11; i++) plan[i] = out[i];
    return 0;
}

int emul_verdict(const uint64_t *cfg, const uint64_t *idx, const uint64_t *dec, uint64_t skip, uint64_t want_out,
                 uint64_t *verd)
{
    Cfg c;
    if (!cfg_of(cfg, &c)) return -1;
    const BatchVerdict v = judge_batch(c, rec_of(idx), rec_of(dec), (size_t)skip, (size_t)want_out);
    const uint64_t out[10] = {v.total, v.part, v.corrupt, v.more_behind, v.good_rsi, v.tail_blocks, v.res_rsi, v.res_tail,
                              v.res_end, v.fetch_off};
    for (int i = 0; i < 10; i++) verd[i] = out[i];
    return 0;
}

// pos is advanced in place; returns the bytes dropped from the front of the resident stream (-1: bad parameters)
int64_t emul_advance(const uint64_t *cfg, uint64_t *pos, const uint64_t *plan, const uint64_t *verd, const uint64_t *idx,
                     uint64_t tail_start)
{
    Cfg c;
    if (!cfg_of(cfg, &c)) return -1;
    StreamPos p = pos_of(pos);
    const size_t drop = advance_stream(c, p, plan_of(plan), verdict_of(verd), rec_of(idx), tail_start);
    pos_to(p, pos);
    return (int64_t)drop;
}

}  // extern "C"
