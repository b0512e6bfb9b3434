/*
 * aec_gpu_sz.h -- SZIP chunks that stay on the device.
 *
 * szlib.h (SZ_BufftoBuffCompress / SZ_BufftoBuffDecompress) takes host buffers and marshals them on the host; the
 * coder underneath (aec_gpu.h) is device-resident.  These entry points are the layer between the two for a caller
 * whose chunks live in HBM (an HDF5 VOL / filter): what the reference's shim does around its one coder call
 * (reference src/sz_compat.c:39-108, 134-166, 208-261) as kernels --
 *   byte planes     32- and 64-bit pixels are coded as 4 / 8 planes of bytes, plane after plane;
 *   line padding    every scan line becomes one RSI: a line that is not a whole number of blocks, and a partial
 *                   last line, are padded with the last pixel (SZ_NN_OPTION_MASK) or with zero;
 *   un-padding      the reverse after decoding.
 * All pointers marked d_ are HIP device pointers; every call only ENQUEUES work on `stream` (a hipStream_t passed as
 * void*), allocates nothing and reads nothing back.  Exported by libaec.so.0.  Only whole pixels are coded: a chunk's
 * trailing fraction of a pixel is not part of the stream and comes back as zero bytes.
 */
#ifndef AEC_GPU_SZ_H
#define AEC_GPU_SZ_H 1

#include "aec_gpu.h"
#include "szlib.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What one chunk of chunk_bytes under an SZ_com_t looks like to the coder. */
typedef struct aec_gpu_sz_layout_s {
    aec_gpu_params coder;     /* bits per sample 8 with byte planes; rsi = ceil(pixels_per_scanline / pixels_per_block);
                                 flags from the option mask (MSB, NN -> AEC_DATA_MSB, AEC_DATA_PREPROCESS) plus
                                 AEC_NOT_ENFORCE, which the encoder needs and the decoder ignores */
    unsigned int word;        /* 0, or 4 / 8: bytes per pixel when byte planes are used */
    unsigned int pixel;       /* container bytes of a coded sample: 1 / 2 / 4 */
    unsigned int fill_repeat; /* 1: padding repeats the last pixel; 0: zero */
    unsigned int passthrough; /* 1: no planes, no padding, whole lines, whole pixels -- the chunk as it lies is the
                                 coder's input and the coder's output is the chunk */
    uint64_t line;            /* bytes of a scan line (with planes: of the concatenated planes) */
    uint64_t padded_line;     /* bytes of the RSI it becomes */
    uint64_t lines;           /* scan lines = RSIs per chunk (the last line may be partial) */
    uint64_t coder_bytes;     /* lines * padded_line: the coder's input / output per chunk */
    uint64_t coded_bytes;     /* the chunk's whole pixels */
} aec_gpu_sz_layout_t;

/* Host arithmetic only.  AEC_CONF_ERROR for what SZ_BufftoBuffCompress or aec_gpu_check_params reject (pixels per
 * block 0, odd or above 64; pixels per scan line 0 or more than 4096 blocks; bits per pixel 0, 33..63, above 64) and
 * for a chunk that holds no whole pixel. */
AEC_GPU_API int aec_gpu_sz_layout(const SZ_com_t *sz, size_t chunk_bytes, aec_gpu_sz_layout_t *layout);

/*
 * n_chunks equal chunks lying back to back at d_src (any alignment) -> their coder inputs back to back at d_coder_in
 * (16-byte aligned, n_chunks * coder_bytes bytes), and the inverse: exactly chunk_bytes per chunk are written at
 * d_dst + i * chunk_bytes (any alignment) and nothing outside them.  Source and destination must not overlap.
 * Chunks and lines that are 16-byte aligned move 16 bytes per lane; byte planes are split and merged in registers
 * when every plane and line is a multiple of 4 bytes and the chunks are 16-byte aligned; everything else (unaligned
 * chunk bases, line tails, padding, a partial last line, planes of odd length) goes byte by byte.
 */
AEC_GPU_API int aec_gpu_sz_marshal_async(const SZ_com_t *sz, const void *d_src, size_t chunk_bytes, uint64_t n_chunks,
                                         void *d_coder_in, void *stream);
AEC_GPU_API int aec_gpu_sz_unmarshal_async(const SZ_com_t *sz, const void *d_coder_out, size_t chunk_bytes,
                                           uint64_t n_chunks, void *d_dst, void *stream);

/*
 * 1 when the one-call forms below take such a batch: the layout is valid and aec_gpu_uniform_batch_ok holds for
 * (coder, coder_bytes, n_chunks).  A stride coder_bytes that is not a multiple of 16 is SERVED: the encoder's fast
 * loads need 16-byte aligned RSIs and it takes its byte-wise loader otherwise, the decoder stores whole blocks from a
 * 16-byte aligned base whatever the RSI size.  When 0 (a chunk of more than 2048 segments of 64 blocks, ...), or when
 * the chunks differ in size: aec_gpu_sz_compress_chunks_async below takes any batch in one call.
 */
AEC_GPU_API int aec_gpu_sz_batch_ok(const SZ_com_t *sz, size_t chunk_bytes, uint64_t n_chunks);

/*
 * SZ_BufftoBuffCompress of n_chunks equal chunks at d_src in one enqueue: marshal into d_work, then
 * aec_gpu_encode_uniform_batch_async.  d_work: n_chunks * coder_bytes bytes, 16-byte aligned, caller-provided; unused
 * (may be NULL) when the layout says passthrough.  d_out, out_cap, d_chunks, d_result: exactly as that call defines
 * them; stream i is byte for byte what SZ_BufftoBuffCompress returns for chunk i.  AEC_CONF_ERROR when
 * aec_gpu_sz_batch_ok says 0.
 */
AEC_GPU_API int aec_gpu_sz_compress_batch_async(aec_gpu_ctx *ctx, const SZ_com_t *sz, const void *d_src,
                                                size_t chunk_bytes, uint64_t n_chunks, void *d_work, void *d_out,
                                                size_t out_cap, aec_gpu_batch_chunk *d_chunks,
                                                aec_gpu_enc_result *d_result, void *stream);

/*
 * SZ_BufftoBuffDecompress of n_chunks streams in one enqueue: aec_gpu_decode_batch_async (d_in, in_bytes,
 * d_chunk_offsets, d_rsi_bit_offsets -- n_chunks * lines entries --, d_results, d_result as there, rsi_per_chunk =
 * lines), then un-marshal to d_dst + i * chunk_bytes.  The decode goes to d_work (n_chunks * coder_bytes bytes,
 * 16-byte aligned), or straight to d_dst when the layout says passthrough and d_dst is 16-byte aligned (d_work may
 * then be NULL).  Per-chunk status is in d_results; the bytes of a chunk whose record is not clean (status != 0 or
 * fewer than `lines` RSIs) are unspecified, every other chunk is exact.
 */
AEC_GPU_API int aec_gpu_sz_decompress_batch_async(aec_gpu_ctx *ctx, const SZ_com_t *sz, const void *d_in,
                                                  size_t in_bytes, const uint64_t *d_chunk_offsets, uint64_t n_chunks,
                                                  size_t chunk_bytes, uint64_t *d_rsi_bit_offsets, void *d_work,
                                                  void *d_dst, aec_gpu_dec_result *d_results,
                                                  aec_gpu_dec_result *d_result, void *stream);

/*
 * Chunks of ANY size under one SZ_com_t, in one call: the marshalling above per chunk around the chunk coder of
 * aec_gpu.h (aec_gpu_encode_chunks_async / aec_gpu_decode_chunks_async: one launch set for the whole batch, no limit on
 * a chunk's segments, and the encoder's RSI table, with which the decoder needs no index pass).  Every array argument
 * is a HOST array of n_chunks entries and is free again when the call returns.
 *
 * aec_gpu_sz_chunks_plan is host arithmetic only (1 = the batch is taken, 0 = it would be refused).  Chunk i has
 * coder_bytes_i = aec_gpu_sz_layout(sz, chunk_bytes[i]).coder_bytes and a room of its own in d_work at work_offsets[i],
 * the running sum of up16(coder_bytes_j), j < i (work_offsets is optional).  Refused, and AEC_CONF_ERROR from the two
 * calls with nothing enqueued: an SZ_com_t aec_gpu_sz_layout rejects; a chunk without a whole pixel; a batch
 * aec_gpu_encode_chunks_plan refuses; totals a launch cannot count -- a chunk of 2^35 bytes or more, or more than 2^25
 * wavefronts of 64 lanes, a lane per 16 bytes of max(coder_bytes_i, chunk_bytes_i) + 30 and every chunk rounded up to
 * whole wavefronts (no launch then counts beyond 2^31 lanes); a missing or misaligned d_work where one is needed.
 * n_chunks == 0: AEC_OK, nothing is enqueued.
 */
typedef struct aec_gpu_sz_chunks_plan_s {
    aec_gpu_params coder;     /* as aec_gpu_sz_layout gives it (the encoder's flags) */
    size_t   work_bytes;      /* d_work: the sum of up16(coder_bytes_i) */
    size_t   out_bound;       /* = aec_gpu_encode_chunks_plan(coder, coder_bytes[]).out_bound: an out_cap that never overflows */
    uint64_t rsi_entries;     /* the sum of lines_i + 1 (= that plan's rsi_entries): entries of d_rsi_bit_offsets */
    size_t   workspace_bytes; /* device memory the context holds for such a batch: the coder's and this layer's
                                 descriptors and wavefront table (aec_gpu_held_bytes counts it, aec_gpu_trim releases it) */
    unsigned direct;          /* 1: every chunk's layout says passthrough */
} aec_gpu_sz_chunks_plan_t;
AEC_GPU_API int aec_gpu_sz_chunks_plan(const SZ_com_t *sz, const uint64_t *chunk_bytes, uint64_t n_chunks,
                                       aec_gpu_sz_chunks_plan_t *plan, uint64_t *work_offsets);

/*
 * SZ_BufftoBuffCompress of n_chunks chunks in one enqueue.  Chunk i is chunk_bytes[i] bytes at d_src + src_offsets[i]:
 * any byte offset, any order; chunks do not overlap and nothing between them is read.  Stream i is byte for byte what
 * SZ_BufftoBuffCompress returns for chunk i; the streams lie back to back in d_out in chunk order.  d_out, out_cap
 * (overflow; nothing is written at or beyond out_cap), d_chunks and d_result: exactly as aec_gpu_encode_chunks_async
 * defines them.  d_rsi_bit_offsets (optional, plan.rsi_entries entries) receives that call's table.
 * d_work (plan.work_bytes bytes, 16-byte aligned): after the call d_work + work_offsets[i] holds chunk i's coder input,
 * coder_bytes_i bytes; the up to 15 bytes between that and the next room are not written, nor is anything outside
 * [d_work, d_work + work_bytes).  When plan.direct holds and every d_src + src_offsets[i] is 16-byte aligned the chunks
 * are coded where they lie and d_work may be NULL.
 * Per chunk: planes are split in registers when the chunk's own layout allows it (see above) and the chunk lies at a
 * 16-byte aligned address; every other chunk of the batch moves by 16-byte groups and bytes.  One odd chunk does not
 * slow the others.  The call synchronises the device only where a buffer of the context grows.
 */
AEC_GPU_API int aec_gpu_sz_compress_chunks_async(aec_gpu_ctx *ctx, const SZ_com_t *sz, const void *d_src,
                                                 const uint64_t *src_offsets, const uint64_t *chunk_bytes,
                                                 uint64_t n_chunks, void *d_work, void *d_out, size_t out_cap,
                                                 aec_gpu_batch_chunk *d_chunks, uint64_t *d_rsi_bit_offsets,
                                                 aec_gpu_enc_result *d_result, void *stream);

/*
 * SZ_BufftoBuffDecompress of n_chunks streams in one enqueue.  d_in, in_bytes, have_table, in_offsets, in_bytes_each,
 * d_rsi_bit_offsets, d_results and d_result are exactly those of aec_gpu_decode_chunks_async with out_bytes[i] =
 * coder_bytes_i and out_offsets[i] = work_offsets[i]: with have_table != 0 the table is the one the compress call wrote,
 * no index pass runs and in_offsets / in_bytes_each may be NULL.  Exactly chunk_bytes[i] bytes are written at
 * d_dst + dst_offsets[i] (any byte offset) and nothing outside them; a trailing fraction of a pixel comes back zero.
 * The bytes of a chunk whose record is not clean are unspecified, every other chunk is exact.  The decode goes to d_work
 * (plan.work_bytes bytes, 16-byte aligned), or straight to d_dst when plan.direct holds and every d_dst + dst_offsets[i]
 * is 16-byte aligned (d_work may then be NULL).
 */
AEC_GPU_API int aec_gpu_sz_decompress_chunks_async(aec_gpu_ctx *ctx, const SZ_com_t *sz, const void *d_in,
                                                   size_t in_bytes, const uint64_t *in_offsets,
                                                   const uint64_t *in_bytes_each, const uint64_t *dst_offsets,
                                                   const uint64_t *chunk_bytes, uint64_t n_chunks,
                                                   uint64_t *d_rsi_bit_offsets, int have_table, void *d_work, void *d_dst,
                                                   aec_gpu_dec_result *d_results, aec_gpu_dec_result *d_result,
                                                   void *stream);

/*
 * Which pixels_per_block?  The length of SZ_BufftoBuffCompress's stream of every chunk of a batch under pixels per block
 * 8, 16, 32 and 64, from ONE read of the chunks: nothing is marshalled to memory, no stream is written and no d_work is
 * needed.  (aec_gpu_estimate_async answers for ONE coder input; SZIP pads every scan line to whole blocks of the candidate
 * size, so the coder's input differs per candidate.)
 *
 * sz gives options_mask and bits_per_pixel; sz->pixels_per_block is ignored.  Candidate i is {options_mask,
 * bits_per_pixel, 8 << i, pixels_per_scanline[i]}; pixels_per_scanline[i] == 0 leaves size i out, pixels_per_scanline ==
 * NULL takes sz->pixels_per_scanline for all four.  (HDF5 derives the scan line from pixels_per_block when a chunk's row
 * is shorter than a block or longer than 128 blocks, hence a scan line per candidate.)  Sizes that share a scan line are
 * evaluated in one pass over the chunks; each further distinct scan line costs one more pass, one behind the other on the
 * stream: plan.passes.
 *
 * src_offsets and chunk_bytes are HOST arrays with the contract of aec_gpu_sz_compress_chunks_async (any byte offset,
 * any order, no overlap, nothing between the chunks is read, free again on return).  d_chunk_bits (optional, n_chunks * 4
 * entries): entry [c * 4 + i] is exactly the `bits` that aec_gpu_sz_compress_chunks_async writes into d_chunks[c] for
 * candidate i, ~0 for a size not asked.  d_estimate->total_bytes[i] is the sum over c of max(1, ceil(bits / 8)), the
 * length of SZ_BufftoBuffCompress's stream of chunk c.
 *
 * AEC_CONF_ERROR with nothing enqueued (the plan returns 0): no size asked; an asked candidate that aec_gpu_sz_layout
 * rejects for any chunk (more than 4096 blocks per line, a chunk without a whole pixel, ...); totals a launch cannot
 * count, by the bounds of aec_gpu_sz_chunks_plan applied to every asked candidate.  n_chunks == 0: AEC_OK, the record
 * holds 0 for every size asked and best is the lowest index asked.
 *
 * The call only enqueues and synchronises only where a buffer of the context grows.  Its workspace -- the 16-bit block
 * records of the sizes of one pass, the per-chunk sums, the chunk descriptors and wavefront tables -- is the context's:
 * aec_gpu_held_bytes counts it, aec_gpu_trim releases it, plan.workspace_bytes is what the context holds after such a
 * call at most.  It shares that buffer with the SZIP chunk calls above, and as any estimate or encode it may not run
 * between a PLAN and its EMIT on the same context.
 */
#define AEC_GPU_SZ_ESTIMATE_SIZES 4           /* pixels_per_block 8, 16, 32, 64 in this order */
typedef struct aec_gpu_sz_estimate_s {
    uint64_t total_bytes[AEC_GPU_SZ_ESTIMATE_SIZES]; /* sum over the chunks of the length of SZ_BufftoBuffCompress's stream; ~0: not asked */
    uint32_t best;                                   /* index of the smallest total_bytes among those asked; ties: the lowest */
    uint32_t pad;                                    /* 0 */
} aec_gpu_sz_estimate_t;
struct aec_gpu_sz_estimate_plan {
    uint32_t evaluated;       /* bit i set: size i is evaluated */
    uint32_t passes;          /* distinct scan lines among the sizes asked */
    uint64_t pieces;          /* pieces of 64 coder samples over all passes: the lanes that code */
    size_t   workspace_bytes; /* device memory the context holds for such a call */
};
AEC_GPU_API int aec_gpu_sz_estimate_plan(const SZ_com_t *sz, const unsigned int pixels_per_scanline[AEC_GPU_SZ_ESTIMATE_SIZES],
                                         const uint64_t *chunk_bytes, uint64_t n_chunks,
                                         struct aec_gpu_sz_estimate_plan *plan);
AEC_GPU_API int aec_gpu_sz_estimate_async(aec_gpu_ctx *ctx, const SZ_com_t *sz,
                                          const unsigned int pixels_per_scanline[AEC_GPU_SZ_ESTIMATE_SIZES], const void *d_src,
                                          const uint64_t *src_offsets, const uint64_t *chunk_bytes, uint64_t n_chunks,
                                          uint64_t *d_chunk_bits, aec_gpu_sz_estimate_t *d_estimate, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AEC_GPU_SZ_H */
