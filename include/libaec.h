/*
 * libaec.h -- C ABI of the MI355X-native adaptive entropy coder.
 *
 * Binary compatible with erget/libaec 0.3.4: the stream structure (reference
 * src/libaec.h:67-97), the flag, return-code and flush constants (:105-149) and the eight
 * entry points (:154-166) have the same names, layout, argument meaning and error behaviour,
 * so a program built against the reference header runs against this library unchanged
 * (shared object name libaec.so.0).  The work behind the entry points is done by HIP kernels
 * on the current HIP device; see DESIGN.md and INTEGRATION.md.
 */
#ifndef LIBAEC_H
#define LIBAEC_H 1

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

struct internal_state;

/* reference src/libaec.h:67-97 -- field order and types are the ABI */
struct aec_stream {
    const unsigned char *next_in;   /* next input byte */
    size_t avail_in;                /* bytes available at next_in */
    size_t total_in;                /* bytes consumed so far */
    unsigned char *next_out;        /* where the next output byte goes */
    size_t avail_out;               /* free bytes at next_out */
    size_t total_out;               /* bytes produced so far */
    unsigned int bits_per_sample;   /* 1..32 */
    unsigned int block_size;        /* samples per block: 8, 16, 32, 64 (any even value <= 64
                                       with AEC_NOT_ENFORCE).  LIMIT of this library: the reference accepts
                                       any even size with AEC_NOT_ENFORCE (src/encode.c:780-783) although
                                       sizes above 64 overrun its own coded-data-set buffer (encode.h:64-66);
                                       here they are AEC_CONF_ERROR -- one lane owns one block */
    unsigned int rsi;               /* blocks per reference sample interval, 1..4096 */
    unsigned int flags;             /* AEC_DATA_* | AEC_RESTRICTED | AEC_PAD_RSI | AEC_NOT_ENFORCE */
    struct internal_state *state;   /* owned by the library between *_init and *_end */
};

/* sample description flags, reference src/libaec.h:105-124 */
#define AEC_DATA_SIGNED 1      /* samples are two's complement */
#define AEC_DATA_3BYTE 2       /* 17..24 bit samples are stored in 3 bytes instead of 4 */
#define AEC_DATA_MSB 4         /* most significant byte first (default: least significant first) */
#define AEC_DATA_PREPROCESS 8  /* run the unit-delay predictor / sign mapper */
#define AEC_RESTRICTED 16      /* restricted code-option set (bits_per_sample <= 4 only) */
#define AEC_PAD_RSI 32         /* decoder: every RSI starts on a byte boundary */
#define AEC_NOT_ENFORCE 64     /* allow non-standard (even) block sizes */

/* return codes, reference src/libaec.h:129-133 */
#define AEC_OK 0
#define AEC_CONF_ERROR (-1)
#define AEC_STREAM_ERROR (-2)
#define AEC_DATA_ERROR (-3)
#define AEC_MEM_ERROR (-4)
#define AEC_RSI_OFFSETS_ERROR (-5)   /* libaec 1.1: offsets not enabled, or enabled too late */

/* flush modes, reference src/libaec.h:141-149 */
#define AEC_NO_FLUSH 0   /* more input may follow */
#define AEC_FLUSH 1      /* this is the last input: drain everything and pad the final byte */

#define LIBAEC_API __attribute__((visibility("default")))

/* streaming interface, reference src/libaec.h:154-160 (encode.c:773-948, decode.c:694-841)
 *
 * WHAT the calls deliver is the reference's, byte for byte; WHEN may differ, because work goes to the device
 * in batches:
 *   aec_encode(AEC_NO_FLUSH) codes the whole RSIs it holds once 1 MiB is staged, or on a call that brings no new
 *     input, or on AEC_FLUSH -- until then avail_out may stay untouched although input was taken.
 *   aec_decode runs a batch on every call EXCEPT for a caller that feeds at most 8 new bytes per call with
 *     AEC_NO_FLUSH while fewer than 4 KiB wait: those bytes are decoded by the next call that brings nothing new
 *     (avail_in == 0) or passes AEC_FLUSH.  A caller that stops as soon as its input is used up must make that
 *     last call (the reference's own callers do: src/aec.c:191-221, tests/check_aec.c:138-166), or pass
 *     AEC_FLUSH (which the reference ignores for decoding, decode.c:797) with its last piece of input.
 * The library has no CPU codec: without a HIP device every call returns AEC_MEM_ERROR. */
LIBAEC_API int aec_encode_init(struct aec_stream *strm);
LIBAEC_API int aec_encode(struct aec_stream *strm, int flush);
LIBAEC_API int aec_encode_end(struct aec_stream *strm);
LIBAEC_API int aec_decode_init(struct aec_stream *strm);
LIBAEC_API int aec_decode(struct aec_stream *strm, int flush);
LIBAEC_API int aec_decode_end(struct aec_stream *strm);

/* one-shot helpers, reference src/libaec.h:165-166 (encode.c:950-963, decode.c:843-854) */
LIBAEC_API int aec_buffer_encode(struct aec_stream *strm);
LIBAEC_API int aec_buffer_decode(struct aec_stream *strm);

/*
 * Extension (no reference counterpart): n independent streams with the same parameters in ONE call --
 * the chunks of an HDF5 / netCDF dataset, where the reference's callers run one aec_buffer_* call per
 * chunk (reference src/sz_compat.c:170, 239).  Only bits_per_sample, block_size, rsi and flags of
 * `params` are read.  src[i] / src_len[i]: the i-th input; dst[i]: its output buffer, dst_len[i] its
 * capacity on entry and the bytes produced on return; status[i] (optional): AEC_OK, AEC_DATA_ERROR
 * (corrupt stream), AEC_STREAM_ERROR (encode: output did not fit, a prefix was written).  The chunks travel
 * through pinned staging (one transfer per piece of 64 MiB); decode: the RSI starts of a whole group of chunks
 * from ONE table launch (low-entropy chunks of tens of KiB and more) or one wavefront per chunk (small chunks),
 * then one decode launch per group; encode: equal chunks of whole RSIs -- the usual HDF5 case -- are analysed,
 * scanned and packed by ONE launch set for all of them (aec_gpu_encode_uniform_batch_async), other shapes by the
 * encoder kernels chunk after chunk.  Batches of more than a few MiB run as up to four parts side by side, each on
 * a HIP stream of its own.  Returns AEC_OK or the last non-OK status.
 */
LIBAEC_API int aec_buffer_encode_batch(const struct aec_stream *params, size_t n, const void *const *src,
                                       const size_t *src_len, void *const *dst, size_t *dst_len, int *status);
LIBAEC_API int aec_buffer_decode_batch(const struct aec_stream *params, size_t n, const void *const *src,
                                       const size_t *src_len, void *const *dst, size_t *dst_len, int *status);

/*
 * RSI offsets and random access: the entry points libaec 1.1 added (same names, arguments and return codes; SONAME
 * still libaec.so.0).  An RSI (reference sample interval) is rsi blocks; an offset is a BIT position in the stream.
 * Nothing here costs anything unless a caller enables offsets or calls aec_decode_range.
 *
 * Bit 0: for the encoder the first bit it wrote after aec_encode_init; for the decoder the first bit of the byte at
 * next_in after aec_decode_init -- after aec_buffer_seek that is the byte the seek moved next_in to (so its table
 * starts at offset % 8, like the stream's total_in, which the seek leaves alone).
 *
 * aec_encode_enable_offsets: after aec_encode_init, before the first aec_encode that takes input (later:
 *   AEC_RSI_OFFSETS_ERROR).  Entry i is the start bit of RSI i's first coded data set.  The count is the number of
 *   RSIs whose first block has been coded so far -- the library stages up to 1 MiB of input before it codes, so it can
 *   lag the input; after AEC_FLUSH it is ceil(blocks / rsi).  AEC_PAD_RSI is ignored by the encoder, as by the
 *   reference (nothing is padded).
 * aec_decode_enable_offsets: after aec_decode_init (and aec_buffer_seek), before the first aec_decode.  Entry i is the
 *   start bit of the i-th RSI whose first coded data set has been decoded (with AEC_PAD_RSI: its byte-aligned start).
 *   For a complete stream the table equals the encoder's however the input was cut into calls.
 * *_count_offsets / *_get_offsets: AEC_RSI_OFFSETS_ERROR on a state without offsets enabled (count also sets
 *   *rsi_offsets_count = 0); get with a buffer of fewer than count entries: AEC_MEM_ERROR, nothing written.  The
 *   tables stay readable until *_end.
 * aec_buffer_seek: on a decoder state on which aec_decode has not run (else AEC_STREAM_ERROR).  Moves next_in forward
 *   by offset / 8 and takes as much off avail_in; the next aec_decode starts at bit offset % 8 of that byte, as at an RSI
 *   start.  total_in is unchanged.  AEC_MEM_ERROR, nothing changed, when the bit lies beyond the input.
 * aec_decode_range(strm, offs, n, pos, size): strm from aec_decode_init, next_in / avail_in the stream from bit 0,
 *   offs[0 .. n) its RSI start bits (the encoder's or the decoder's table).  Writes bytes [pos, pos + size) of what
 *   aec_buffer_decode of the whole stream produces (byte counts: need not be sample-aligned) to next_out and advances
 *   next_out / avail_out / total_out by size; next_in / avail_in / total_in stay as they are.  Any number of calls may
 *   follow on one state, then aec_decode_end.  Only the RSIs the window touches are decoded -- the last of them up to
 *   the block that holds byte pos + size - 1 -- and no index pass runs.  With R = rsi * block_size * bytes per sample:
 *     size == 0                                                   AEC_OK, nothing written
 *     pos / R >= n                                                AEC_DATA_ERROR, nothing written
 *     avail_out < size                                            AEC_MEM_ERROR, nothing written
 *     offs[pos / R .. min((pos + size - 1) / R + 1, n - 1)] not strictly increasing or not below 8 * avail_in
 *                                                                 AEC_DATA_ERROR, nothing written (host-side check)
 *     the window needs an RSI beyond the table                    AEC_DATA_ERROR, nothing written
 *     aec_decode has run on this state                            AEC_STREAM_ERROR, nothing written
 *     the stream ends before byte pos + size, or an RSI the window decodes whole does not end exactly at the next
 *     entry (rounded up to a byte with AEC_PAD_RSI), where there is one: the table is not this stream's
 *                                                                 AEC_DATA_ERROR; [next_out, next_out + size)
 *                                                                 unspecified, next_out not advanced
 *   Whatever the table says, no byte outside [next_out, next_out + size) is written and nothing beyond
 *   next_in + avail_in is read.  A table that is wrong in a way the decoder cannot see (an entry that still lands on a
 *   coded data set of the right kind, inside an RSI the window only decodes in part) gives wrong bytes, not an error.
 */
LIBAEC_API int aec_encode_enable_offsets(struct aec_stream *strm);
LIBAEC_API int aec_encode_count_offsets(struct aec_stream *strm, size_t *rsi_offsets_count);
LIBAEC_API int aec_encode_get_offsets(struct aec_stream *strm, size_t *rsi_offsets, size_t rsi_offsets_count);
LIBAEC_API int aec_buffer_seek(struct aec_stream *strm, size_t offset);
LIBAEC_API int aec_decode_enable_offsets(struct aec_stream *strm);
LIBAEC_API int aec_decode_count_offsets(struct aec_stream *strm, size_t *rsi_offsets_count);
LIBAEC_API int aec_decode_get_offsets(struct aec_stream *strm, size_t *rsi_offsets, size_t rsi_offsets_count);
LIBAEC_API int aec_decode_range(struct aec_stream *strm, const size_t *rsi_offsets, size_t rsi_offsets_count,
                                size_t pos, size_t size);

#ifdef __cplusplus
}
#endif
#endif /* LIBAEC_H */
