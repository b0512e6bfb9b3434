/*
 * aec_gpu_grib.h -- GRIB2 CCSDS packing (data representation template 5.42 / 7.42, ecCodes' grid_ccsds) and simple packing
 * (template 5.0 / 7.0, grid_simple) that stay on the device: float fields to section-7 streams and back, and one kind of
 * stream to the other; and complex packing (templates 5.2 / 5.3), read into floats or into either kind of stream and written
 * from floats or from either kind of stream.
 *
 * Between a field of floats and the coder (aec_gpu.h) sits GRIB2's simple packing, WMO regulation 92.9.4:
 *       Y * 10^D = R + X * 2^E
 * R an IEEE float32, E and D small integers, X an unsigned integer of nbits bits.  A writer finds the field's minimum
 * and maximum, chooses R and E, quantises every value to X and codes the X; a reader decodes the X and reverses the
 * formula.  These entry points are that layer for a caller whose fields live in HBM (a model that writes packed
 * messages, a training pipeline that reads them), as aec_gpu_sz.h is the layer for SZIP chunks.  All pointers marked
 * d_ are HIP device pointers; every call only ENQUEUES work on `stream` (a hipStream_t passed as void*), allocates
 * nothing the context does not keep and reads nothing back.  Exported by libaec.so.0.
 *
 * THE CONTRACT
 * A batch is n_fields fields of ONE element type (elem: AEC_GPU_GRIB_F32 or AEC_GPU_GRIB_F64) under ONE template
 * (nbits 1..32, the compression-options octet, block size, reference sample interval); R, E and D are per field.
 * Field i is n_values[i] >= 1 values at d_src + src_offsets[i]: n_values and src_offsets are HOST arrays (free again
 * when the call returns), the offsets are multiples of the element size (so is d_src) and otherwise arbitrary, the
 * fields lie in any order, do not overlap, and nothing between them is read.
 *
 * All quantisation arithmetic is IEEE double, one correctly rounded operation at a time, never contracted into a fused
 * multiply-add (which rounds once where this contract rounds twice):
 *   p    = 10^|D|, exact in a double for |D| <= 22 (from a table)
 *   s(y) = y * p for D > 0, y / p for D < 0, y for D = 0
 * Pack
 *   1. lo = s(minimum of the field), hi = s(maximum); -0.0 counts as +0.0
 *   2. R  = the largest float32 <= lo
 *   3. range = hi - (double)R;  M = 2^nbits - 1
 *   4. E  = the smallest integer with range * 2^-E <= M, held to [-127, 127]
 *   5. X  = trunc((s(y) - R) * 2^-E + 0.5)      (the scaling by a power of two is exact; ties go UP, this is not rint)
 *   Every step is monotone and M is exact, so 0 <= X <= M without clamping -- except where E had to be held at 127 (a
 *   range beyond 2^127 * M: nbits 1 or 2 and extremes near +-FLT_MAX): an X that would exceed M is then held to M, and a
 *   field in which one was gets status bit 2.  (Holding E does not by itself flag a field: up to a range of
 *   2^127 * (M + 0.5) every X still rounds to at most M, and nothing is held.)
 *   A constant field (lo == hi) gets E = 0 and X = 0 throughout: a GRIB writer sets nbits 0 for it and drops section 7.
 *   With have_params the caller supplies R and E per field (re-packing with a source message's parameters, |E| <= 1022);
 *   X then follows the formula for every field, is held to [0, M], and a field that needed that gets status bit 2.
 * Unpack
 *   v = X * 2^E + (double)R (the product is exact, the sum rounded once), Y = v / p (D > 0), v * p (D < 0) or v, then
 *   one rounding to the element type.
 * This is the WMO definition.  It is NOT claimed to be bit-identical to ecCodes' floats: ecCodes builds its powers of
 * ten by repeated multiplication.  The STREAMS are bit-identical to what any libaec gives for the same X.
 *
 * X lie little-endian in containers of 1 byte (nbits <= 8), 2 bytes (<= 16) or 4 bytes (<= 32), never 3.
 *
 * SECTION 6 BITMAPS (the *_bitmap_* calls at the end of this header)
 * A field of N = n_points[i] grid points has a bitmap of N bits in ceil(N / 8) bytes at d_bitmap + bitmap_offsets[i] (any
 * byte; neighbouring bitmaps may touch): point k is bit 7 - k % 8 of byte k / 8, most significant bit first, 1 = present,
 * what numpy.packbits writes.  Section 7 holds the X of the present points only, in grid order; n_values[i] -- section 5
 * octets 6-9 -- is the number of present points and stays a HOST number: the rooms, the coder's tables and out_bound are
 * host arithmetic over it.  A reader takes it from the message; a writer, whose mask is static, gets it once from
 * aec_gpu_grib_bitmap_async.  The device still counts every bitmap: a field whose bitmap does not hold n_values[i] ones
 * gets status bit 3 (AEC_GPU_GRIB_MISMATCH); its X, stream and values are unspecified, but no access leaves its room, its
 * bitmap or its n_points elements whatever the bitmap holds, and every other field of the batch is exact.  Bits of the last
 * byte behind point N - 1 are ignored when read and written as 0.
 *
 * SIMPLE PACKING (template 5.0 / 7.0, ecCodes' grid_simple; the *_simple_* and *_bits_* calls at the end of this header)
 * The same R, E, D and X under the same aec_gpu_grib_template, with X stored as a plain string of nbits-bit integers instead
 * of going through the coder: value j of a field of n = n_values[i] values is the bits [j * nbits, (j + 1) * nbits) of its
 * stream, bit b of a stream is bit 7 - b % 8 of byte b / 8, most significant bit first, and the unused low bits of the last
 * of its S = ceil(n * nbits / 8) bytes are 0 -- the big-endian integer sum X_j * 2^(nbits * (n - 1 - j)) shifted left to a
 * whole byte.  Streams lie at d_simple + simple_offsets[i] (HOST array): at any byte, neighbours may touch, in any order.
 * Rooms, work_offsets and containers are those of aec_gpu_grib_plan (block_size and rsi still size the rooms), so the
 * calls compose with everything above through d_work: floats to 5.0 streams and back, 5.0 streams to 5.42 streams and back
 * without a float being touched (R, E, D and nbits pass from one section 5 to the other unchanged: lossless by
 * construction), and, through aec_gpu_grib_quantise_bitmap_async / aec_gpu_grib_dequantise_bitmap_async, fields with
 * bitmaps -- these need no entry point of their own.
 *
 * COMPLEX PACKING (templates 5.2 / 7.2 and, with spatial differencing, 5.3 / 7.3 -- what NCEP writes GFS, NAM, HRRR and RAP
 * in; the *_complex_* calls at the end of this header).  READING: streams to X rooms, and from there to floats, to 5.42
 * streams or (through aec_gpu_grib_bits_pack_async) to 5.0 streams.  WRITING (THE WRITER'S RULE below): X rooms to streams with
 * groups of a fixed length, from floats, from 5.42 streams or from 5.0 streams.  R, E and D pass from one section 5 to the
 * other unchanged and only the integers X move from one container to the other, so the conversions are lossless.
 * Bits are counted as in simple packing (bit b of a stream is bit 7 - b % 8 of byte b / 8; an integer of w bits is
 * big-endian).  What section 5 says comes per field in a HOST aec_gpu_grib_complex_field.  Section 7 of field i is the
 * complex_bytes_each[i] bytes at d_complex + complex_offsets[i] (HOST arrays; any byte, neighbours may touch, any order):
 *   1. extra descriptors, for order >= 1 and extra_octets > 0: ival1, then ival2 if order = 2, then minsd, each extra_octets
 *      octets in sign-magnitude form (the first bit is the sign, the rest the magnitude; "minus zero" is 0).  With
 *      extra_octets = 0 all three are 0.
 *   2. group references: NG integers of ref_bits bits, then zero bits up to a whole byte (ref_bits 0: all 0, the part is empty)
 *   3. group widths: NG integers of width_bits bits, padded to a byte; width_g = width_ref + stored
 *   4. group lengths: NG integers of length_bits bits, padded to a byte; len_g = length_ref + stored * length_inc, except
 *      len_(NG-1) = last_length (the stored value of the last group is ignored)
 *   5. packed values: group after group without padding, len_g integers of width_g bits each (none for width 0)
 * With n = n_values[i]:  s_j = ref_g + packed_j for value j of group g;  order 0: X_j = s_j;  order 1: X_0 = ival1,
 * X_j = X_(j-1) + s_j + minsd;  order 2: X_0 = ival1, X_1 = ival2, X_j = 2 X_(j-1) - X_(j-2) + s_j + minsd.  The first `order`
 * values of the packed string are parsed and ignored; with n = 1 and order 2, ival2 is read past and not used.  ALL
 * ARITHMETIC IS TWO'S COMPLEMENT MODULO 2^64: a second-order sum may pass through values far outside 32 bits and still land
 * exactly.
 * X goes into the plan's rooms under the TARGET template t: containers follow t->nbits, the last block is padded with the
 * last X -- byte for byte the room aec_gpu_grib_quantise_async leaves for the same X.  d_cx (n_fields aec_gpu_grib_cx on the
 * device) receives x_min and x_max, the signed reading of the modulo-2^64 X, and status bits:
 *   AEC_GPU_GRIB_CX_RANGE      some X lies outside [0, 2^nbits - 1].  The stored X are taken modulo 2^nbits (the coder never
 *                              sees a sample out of range); x_min and x_max are exact, so the caller can choose a wider
 *                              nbits and call again.
 *   AEC_GPU_GRIB_CX_MALFORMED  the group lengths do not sum to n, or a width exceeds 32, or the packed values end behind
 *                              complex_bytes_each[i].  The field's X, x_min, x_max and RANGE bit are then unspecified, its
 *                              whole room is still written, and every other field is exact.
 * No load leaves [d_complex + complex_offsets[i], + complex_bytes_each[i]), no store leaves the field's room, d_cx or the
 * context's workspace, whatever the bytes contain.  The device's running sums do not wrap -- THE RULE: a group length above n
 * counts as n + 1, a width above 32 counts as all the bits the stream has left and one more, and the running sums of lengths
 * and of bits are held at n + 1 and at 8 * (bytes behind the tables) + 1; a sum that reached its cap is MALFORMED.  An
 * integer that would cross the stream's end reads as 0.
 * The host answers AEC_CONF_ERROR with nothing enqueued for: whatever aec_gpu_grib_plan refuses for t and n_values;
 * missing != 0; order > 2; extra_octets > 8 (order >= 1); a bit count above 32; n_groups == 0 or n_groups > n_values[i];
 * complex_bytes_each[i] smaller than the extra descriptors plus the three tables, or 2^35 and more; a stream that leaves
 * [0, complex_bytes); more than 2^31 - 1 groups or 2^25 tiles of 64 groups in a batch.
 * THE WRITER'S RULE.  Writing shares the stream definition above (items 1 - 5) and fixes every bit of the output.  A batch is
 * written under one aec_gpu_grib_complex_write: the order o (0: template 5.2; 1 or 2: template 5.3) and the group length G (16,
 * 32, 64, 128 or 256).  The input is X_0 .. X_(n-1), the field's room taken modulo 2^nbits as aec_gpu_grib_bits_pack_async takes
 * it; the samples that pad the last block are never used.
 *   differences  d_j for j >= o is X_j (o = 0), X_j - X_(j-1) (o = 1) or X_j - 2 X_(j-1) + X_(j-2) (o = 2), exact signed integers.
 *                minsd is the smallest d_j, j >= o, for o >= 1; 0 for o = 0 and where there is no such j (n <= o).
 *                s_j = d_j - minsd, so 0 <= s_j < 2^(nbits + o).
 *   groups       NG = ceil(n / G); group g holds the values [g G, min(n, (g + 1) G)), its COUNTED values are those with j >= o.
 *                ref_g is the smallest s_j of the counted values, width_g the bit length of (largest s_j - ref_g); both are 0
 *                for a group without a counted value.  packed_j = s_j - ref_g for counted values and 0 for the first o values,
 *                which a reader parses and ignores.
 *   section 5    ref_bits is the bit length of the largest ref_g, width_ref the smallest width_g, width_bits the bit length of
 *                (largest width_g - width_ref); length_ref = G, length_inc = 1, length_bits = 0 (the lengths table is empty),
 *                last_length = n - (NG - 1) G; extra_octets = ceil((nbits + o) / 8) for o >= 1, else 0 -- a function of the
 *                template alone; missing = 0; ival1 = X_0, ival2 = X_1 (0 when n = 1); minsd in sign and magnitude, zero
 *                written as plus zero.
 * The host refuses nbits + o > 32: that keeps every s_j, reference and width within 32 bits, so the writer has no status bit.
 * The stream of field i is S_i bytes, a number only the device knows; B_i = head + ceil(NG (nbits + o) / 8) + ceil(6 NG / 8) +
 * ceil(n (nbits + o) / 8), head = (o + 1) * extra_octets for o >= 1 and else 0, is host arithmetic and S_i <= B_i always.
 * Streams go to d_complex + complex_offsets[i] (a HOST array: any byte, any order); the host checks that every range
 * [complex_offsets[i], + B_i) lies inside [0, complex_cap) and that no two of them overlap.  EXACTLY S_i BYTES ARE WRITTEN, EACH
 * ONCE: the bytes from S_i to B_i are not touched, nothing else is written except d_cxw and the context's workspace, and S_i
 * may be 0 (a field of zeros at order 0 has no head, no reference bits and no width bits).  d_cxw (n_fields aec_gpu_grib_cxw on
 * the device, 8-byte aligned) receives per field what goes into section 5 -- what the reading calls take back as their
 * aec_gpu_grib_complex_field -- and S_i.  No load leaves the n values of a field's room.
 * The host answers AEC_CONF_ERROR with nothing enqueued for: whatever aec_gpu_grib_plan refuses; order > 2; a group_length
 * outside the five values; nbits + order > 32; a d_work off its 16 bytes or a d_cxw off its 8; a range [off_i, off_i + B_i) that
 * leaves complex_cap or overlaps another; more than 2^31 - 1 groups in a batch or more than 2^25 wavefronts in a launch.
 * Out of scope: missing-value management 1 and 2 (it needs the present-point count back on the host; a follow-up that maps
 * onto the bitmap calls); NG = 0 (constant fields); adaptive or variable-length grouping and groups shorter than 16 (every
 * grouping is a valid stream: fixed groups cost about (ref_bits + width_bits) / G bits a value over the ideal); placing the
 * written streams back to back (it needs a scan across fields); the row-by-row packings 5.50 and up.  Fields with a section
 * 6 bitmap compose through d_work with aec_gpu_grib_dequantise_bitmap_async and aec_gpu_grib_quantise_bitmap_async, as for
 * simple packing.
 *
 * OUT OF SCOPE: fields without a present point (a writer sets nbits 0 and drops section 7), bitmap indicator 254 and
 * predefined bitmaps (the caller hands over whichever bitmap applies); adaptive grouping in written complex packing, complex
 * packing with missing-value management or without a group, the row-by-row (second-order) packings 5.50 and up and the JPEG and PNG
 * packings; parsing or writing GRIB messages themselves; a quantiser fused into the encoder or into the bit packer.
 */
#ifndef AEC_GPU_GRIB_H
#define AEC_GPU_GRIB_H 1

#include "aec_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AEC_GPU_GRIB_F32 4      /* elem: the element type by its size */
#define AEC_GPU_GRIB_F64 8

#define AEC_GPU_GRIB_BAD      1u  /* status bit 0: the field holds a non-finite value, or |lo| or |hi| exceeds FLT_MAX; its
                                     stream and X are unspecified, every other field of the batch is exact */
#define AEC_GPU_GRIB_CONSTANT 2u  /* status bit 1: lo == hi */
#define AEC_GPU_GRIB_CLAMPED  4u  /* status bit 2: an X of a field that is not bad was held to [0, M] -- under have_params,
                                     or where E was held at 127 */
#define AEC_GPU_GRIB_MISMATCH 8u  /* status bit 3 (the *_bitmap_* calls): the field's bitmap does not hold n_values[i] ones; its
                                     X, stream and values are unspecified, every other field of the batch is exact */

/* Template 5.42 as far as it is shared by a batch */
typedef struct aec_gpu_grib_template_s {
    unsigned int nbits;       /* octet 20: bits per packed value */
    unsigned int options;     /* octet 22, the CCSDS compression options mask (libaec.h's AEC_* flags) */
    unsigned int block_size;  /* octet 23 */
    unsigned int rsi;         /* octets 24-25: reference sample interval */
} aec_gpu_grib_template;

/* The per-field record, 16 bytes: what the caller writes into section 5 (R octets 12-15, E 16-17, D 18-19), on the
 * device after a pack (d_fields) and on the host where the caller supplies parameters (params). */
typedef struct aec_gpu_grib_field_s {
    float R;
    int32_t E;
    int32_t D;
    uint32_t status;          /* AEC_GPU_GRIB_* bits; ignored in params */
} aec_gpu_grib_field;

typedef struct aec_gpu_grib_layout_s {
    aec_gpu_params coder;     /* bits_per_sample = nbits; flags = the mask's AEC_DATA_PREPROCESS | AEC_RESTRICTED | AEC_PAD_RSI
                                 bits plus AEC_NOT_ENFORCE, which the encoder needs and the decoder ignores.  The mask's
                                 AEC_DATA_MSB and AEC_DATA_3BYTE bits are ignored: they say how samples lie in memory and
                                 never change a stream.  AEC_PAD_RSI is the coder's (libaec.h): the ENCODER ignores it, as
                                 the reference's does, so a pack under it writes unpadded streams -- which an unpack reads
                                 with the pack's table, but not bare: a decoder under it expects every RSI on a byte, as
                                 a producer that pads writes them */
    unsigned int container;   /* bytes of an X in memory: 1 / 2 / 4 */
} aec_gpu_grib_layout_t;

/* Host arithmetic only.  AEC_CONF_ERROR for AEC_DATA_SIGNED in the mask, nbits 0 (a constant field has no section 7:
 * there is nothing to code) or above 32, |D| > 22, and whatever aec_gpu_check_params refuses for the coder. */
AEC_GPU_API int aec_gpu_grib_layout(const aec_gpu_grib_template *t, int D, aec_gpu_grib_layout_t *layout);

/*
 * aec_gpu_grib_plan is host arithmetic only (1 = the batch is taken, 0 = it would be refused).  Field i has blocks_i =
 * ceil(n_values[i] / block_size) blocks and a room of its own in d_work at work_offsets[i], the running sum of
 * up16(blocks_j * block_size * container), j < i (work_offsets is optional).  Refused, and AEC_CONF_ERROR from the calls
 * below with nothing enqueued: a template aec_gpu_grib_layout rejects; an elem that is neither; a field without a value;
 * a batch aec_gpu_encode_chunks_plan or aec_gpu_decode_chunks_plan refuses; totals a launch cannot count -- more than
 * 2^31 - 1 fields, a field of 2^35 bytes or more (values or room), or more than 2^25 wavefronts of 64 lanes, a wavefront
 * per 4 KiB of a field's values and one per 1 KiB of its room, every field rounded up to whole wavefronts.
 */
typedef struct aec_gpu_grib_plan_s {
    aec_gpu_params coder;     /* as aec_gpu_grib_layout gives it (the encoder's flags) */
    size_t   work_bytes;      /* d_work: the sum of up16(blocks_i * block_size * container) */
    size_t   out_bound;       /* = aec_gpu_encode_chunks_plan(coder, rooms).out_bound: an out_cap that never overflows */
    uint64_t rsi_entries;     /* = that plan's rsi_entries: entries of d_rsi_bit_offsets */
    size_t   workspace_bytes; /* device memory the context holds for such a batch: the coder's (encode or decode, the
                                 larger) and this layer's descriptors, wavefront table and extremes (aec_gpu_held_bytes
                                 counts it, aec_gpu_trim releases it; it is the buffer of the SZIP chunk calls) */
} aec_gpu_grib_plan_t;
AEC_GPU_API int aec_gpu_grib_plan(const aec_gpu_grib_template *t, int elem, const uint64_t *n_values, uint64_t n_fields,
                                  aec_gpu_grib_plan_t *plan, uint64_t *work_offsets);

/*
 * Pack n_fields fields in one enqueue: minimum and maximum, the parameters, the quantisation into d_work, then
 * aec_gpu_encode_chunks_async over the rooms.  D (host array, n_fields entries) gives every field's decimal scale
 * factor; with have_params != 0, params (host array, n_fields entries) gives R and E and its D is ignored.
 * d_work (plan.work_bytes bytes, 16-byte aligned): after the call d_work + work_offsets[i] holds field i's X, the last
 * block padded with the last X (nothing behind the field is read); the up to 15 bytes between that and the next room
 * are not written, nor is anything outside [d_work, d_work + work_bytes).
 * d_out, out_cap (overflow; nothing is written at or beyond out_cap), d_chunks, d_rsi_bit_offsets (optional) and
 * d_result: exactly as aec_gpu_encode_chunks_async defines them.  Section 7 of field i is the ceil(bits / 8) bytes at
 * base_bits / 8 of d_out: byte for byte aec_buffer_encode of its X.
 * d_fields (n_fields records): R, E, D and status of every field.
 * Nothing returns to the host; the device is synchronised only where a buffer of the context grows.
 * n_fields == 0: AEC_OK, nothing is enqueued.
 */
AEC_GPU_API int aec_gpu_grib_pack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src,
                                        const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D,
                                        int have_params, const aec_gpu_grib_field *params, uint64_t n_fields, void *d_work,
                                        void *d_out, size_t out_cap, aec_gpu_batch_chunk *d_chunks,
                                        uint64_t *d_rsi_bit_offsets, aec_gpu_grib_field *d_fields,
                                        aec_gpu_enc_result *d_result, void *stream);

/*
 * Unpack n_fields streams in one enqueue: aec_gpu_decode_chunks_async into d_work (out_offsets = work_offsets,
 * out_bytes = the rooms), then the reverse formula with params[i] (host array: R, E, D as section 5 gives them).
 * d_in, in_bytes, in_offsets, in_bytes_each, d_rsi_bit_offsets, have_table, d_results and d_result are exactly those of
 * aec_gpu_decode_chunks_async: with have_table != 0 the table is the one the pack call wrote and no index pass runs;
 * with have_table == 0 the index pass runs first, for messages of a foreign producer, whose streams may lie at any byte.
 * Exactly n_values[i] elements are written at d_dst + dst_offsets[i] (multiples of the element size, as d_dst) and
 * nothing outside them.  The values of a field whose record in d_results is not clean are unspecified, every other
 * field is exact.
 */
AEC_GPU_API int aec_gpu_grib_unpack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_in,
                                          size_t in_bytes, const uint64_t *in_offsets, const uint64_t *in_bytes_each,
                                          const uint64_t *n_values, const aec_gpu_grib_field *params,
                                          const uint64_t *dst_offsets, uint64_t n_fields, uint64_t *d_rsi_bit_offsets,
                                          int have_table, void *d_work, void *d_dst, aec_gpu_dec_result *d_results,
                                          aec_gpu_dec_result *d_result, void *stream);

/* The two halves alone, for callers that drive the coder themselves: pack without the encoder (d_work and d_fields as
 * above), and unpack without the decoder (d_work holds the X in the plan's rooms). */
AEC_GPU_API int aec_gpu_grib_quantise_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src,
                                            const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D,
                                            int have_params, const aec_gpu_grib_field *params, uint64_t n_fields,
                                            void *d_work, aec_gpu_grib_field *d_fields, void *stream);
AEC_GPU_API int aec_gpu_grib_dequantise_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_work,
                                              const uint64_t *n_values, const aec_gpu_grib_field *params,
                                              const uint64_t *dst_offsets, uint64_t n_fields, void *d_dst, void *stream);

/*
 * ---- section 6 bitmaps ----------------------------------------------------------------------------------------------------
 * aec_gpu_grib_bitmap_plan is host arithmetic only (1 = taken, 0 = refused).  plan is what aec_gpu_grib_plan gives for
 * n_values (rooms, work_offsets, out_bound and rsi_entries are identical), its workspace_bytes grown by this layer's
 * bitmap descriptors, per-tile counts and bases and the tile table.  tile_points (AEC_GPU_GRIB_TILE_POINTS) is the grid
 * points one wavefront of the bitmap kernels owns, tiles the sum of ceil(n_points[i] / tile_points).  Refused, and
 * AEC_CONF_ERROR from the calls below with nothing enqueued: whatever aec_gpu_grib_plan refuses (n_values[i] == 0 among it:
 * a field without a present point has no section 7); n_values[i] > n_points[i]; a field of 2^35 bytes or more; more than
 * 2^25 wavefronts (tiles) in a launch.
 */
#define AEC_GPU_GRIB_TILE_POINTS 1024u
typedef struct aec_gpu_grib_bitmap_plan_s {
    aec_gpu_grib_plan_t plan;
    uint64_t tile_points;
    uint64_t tiles;
} aec_gpu_grib_bitmap_plan_t;
AEC_GPU_API int aec_gpu_grib_bitmap_plan(const aec_gpu_grib_template *t, int elem, const uint64_t *n_points,
                                         const uint64_t *n_values, uint64_t n_fields, aec_gpu_grib_bitmap_plan_t *plan,
                                         uint64_t *work_offsets);

/*
 * Section 6 from values: point k of field i (n_points[i] >= 1 elements at d_src + src_offsets[i]) is MISSING iff its value
 * == (T)missing -- IEEE equality, so either zero matches a zero missing -- and, if missing is a NaN, iff it is a NaN.
 * Exactly ceil(n_points[i] / 8) bytes are written at d_bitmap + bitmap_offsets[i] (HOST array, any byte), the unused low
 * bits of the last byte 0, and nothing else.  d_counts[i] (n_fields uint64_t on the device) receives the number of ones:
 * the n_values[i] of the calls below.  Refused: an elem that is neither, a field without a point or of 2^35 bytes or more,
 * more than 2^25 tiles.
 */
AEC_GPU_API int aec_gpu_grib_bitmap_async(aec_gpu_ctx *ctx, int elem, const void *d_src, const uint64_t *src_offsets,
                                          const uint64_t *n_points, double missing, uint64_t n_fields, void *d_bitmap,
                                          const uint64_t *bitmap_offsets, uint64_t *d_counts, void *stream);

/*
 * aec_gpu_grib_pack_async over fields with bitmaps.  src_offsets[i] and n_points[i] describe the WHOLE grid, n_values[i] the
 * present points.  Absent points are loaded at most: they never enter the minimum, the maximum, the status or an X and
 * may hold NaN, Inf or 1e300.  Everything the call leaves -- d_work, d_out, d_chunks, the RSI table, d_result, d_fields --
 * is byte for byte what aec_gpu_grib_pack_async leaves for the fields compacted to their present points (a field whose
 * bitmap is all ones: exactly that call's); no compacted copy of the floats is written anywhere.  The exception is a
 * field with AEC_GPU_GRIB_MISMATCH in its record, and, the streams lying back to back, the places (not the bytes) of the
 * streams behind it.  have_params as there.
 */
AEC_GPU_API int aec_gpu_grib_pack_bitmap_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src,
                                               const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D,
                                               int have_params, const aec_gpu_grib_field *params, uint64_t n_fields, void *d_work,
                                               void *d_out, size_t out_cap, aec_gpu_batch_chunk *d_chunks,
                                               uint64_t *d_rsi_bit_offsets, aec_gpu_grib_field *d_fields,
                                               aec_gpu_enc_result *d_result, const void *d_bitmap, const uint64_t *bitmap_offsets,
                                               const uint64_t *n_points, void *stream);

/*
 * aec_gpu_grib_unpack_async into whole grids.  Exactly n_points[i] elements are written at d_dst + dst_offsets[i]: a
 * present point k gets the dequantised X of rank (ones in front of k), an absent point the bits of (T)missing -- the HOST
 * casts it once and the kernel stores those bits, so a NaN's payload is the host's.  d_status (n_fields uint32_t on the
 * device): 0 or AEC_GPU_GRIB_MISMATCH.  With the pack's table or bare (have_table == 0), as there.
 */
AEC_GPU_API int aec_gpu_grib_unpack_bitmap_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_in,
                                                 size_t in_bytes, const uint64_t *in_offsets, const uint64_t *in_bytes_each,
                                                 const uint64_t *n_values, const aec_gpu_grib_field *params,
                                                 const uint64_t *dst_offsets, uint64_t n_fields, uint64_t *d_rsi_bit_offsets,
                                                 int have_table, void *d_work, void *d_dst, aec_gpu_dec_result *d_results,
                                                 aec_gpu_dec_result *d_result, const void *d_bitmap,
                                                 const uint64_t *bitmap_offsets, const uint64_t *n_points, double missing,
                                                 uint32_t *d_status, void *stream);

/* The two halves alone, as aec_gpu_grib_quantise_async / aec_gpu_grib_dequantise_async */
AEC_GPU_API int aec_gpu_grib_quantise_bitmap_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src,
                                                   const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D,
                                                   int have_params, const aec_gpu_grib_field *params, uint64_t n_fields,
                                                   void *d_work, aec_gpu_grib_field *d_fields, const void *d_bitmap,
                                                   const uint64_t *bitmap_offsets, const uint64_t *n_points, void *stream);
AEC_GPU_API int aec_gpu_grib_dequantise_bitmap_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem,
                                                     const void *d_work, const uint64_t *n_values,
                                                     const aec_gpu_grib_field *params, const uint64_t *dst_offsets,
                                                     uint64_t n_fields, void *d_dst, const void *d_bitmap,
                                                     const uint64_t *bitmap_offsets, const uint64_t *n_points, double missing,
                                                     uint32_t *d_status, void *stream);

/*
 * ---- simple packing (templates 5.0 / 7.0) ---------------------------------------------------------------------------------
 * aec_gpu_grib_simple_plan is host arithmetic only (1 = taken, 0 = refused; it refuses whatever aec_gpu_grib_plan refuses).
 * plan is what aec_gpu_grib_plan gives for n_values; this layer's descriptors and wavefront table take the place of the
 * GRIB layer's in the context's buffer, so workspace_bytes grows by nothing.  simple_bytes is the sum of S_i =
 * ceil(n_values[i] * nbits / 8); simple_offsets (optional, n_fields entries) receives their running sum: streams back to
 * back, no padding.  nbits is 1 .. 32.
 */
typedef struct aec_gpu_grib_simple_plan_s {
    aec_gpu_grib_plan_t plan;
    size_t simple_bytes;
} aec_gpu_grib_simple_plan_t;
AEC_GPU_API int aec_gpu_grib_simple_plan(const aec_gpu_grib_template *t, int elem, const uint64_t *n_values, uint64_t n_fields,
                                         aec_gpu_grib_simple_plan_t *plan, uint64_t *work_offsets, uint64_t *simple_offsets);

/*
 * Rooms to streams: the X of field i, in the plan's room at d_work + work_offsets[i] (16-byte aligned, as everywhere), to the
 * S_i bytes at d_simple + simple_offsets[i].  Exactly those bytes are written, each once, and nothing else; X is taken
 * modulo 2^nbits, so a stray high bit in a container never reaches a neighbouring value.  n_fields == 0: AEC_OK, nothing
 * is enqueued (so for every call below).
 */
AEC_GPU_API int aec_gpu_grib_bits_pack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const uint64_t *n_values,
                                             uint64_t n_fields, const void *d_work, void *d_simple, const uint64_t *simple_offsets,
                                             void *stream);

/*
 * Streams to rooms.  The whole room of every field is written, the last block padded with the last X: byte for byte the room
 * aec_gpu_grib_quantise_async leaves for the same X; the up to 15 bytes between rooms are not written.  simple_bytes_each
 * (optional, HOST array) gives section 7's data length per message.  AEC_CONF_ERROR with nothing enqueued: a field with
 * simple_bytes_each[i] < S_i, or a stream that leaves [0, simple_bytes).  No load leaves [d_simple, d_simple + simple_bytes).
 */
AEC_GPU_API int aec_gpu_grib_bits_unpack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const uint64_t *n_values,
                                               uint64_t n_fields, const void *d_simple, size_t simple_bytes,
                                               const uint64_t *simple_offsets, const uint64_t *simple_bytes_each, void *d_work,
                                               void *stream);

/*
 * Floats to 5.0 streams: aec_gpu_grib_quantise_async (same arguments, same refusals, have_params as there; d_work and d_fields
 * come out exactly as it leaves them), then aec_gpu_grib_bits_pack_async.  The stream of a field whose record says bad is
 * unspecified, S_i bytes all the same.
 */
AEC_GPU_API int aec_gpu_grib_simple_pack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_src,
                                               const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D,
                                               int have_params, const aec_gpu_grib_field *params, uint64_t n_fields, void *d_work,
                                               aec_gpu_grib_field *d_fields, void *d_simple, const uint64_t *simple_offsets,
                                               void *stream);

/* 5.0 streams to floats: aec_gpu_grib_bits_unpack_async into d_work, then aec_gpu_grib_dequantise_async. */
AEC_GPU_API int aec_gpu_grib_simple_unpack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem, const void *d_simple,
                                                 size_t simple_bytes, const uint64_t *simple_offsets,
                                                 const uint64_t *simple_bytes_each, const uint64_t *n_values,
                                                 const aec_gpu_grib_field *params, const uint64_t *dst_offsets, uint64_t n_fields,
                                                 void *d_work, void *d_dst, void *stream);

/*
 * grid_simple to grid_ccsds: aec_gpu_grib_bits_unpack_async, then aec_gpu_encode_chunks_async over the rooms.  d_work, d_out,
 * d_chunks, d_rsi_bit_offsets and d_result are byte for byte what aec_gpu_grib_pack_async leaves for fields that quantise to
 * the same X.  No float is touched and no d_fields is written: the caller carries R, E, D and nbits over from section 5.
 */
AEC_GPU_API int aec_gpu_grib_simple_to_ccsds_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const void *d_simple,
                                                   size_t simple_bytes, const uint64_t *simple_offsets,
                                                   const uint64_t *simple_bytes_each, const uint64_t *n_values, uint64_t n_fields,
                                                   void *d_work, void *d_out, size_t out_cap, aec_gpu_batch_chunk *d_chunks,
                                                   uint64_t *d_rsi_bit_offsets, aec_gpu_enc_result *d_result, void *stream);

/*
 * grid_ccsds to grid_simple: aec_gpu_decode_chunks_async into d_work (with the pack's table, or bare with have_table == 0;
 * d_in .. have_table, d_results and d_result as in aec_gpu_grib_unpack_async), then aec_gpu_grib_bits_pack_async.  A field
 * whose record in d_results is not clean gets an unspecified stream of exactly its S_i bytes; every other field is exact.
 */
AEC_GPU_API int aec_gpu_grib_ccsds_to_simple_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, const void *d_in,
                                                   size_t in_bytes, const uint64_t *in_offsets, const uint64_t *in_bytes_each,
                                                   const uint64_t *n_values, uint64_t n_fields, uint64_t *d_rsi_bit_offsets,
                                                   int have_table, void *d_work, aec_gpu_dec_result *d_results,
                                                   aec_gpu_dec_result *d_result, void *d_simple, const uint64_t *simple_offsets,
                                                   void *stream);

/*
 * ---- complex packing (templates 5.2 / 5.3), reading -----------------------------------------------------------------------
 * What section 5 of one message says (HOST; the contract is COMPLEX PACKING at the head of this file).
 */
typedef struct aec_gpu_grib_complex_field_s {
    uint32_t ref_bits;      /* octet 20: bits of a group reference, 0..32 */
    uint32_t n_groups;      /* octets 32-35: NG >= 1 */
    uint32_t width_ref;     /* octet 36 */
    uint32_t width_bits;    /* octet 37: 0..32 */
    uint32_t length_ref;    /* octets 38-41 */
    uint32_t length_inc;    /* octet 42 */
    uint32_t last_length;   /* octets 43-46: true length of the last group */
    uint32_t length_bits;   /* octet 47: 0..32 */
    uint32_t order;         /* 0: template 5.2; 1 or 2: template 5.3 octet 48 */
    uint32_t extra_octets;  /* 5.3 octet 49: 0..8; ignored for order 0 */
    uint32_t missing;       /* octet 23: must be 0 (see out of scope) */
} aec_gpu_grib_complex_field;

#define AEC_GPU_GRIB_CX_RANGE     1u  /* some X lies outside [0, 2^nbits - 1]; the stored X are taken modulo 2^nbits */
#define AEC_GPU_GRIB_CX_MALFORMED 2u  /* lengths do not sum to n, a width above 32, or the packed values leave the stream */

/* the per-field record of an expansion, on the device (d_cx), 24 bytes */
typedef struct aec_gpu_grib_cx_s {
    int64_t x_min, x_max;   /* the signed reading of the modulo-2^64 X */
    uint32_t status;        /* AEC_GPU_GRIB_CX_* bits */
    uint32_t pad;           /* written as 0 */
} aec_gpu_grib_cx;

/*
 * Host arithmetic only (1 = taken, 0 = refused: whatever aec_gpu_grib_plan refuses, and what the contract lists of the
 * descriptors).  plan is what aec_gpu_grib_plan gives for t and n_values, its workspace_bytes grown by this layer's
 * descriptors, group tables (24 bytes a group) and tile aggregates.  tile_values = 1024 / container is the values one
 * wavefront of the value kernels owns (1 KiB of room), value_tiles the sum of ceil(room_i / 1024), group_tiles the sum of
 * ceil(n_groups_i / 64).
 */
typedef struct aec_gpu_grib_complex_plan_s {
    aec_gpu_grib_plan_t plan;
    uint64_t tile_values;
    uint64_t value_tiles;
    uint64_t group_tiles;
} aec_gpu_grib_complex_plan_t;
AEC_GPU_API int aec_gpu_grib_complex_plan(const aec_gpu_grib_template *t, int elem, const uint64_t *n_values,
                                          const aec_gpu_grib_complex_field *fields, uint64_t n_fields,
                                          aec_gpu_grib_complex_plan_t *plan, uint64_t *work_offsets);

/* Streams to rooms, and d_cx (8-byte aligned).  d_work: the plan's work_bytes, 16-byte aligned; the up to 15 bytes between
 * rooms are not written.  n_fields == 0: AEC_OK, nothing is enqueued (so for the two calls below). */
AEC_GPU_API int aec_gpu_grib_complex_expand_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t,
                                                  const aec_gpu_grib_complex_field *fields, const uint64_t *n_values,
                                                  uint64_t n_fields, const void *d_complex, size_t complex_bytes,
                                                  const uint64_t *complex_offsets, const uint64_t *complex_bytes_each, void *d_work,
                                                  aec_gpu_grib_cx *d_cx, void *stream);

/* 5.2 / 5.3 streams to floats: the expansion, then aec_gpu_grib_dequantise_async with the caller's R, E and D (params,
 * dst_offsets and d_dst as there).  The values of a field whose record says RANGE or MALFORMED are those of its stored X. */
AEC_GPU_API int aec_gpu_grib_complex_unpack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t, int elem,
                                                  const aec_gpu_grib_complex_field *fields, const void *d_complex, size_t complex_bytes,
                                                  const uint64_t *complex_offsets, const uint64_t *complex_bytes_each,
                                                  const uint64_t *n_values, const aec_gpu_grib_field *params,
                                                  const uint64_t *dst_offsets, uint64_t n_fields, void *d_work, void *d_dst,
                                                  aec_gpu_grib_cx *d_cx, void *stream);

/* 5.2 / 5.3 streams to 5.42 streams: the expansion, then aec_gpu_encode_chunks_async over the rooms.  d_work, d_out, d_chunks,
 * d_rsi_bit_offsets and d_result are byte for byte what aec_gpu_grib_pack_async leaves for fields that quantise to the same
 * X.  No float is touched: the caller carries R, E and D over from section 5 and writes t->nbits into the new one. */
AEC_GPU_API int aec_gpu_grib_complex_to_ccsds_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t,
                                                    const aec_gpu_grib_complex_field *fields, const void *d_complex,
                                                    size_t complex_bytes, const uint64_t *complex_offsets,
                                                    const uint64_t *complex_bytes_each, const uint64_t *n_values, uint64_t n_fields,
                                                    void *d_work, void *d_out, size_t out_cap, aec_gpu_batch_chunk *d_chunks,
                                                    uint64_t *d_rsi_bit_offsets, aec_gpu_enc_result *d_result,
                                                    aec_gpu_grib_cx *d_cx, void *stream);

/*
 * ---- complex packing (templates 5.2 / 5.3), writing -----------------------------------------------------------------------
 * What a batch is written under (HOST; the contract is THE WRITER'S RULE at the head of this file).
 */
typedef struct aec_gpu_grib_complex_write_s {
    uint32_t order;          /* 0: template 5.2;  1 or 2: template 5.3 */
    uint32_t group_length;   /* G: 16, 32, 64, 128 or 256 */
} aec_gpu_grib_complex_write;

/* the per-field record of a write, on the device (d_cxw), 56 bytes */
typedef struct aec_gpu_grib_cxw_s {
    aec_gpu_grib_complex_field desc;   /* 44 bytes: what goes into section 5, and what the reader calls take back */
    uint32_t pad;                      /* written as 0 */
    uint64_t bytes;                    /* S_i: section 7's data length */
} aec_gpu_grib_cxw;

/*
 * Host arithmetic only (1 = taken, 0 = refused: whatever aec_gpu_grib_plan refuses, and what the writer's rule lists).  plan is
 * what aec_gpu_grib_plan gives for t and n_values, its workspace_bytes grown by this layer's descriptors, per-field records,
 * tile totals (32 bytes a value tile) and group tables (12 bytes a group).  complex_bound is the sum of B_i; complex_offsets
 * (optional, n_fields entries) receives their running sum.  tile_values = 1024 / container and value_tiles are those of
 * aec_gpu_grib_complex_plan, group_tiles the sum of ceil(NG_i / 256) (a wavefront of the table kernel owns 256 groups),
 * out_tiles the sum of ceil(ceil(n_i (nbits + order) / 8) / 1024) (a wavefront of the value kernel owns 1 KiB of the packed
 * string at its longest).
 */
typedef struct aec_gpu_grib_complex_write_plan_s {
    aec_gpu_grib_plan_t plan;
    size_t   complex_bound;
    uint64_t tile_values;
    uint64_t value_tiles;
    uint64_t group_tiles;
    uint64_t out_tiles;
} aec_gpu_grib_complex_write_plan_t;
AEC_GPU_API int aec_gpu_grib_complex_write_plan(const aec_gpu_grib_template *t, const aec_gpu_grib_complex_write *w, int elem,
                                                const uint64_t *n_values, uint64_t n_fields,
                                                aec_gpu_grib_complex_write_plan_t *plan, uint64_t *work_offsets,
                                                uint64_t *complex_offsets);

/* Rooms to streams: the X of field i, in the plan's room at d_work + work_offsets[i], to S_i bytes at d_complex +
 * complex_offsets[i], and its record to d_cxw.  d_work is only read.  n_fields == 0: AEC_OK, nothing is enqueued (so for the
 * three calls below). */
AEC_GPU_API int aec_gpu_grib_complex_write_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t,
                                                 const aec_gpu_grib_complex_write *w, const uint64_t *n_values, uint64_t n_fields,
                                                 const void *d_work, void *d_complex, size_t complex_cap,
                                                 const uint64_t *complex_offsets, aec_gpu_grib_cxw *d_cxw, void *stream);

/* Floats to 5.2 / 5.3 streams: aec_gpu_grib_quantise_async (same arguments, same refusals, have_params as there; d_work and
 * d_fields come out exactly as it leaves them), then the writer.  The stream of a field whose record in d_fields says bad is
 * unspecified, at most B_i bytes inside its own range, and its d_cxw record says how many. */
AEC_GPU_API int aec_gpu_grib_complex_pack_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t,
                                                const aec_gpu_grib_complex_write *w, int elem, const void *d_src,
                                                const uint64_t *src_offsets, const uint64_t *n_values, const int32_t *D,
                                                int have_params, const aec_gpu_grib_field *params, uint64_t n_fields, void *d_work,
                                                aec_gpu_grib_field *d_fields, void *d_complex, size_t complex_cap,
                                                const uint64_t *complex_offsets, aec_gpu_grib_cxw *d_cxw, void *stream);

/* grid_ccsds to 5.2 / 5.3: aec_gpu_decode_chunks_async into d_work (with the pack's table, or bare with have_table == 0; d_in ..
 * have_table, d_results and d_result as in aec_gpu_grib_ccsds_to_simple_async), then the writer.  A field whose record in
 * d_results is not clean gets an unspecified stream of at most B_i bytes inside its own range and a record whose bytes <= B_i;
 * every other field is exact. */
AEC_GPU_API int aec_gpu_grib_ccsds_to_complex_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t,
                                                    const aec_gpu_grib_complex_write *w, const void *d_in, size_t in_bytes,
                                                    const uint64_t *in_offsets, const uint64_t *in_bytes_each,
                                                    const uint64_t *n_values, uint64_t n_fields, uint64_t *d_rsi_bit_offsets,
                                                    int have_table, void *d_work, aec_gpu_dec_result *d_results,
                                                    aec_gpu_dec_result *d_result, void *d_complex, size_t complex_cap,
                                                    const uint64_t *complex_offsets, aec_gpu_grib_cxw *d_cxw, void *stream);

/* grid_simple to 5.2 / 5.3: aec_gpu_grib_bits_unpack_async (d_simple .. simple_bytes_each and its refusals as there), then the
 * writer. */
AEC_GPU_API int aec_gpu_grib_simple_to_complex_async(aec_gpu_ctx *ctx, const aec_gpu_grib_template *t,
                                                     const aec_gpu_grib_complex_write *w, const void *d_simple, size_t simple_bytes,
                                                     const uint64_t *simple_offsets, const uint64_t *simple_bytes_each,
                                                     const uint64_t *n_values, uint64_t n_fields, void *d_work, void *d_complex,
                                                     size_t complex_cap, const uint64_t *complex_offsets, aec_gpu_grib_cxw *d_cxw,
                                                     void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AEC_GPU_GRIB_H */
