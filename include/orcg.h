/*
 * orcg.h — C ABI of the MI355X-native ORC column-stream decoder (liborcgpu).
 *
 * This is the drop-in boundary for the reference's stream-decoder hot path.
 * Every entry point is plain C (pointers + sizes, no torch / HIP C++ types);
 * hipStream_t travels as void*. The reference interfaces each group replaces
 * are cited inline (paths relative to the apache/orc checkout). No exceptions
 * cross this ABI: every call returns an ORCG_* status and the message is
 * available from orcg_ctx_last_error() / orcg_*_last_error(). The C++ adapter
 * (orc_amd/csrc/GpuRleDecoder.hh) rethrows them as orc::ParseError /
 * orc::InvalidArgument with the reference's messages
 * (c++/include/orc/Exceptions.hh:40-60); the JNI shim in INTEGRATION.md throws
 * java.io.IOException.
 *
 * Memory ownership: the caller owns every src/dst buffer and
 * the library never frees caller memory. Device scratch lives in an orcg_ctx,
 * one per reader thread (reentrant; contexts are not shared between threads).
 *
 * Value semantics are those of orc::RleDecoderV2 (c++/src/RleDecoderV2.cc):
 * zigzag for signed streams, int64 wraparound, static_cast narrowing for
 * int32/int16 outputs, and null slots (not_null[i] == 0) left untouched.
 */
#ifndef ORCG_H
#define ORCG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status ------------------------------------------------------------ */
enum {
  ORCG_OK = 0,
  ORCG_PARSE_ERROR = 1,      /* orc::ParseError (corrupt / truncated stream) */
  ORCG_INVALID_ARGUMENT = 2, /* orc::InvalidArgument (bad call, bad position) */
  ORCG_DEVICE_ERROR = 3,     /* HIP runtime failure or no usable device */
  ORCG_OUT_OF_MEMORY = 4
};

/* ---- context (one per reader thread) ------------------------------------ */
typedef struct orcg_ctx orcg_ctx;

/* Create a context bound to HIP device `device`, with its own non-blocking
 * stream. Replaces nothing in the reference (the reference has no device);
 * it is the owner of device scratch that MemoryPool (c++/include/orc/
 * MemoryPool.hh:27-33) plays for host buffers. */
int orcg_ctx_create(int device, orcg_ctx** out);
void orcg_ctx_destroy(orcg_ctx* ctx);

/* Pinned (page-locked) host memory, the allocator of the C++ adapter's
 * PinnedMemoryPool (an orc::MemoryPool, c++/include/orc/MemoryPool.hh:27-33):
 * batches in pinned memory can be DMA'd to a device without a staging copy.
 * NULL on failure. */
void* orcg_host_alloc(uint64_t bytes);
void orcg_host_free(void* p);
/* Use an external stream (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL restores the context's own stream.
 * Ordering contract of every *_device entry: the launch is queued on the
 * context stream and nothing else. The context's own stream is
 * non-blocking, so it is NOT ordered after work on the legacy NULL stream or
 * any other stream: a caller that fills or copies d_src / d_segs / d_dst on
 * stream P must either pass P here, or make the context stream wait on an
 * event recorded on P (hipStreamWaitEvent(orcg_ctx_stream(ctx), ev, 0))
 * before the call. Consumers of d_dst order after the context stream the
 * same way (tests/test_gpu_stream_order.py). */
int orcg_ctx_set_stream(orcg_ctx* ctx, void* hip_stream);
void* orcg_ctx_stream(orcg_ctx* ctx);
/* Wait for the context stream and collect any device-side decode error of
 * the launches issued since the last call (first error in value order). */
int orcg_ctx_synchronize(orcg_ctx* ctx);
const char* orcg_ctx_last_error(const orcg_ctx* ctx);
/* Value index (row) of the last device-side error collected on this context:
 * the first failing value in value order of that launch. */
uint64_t orcg_ctx_last_error_value(const orcg_ctx* ctx);

/* Kernel selection for RLEv2 decode (tuning / A-B measurement). TILED (the
 * default) stages segment chunks through LDS by LDS-DMA and walks headers in
 * LDS; WAVE_WALK is one wavefront per segment reading HBM directly. Both are
 * bit-identical. */
enum { ORCG_RLEV2_TILED = 0, ORCG_RLEV2_WAVE_WALK = 1 };
/* Other accepted values pin one instance of the tiled kernel (used by the
 * parity tests to cover every instance the default may pick, and by A/B
 * timing); orcg_rlev2_variants lists them: 2 = 33 KB register-filled serial
 * windows with the flat DIRECT prologue, W=64 runs in aligned 16-byte chunks
 * (the default's for >= 5 stream bytes per value), 3 = 21 KB serial windows + dense drain, 4 / 5 = dense 8.5 /
 * 12.5 KB, 6 = the union instance in two passes, 7 = 33 KB serial + dense
 * drain, 8 = the union instance in one pass, 9 = 2 without the flat DIRECT
 * prologue (its A/B control), 10 = 2 with the prologue's 8-byte accesses at
 * every width (the A/B control of the 16-byte chunks). Unknown values:
 * INVALID_ARGUMENT. */
int orcg_ctx_set_rlev2_variant(orcg_ctx* ctx, int variant);
/* Writes up to `cap` accepted variant ids to `out`; returns how many exist. */
int orcg_rlev2_variants(int* out, int cap);

const char* orcg_version(void);
/* Number of visible HIP devices (0 when none; never aborts). */
int orcg_device_count(void);
/* Page-lock / release caller host memory for asynchronous D2H copies (e.g.
 * each rank's slice of a shared host batch, orc_amd/shard.py). */
int orcg_host_register(void* host, uint64_t bytes);
int orcg_host_unregister(void* host);

/* ---- segments: the ORC-native parallel sync points ----------------------
 * A segment is a run-aligned byte offset in an uncompressed (or already
 * decompressed) stream plus the index of the first value of the run that
 * starts there. Row-index positions (site/specification/ORCv1.md:1266-1272;
 * recorded by RleEncoderV2::recordPosition) are exactly this: (byte offset of
 * the run start, values of that run to skip). Segment k covers every run
 * whose first byte lies in [segs[k].byte_offset, segs[k+1].byte_offset)
 * (the last one runs to the end of the stream). */
typedef struct orcg_segment {
  uint64_t byte_offset;
  uint64_t value_index;
} orcg_segment;

/* ---- RLEv2 integer streams ----------------------------------------------
 * Replaces the run loop of orc::RleDecoderV2::next<T>
 * (c++/src/RleDecoderV2.cc:132-453) and its bit unpackers
 * BitUnpackDefault/BitUnpackAVX512::readLongs (c++/src/BpackingDefault.cc:
 * 330-366, c++/src/BpackingAvx512.cc:2443-2586) for a whole stream or a
 * row-group range at once. */

/* Host run walk: reads only run headers (the host holds the bytes after
 * decompression) and cuts the stream into segments of at most
 * ~max_segment_bytes / max_segment_values. It also finds the first corrupt
 * run, reported lazily by the decoders exactly where the reference would
 * throw (RleDecoderV2.cc:38, :307, :328-330, :412-415).
 * One limit is this library's own: a DELTA run's two base-128 varints must
 * end within the run's first 64 bytes (two bytes of header and padded
 * varints of up to 62 bytes together; no writer emits more than 22). A longer
 * header is reported as "bad read in RleDecoderV2::readByte" at the run's
 * first value, by the plan and by every device decoder alike. */
typedef struct orcg_rlev2_plan orcg_rlev2_plan;
int orcg_rlev2_plan_create(const uint8_t* src, uint64_t src_len, uint64_t max_segment_bytes,
                           uint64_t max_segment_values, orcg_rlev2_plan** out);
void orcg_rlev2_plan_destroy(orcg_rlev2_plan* plan);
/* values decodable before the first corrupt run (all values if none) */
uint64_t orcg_rlev2_plan_values(const orcg_rlev2_plan* plan);
uint64_t orcg_rlev2_plan_segments(const orcg_rlev2_plan* plan, const orcg_segment** segs);
/* ORCG_OK, or the status of the first corrupt run (*at_value = its first
 * value index, *msg = the reference's ParseError text). */
int orcg_rlev2_plan_error(const orcg_rlev2_plan* plan, uint64_t* at_value, const char** msg);

/* Device-resident decode (asynchronous on the context stream).
 * d_src: stream bytes in HBM; d_segs: segment table in HBM (nsegs entries);
 * values with index v in [value_begin, value_begin + nvalues) are written
 * dense to d_dst[v - value_begin] as int64/int32/int16 (dst_bytes 8/4/2).
 * Corrupt runs set the context's device error record (see
 * orcg_ctx_synchronize). */
int orcg_rlev2_decode_device(orcg_ctx* ctx, const uint8_t* d_src, uint64_t src_len, int is_signed,
                             const orcg_segment* d_segs, uint64_t nsegs, uint64_t value_begin,
                             uint64_t nvalues, void* d_dst, int dst_bytes);

/* Same, but the segment table is the column's ROW_INDEX positions as the
 * writer records them: d_positions[2*g] = byte offset of the run holding row
 * g*rows_per_group, d_positions[2*g+1] = values of that run to skip
 * (ORCv1.md:1266-1272; RleDecoderV2::seek, RleDecoderV2.cc:109-117). The
 * first value of segment g is g*rows_per_group - skip. No host work. */
int orcg_rlev2_decode_positions_device(orcg_ctx* ctx, const uint8_t* d_src, uint64_t src_len,
                                       int is_signed, const uint64_t* d_positions,
                                       uint64_t ngroups, uint64_t rows_per_group,
                                       uint64_t value_begin, uint64_t nvalues, void* d_dst,
                                       int dst_bytes);

/* Host-buffer decode (the SURVEY.md §8b sketch): H2D, decode, D2H; with a
 * not_null mask the n positions receive values in order and null slots are
 * left untouched (RleDecoderV2::copyDataFromBuffer, :437-453). Synchronous. */
int orcg_rlev2_decode_i64(orcg_ctx* ctx, const uint8_t* src, uint64_t src_len, int is_signed,
                          const char* not_null, uint64_t n, int64_t* dst);
int orcg_rlev2_decode_i32(orcg_ctx* ctx, const uint8_t* src, uint64_t src_len, int is_signed,
                          const char* not_null, uint64_t n, int32_t* dst);
int orcg_rlev2_decode_i16(orcg_ctx* ctx, const uint8_t* src, uint64_t src_len, int is_signed,
                          const char* not_null, uint64_t n, int16_t* dst);

/* ---- stateful decoder: drop-in for orc::RleDecoder ----------------------
 * Mirrors class RleDecoder (c++/src/RLE.hh:109-141) as created by
 * createRleDecoder(stream, isSigned, RleVersion_2, pool, metrics)
 * (c++/src/RLE.hh:163, c++/src/RLE.cc:48-60): the stream is bulk-decoded on
 * the device on creation and next()/skip()/seek() serve slices, so run state
 * persists across calls of any size and errors surface at the same value as
 * in the reference. */
typedef struct orcg_rle_decoder orcg_rle_decoder;
int orcg_rle_decoder_create(orcg_ctx* ctx, const uint8_t* src, uint64_t src_len, int is_signed,
                            int rle_version, orcg_rle_decoder** out);
void orcg_rle_decoder_destroy(orcg_rle_decoder* dec);
int orcg_rle_decoder_next_i64(orcg_rle_decoder* dec, int64_t* data, uint64_t n, const char* not_null);
int orcg_rle_decoder_next_i32(orcg_rle_decoder* dec, int32_t* data, uint64_t n, const char* not_null);
int orcg_rle_decoder_next_i16(orcg_rle_decoder* dec, int16_t* data, uint64_t n, const char* not_null);
/* RleDecoder::skip (RleDecoderV2.cc:119-130) */
int orcg_rle_decoder_skip(orcg_rle_decoder* dec, uint64_t n);
/* RleDecoder::seek(PositionProvider&) (RleDecoderV2.cc:109-117) for an
 * uncompressed stream: positions = {byte offset, values to skip}. */
int orcg_rle_decoder_seek(orcg_rle_decoder* dec, const uint64_t* positions, uint64_t npositions);
/* Java face (java/core/src/java/org/apache/orc/impl/
 * RunLengthIntegerReaderV2.java:371-396, nextVector): null slots get 1 and
 * *is_repeating reports whether every slot holds the same value. is_null may
 * be NULL (no nulls). */
int orcg_rle_decoder_next_vector_java(orcg_rle_decoder* dec, int64_t* vector, const uint8_t* is_null,
                                      uint64_t n, int* is_repeating);
/* The int[] overload (RunLengthIntegerReaderV2.java:399-411): values narrowed
 * to int32 ((int) next()), null slots 1; with a null mask, a vector that is
 * repeating with isNull[0] is left untouched; isRepeating is an input only. */
int orcg_rle_decoder_next_vector_java_int(orcg_rle_decoder* dec, int32_t* vector, const uint8_t* is_null, uint64_t n,
                                          int is_repeating);
const char* orcg_rle_decoder_last_error(const orcg_rle_decoder* dec);
/* A decoder with Java's rules: new RunLengthIntegerReaderV2(input, signed,
 * skipCorrupt) (java/core/src/java/org/apache/orc/impl/
 * RunLengthIntegerReaderV2.java:47-52), for the Java faces above. Where the
 * Java reader differs from the C++ one (it checks less):
 *  - a DELTA run with a bit width and one value (length byte 0) is not an
 *    error: Java emits the first value and first + deltaBase (:125-145);
 *  - PATCHED_BASE with pw + pgw > 64 fails with Java's IOException text
 *    ("Corruption in ORC data encountered. To skip reading corrupted data,
 *    set hive.exec.orc.skip.corrupt.data to true", ORCG_PARSE_ERROR) unless
 *    skip_corrupt, which decodes it reading the patch list at
 *    getClosestFixedBits(pw + pgw) bits an entry with Java's shift semantics
 *    (:196-260: pw = 64 leaves no patch bits, so the values are base + the
 *    packed literals);
 *  - PATCHED_BASE with pl == 0 fails as Java's unpackedPatch[0] does
 *    (ArrayIndexOutOfBoundsException "Index 0 out of bounds for length 0",
 *    ORCG_PARSE_ERROR), after the run's bytes are read.
 * Truncated runs keep the C++ reader's "bad read" errors (Java's InStream
 * returns -1 bytes there instead of failing). Decoded by the wave-walk
 * kernel (ORCG_RLEV2_WAVE_WALK). */
int orcg_rle_decoder_create_java(orcg_ctx* ctx, const uint8_t* src, uint64_t src_len, int is_signed,
                                 int skip_corrupt, orcg_rle_decoder** out);

/* ---- byte RLE / boolean RLE (PRESENT, BOOLEAN, BYTE streams) -------------
 * Replaces ByteRleDecoderImpl / BooleanRleDecoderImpl (c++/src/ByteRLE.hh:
 * 71-126, ByteRLE.cc:359-643). Segments index decoded BYTES; byte-RLE
 * row-index positions are (byte offset, bytes to skip) and boolean ones add
 * the bits consumed of the next byte (ByteRLE.cc:409-417, :549-560). The
 * plan accessors above (orcg_rlev2_plan_*) apply to byte plans too. */
int orcg_byterle_plan_create(const uint8_t* src, uint64_t src_len, uint64_t max_segment_bytes,
                             uint64_t max_segment_values, orcg_rlev2_plan** out);
/* decoded bytes [value_begin, value_begin + nvalues) -> d_dst */
int orcg_byterle_decode_device(orcg_ctx* ctx, const uint8_t* d_src, uint64_t src_len,
                               const orcg_segment* d_segs, uint64_t nsegs, uint64_t value_begin,
                               uint64_t nvalues, uint8_t* d_dst);
/* rows (bits, MSB first) [row_begin, row_begin + nrows) -> one char 0/1 per row */
int orcg_boolrle_decode_device(orcg_ctx* ctx, const uint8_t* d_src, uint64_t src_len,
                               const orcg_segment* d_segs, uint64_t nsegs, uint64_t row_begin,
                               uint64_t nrows, uint8_t* d_dst);
/* The same decode with what the file reader passes along: d_nrows (device,
 * may be NULL) holds the row count, read by the kernel, with nrows the
 * host-side bound of it (the size of d_dst); the decode adds the number of
 * set rows it writes to *d_ones (device, may be NULL; not zeroed here). */
int orcg_boolrle_decode_counted_device(orcg_ctx* ctx, const uint8_t* d_src, uint64_t src_len,
                                       const orcg_segment* d_segs, uint64_t nsegs, uint64_t row_begin,
                                       uint64_t nrows, const uint64_t* d_nrows, uint8_t* d_dst,
                                       uint64_t* d_ones);

/* Stateful drop-in for orc::ByteRleDecoder as created by
 * createByteRleDecoder / createBooleanRleDecoder (c++/src/ByteRLE.hh:114,126):
 * next(data, n, notNull) leaves null slots untouched (byte) or writes 0
 * (boolean); seek takes 2 (byte) or 3 (boolean) position values. */
typedef struct orcg_byte_rle_decoder orcg_byte_rle_decoder;
int orcg_byte_rle_decoder_create(orcg_ctx* ctx, const uint8_t* src, uint64_t src_len, int boolean,
                                 orcg_byte_rle_decoder** out);
void orcg_byte_rle_decoder_destroy(orcg_byte_rle_decoder* dec);
int orcg_byte_rle_decoder_next(orcg_byte_rle_decoder* dec, char* data, uint64_t n, const char* not_null);
int orcg_byte_rle_decoder_skip(orcg_byte_rle_decoder* dec, uint64_t n);
int orcg_byte_rle_decoder_seek(orcg_byte_rle_decoder* dec, const uint64_t* positions, uint64_t npositions);
const char* orcg_byte_rle_decoder_last_error(const orcg_byte_rle_decoder* dec);

/* ---- Java TreeReader face (java/core/src/java/org/apache/orc/impl/
 * TreeReaderFactory.java): the ColumnVector fields a JNI shim fills, built
 * from the GPU-decoded streams of the stateful decoders above. Java boolean[]
 * travels as one byte per row (1 = true). Errors: the status, and the message
 * from orcg_java_last_error() (this thread's last failure). */
const char* orcg_java_last_error(void);
/* TreeReader.nextVector (TreeReaderFactory.java:405-441): `present` is the
 * column's PRESENT stream as a boolean decoder (BitFieldReader,
 * BitFieldReader.java:30-57; NULL = no PRESENT stream), parent_is_null the
 * parent's isNull (NULL = none). Writes is_null[batch] and *no_nulls; with a
 * PRESENT stream or a parent mask *is_repeating = !noNulls && every row null,
 * otherwise *is_repeating is left unchanged (as the reference leaves it). */
int orcg_java_tree_present_next(orcg_byte_rle_decoder* present, const uint8_t* parent_is_null, uint64_t batch,
                                uint8_t* is_null, int* no_nulls, int* is_repeating);
/* StringDictionaryTreeReader.nextVector's readDictionaryByteArray
 * (TreeReaderFactory.java:2396-2478), no filter context: the DATA indices
 * through RunLengthIntegerReaderV2.nextVector (`data`, unsigned; scratch =
 * the reader's scratchlcv.vector, kept by the caller across batches), then
 * BytesColumnVector.setRef(i, dictionaryBuffer, start[i], length[i]) per row:
 * start = dictionaryOffsets[idx], length = the next offset - start, or
 * buffer_len - start for the last array entry (getDictionaryEntryLength);
 * null rows (0, 0); a repeating index vector sets row 0 only and returns
 * *is_repeating = 1. is_null / *no_nulls / *is_repeating come in from
 * orcg_java_tree_present_next (the result vector's fields). has_buffer = 0
 * (dictionaryBuffer == null): non-null rows get the empty string, or with
 * dict_offsets NULL too the batch becomes one repeating null. An index
 * outside the offsets array: ORCG_PARSE_ERROR with Java's
 * "Index i out of bounds for length n". */
int orcg_java_dictionary_next(orcg_rle_decoder* data, const int32_t* dict_offsets, uint64_t dict_offsets_len,
                              int has_buffer, int64_t buffer_len, uint8_t* is_null, int* no_nulls, int* is_repeating,
                              uint64_t batch, int64_t* scratch, int32_t* start, int32_t* length);

/* ---- RLEv1 (DIRECT / DICTIONARY encodings, format 0.11 files) ------------
 * Replaces RleDecoderV1 (c++/src/RLEv1.hh:51-96, RLEv1.cc:140-300) as chosen
 * by createRleDecoder for RleVersion_1 (c++/src/RLE.cc:48-60). Plans cut the
 * stream at control bytes; the plan accessors (orcg_rlev2_plan_*) apply.
 * Truncated streams raise "bad read in readByte" (RLEv1.cc:141-146). */
int orcg_rlev1_plan_create(const uint8_t* src, uint64_t src_len, uint64_t max_segment_bytes,
                           uint64_t max_segment_values, orcg_rlev2_plan** out);
int orcg_rlev1_decode_device(orcg_ctx* ctx, const uint8_t* d_src, uint64_t src_len, int is_signed,
                             const orcg_segment* d_segs, uint64_t nsegs, uint64_t value_begin,
                             uint64_t nvalues, void* d_dst, int dst_bytes);
/* RleDecoderV1::next<T>(data, n, notNull) over a whole host stream. */
int orcg_rlev1_decode_i64(orcg_ctx* ctx, const uint8_t* src, uint64_t src_len, int is_signed,
                          const char* not_null, uint64_t n, int64_t* data);
int orcg_rlev1_decode_i32(orcg_ctx* ctx, const uint8_t* src, uint64_t src_len, int is_signed,
                          const char* not_null, uint64_t n, int32_t* data);

/* ---- nullable columns and string dictionaries ----------------------------
 * Null scatter (RleDecoderV2::copyDataFromBuffer with notNull,
 * RleDecoderV2.cc:437-453): dense values -> the non-null rows of d_out
 * (width 8/4/2/1 bytes). fill_nulls = 0 leaves null slots untouched (C++);
 * 1 writes fill_value there (Java's 1, RunLengthIntegerReaderV2.java:371-396). */
int orcg_scatter_not_null_device(orcg_ctx* ctx, const void* d_dense, const uint8_t* d_not_null,
                                 uint64_t n, void* d_out, int width, int fill_nulls,
                                 int64_t fill_value);
/* Dictionary LENGTH values -> offsets[dict_size + 1] (loadStringDictionary,
 * c++/src/DictionaryLoader.cc:69-80). */
int orcg_dict_offsets_device(orcg_ctx* ctx, const int64_t* d_lengths, uint64_t dict_size,
                             int64_t* d_offsets);
/* Per non-null row: start = offsets[idx], length = offsets[idx+1] -
 * offsets[idx]; idx >= dict_size raises "Entry index out of range in
 * StringDictionaryColumn" (StringDictionaryColumnReader::next,
 * c++/src/ColumnReader.cc:561-594). Starts are blob-relative: the C++ adapter
 * adds the host blob base after D2H. index_width 8 or 4. */
int orcg_dict_gather_device(orcg_ctx* ctx, const void* d_indices, int index_width,
                            const uint8_t* d_not_null, uint64_t n, const int64_t* d_offsets,
                            uint64_t dict_size, int64_t* d_start, int64_t* d_length);
/* Decimal64ColumnReader / Decimal128ColumnReader::next value decode
 * (c++/src/ColumnReader.cc:1300-1527) over a device-resident DATA stream of
 * zigzag varints and the values' scales (the decoded SECONDARY stream):
 * nvalues values rescaled to `scale`. precision <= 18: int64 d_out[nvalues]
 * ("Decimal scale out of range" past 18 digits, readInt64 :1342-1349);
 * precision > 18: int64 d_out[2 * nvalues], [hi, lo] per value (orc::Int128).
 * precision == 0: Hive 0.11 decimals (DecimalHive11ColumnReader, :1578-1692),
 * Int128 layout rescaled to `scale` (the forced scale, RowReaderOptions::
 * forcedScaleOnHive11Decimal, 6 by default); a value past 128 bits or 38
 * digits is "Hive 0.11 decimal was more than 38 digits." (the reference's
 * default throwOnHive11DecimalOverflow). Fewer varints than nvalues: "Read past end of stream in
 * Decimal64ColumnReader". Synchronous. */
int orcg_decimal_decode_device(orcg_ctx* ctx, const uint8_t* d_src, uint64_t src_len, const int64_t* d_scales,
                               uint64_t nvalues, uint32_t precision, int32_t scale, void* d_out);
/* Hive 0.11 decimals (precision 0) under RowReaderOptions::
 * throwOnHive11DecimalOverflow (c++/include/orc/Reader.hh:258-271;
 * DecimalHive11ColumnReader::next, c++/src/ColumnReader.cc:1638-1680): 1 is
 * orcg_decimal_decode_device(precision 0); 0 replaces every value past 128
 * bits or 38 digits by NULL instead of raising: d_keep[k] (nvalues bytes) is 0
 * for such a value (its slot holds 0) and 1 otherwise. Synchronous. */
int orcg_hive11_decimal_decode_device(orcg_ctx* ctx, const uint8_t* d_src, uint64_t src_len, const int64_t* d_scales,
                                      uint64_t nvalues, int32_t scale, int throw_on_overflow, void* d_out,
                                      uint8_t* d_keep);
/* TimestampColumnReader::next value construction (c++/src/ColumnReader.cc
 * :318-347) in place: seconds += epoch (1420070400 for UTC writers), nanos
 * from the trailing-zero code; writer and reader zones with equal rules. */
int orcg_timestamp_decode_device(orcg_ctx* ctx, int64_t* d_seconds, int64_t* d_nanos, uint64_t n, int64_t epoch);

/* ---- Time zone rules (c++/src/Timezone.hh / Timezone.cc). Host only: none
 * of the orcg_timezone_* entries touches a GPU. */
typedef struct orcg_timezone orcg_timezone;
/* getTimezone(filename, bytes) (Timezone.cc:815-818): TZif v1 / v2+ bytes
 * (parseZoneFile, :869-946; in a v2+ file the 64-bit block and its POSIX
 * footer rule, :196-466). A bad file is ORCG_PARSE_ERROR with the reference's
 * TimezoneError text in orcg_timezone_last_error() ("non-tzfile <name>",
 * "tzfile too short <name> needs N and has M", "name out of range in variant
 * ...", "tzfile rule out of range ...", "<what> at <pos> in '<rule>'"). */
int orcg_timezone_parse(const char* name, const uint8_t* tzif, uint64_t len, orcg_timezone** out);
/* getTimezoneByName (Timezone.cc:759-810): the US aliases (:47-59), then
 * <dir>/<name> with <dir> = $TZDIR, else $CONDA_PREFIX/share/zoneinfo, else
 * /usr/share/zoneinfo (getTimezoneDirectory, :681-695). The UTC names (GMT,
 * UTC, Etc/UTC, ...) resolve to a built-in zero-offset zone without a file.
 * A name that is empty, longer than 255 bytes, absolute or has a ".."
 * component is not opened. Not found: ORCG_INVALID_ARGUMENT. */
int orcg_timezone_load(const char* name, orcg_timezone** out);
void orcg_timezone_destroy(orcg_timezone* tz);
/* Timezone::getVersion (1: 32-bit block, 2: 64-bit block) */
uint64_t orcg_timezone_version(const orcg_timezone* tz);
/* Timezone::getEpoch (Timezone.cc:664-679): 2015-01-01 00:00:00 in the zone */
int64_t orcg_timezone_epoch(const orcg_timezone* tz);
/* Timezone::getVariant (Timezone.cc:948-963; FutureRuleImpl::getVariant
 * :275-290 past the last transition). *name is valid until destroy. */
int orcg_timezone_variant(const orcg_timezone* tz, int64_t clk, int64_t* gmt_offset, int* is_dst, const char** name);
/* Timezone::convertToUTC / convertFromUTC (Timezone.cc:608-616) */
int64_t orcg_timezone_convert_to_utc(const orcg_timezone* tz, int64_t clk);
int64_t orcg_timezone_convert_from_utc(const orcg_timezone* tz, int64_t clk);
/* this thread's last orcg_timezone_parse / _load failure */
const char* orcg_timezone_last_error(void);
/* TimestampColumnReader::next with different writer and reader zones
 * (c++/src/ColumnReader.cc:318-347), in place: seconds += the writer zone's
 * epoch, nanos from the trailing-zero code, then the wall-clock adjustment
 * between the zones' variants (:333-345). Uploads both zones' tables for the
 * call; the same zone on both sides is orcg_timestamp_decode_device with that
 * zone's epoch. Synchronous. */
int orcg_timestamp_decode_tz_device(orcg_ctx* ctx, int64_t* d_seconds, int64_t* d_nanos, uint64_t n,
                                    const orcg_timezone* writer_tz, const orcg_timezone* reader_tz);
/* Measurement helper (no reference counterpart): `iters` timed launches over
 * n values, each on a fresh device copy of d_*_in; ms_out[i] = HIP-event time
 * of launch i. mode 0: the unadjusted kernel of orcg_timestamp_decode_device
 * with the writer zone's epoch; 1: the zone-adjusting kernel. */
int orcg_timestamp_tz_bench(orcg_ctx* ctx, const int64_t* d_seconds_in, const int64_t* d_nanos_in,
                            int64_t* d_seconds, int64_t* d_nanos, uint64_t n, const orcg_timezone* writer_tz,
                            const orcg_timezone* reader_tz, int mode, uint32_t iters, double* ms_out);

/* ---- schema evolution: numeric and decimal conversions --------------------
 * One decoded column converted to the kind of a read type, value for value as
 * the reference's ConvertColumnReader does (c++/src/ConvertColumnReader.cc:
 * 59-207 numeric -> numeric, :342-415 numeric -> decimal, :491-563 decimal ->
 * numeric, :566-617 decimal -> decimal; convertDecimal, c++/src/Int128.cc:
 * 534-624). The source class names how the n values lie in d_src (the batch
 * layout of orcg_reader.h): */
enum {
  ORCG_CONVERT_INT64 = 0,     /* int64: boolean, tinyint, smallint, int, bigint */
  ORCG_CONVERT_FLOAT = 1,     /* double holding a float value: float */
  ORCG_CONVERT_DOUBLE = 2,    /* double */
  ORCG_CONVERT_DECIMAL64 = 3, /* int64, unscaled at src_scale */
  ORCG_CONVERT_DECIMAL128 = 4 /* [hi, lo] int64 pairs, unscaled at src_scale */
};
/* target_kind is the read type's Type.Kind (ORCG_TYPE_BOOLEAN .. ORCG_TYPE_DOUBLE
 * or ORCG_TYPE_DECIMAL with precision and scale; src_scale counts for decimal
 * sources only). d_out receives int64 (boolean and the integers: the narrowed
 * value), double (float: the float-rounded value; double), int64 (decimal,
 * precision <= 18) or [hi, lo] int64 pairs (precision > 18). d_not_null (NULL =
 * every row set) is only read; d_out_not_null[n] is always written: 1 for a
 * set row whose value the target holds, else 0, and such a row's slot holds 0.
 * *nulled = the set rows the conversion turned into NULLs (handleOverflow,
 * :66-76). With throw_on_overflow the first of them in value order fails the
 * call: ORCG_PARSE_ERROR, "Overflow when convert from <source> to <target>"
 * (the reference's SchemaEvolutionError, which prints typeid names), its row in
 * no particular slot of the outputs. Synchronous. */
int orcg_convert_column_device(orcg_ctx* ctx, const void* d_src, int src_class, int32_t src_scale, uint64_t n,
                               const uint8_t* d_not_null, uint32_t target_kind, uint32_t precision, uint32_t scale,
                               int throw_on_overflow, void* d_out, uint8_t* d_out_not_null, uint64_t* nulled);

/* Measurement helper (no reference counterpart): `iters` timed launches of
 * that conversion (overflows nulled), ms_out[i] = HIP-event time of launch i. */
int orcg_convert_bench(orcg_ctx* ctx, const void* d_src, int src_class, int32_t src_scale, uint64_t n,
                       const uint8_t* d_not_null, uint32_t target_kind, uint32_t precision, uint32_t scale, void* d_out,
                       uint8_t* d_out_not_null, uint32_t iters, double* ms_out);

/* IntegerColumnReader<LongVectorBatch>::next for a whole stripe column
 * (c++/src/ColumnReader.cc:81-104, 224-258): PRESENT (boolean RLE; NULL/0 if
 * the column has no nulls) + DATA (RLEv2) host streams -> not_null[n] and
 * data[n] with null slots untouched. */
int orcg_decode_integer_column(orcg_ctx* ctx, const uint8_t* present, uint64_t present_len,
                               const uint8_t* data, uint64_t data_len, int is_signed, uint64_t n,
                               int64_t* out, char* not_null);

/* ---- synthetic streams (writer side, for benchmarks and tests) ----------
 * A minimal RLEv2 writer: DIRECT runs of up to 512 values at the smallest
 * width from the 5-bit table (aligned = round the width up to the
 * byte-aligned set, as RleEncoderV2's SPEED strategy does,
 * c++/src/RleEncoderV2.cc). Optionally records row-index positions
 * ({byte offset, values to skip} per rows_per_group) the way
 * RleEncoderV2::recordPosition does. */
int orcg_rlev2_encode_direct(const int64_t* values, uint64_t n, int is_signed, int aligned,
                             uint8_t* dst, uint64_t dst_cap, uint64_t* out_len,
                             uint64_t rows_per_group, uint64_t* positions);
/* General run builder: run i encodes the next lengths[i] values with
 * kinds[i] (0 SHORT_REPEAT, 1 DIRECT, 2 PATCHED_BASE, 3 DELTA); fails with
 * ORCG_INVALID_ARGUMENT if the values are not representable that way.
 * run_offsets (optional, nruns entries) receives each run's byte offset. */
int orcg_rlev2_encode_runs(const int64_t* values, uint64_t n, int is_signed, const uint8_t* kinds,
                           const uint32_t* lengths, uint64_t nruns, uint8_t* dst, uint64_t dst_cap,
                           uint64_t* out_len, uint64_t* run_offsets);

/* ---- Snappy chunks inflated on the device ---------------------------------
 * ORC's block compression cuts a stream into independent chunks (3-byte
 * headers; ORCv1.md "Compression"). A Snappy chunk states its decompressed
 * length in its preamble, so a stream is laid out without inflating anything:
 * the plan is a table of chunks, the device inflates them in one launch.
 * Offsets are relative to the source / destination buffers of the decode
 * call. A stored ("original") chunk is a plain copy. */
#define ORCG_SNAPPY_STORED 1u
typedef struct orcg_snappy_chunk {
  uint64_t src_offset, src_bytes; /* the chunk's body (a raw Snappy block, or the stored bytes) */
  uint64_t dst_offset, dst_bytes; /* its decompressed bytes */
  uint64_t flags;                 /* ORCG_SNAPPY_STORED */
} orcg_snappy_chunk;

/* out[0] = bytes of decompressed history a chunk keeps on chip (a copy that
 * reaches further back reads the output instead), out[1] = threads per chunk. */
void orcg_snappy_device_info(uint32_t out[2]);
/* The plan of `len` host bytes holding chunks framed by ORC's 3-byte headers:
 * one table entry per chunk, sources at their offsets in `src`, destinations
 * consecutive from 0. A compressed chunk's preamble is read with the host
 * decoder's two checks ("snappy: bad length", "snappy: output exceeds the
 * compression block size"; a cut header is "Read past EOF in
 * DecompressionStream::readBuffer"): ORCG_PARSE_ERROR with the text in
 * *error (static storage). table (may be null) receives up to `cap` entries;
 * *nchunks the number of chunks, *total the decompressed bytes. */
int orcg_snappy_plan(const uint8_t* src, uint64_t len, uint64_t block_size, orcg_snappy_chunk* table, uint64_t cap,
                     uint64_t* nchunks, uint64_t* total, const char** error);
/* Inflates the nchunks chunks of `table` (host memory) from the device bytes
 * d_src[0, src_len) into d_dst[0, dst_len): one launch, synchronous. Chunks
 * must lie inside the buffers (ORCG_INVALID_ARGUMENT). Nothing outside a
 * chunk's destination range is written, whatever the input. A corrupt chunk
 * fails with ORCG_PARSE_ERROR and the host decoder's text ("snappy: truncated
 * literal", "snappy: literal out of range", "snappy: truncated copy",
 * "snappy: copy out of range", "snappy: length mismatch"; the latter also
 * when a preamble disagrees with dst_bytes); orcg_ctx_last_error_value is the
 * lowest failing chunk's index. */
int orcg_snappy_decompress_device(orcg_ctx* ctx, const uint8_t* d_src, uint64_t src_len,
                                  const orcg_snappy_chunk* table, uint64_t nchunks, uint8_t* d_dst, uint64_t dst_len);

/* ---- LZ4 chunks inflated on the device ------------------------------------
 * The same for LZ4 (raw blocks, the codec of ORC's LZ4 files). A block does
 * not state its decompressed length: the plan walks its sequence tokens
 * (copying nothing) and runs every check of the block there, so a corrupt
 * block fails the plan. The rules are the format's safety rules: a literal
 * lies inside the input and the output, an offset is neither 0 nor past the
 * output so far, a match ends inside the output, the block ends with a literal
 * run. They accept every block a writer produces. liblz4, which the host path
 * calls, differs on crafted blocks in two ways: it may accept a zero offset,
 * and it refuses blocks that break its compressor's end-of-block margins. The
 * table entry is Snappy's; dst_bytes is the walked size. */
#define ORCG_LZ4_STORED 1u
typedef orcg_snappy_chunk orcg_lz4_chunk;

/* out[0] = bytes of decompressed history a chunk keeps on chip (every LZ4
 * offset lies inside it), out[1] = threads per chunk. */
void orcg_lz4_device_info(uint32_t out[2]);
/* As orcg_snappy_plan. The one text of a failing block is "Corrupt lz4
 * compressed block", also when it inflates past min(block_size, 2^31 - 1). */
int orcg_lz4_plan(const uint8_t* src, uint64_t len, uint64_t block_size, orcg_lz4_chunk* table, uint64_t cap,
                  uint64_t* nchunks, uint64_t* total, const char** error);
/* As orcg_snappy_decompress_device. The kernel repeats every check of the
 * plan (the table is not trusted) and that a block ends at dst_bytes exactly:
 * ORCG_PARSE_ERROR "Corrupt lz4 compressed block", orcg_ctx_last_error_value
 * = the lowest failing chunk's index. */
int orcg_lz4_decompress_device(orcg_ctx* ctx, const uint8_t* d_src, uint64_t src_len, const orcg_lz4_chunk* table,
                               uint64_t nchunks, uint8_t* d_dst, uint64_t dst_len);

/* (Roofline calibration copies, orcg_probe_copy, live only in the A/B build
 * liborcgpu_ab.so: orc_amd/csrc/probe_kernels.hip.) */

#ifdef __cplusplus
}
#endif
#endif /* ORCG_H */
