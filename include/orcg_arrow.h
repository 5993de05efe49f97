/*
 * orcg_arrow.h — a decoded stripe as Arrow arrays (Arrow C Data / C Device
 * Data interface), laid out on the device by the kernels of arrow_kernels.hip.
 *
 * The reader's batches (include/orcg_reader.h) are the reference's widest
 * layout: int64 for every integer, double for float, a byte of validity per
 * row, [hi, lo] decimals, two arrays per timestamp, (start, length) strings.
 * The export re-lays them in HBM into the Arrow form pyarrow's ORC reader
 * gives for the same file (python/pyarrow/_orc.pyx over the ORC C++ adapter):
 *
 *   boolean                          bool (bitmap)
 *   tinyint / smallint / int / bigint  int8 / int16 / int32 / int64
 *   float / double                   float32 / float64
 *   date                             date32[day]
 *   timestamp                        timestamp[ns]
 *   timestamp with local time zone   timestamp[ns, UTC]
 *   decimal(p, s)                    decimal128(p, s); precision 0 (Hive 0.11):
 *                                    decimal128(38, orcg_reader_hive11_scale())
 *   string / varchar / char          string (int32 offsets)   [char: see DESIGN.md 3.10]
 *   binary                           binary
 *   list / map                       list<item: T> / map<K, V> (int32 offsets)
 *   struct                           struct, field names from the file
 *   union                            not exported (ORCG_INVALID_ARGUMENT)
 *
 * Every buffer the export lays out is 64-byte aligned and zero padded to a
 * multiple of 64 bytes; bitmaps are LSB first. `offset` is always 0.
 */
#ifndef ORCG_ARROW_H
#define ORCG_ARROW_H

#include "orcg_reader.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ABI-stable structures of the Arrow specification (format/
 * CDataInterface.rst, format/CDeviceDataInterface.rst), under its guards. */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE

#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4

struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};

struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};

#endif /* ARROW_C_DATA_INTERFACE */

#ifndef ARROW_C_DEVICE_DATA_INTERFACE
#define ARROW_C_DEVICE_DATA_INTERFACE

typedef int32_t ArrowDeviceType;

#define ARROW_DEVICE_CPU 1
#define ARROW_DEVICE_CUDA 2
#define ARROW_DEVICE_CUDA_HOST 3
#define ARROW_DEVICE_OPENCL 4
#define ARROW_DEVICE_VULKAN 7
#define ARROW_DEVICE_METAL 8
#define ARROW_DEVICE_VPI 9
#define ARROW_DEVICE_ROCM 10
#define ARROW_DEVICE_ROCM_HOST 11
#define ARROW_DEVICE_EXT_DEV 12
#define ARROW_DEVICE_CUDA_MANAGED 13
#define ARROW_DEVICE_ONEAPI 14
#define ARROW_DEVICE_WEBGPU 15
#define ARROW_DEVICE_HEXAGON 16

struct ArrowDeviceArray {
  struct ArrowArray array;
  int64_t device_id;
  ArrowDeviceType device_type;
  void* sync_event;
  int64_t reserved[3];
};

#endif /* ARROW_C_DEVICE_DATA_INTERFACE */

/* Bytes of an exported buffer holding `bytes` of payload (64-byte padding). */
#define ORCG_ARROW_PADDED(bytes) (((uint64_t)(bytes) + 63u) & ~(uint64_t)63u)

/* ---- Column-level entries: one kernel family each, on device arrays the
 * caller owns (no file needed). Synchronous on the context's stream. Output
 * buffers are `*_bytes` long, which must be ORCG_ARROW_PADDED of the payload;
 * the padding is zeroed. ---- */

/* not_null bytes [n] -> LSB-first bitmap and the null count. d_not_null NULL
 * (a column without a mask): nothing is written, *null_count = 0 (the Arrow
 * array then carries no validity buffer). */
int orcg_arrow_validity_device(orcg_ctx* ctx, const uint8_t* d_not_null, uint64_t n, uint8_t* d_bitmap,
                               uint64_t bitmap_bytes, uint64_t* null_count);

/* Fixed-width forms. d_src2 is the nanosecond array of ORCG_ARROW_TIMESTAMP_NS
 * (NULL otherwise). */
enum {
  ORCG_ARROW_INT8 = 0,    /* int64 -> int8  (the values are already narrowed: a truncating store) */
  ORCG_ARROW_INT16 = 1,   /* int64 -> int16 */
  ORCG_ARROW_INT32 = 2,   /* int64 -> int32 (also date32) */
  ORCG_ARROW_BOOL = 3,    /* int64 -> bitmap, bit = value != 0 */
  ORCG_ARROW_FLOAT32 = 4, /* double holding a float -> float32 */
  ORCG_ARROW_DEC64 = 5,   /* Decimal64 int64 -> 16-byte little-endian, sign-extended */
  ORCG_ARROW_DEC128 = 6,  /* Decimal128 [hi, lo] -> [lo, hi] */
  /* (seconds, nanos) -> seconds * 10^9 + nanos as a wrapping int64 (two's
   * complement, modulo 2^64). The ORC C++ Arrow adapter multiplies in signed
   * int64, undefined past about +-292 years from 1970; here the wrap is
   * defined. */
  ORCG_ARROW_TIMESTAMP_NS = 7
};
int orcg_arrow_fixed_device(orcg_ctx* ctx, int form, const void* d_src, const void* d_src2, uint64_t n, void* d_out,
                            uint64_t out_bytes);

/* int32 offsets [n + 1]: from list / map int64 offsets [n + 1] (d_offsets64),
 * or (d_offsets64 NULL) from a direct string column's lengths [n], the rows
 * whose d_not_null byte is 0 counting 0 (d_not_null NULL: every row set),
 * scanned again with the reader's single-pass int64 scan. A last offset above
 * 2^31 - 1 fails with ORCG_INVALID_ARGUMENT, "... offsets do not fit int32". */
int orcg_arrow_offsets_device(orcg_ctx* ctx, const int64_t* d_offsets64, const int64_t* d_lengths,
                              const uint8_t* d_not_null, uint64_t n, int32_t* d_out, uint64_t out_bytes);

/* A dictionary-encoded string column (index [n], dict_offsets [dict_size + 1]
 * into blob).
 *  dictionary = 0: a materialised string array. d_out: int32 offsets [n + 1]
 *    (null rows are empty); d_data: the rows' bytes, gathered contiguously;
 *    *data_bytes = the bytes gathered. d_data NULL asks for the size: the
 *    offsets are written, *data_bytes is set and nothing is gathered.
 *    Otherwise data_cap must be at least ORCG_ARROW_PADDED(*data_bytes)
 *    (ORCG_INVALID_ARGUMENT if not).
 *  dictionary = 1: an Arrow dictionary<int32, string>. d_out: int32 indices [n]
 *    (the slot of a null row holds what index[] holds, 0 in the reader's
 *    batches); d_data: the dictionary values' int32 offsets [dict_size + 1]
 *    (their data buffer is blob itself); *data_bytes = 4 * (dict_size + 1). */
int orcg_arrow_dict_strings_device(orcg_ctx* ctx, int dictionary, const int64_t* d_index, const uint8_t* d_not_null,
                                   uint64_t n, const int64_t* d_dict_offsets, uint64_t dict_size,
                                   const uint8_t* d_blob, uint64_t blob_len, int32_t* d_out, uint64_t out_bytes,
                                   void* d_data, uint64_t data_cap, uint64_t* data_bytes);

/* Measurement helper (scripts/ab_arrow.py): `iters` launches of one kernel,
 * each timed alone with HIP events into ms_out[iters]. kind VALIDITY: p0 =
 * not_null [n]; FIXED: `form`, p0 / p1 = src / src2; GATHER: p0 = int32 output
 * offsets [n + 1], p1 = index [n], p2 = dict_offsets [dict_size + 1], p3 =
 * blob, total = offsets[n]. out_bytes as for the entry of that kernel. */
enum { ORCG_ARROW_BENCH_VALIDITY = 0, ORCG_ARROW_BENCH_FIXED = 1, ORCG_ARROW_BENCH_GATHER = 2 };
int orcg_arrow_bench(orcg_ctx* ctx, int kind, int form, const void* p0, const void* p1, const void* p2, const void* p3,
                     uint64_t n, uint64_t dict_size, uint64_t blob_len, void* d_out, uint64_t out_bytes,
                     uint64_t total, uint32_t iters, double* ms_out);

/* ---- Reader entries ---- */

/* The Arrow schema the export has: a struct ("+s") of the selected top-level
 * fields (orcg_reader_select), under a read type the read kinds. Host only:
 * works on a reader opened with ctx == NULL. dictionary != 0: a string column
 * that is dictionary-encoded in the stripe last decoded (none, when no stripe
 * was decoded) is reported as dictionary<int32, string>. A selected union
 * column fails: ORCG_INVALID_ARGUMENT, "union column <id> is not exported to
 * Arrow". The caller releases *out (out->release). */
int orcg_reader_arrow_schema(const orcg_reader* r, int dictionary, struct ArrowSchema* out);

/* The stripe last decoded by orcg_reader_read_stripe as one struct array of
 * the selected top-level fields, every buffer a device pointer: device_type
 * ARROW_DEVICE_ROCM, device_id the context's device, sync_event NULL (the
 * call synchronises the context's stream before it returns).
 *
 * Lifetime: the buffers belong to the reader. They stay valid until the
 * reader decodes its next stripe (any read_stripe / read_stripes call, which
 * reuses the stripe's device memory) or is destroyed; release() frees only
 * the export's bookkeeping (the ArrowArray structures), never device memory,
 * and may be called before or after that. The re-laid buffers sit in one
 * contiguous region of the stripe's device arena; buffers that need no
 * re-layout (int64, float64, a direct string column's bytes, a dictionary's
 * bytes) are the decode's own.
 *
 * dictionary != 0: string columns dictionary-encoded in this stripe export as
 * dictionary<int32, string> (index narrowed, the dictionary's offsets narrowed,
 * its bytes not copied) and a DIRECT-encoded stripe of the same column as
 * plain string: use it per stripe, with orcg_reader_arrow_schema(r, 1, ...)
 * taken after the stripe's decode.
 *
 * Errors (ORCG_INVALID_ARGUMENT), the first offending column in column order:
 * a selected union column; a column that was not decoded ("column <id> was
 * not decoded (...)", e.g. a timestamp whose writer zone did not resolve);
 * "column <id>: offsets do not fit int32 (the last offset is above 2^31 - 1)". */
int orcg_reader_export_arrow_device(orcg_reader* r, int dictionary, struct ArrowDeviceArray* out);

/* The same arrays in one host allocation owned by the array (release() frees
 * it): the contiguous device region arrives in one device-to-host copy, the
 * buffers that were not re-laid in one copy each. */
int orcg_reader_export_arrow_host(orcg_reader* r, int dictionary, struct ArrowArray* out);

#ifdef __cplusplus
}
#endif
#endif /* ORCG_ARROW_H */
