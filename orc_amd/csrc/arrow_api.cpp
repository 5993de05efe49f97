// Column-level C entries of the Arrow export (include/orcg_arrow.h): each runs
// one kernel family of arrow_kernels.hip on device arrays the caller owns, so
// the kernels are tested without a file. Synchronous.
#include "arrow_internal.hh"

using namespace orcg;
using namespace orcg::arrow;

namespace {

// The entries' small device block (kScratchNotNull): [0] the export's error
// word, [1] a null count, [2] a scan total.
struct Block {
  unsigned long long* d = nullptr;
  unsigned long long h[3] = {kNoError, 0, 0};
};

int block_init(Ctx* c, Block* b) {
  void* p;
  int rc = scratch(c, kScratchNotNull, sizeof b->h, &p);
  if (rc) return rc;
  b->d = (unsigned long long*)p;
  return hip_check(c, hipMemcpyAsync(b->d, b->h, sizeof b->h, hipMemcpyHostToDevice, c->stream), "H2D export block");
}

// wait for the stream, then the block's words
int block_read(Ctx* c, Block* b) {
  int rc = sync_ctx(c);
  if (rc) return rc;
  return hip_check(c, hipMemcpy(b->h, b->d, sizeof b->h, hipMemcpyDeviceToHost), "D2H export block");
}

int block_error(Ctx* c, const Block& b) {
  if (b.h[0] == kNoError) return ORCG_OK;
  c->last_error_value = b.h[0] >> 8;
  if ((b.h[0] & 0xff) == kArrowDictIndex)
    return set_error(c, ORCG_PARSE_ERROR, "Entry index out of range in StringDictionaryColumn");
  return set_error(c, ORCG_INVALID_ARGUMENT, "offsets do not fit int32 (the last offset is above 2^31 - 1)");
}

// masked row lengths -> int64 scan (scratch 2, 4) -> *scan (n + 1), total in block[2]
int scan_rows(Ctx* c, const int64_t* d_lengths, const int64_t* d_index, const int64_t* d_dict_offsets,
              uint64_t dict_size, const uint8_t* d_nn, uint64_t n, Block& b, int64_t** scan) {
  void *lens = nullptr, *sc = nullptr;
  int rc = scratch(c, kScratchDense, 8 * std::max<uint64_t>(n, 1), &lens);
  if (!rc) rc = scratch(c, kScratchColumn, 8 * (n + 1), &sc);
  if (!rc) rc = launch_row_lengths(c, d_lengths, d_index, d_dict_offsets, dict_size, d_nn, n, (int64_t*)lens, b.d);
  if (!rc) rc = launch_exclusive_scan(c, (const int64_t*)lens, n, (int64_t*)sc, nullptr, (uint64_t*)(b.d + 2));
  *scan = (int64_t*)sc;
  return rc;
}

}  // namespace

extern "C" {

int orcg_arrow_validity_device(orcg_ctx* c, const uint8_t* d_not_null, uint64_t n, uint8_t* d_bitmap,
                               uint64_t bitmap_bytes, uint64_t* null_count) {
  if (!c || !null_count) return ORCG_INVALID_ARGUMENT;
  *null_count = 0;
  if (!d_not_null || n == 0) return ORCG_OK;  // no mask: no validity buffer
  (void)hipSetDevice(c->device);
  Block b;
  int rc = block_init(c, &b);
  if (!rc) rc = launch_validity(c, d_not_null, n, d_bitmap, bitmap_bytes, b.d + 1);
  if (!rc) rc = block_read(c, &b);
  if (rc) return rc;
  *null_count = b.h[1];
  return ORCG_OK;
}

int orcg_arrow_fixed_device(orcg_ctx* c, int form, const void* d_src, const void* d_src2, uint64_t n, void* d_out,
                            uint64_t out_bytes) {
  if (!c) return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  const int rc = launch_fixed(c, form, d_src, d_src2, n, d_out, out_bytes);
  return rc ? rc : sync_ctx(c);
}

int orcg_arrow_offsets_device(orcg_ctx* c, const int64_t* d_offsets64, const int64_t* d_lengths,
                              const uint8_t* d_not_null, uint64_t n, int32_t* d_out, uint64_t out_bytes) {
  if (!c || (!d_offsets64 && n && !d_lengths)) return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  Block b;
  int rc = block_init(c, &b);
  const int64_t* src = d_offsets64;
  if (!rc && !src) {
    int64_t* scan = nullptr;
    rc = scan_rows(c, d_lengths, nullptr, nullptr, 0, d_not_null, n, b, &scan);
    src = scan;
  }
  if (!rc) rc = launch_narrow_offsets(c, src, n + 1, d_out, out_bytes, b.d);
  if (!rc) rc = block_read(c, &b);
  return rc ? rc : block_error(c, b);
}

int orcg_arrow_dict_strings_device(orcg_ctx* c, int dictionary, const int64_t* d_index, const uint8_t* d_not_null,
                                   uint64_t n, const int64_t* d_dict_offsets, uint64_t dict_size,
                                   const uint8_t* d_blob, uint64_t blob_len, int32_t* d_out, uint64_t out_bytes,
                                   void* d_data, uint64_t data_cap, uint64_t* data_bytes) {
  if (!c || !data_bytes || !d_dict_offsets || (n && !d_index)) return ORCG_INVALID_ARGUMENT;
  *data_bytes = 0;
  (void)hipSetDevice(c->device);
  Block b;
  int rc = block_init(c, &b);
  if (rc) return rc;
  if (dictionary) {
    *data_bytes = 4 * (dict_size + 1);
    if (data_cap < padded(*data_bytes))
      return set_error(c, ORCG_INVALID_ARGUMENT, "the dictionary offsets buffer is too small");
    rc = launch_fixed(c, ORCG_ARROW_INT32, d_index, nullptr, n, d_out, out_bytes);
    if (!rc) rc = launch_narrow_offsets(c, d_dict_offsets, dict_size + 1, (int32_t*)d_data, padded(*data_bytes), b.d);
    if (!rc) rc = block_read(c, &b);
    return rc ? rc : block_error(c, b);
  }
  int64_t* scan = nullptr;
  rc = scan_rows(c, nullptr, d_index, d_dict_offsets, dict_size, d_not_null, n, b, &scan);
  if (!rc) rc = launch_narrow_offsets(c, scan, n + 1, d_out, out_bytes, b.d);
  if (!rc) rc = block_read(c, &b);
  if (!rc) rc = block_error(c, b);
  if (rc) return rc;
  *data_bytes = b.h[2];
  if (!d_data) return ORCG_OK;  // the size was asked for
  if (data_cap < padded(b.h[2])) return set_error(c, ORCG_INVALID_ARGUMENT, "the string data buffer is too small");
  rc = launch_dict_gather_bytes(c, d_out, d_index, n, d_dict_offsets, dict_size, d_blob, blob_len, (uint8_t*)d_data,
                                b.h[2], padded(b.h[2]));
  return rc ? rc : sync_ctx(c);
}

// Measurement helper (no reference counterpart; scripts/ab_arrow.py): `iters`
// timed launches of one kernel, HIP events around the launch alone (the
// kernels read their inputs only, so every launch sees the same arrays).
int orcg_arrow_bench(orcg_ctx* c, int kind, int form, const void* p0, const void* p1, const void* p2, const void* p3,
                     uint64_t n, uint64_t dict_size, uint64_t blob_len, void* d_out, uint64_t out_bytes,
                     uint64_t total, uint32_t iters, double* ms_out) {
  if (!c || !ms_out || !n || !d_out) return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  Block b;
  int rc = block_init(c, &b);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!rc) rc = hip_check(c, hipEventCreate(&e0), "hipEventCreate");
  if (!rc) rc = hip_check(c, hipEventCreate(&e1), "hipEventCreate");
  for (uint32_t i = 0; i < iters && !rc; ++i) {
    rc = hip_check(c, hipEventRecord(e0, c->stream), "hipEventRecord");
    if (rc) break;
    switch (kind) {
      case ORCG_ARROW_BENCH_VALIDITY:
        rc = launch_validity(c, (const uint8_t*)p0, n, (uint8_t*)d_out, out_bytes, b.d + 1);
        break;
      case ORCG_ARROW_BENCH_FIXED: rc = launch_fixed(c, form, p0, p1, n, d_out, out_bytes); break;
      case ORCG_ARROW_BENCH_GATHER:
        rc = launch_dict_gather_bytes(c, (const int32_t*)p0, (const int64_t*)p1, n, (const int64_t*)p2, dict_size,
                                      (const uint8_t*)p3, blob_len, (uint8_t*)d_out, total, out_bytes);
        break;
      default: rc = set_error(c, ORCG_INVALID_ARGUMENT, "unknown Arrow bench kind");
    }
    if (!rc) rc = hip_check(c, hipEventRecord(e1, c->stream), "hipEventRecord");
    if (!rc) rc = sync_ctx(c);
    float ms = 0;
    if (!rc) rc = hip_check(c, hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    ms_out[i] = ms;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

}  // extern "C"
