// C ABI of the decimal and timestamp value decoders (include/orcg.h):
// device-resident streams, the same kernels the file reader uses
// (decimal_kernels.hip).
#include "orcg_internal.hh"
#include "timezone.hh"

using namespace orcg;

extern "C" {

static int decimal_decode(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len, const int64_t* d_scales,
                          uint64_t nvalues, uint32_t precision, int32_t scale, void* d_out, uint8_t* d_keep) {
  if (!c || (src_len && !d_src) || (nvalues && (!d_scales || !d_out)) || precision > 38)
    return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  const uint64_t ntiles_max = src_len / kVarintTile + 2;
  void *d_counts, *d_base;
  int rc = scratch(c, kScratchTileCounts, ntiles_max * sizeof(int64_t), &d_counts);
  if (!rc) rc = scratch(c, kScratchTileOffsets, (ntiles_max + 1) * sizeof(int64_t), &d_base);
  if (rc) return rc;
  uint64_t ntiles = 0;
  if ((rc = launch_varint_tile_counts(c, d_src, src_len, (int64_t*)d_counts, &ntiles))) return rc;
  uint64_t total = 0;
  if (ntiles) {
    if ((rc = launch_exclusive_scan(c, (const int64_t*)d_counts, ntiles, (int64_t*)d_base))) return rc;
    if ((rc = hip_check(c, hipMemcpyAsync(&total, (int64_t*)d_base + ntiles, 8, hipMemcpyDeviceToHost, c->stream),
                        "D2H varint count")))
      return rc;
    if ((rc = sync_ctx(c))) return rc;
  }
  if (total < nvalues) return set_error(c, ORCG_PARSE_ERROR, "Read past end of stream in Decimal64ColumnReader");
  const int mode = precision == 0 ? (d_keep ? 3 : 2) : (precision > 18 ? 1 : 0);
  if ((rc = launch_varint_decimal(c, d_src, src_len, (const int64_t*)d_base, d_scales, nvalues, scale, mode, d_out,
                                  d_keep)))
    return rc;
  return sync_ctx(c);
}

int orcg_decimal_decode_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len, const int64_t* d_scales,
                               uint64_t nvalues, uint32_t precision, int32_t scale, void* d_out) {
  return decimal_decode(c, d_src, src_len, d_scales, nvalues, precision, scale, d_out, nullptr);
}

int orcg_hive11_decimal_decode_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len, const int64_t* d_scales,
                                      uint64_t nvalues, int32_t scale, int throw_on_overflow, void* d_out,
                                      uint8_t* d_keep) {
  if (!throw_on_overflow && nvalues && !d_keep) return ORCG_INVALID_ARGUMENT;
  return decimal_decode(c, d_src, src_len, d_scales, nvalues, 0, scale, d_out, throw_on_overflow ? nullptr : d_keep);
}

int orcg_timestamp_decode_device(orcg_ctx* c, int64_t* d_seconds, int64_t* d_nanos, uint64_t n, int64_t epoch) {
  if (!c || (n && (!d_seconds || !d_nanos))) return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  const int rc = launch_timestamp(c, d_seconds, d_nanos, n, epoch);
  return rc ? rc : sync_ctx(c);
}

int orcg_timestamp_decode_tz_device(orcg_ctx* c, int64_t* d_seconds, int64_t* d_nanos, uint64_t n,
                                    const orcg_timezone* writer_tz, const orcg_timezone* reader_tz) {
  const tz::Zone *w = tz::zone_of(writer_tz), *r = tz::zone_of(reader_tz);
  if (!c || !w || !r || (n && (!d_seconds || !d_nanos))) return ORCG_INVALID_ARGUMENT;
  // sameTimezone_ (ColumnReader.cc:286): no adjustment, today's kernel
  if (w == r) return orcg_timestamp_decode_device(c, d_seconds, d_nanos, n, w->epoch());
  (void)hipSetDevice(c->device);
  const std::vector<int64_t> wt = w->device_table(), rt = r->device_table();
  int64_t* d_tab = nullptr;
  int rc = hip_check(c, hipMalloc((void**)&d_tab, (wt.size() + rt.size()) * 8), "time zone table allocation");
  if (rc) return rc;
  rc = hip_check(c, hipMemcpy(d_tab, wt.data(), wt.size() * 8, hipMemcpyHostToDevice), "H2D time zone table");
  if (!rc)
    rc = hip_check(c, hipMemcpy(d_tab + wt.size(), rt.data(), rt.size() * 8, hipMemcpyHostToDevice),
                   "H2D time zone table");
  if (!rc)
    rc = launch_timestamp_tz(c, d_seconds, d_nanos, n, TzTable{d_tab, (uint32_t)wt.size()},
                             TzTable{d_tab + wt.size(), (uint32_t)rt.size()});
  if (!rc) rc = sync_ctx(c);
  (void)hipFree(d_tab);
  return rc;
}

// Measurement helper (no reference counterpart; scripts/ab_timestamp_tz.py):
// `iters` timed launches over n values, each on a fresh device copy of the
// inputs (the kernels work in place), HIP events around the launch alone.
// mode 0: timestamp_kernel with the writer zone's epoch (no adjustment, the
// baseline); 1: timestamp_tz_kernel.
int orcg_timestamp_tz_bench(orcg_ctx* c, const int64_t* d_seconds_in, const int64_t* d_nanos_in, int64_t* d_seconds,
                            int64_t* d_nanos, uint64_t n, const orcg_timezone* writer_tz,
                            const orcg_timezone* reader_tz, int mode, uint32_t iters, double* ms_out) {
  const tz::Zone *w = tz::zone_of(writer_tz), *r = tz::zone_of(reader_tz);
  if (!c || !w || !r || !n || !d_seconds_in || !d_nanos_in || !d_seconds || !d_nanos || !ms_out || mode < 0 ||
      mode > 1)
    return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  const std::vector<int64_t> wt = w->device_table(), rt = r->device_table();
  int64_t* d_tab = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = hip_check(c, hipMalloc((void**)&d_tab, (wt.size() + rt.size()) * 8), "time zone table allocation");
  if (!rc) rc = hip_check(c, hipMemcpy(d_tab, wt.data(), wt.size() * 8, hipMemcpyHostToDevice), "H2D zone table");
  if (!rc)
    rc = hip_check(c, hipMemcpy(d_tab + wt.size(), rt.data(), rt.size() * 8, hipMemcpyHostToDevice), "H2D zone table");
  if (!rc) rc = hip_check(c, hipEventCreate(&e0), "hipEventCreate");
  if (!rc) rc = hip_check(c, hipEventCreate(&e1), "hipEventCreate");
  const TzTable wtab{d_tab, (uint32_t)wt.size()}, rtab{d_tab + wt.size(), (uint32_t)rt.size()};
  for (uint32_t i = 0; i < iters && !rc; ++i) {
    rc = hip_check(c, hipMemcpyAsync(d_seconds, d_seconds_in, n * 8, hipMemcpyDeviceToDevice, c->stream), "D2D");
    if (!rc) rc = hip_check(c, hipMemcpyAsync(d_nanos, d_nanos_in, n * 8, hipMemcpyDeviceToDevice, c->stream), "D2D");
    if (!rc) rc = hip_check(c, hipEventRecord(e0, c->stream), "hipEventRecord");
    if (!rc)
      rc = mode == 0 ? launch_timestamp(c, d_seconds, d_nanos, n, w->epoch())
                     : launch_timestamp_tz(c, d_seconds, d_nanos, n, wtab, rtab);
    if (!rc) rc = hip_check(c, hipEventRecord(e1, c->stream), "hipEventRecord");
    if (!rc) rc = sync_ctx(c);
    float ms = 0;
    if (!rc) rc = hip_check(c, hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    ms_out[i] = ms;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_tab) (void)hipFree(d_tab);
  return rc;
}

}  // extern "C"
