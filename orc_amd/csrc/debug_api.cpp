// Test hooks of the C ABI (orcg_debug_*): launchers the suite drives directly.
#include <vector>

#include "orcg_internal.hh"

// Test hook (tests/test_gpu_scan.py): the reader's exclusive scan of int64
// values, d_out[0..n] (n + 1 entries), on the context's stream.
extern "C" int orcg_debug_exclusive_scan(orcg_ctx* c, const int64_t* d_in, uint64_t n, int64_t* d_out) {
  if (!c || (n && !d_in) || !d_out) return ORCG_INVALID_ARGUMENT;
  hipSetDevice(c->device);
  return orcg::launch_exclusive_scan(c, d_in, n, d_out);
}

// Test hook: the next look-back launch on this context uses epoch `e` + 1
// (tests/test_gpu_scan.py runs across the 16-bit epoch wrap in a few launches).
extern "C" int orcg_debug_set_lb_epoch(orcg_ctx* c, uint32_t e) {
  if (!c || e > 0xffffu) return ORCG_INVALID_ARGUMENT;
  c->lb_epoch = e;
  return ORCG_OK;
}

// Test hook (tests/test_gpu_column_shapes.py): the same scan with its
// StringDirect checks, d_flags2[0] |= a negative input, d_flags2[1] |= the
// running total wrapped, and *d_total = d_out[n] (either may be null).
extern "C" int orcg_debug_exclusive_scan_flags(orcg_ctx* c, const int64_t* d_in, uint64_t n, int64_t* d_out,
                                               uint64_t* d_flags2, uint64_t* d_total) {
  if (!c || (n && !d_in) || !d_out) return ORCG_INVALID_ARGUMENT;
  hipSetDevice(c->device);
  return orcg::launch_exclusive_scan(c, d_in, n, d_out, d_flags2, d_total);
}

// Test hook (tests/test_gpu_column_shapes.py): the stripe's batched
// dictionary launch. A job is DictJob's caller-filled fields, every pointer a
// device pointer; err = null reports into the context's error record.
struct orcg_debug_dict_job {
  const int64_t* lengths;
  uint64_t dict_size;
  int64_t* offsets;
  uint64_t* summary;
  const int64_t* idx;
  const uint8_t* nn;
  uint64_t n;
  int64_t* start;
  int64_t* len;
  unsigned long long* err;
};

extern "C" int orcg_debug_dict_multi(orcg_ctx* c, const orcg_debug_dict_job* jobs, uint32_t njobs) {
  if (!c || (njobs && !jobs)) return ORCG_INVALID_ARGUMENT;
  std::vector<orcg::DictJob> js(njobs);
  for (uint32_t j = 0; j < njobs; ++j) {
    const orcg_debug_dict_job& s = jobs[j];
    if ((s.dict_size && !s.lengths) || !s.offsets || !s.summary || (s.n && (!s.idx || !s.start || !s.len)))
      return ORCG_INVALID_ARGUMENT;
    js[j] = orcg::DictJob{s.lengths, s.dict_size, s.offsets, s.summary, s.idx, s.nn,
                          s.n,       s.start,     s.len,     s.err ? s.err : c->d_err, 0};
  }
  hipSetDevice(c->device);
  return orcg::launch_dict_multi(c, js.data(), njobs);
}

// Test hook (tests/test_gpu_column_shapes.py): a masked row-index stream's
// prefix (G + 1) and segment table (G pairs), by the fused look-back launch or
// by the count + scan + table launches (the counts go to kScratchMisc).
extern "C" int orcg_debug_rg_segments(orcg_ctx* c, const uint8_t* d_mask, uint64_t n, const int64_t* d_rows,
                                      uint64_t G, const int64_t* d_trip, int boolean, int fused, int64_t* d_prefix,
                                      uint64_t* d_seg) {
  if (!c || (n && !d_mask) || (G && (!d_rows || !d_trip || !d_prefix || !d_seg))) return ORCG_INVALID_ARGUMENT;
  hipSetDevice(c->device);
  if (fused) return orcg::launch_rg_prefix_segtab(c, d_mask, n, d_rows, G, d_trip, boolean != 0, d_prefix, d_seg);
  void* counts = nullptr;
  int rc = orcg::scratch(c, orcg::kScratchMisc, (G + 1) * sizeof(int64_t), &counts);
  if (!rc) rc = orcg::launch_rg_prefix(c, d_mask, n, d_rows, G, (int64_t*)counts, d_prefix);
  return rc ? rc : orcg::launch_rg_segtab(c, d_trip, d_prefix, G, boolean != 0, d_seg);
}

// Test hook (tests/test_gpu_column_shapes.py): a union's tags as decode_union
// runs them: the bad-tag check, then per child the flags, their scan and the
// rows' offsets; d_counts[k] = the rows child k reads (kScratchDense, kScratchColumn).
extern "C" int orcg_debug_union(orcg_ctx* c, const uint8_t* d_tags, uint64_t n, uint32_t nchildren,
                                int64_t* d_offsets, int64_t* d_counts, uint64_t* d_first_bad) {
  if (!c || (n && (!d_tags || !d_offsets)) || (nchildren && !d_counts) || !d_first_bad || nchildren > 256)
    return ORCG_INVALID_ARGUMENT;
  hipSetDevice(c->device);
  void *flags = nullptr, *scan = nullptr;
  int rc = orcg::scratch(c, orcg::kScratchDense, (n + 1) * sizeof(int64_t), &flags);
  if (!rc) rc = orcg::scratch(c, orcg::kScratchColumn, (n + 1) * sizeof(int64_t), &scan);
  if (!rc) rc = orcg::launch_union_check(c, d_tags, n, nchildren, d_first_bad);
  for (uint32_t k = 0; !rc && k < nchildren; ++k) {
    if ((rc = orcg::launch_union_flags(c, d_tags, n, k, (int64_t*)flags)) ||
        (rc = orcg::launch_exclusive_scan(c, (const int64_t*)flags, n, (int64_t*)scan)) ||
        (rc = orcg::launch_union_offsets(c, d_tags, n, k, (const int64_t*)scan, d_offsets)))
      break;
    rc = orcg::hip_check(c, hipMemcpyAsync(d_counts + k, (const int64_t*)scan + n, sizeof(int64_t),
                                           hipMemcpyDeviceToDevice, c->stream), "union count copy");
  }
  return rc;
}
