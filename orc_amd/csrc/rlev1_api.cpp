// RLEv1 C ABI (orcg_rlev1_*). The plan (host_plan.hh) walks the control bytes
// and varint terminators of a host stream and cuts it into header-aligned
// segments for rlev1_kernel; it decodes no values.
#include "host_decode.hh"

using namespace orcg;

template <typename T>
static int v1_decode_host(orcg_ctx* c, const uint8_t* src, uint64_t len, int is_signed, const char* not_null,
                          uint64_t n, T* dst) {
  if (!c || (len && !src) || (n && !dst)) return ORCG_INVALID_ARGUMENT;
  std::unique_ptr<orcg_rlev2_plan> plan(make_v1_plan(src, len, 16u << 10, 8192));
  return decode_host_rows(c, src, len, *plan, kErrV1BadRead, not_null, n, dst,
                          [=](const uint8_t* d_src, uint64_t l, const uint64_t* d_seg, uint64_t nsegs, uint64_t count,
                              void* d_out) {
                            return launch_rlev1(c, d_src, l, is_signed, d_seg, nsegs, 0, count, d_out, sizeof(T));
                          });
}

extern "C" {

int orcg_rlev1_plan_create(const uint8_t* src, uint64_t len, uint64_t max_bytes, uint64_t max_values,
                           orcg_rlev2_plan** out) {
  if (!out || (len && !src)) return ORCG_INVALID_ARGUMENT;
  *out = make_v1_plan(src, len, max_bytes ? max_bytes : (16u << 10), max_values ? max_values : 8192);
  return ORCG_OK;
}

int orcg_rlev1_decode_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len, int is_signed,
                             const orcg_segment* d_segs, uint64_t nsegs, uint64_t value_begin, uint64_t nvalues,
                             void* d_dst, int dst_bytes) {
  if (!c || (nsegs && (!d_src || !d_segs)) || (nvalues && !d_dst)) return ORCG_INVALID_ARGUMENT;
  hipSetDevice(c->device);
  return launch_rlev1(c, d_src, src_len, is_signed, (const uint64_t*)d_segs, nsegs, value_begin, nvalues, d_dst,
                      dst_bytes);
}

int orcg_rlev1_decode_i64(orcg_ctx* c, const uint8_t* s, uint64_t l, int sg, const char* nn, uint64_t n,
                          int64_t* d) {
  return v1_decode_host(c, s, l, sg, nn, n, d);
}
int orcg_rlev1_decode_i32(orcg_ctx* c, const uint8_t* s, uint64_t l, int sg, const char* nn, uint64_t n,
                          int32_t* d) {
  return v1_decode_host(c, s, l, sg, nn, n, d);
}

}  // extern "C"
