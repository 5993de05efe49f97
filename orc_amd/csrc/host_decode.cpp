// Host-stream decoding shared by the three formats (host_decode.hh).
#include "host_decode.hh"

namespace orcg {

int decode_host_stream(Ctx* c, const uint8_t* src, uint64_t len, const orcg_rlev2_plan& plan, uint64_t count,
                       int width, void* out, const HostLaunch& launch) {
  if (count == 0) return ORCG_OK;
  (void)hipSetDevice(c->device);
  const size_t seg_bytes = plan.segs.size() * sizeof(orcg_segment), out_bytes = count * (size_t)width;
  void *d_src, *d_seg, *d_out;
  // (the kernels read the stream, and byte RLE writes its output, in whole
  // 16-byte words)
  int rc = scratch(c, kScratchStream, len + 16, &d_src);
  if (!rc) rc = scratch(c, kScratchSegments, seg_bytes, &d_seg);
  if (!rc) rc = scratch(c, kScratchDense, out_bytes + 16, &d_out);
  if (rc) return rc;
  rc = hip_check(c, hipMemcpyAsync(d_src, src, len, hipMemcpyHostToDevice, c->stream), "H2D stream");
  if (!rc)
    rc = hip_check(c, hipMemcpyAsync(d_seg, plan.segs.data(), seg_bytes, hipMemcpyHostToDevice, c->stream),
                   "H2D segments");
  if (!rc) rc = launch((const uint8_t*)d_src, len, (const uint64_t*)d_seg, plan.segs.size(), count, d_out);
  if (!rc) rc = hip_check(c, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream), "D2H values");
  if (!rc) rc = sync_ctx(c);
  return rc;
}

uint64_t count_set(const char* nn, uint64_t n) {
  if (!nn) return n;
  uint64_t k = 0;
  for (uint64_t i = 0; i < n; ++i) k += nn[i] ? 1 : 0;
  return k;
}

int HostCursor::load_from(uint64_t from) {
  origin = from;
  cursor = 0;
  const uint8_t* s = src.data() + from;
  const uint64_t len = src.size() - from;
  plan.reset(plan_suffix(s, len));
  const int rc = decode_suffix(s, len);
  return rc ? fail(rc, ctx->last_error) : ORCG_OK;
}

int HostCursor::seek_group(uint64_t byte, uint64_t* vi) {
  *vi = byte >= origin ? locate(*plan, src.data() + origin, src.size() - origin, byte - origin, group) : kNotFound;
  if (*vi != kNotFound) return ORCG_OK;
  *vi = 0;
  return load_from(byte);
}

}  // namespace orcg
