// Decoding host streams, shared by the RLEv2, RLEv1 and byte RLE C ABI: the
// round trip through device scratch, not-null placement, and the cursor under
// the stateful decoders.
#pragma once

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "orcg_internal.hh"

namespace orcg {

// Enqueues a format's decode of the first `count` values of a staged stream.
using HostLaunch = std::function<int(const uint8_t* d_src, uint64_t len, const uint64_t* d_segs, uint64_t nsegs,
                                     uint64_t count, void* d_out)>;
// The host round trip: stream and segments to scratch, `launch`, the first
// `count` elements of `width` bytes back to host `out`, and the sync that
// collects device errors. count == 0: nothing is launched.
int decode_host_stream(Ctx* c, const uint8_t* src, uint64_t len, const orcg_rlev2_plan& plan, uint64_t count,
                       int width, void* out, const HostLaunch& launch);

// The set bytes of not_null[0..n); n without a mask.
uint64_t count_set(const char* nn, uint64_t n);

// Dense values into the set rows of dst[0..n) (every row without a mask),
// until `limit` are placed; returns how many. Null slots passed on the way
// stay untouched, or get 0 (zero_nulls: BooleanRleDecoderImpl::next).
template <typename T, typename Dense>
uint64_t place_dense(T* dst, const Dense& dense, const char* nn, uint64_t n, uint64_t limit = ~0ull,
                     bool zero_nulls = false) {
  uint64_t j = 0;
  for (uint64_t i = 0; i < n && j < limit; ++i) {
    if (nn && !nn[i]) {
      if (zero_nulls) dst[i] = 0;
      continue;
    }
    dst[i] = (T)dense[j++];
  }
  return j;
}

// One-shot decode of n rows of a planned stream: the set rows' values, decoded
// dense and placed. More set rows than the plan holds fail with the plan's
// error, or `eof` where the stream just ends.
template <typename T>
int decode_host_rows(Ctx* c, const uint8_t* src, uint64_t len, const orcg_rlev2_plan& plan, uint32_t eof,
                     const char* nn, uint64_t n, T* dst, const HostLaunch& launch) {
  const uint64_t k = count_set(nn, n);
  if (k > plan.values) {
    const uint32_t e = plan.err != kErrNone ? plan.err : eof;
    return set_error(c, dev_error_status(e), dev_error_message(e));
  }
  if (!nn) return decode_host_stream(c, src, len, plan, k, sizeof(T), dst, launch);
  std::vector<T> dense(k);
  const int rc = decode_host_stream(c, src, len, plan, k, sizeof(T), dense.data(), launch);
  if (!rc) place_dense(dst, dense.data(), nn, n);
  return rc;
}

// What the stateful decoders share: the stream, the decoding of its suffix
// from `origin` (planned and decoded whole on the GPU) and a cursor into it.
struct HostCursor {
  Ctx* ctx = nullptr;
  std::vector<uint8_t> src;
  std::unique_ptr<orcg_rlev2_plan> plan;
  uint64_t origin = 0;  // stream byte offset the decoded values start at
  uint64_t cursor = 0;
  std::string last_error;
  const GroupParser group;  // the format's group parser (seeks walk headers with it)

  explicit HostCursor(GroupParser g) : group(g) {}
  virtual ~HostCursor() = default;
  int fail(int status, const std::string& m) {
    last_error = m;
    return status;
  }
  // format hooks: plan a stream suffix; decode all plan->values values of it
  virtual orcg_rlev2_plan* plan_suffix(const uint8_t* s, uint64_t len) const = 0;
  virtual int decode_suffix(const uint8_t* s, uint64_t len) = 0;
  // (Re)decode the stream suffix starting at byte `from`.
  int load_from(uint64_t from);
  // *vi = the value index of the group that starts at stream byte `byte`, if
  // it is a group start of the current decoding; else the stream is decoded
  // again from that byte and *vi = 0.
  int seek_group(uint64_t byte, uint64_t* vi);
};

// The *_decoder_create* entry points: a decoder over a copy of the stream,
// set up by `init` (a status) and decoded from byte 0.
template <typename D, typename Init>
int create_decoder(orcg_ctx* c, const uint8_t* src, uint64_t len, D** out, Init init) {
  if (!c || !out || (len && !src)) return ORCG_INVALID_ARGUMENT;
  *out = nullptr;
  std::unique_ptr<D> d(new D());
  d->ctx = c;
  d->src.assign(src, src + len);
  int rc = init(*d);
  if (!rc && (rc = d->load_from(0))) c->last_error = d->last_error;
  if (!rc) *out = d.release();
  return rc;
}

}  // namespace orcg
