// liborcgpu C ABI for RLEv2 streams: the host run planner's entry points, the
// device and one-shot host decodes and the stateful drop-in decoder for
// orc::RleDecoder (c++/src/RLE.hh:109-163) with its Java vectors. Kernels
// live in rlev2_*.hip.
#include <string.h>

#include "host_decode.hh"

using namespace orcg;

namespace {

// launch_rlev2 (or, under Java's rules, the wave-walk kernel that has them)
// over a staged host stream.
HostLaunch rlev2_launch(Ctx* c, int is_signed, int width, int java = 0) {
  return [=](const uint8_t* d_src, uint64_t len, const uint64_t* d_seg, uint64_t nsegs, uint64_t count, void* d_out) {
    Rlev2Args a{};
    a.src = d_src;
    a.src_len = len;
    a.is_signed = is_signed;
    a.segtab = d_seg;
    a.nsegs = nsegs;
    a.nvalues = count;
    a.dst = d_out;
    a.dst_bytes = width;
    return java ? launch_rlev2_decode(c, a, java) : launch_rlev2(c, a);
  };
}

template <typename T>
int decode_host(orcg_ctx* c, const uint8_t* src, uint64_t len, int is_signed, const char* not_null, uint64_t n,
                T* dst) {
  if (!c || (len && !src) || (n && !dst)) return ORCG_INVALID_ARGUMENT;
  std::unique_ptr<orcg_rlev2_plan> plan(make_plan(src, len, 16u << 10, 8192));
  return decode_host_rows(c, src, len, *plan, kErrBadRead, not_null, n, dst, rlev2_launch(c, is_signed, sizeof(T)));
}

}  // namespace

extern "C" {

// ---- plan ----------------------------------------------------------------
int orcg_rlev2_plan_create(const uint8_t* src, uint64_t len, uint64_t max_bytes, uint64_t max_values,
                           orcg_rlev2_plan** out) {
  if (!out || (len && !src)) return ORCG_INVALID_ARGUMENT;
  *out = make_plan(src, len, max_bytes ? max_bytes : (16u << 10), max_values ? max_values : 8192);
  return ORCG_OK;
}
void orcg_rlev2_plan_destroy(orcg_rlev2_plan* p) { delete p; }
uint64_t orcg_rlev2_plan_values(const orcg_rlev2_plan* p) { return p ? p->values : 0; }
uint64_t orcg_rlev2_plan_segments(const orcg_rlev2_plan* p, const orcg_segment** segs) {
  if (!p) return 0;
  if (segs) *segs = p->segs.data();
  return p->segs.size();
}
int orcg_rlev2_plan_error(const orcg_rlev2_plan* p, uint64_t* at, const char** msg) {
  if (!p || p->err == kErrNone) return ORCG_OK;
  if (at) *at = p->err_at;
  if (msg) *msg = dev_error_message(p->err);
  return dev_error_status(p->err);
}

// ---- device entry points ---------------------------------------------------
int orcg_rlev2_decode_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len, int is_signed,
                             const orcg_segment* d_segs, uint64_t nsegs, uint64_t value_begin,
                             uint64_t nvalues, void* d_dst, int dst_bytes) {
  if (!c || (nsegs && (!d_src || !d_segs)) || (nvalues && !d_dst)) return ORCG_INVALID_ARGUMENT;
  hipSetDevice(c->device);
  Rlev2Args a{};
  a.src = d_src;
  a.src_len = src_len;
  a.is_signed = is_signed;
  a.segtab = (const uint64_t*)d_segs;
  a.nsegs = nsegs;
  a.value_begin = value_begin;
  a.nvalues = nvalues;
  a.dst = d_dst;
  a.dst_bytes = dst_bytes;
  return launch_rlev2(c, a);
}

int orcg_rlev2_decode_positions_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len,
                                       int is_signed, const uint64_t* d_positions, uint64_t ngroups,
                                       uint64_t rows_per_group, uint64_t value_begin,
                                       uint64_t nvalues, void* d_dst, int dst_bytes) {
  if (!c || (ngroups && (!d_src || !d_positions)) || (nvalues && !d_dst) || rows_per_group == 0)
    return ORCG_INVALID_ARGUMENT;
  hipSetDevice(c->device);
  Rlev2Args a{};
  a.src = d_src;
  a.src_len = src_len;
  a.is_signed = is_signed;
  a.segtab = d_positions;
  a.nsegs = ngroups;
  a.positions = true;
  a.rows_per_group = rows_per_group;
  a.value_begin = value_begin;
  a.nvalues = nvalues;
  a.dst = d_dst;
  a.dst_bytes = dst_bytes;
  return launch_rlev2(c, a);
}

// ---- host-buffer decode ----------------------------------------------------
int orcg_rlev2_decode_i64(orcg_ctx* c, const uint8_t* s, uint64_t l, int sg, const char* nn, uint64_t n,
                          int64_t* d) {
  return decode_host(c, s, l, sg, nn, n, d);
}
int orcg_rlev2_decode_i32(orcg_ctx* c, const uint8_t* s, uint64_t l, int sg, const char* nn, uint64_t n,
                          int32_t* d) {
  return decode_host(c, s, l, sg, nn, n, d);
}
int orcg_rlev2_decode_i16(orcg_ctx* c, const uint8_t* s, uint64_t l, int sg, const char* nn, uint64_t n,
                          int16_t* d) {
  return decode_host(c, s, l, sg, nn, n, d);
}

// IntegerColumnReader<LongVectorBatch>::next over a whole stripe column
// (ColumnReader.cc:81-104, 224-258): PRESENT (boolean RLE, may be absent)
// and DATA (RLEv2) host streams -> not_null[n] (1 = value present) and
// data[n]; null slots of `data` are left untouched.
int orcg_decode_integer_column(orcg_ctx* c, const uint8_t* present, uint64_t present_len, const uint8_t* data,
                               uint64_t data_len, int is_signed, uint64_t n, int64_t* out, char* not_null) {
  if (!c || (n && !out) || (data_len && !data) || (present_len && !present)) return ORCG_INVALID_ARGUMENT;
  std::vector<char> nn;
  if (present && present_len) {
    orcg_byte_rle_decoder* pd = nullptr;
    int rc = orcg_byte_rle_decoder_create(c, present, present_len, 1, &pd);
    if (rc) return rc;
    std::unique_ptr<orcg_byte_rle_decoder, void (*)(orcg_byte_rle_decoder*)> guard(pd, orcg_byte_rle_decoder_destroy);
    nn.assign(n, 0);
    if (n && (rc = orcg_byte_rle_decoder_next(pd, nn.data(), n, nullptr)))
      return set_error(c, rc, orcg_byte_rle_decoder_last_error(pd));
    if (not_null) memcpy(not_null, nn.data(), n);
  } else if (not_null) {
    memset(not_null, 1, n);
  }
  const char* mask = nn.empty() ? nullptr : nn.data();
  std::unique_ptr<orcg_rlev2_plan> plan(make_plan(data, data_len, 16u << 10, 8192));
  return decode_host_rows(c, data, data_len, *plan, kErrBadRead, mask, n, out, rlev2_launch(c, is_signed, 8));
}

}  // extern "C"

// ---- stateful decoder ----------------------------------------------------------
struct orcg_rle_decoder : HostCursor {
  int is_signed = 0;
  int java = 0;  // Java's RunLengthIntegerReaderV2 rules (launch_rlev2_decode `java`)
  std::vector<int64_t> values;  // dense decoded values from `origin`

  orcg_rle_decoder() : HostCursor(host_parse_run) {}
  orcg_rlev2_plan* plan_suffix(const uint8_t* s, uint64_t len) const override {
    return make_plan(s, len, 16u << 10, 8192, java);
  }
  int decode_suffix(const uint8_t* s, uint64_t len) override {
    values.assign(plan->values, 0);
    return decode_host_stream(ctx, s, len, *plan, plan->values, 8, values.data(),
                              rlev2_launch(ctx, is_signed, 8, java));
  }
  int need(uint64_t k) {
    if (cursor + k <= values.size()) return ORCG_OK;
    const uint32_t e = plan->err != kErrNone ? plan->err : (uint32_t)kErrBadRead;
    return fail(dev_error_status(e), dev_error_message(e));
  }
  template <typename T>
  int next(T* data, uint64_t n, const char* nn) {
    if (n && !data) return fail(ORCG_INVALID_ARGUMENT, "null data");
    // values up to the failing run are delivered before the error, like the
    // reference's partially filled batch
    const uint64_t k = count_set(nn, n), avail = std::min<uint64_t>(k, values.size() - cursor);
    place_dense(data, values.data() + cursor, nn, n, avail);
    cursor += avail;
    return need(k - avail);
  }
  // IntegerReader.nextVector's rows: the non-null ones decoded, null slots 1
  template <typename T>
  int next_java(T* vector, const uint8_t* is_null, uint64_t n) {
    if (!is_null) return next(vector, n, nullptr);
    std::vector<char> nn(n);
    for (uint64_t i = 0; i < n; ++i) nn[i] = is_null[i] ? 0 : 1;
    const int rc = next(vector, n, nn.data());
    if (rc) return rc;
    for (uint64_t i = 0; i < n; ++i)
      if (is_null[i]) vector[i] = 1;
    return ORCG_OK;
  }
};

extern "C" {

int orcg_rle_decoder_create(orcg_ctx* c, const uint8_t* src, uint64_t len, int is_signed,
                            int version, orcg_rle_decoder** out) {
  return create_decoder(c, src, len, out, [&](orcg_rle_decoder& d) {
    d.is_signed = is_signed;
    return version == 2 ? ORCG_OK
                        : set_error(c, ORCG_INVALID_ARGUMENT, "only RleVersion_2 streams decode on the GPU");
  });
}

// new RunLengthIntegerReaderV2(input, signed, skipCorrupt)
// (java/core/src/java/org/apache/orc/impl/RunLengthIntegerReaderV2.java:47-52)
int orcg_rle_decoder_create_java(orcg_ctx* c, const uint8_t* src, uint64_t len, int is_signed, int skip_corrupt,
                                 orcg_rle_decoder** out) {
  return create_decoder(c, src, len, out, [&](orcg_rle_decoder& d) {
    d.is_signed = is_signed;
    d.java = skip_corrupt ? 2 : 1;
    return ORCG_OK;
  });
}

void orcg_rle_decoder_destroy(orcg_rle_decoder* d) { delete d; }

int orcg_rle_decoder_next_i64(orcg_rle_decoder* d, int64_t* data, uint64_t n, const char* nn) {
  return d ? d->next(data, n, nn) : ORCG_INVALID_ARGUMENT;
}
int orcg_rle_decoder_next_i32(orcg_rle_decoder* d, int32_t* data, uint64_t n, const char* nn) {
  return d ? d->next(data, n, nn) : ORCG_INVALID_ARGUMENT;
}
int orcg_rle_decoder_next_i16(orcg_rle_decoder* d, int16_t* data, uint64_t n, const char* nn) {
  return d ? d->next(data, n, nn) : ORCG_INVALID_ARGUMENT;
}

int orcg_rle_decoder_skip(orcg_rle_decoder* d, uint64_t n) {
  if (!d) return ORCG_INVALID_ARGUMENT;
  const uint64_t avail = std::min<uint64_t>(n, d->values.size() - d->cursor);
  d->cursor += avail;
  return d->need(n - avail);
}

int orcg_rle_decoder_seek(orcg_rle_decoder* d, const uint64_t* pos, uint64_t npos) {
  if (!d) return ORCG_INVALID_ARGUMENT;
  if (!pos || npos < 2) return d->fail(ORCG_INVALID_ARGUMENT, "uncompressed RLE position needs 2 values");
  if (pos[0] > d->src.size()) return d->fail(ORCG_INVALID_ARGUMENT, "Seek past end of stream");
  const int rc = d->seek_group(pos[0], &d->cursor);
  return rc ? rc : orcg_rle_decoder_skip(d, pos[1]);
}

int orcg_rle_decoder_next_vector_java(orcg_rle_decoder* d, int64_t* vector, const uint8_t* is_null,
                                      uint64_t n, int* is_repeating) {
  if (!d || (n && !vector) || !is_repeating) return ORCG_INVALID_ARGUMENT;
  // RunLengthIntegerReaderV2.nextVector (RunLengthIntegerReaderV2.java:371-396)
  if (*is_repeating && is_null && n > 0 && is_null[0]) return ORCG_OK;
  const int rc = d->next_java(vector, is_null, n);
  if (rc) return rc;
  bool rep = true;
  for (uint64_t i = 1; i < n && rep; ++i)
    rep = vector[0] == vector[i] && (!is_null || is_null[0] == is_null[i]);
  *is_repeating = rep ? 1 : 0;
  return ORCG_OK;
}

int orcg_rle_decoder_next_vector_java_int(orcg_rle_decoder* d, int32_t* vector, const uint8_t* is_null, uint64_t n,
                                          int is_repeating) {
  if (!d || (n && !vector)) return ORCG_INVALID_ARGUMENT;
  // RunLengthIntegerReaderV2.nextVector(ColumnVector, int[], int)
  // (RunLengthIntegerReaderV2.java:399-411): (int) narrowing, null slots 1,
  // an all-null repeating vector is left alone, isRepeating is not computed
  if (is_null && is_repeating && n > 0 && is_null[0]) return ORCG_OK;
  return d->next_java(vector, is_null, n);
}

const char* orcg_rle_decoder_last_error(const orcg_rle_decoder* d) {
  return d ? d->last_error.c_str() : "";
}

}  // extern "C"
