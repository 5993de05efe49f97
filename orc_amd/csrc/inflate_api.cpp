// liborcgpu C ABI for Snappy and LZ4 chunks inflated on the device: the plan
// (inflate_plan.hh) and the launch (inflate_kernels.hip).
#include "inflate_plan.hh"
#include "orcg_internal.hh"

using namespace orcg;

namespace {

typedef int (*InflateLaunch)(Ctx*, const uint8_t*, const orcg_snappy_chunk*, uint64_t, uint8_t*, unsigned long long*);

// The argument checks, the table's upload and the synchronous launch of both codecs.
int decompress_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len, const orcg_snappy_chunk* table,
                      uint64_t nchunks, uint8_t* d_dst, uint64_t dst_len, const char* codec, InflateLaunch launch) {
  if (!c || (nchunks && !table) || (src_len && !d_src) || (dst_len && !d_dst)) return ORCG_INVALID_ARGUMENT;
  for (uint64_t i = 0; i < nchunks; ++i) {
    const orcg_snappy_chunk& k = table[i];
    if (k.src_offset > src_len || k.src_bytes > src_len - k.src_offset || k.dst_offset > dst_len ||
        k.dst_bytes > dst_len - k.dst_offset || k.src_bytes >= kSnappyMaxBytes || k.dst_bytes >= kSnappyMaxBytes)
      return set_error(c, ORCG_INVALID_ARGUMENT,
                       std::string(codec) + " chunk " + std::to_string(i) + " lies outside its buffers");
  }
  if (nchunks == 0) return ORCG_OK;
  (void)hipSetDevice(c->device);
  void* d_table = nullptr;
  const size_t bytes = (size_t)nchunks * sizeof(orcg_snappy_chunk);
  int rc = scratch(c, kScratchSegments, bytes, &d_table);
  if (rc) return rc;
  rc = hip_check(c, hipMemcpyAsync(d_table, table, bytes, hipMemcpyHostToDevice, c->stream), "upload chunk table");
  if (rc) return rc;
  // the table is pageable host memory: the copy has left it once the stream is idle (sync_ctx below)
  rc = launch(c, d_src, (const orcg_snappy_chunk*)d_table, nchunks, d_dst, nullptr);
  const int rs = sync_ctx(c);
  return rc ? rc : rs;
}

}  // namespace

extern "C" {

void orcg_snappy_device_info(uint32_t out[2]) {
  if (!out) return;
  out[0] = kSnappyRing;
  out[1] = kSnappyThreads;
}

int orcg_snappy_plan(const uint8_t* src, uint64_t len, uint64_t block_size, orcg_snappy_chunk* table, uint64_t cap,
                     uint64_t* nchunks, uint64_t* total, const char** error) {
  if ((len && !src) || !nchunks || !total) return ORCG_INVALID_ARGUMENT;
  std::vector<orcg_snappy_chunk> t;
  const char* err = "";
  *nchunks = *total = 0;
  if (!plan_snappy_framed(src, len, block_size, t, total, &err)) {
    if (error) *error = err;
    return ORCG_PARSE_ERROR;
  }
  *nchunks = t.size();
  if (table) std::copy(t.begin(), t.begin() + std::min<uint64_t>(cap, t.size()), table);
  return ORCG_OK;
}

int orcg_snappy_decompress_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len,
                                  const orcg_snappy_chunk* table, uint64_t nchunks, uint8_t* d_dst,
                                  uint64_t dst_len) {
  return decompress_device(c, d_src, src_len, table, nchunks, d_dst, dst_len, "snappy", launch_snappy_inflate);
}

void orcg_lz4_device_info(uint32_t out[2]) {
  if (!out) return;
  out[0] = kLz4Ring;
  out[1] = kLz4Threads;
}

int orcg_lz4_plan(const uint8_t* src, uint64_t len, uint64_t block_size, orcg_lz4_chunk* table, uint64_t cap,
                  uint64_t* nchunks, uint64_t* total, const char** error) {
  if ((len && !src) || !nchunks || !total) return ORCG_INVALID_ARGUMENT;
  std::vector<orcg_lz4_chunk> t;
  const char* err = "";
  *nchunks = *total = 0;
  if (!plan_lz4_framed(src, len, block_size, t, total, &err)) {
    if (error) *error = err;
    return ORCG_PARSE_ERROR;
  }
  *nchunks = t.size();
  if (table) std::copy(t.begin(), t.begin() + std::min<uint64_t>(cap, t.size()), table);
  return ORCG_OK;
}

int orcg_lz4_decompress_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len, const orcg_lz4_chunk* table,
                               uint64_t nchunks, uint8_t* d_dst, uint64_t dst_len) {
  return decompress_device(c, d_src, src_len, table, nchunks, d_dst, dst_len, "lz4", launch_lz4_inflate);
}

}  // extern "C"
