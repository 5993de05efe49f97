#include "inflate_plan.hh"

#include <algorithm>

namespace orcg {

namespace {
const char* const kPastEof = "Read past EOF in DecompressionStream::readBuffer";
}

bool plan_snappy_chunks(const uint8_t* file, uint64_t file_len, const PlanChunk* chunks, size_t nchunks,
                        uint64_t block_size, uint64_t dst_base, std::vector<orcg_snappy_chunk>& table,
                        uint64_t* total, const char** err) {
  const size_t keep = table.size();
  auto fail = [&](const char* m) {
    table.resize(keep);
    *err = m;
    return false;
  };
  // the kernel's offsets are 32-bit: a larger block size is not taken at its word
  const uint64_t cap = block_size < kSnappyMaxBytes ? block_size : kSnappyMaxBytes - 1;
  uint64_t at = dst_base;
  for (size_t i = 0; i < nchunks; ++i) {
    const PlanChunk& c = chunks[i];
    if (c.src_off > file_len || c.src_len > file_len - c.src_off || c.src_len >= kSnappyMaxBytes) return fail(kPastEof);
    uint64_t ulen = c.src_len;
    if (!c.original) {
      // the preamble, as snappy_decompress reads it
      const uint8_t* p = file + c.src_off;
      const uint8_t* const end = p + c.src_len;
      ulen = 0;
      for (int sh = 0;; sh += 7) {
        if (p >= end || sh > 35) return fail("snappy: bad length");
        const uint8_t b = *p++;
        ulen |= (uint64_t)(b & 0x7f) << sh;
        if (!(b & 0x80)) break;
      }
      if (ulen > cap) return fail("snappy: output exceeds the compression block size");
    }
    if (at + ulen < at) return fail(kPastEof);
    table.push_back({c.src_off, c.src_len, at, ulen, c.original ? (uint64_t)ORCG_SNAPPY_STORED : 0});
    at += ulen;
  }
  *total = at - dst_base;
  return true;
}

namespace {
// [0, len) cut at ORC's 3-byte chunk headers
bool cut_frames(const uint8_t* bytes, uint64_t len, std::vector<PlanChunk>& chunks, const char** err) {
  uint64_t p = 0;
  while (p < len) {
    if (len - p < 3) {
      *err = kPastEof;
      return false;
    }
    const uint32_t h = (uint32_t)bytes[p] | ((uint32_t)bytes[p + 1] << 8) | ((uint32_t)bytes[p + 2] << 16);
    PlanChunk c{p + 3, h >> 1, (h & 1u) != 0};
    if (c.src_len > len - c.src_off) {
      *err = kPastEof;
      return false;
    }
    chunks.push_back(c);
    p = c.src_off + c.src_len;
  }
  return true;
}
}  // namespace

bool plan_snappy_framed(const uint8_t* bytes, uint64_t len, uint64_t block_size,
                        std::vector<orcg_snappy_chunk>& table, uint64_t* total, const char** err) {
  std::vector<PlanChunk> chunks;
  if (!cut_frames(bytes, len, chunks, err)) return false;
  return plan_snappy_chunks(bytes, len, chunks.data(), chunks.size(), block_size, 0, table, total, err);
}

bool lz4_block_size(const uint8_t* in, uint64_t n, uint64_t cap, uint64_t* out_len) {
  uint64_t p = 0, o = 0;  // o <= cap throughout
  // a length's extension bytes; false: the input ended, or the length passed `room`
  auto extend = [&](uint64_t& len, uint64_t room) {
    for (;;) {
      if (p >= n) return false;
      const uint8_t b = in[p++];
      len += b;
      if (len > room) return false;
      if (b != 255) return true;
    }
  };
  for (;;) {
    if (p >= n) return false;
    const uint8_t token = in[p++];
    uint64_t lit = token >> 4;
    if (lit == 15 && !extend(lit, std::min(n - p, cap - o))) return false;
    if (lit > n - p || lit > cap - o) return false;
    p += lit;
    o += lit;
    if (p == n) {
      *out_len = o;
      return true;
    }
    if (n - p < 2) return false;
    const uint32_t off = (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8);
    p += 2;
    uint64_t match = token & 15u;
    if (match == 15 && !extend(match, cap - o)) return false;
    match += 4;
    if (off == 0 || off > o || match > cap - o) return false;
    o += match;
  }
}

bool plan_lz4_chunks(const uint8_t* file, uint64_t file_len, const PlanChunk* chunks, size_t nchunks,
                     uint64_t block_size, uint64_t dst_base, std::vector<orcg_lz4_chunk>& table, uint64_t* total,
                     const char** err) {
  const size_t keep = table.size();
  auto fail = [&](const char* m) {
    table.resize(keep);
    *err = m;
    return false;
  };
  const uint64_t cap = block_size < kSnappyMaxBytes ? block_size : kSnappyMaxBytes - 1;
  uint64_t at = dst_base;
  for (size_t i = 0; i < nchunks; ++i) {
    const PlanChunk& c = chunks[i];
    if (c.src_off > file_len || c.src_len > file_len - c.src_off || c.src_len >= kSnappyMaxBytes) return fail(kPastEof);
    uint64_t ulen = c.src_len;
    if (!c.original && !lz4_block_size(file + c.src_off, c.src_len, cap, &ulen))
      return fail("Corrupt lz4 compressed block");
    if (at + ulen < at) return fail(kPastEof);
    table.push_back({c.src_off, c.src_len, at, ulen, c.original ? (uint64_t)ORCG_LZ4_STORED : 0});
    at += ulen;
  }
  *total = at - dst_base;
  return true;
}

bool plan_lz4_framed(const uint8_t* bytes, uint64_t len, uint64_t block_size, std::vector<orcg_lz4_chunk>& table,
                     uint64_t* total, const char** err) {
  std::vector<PlanChunk> chunks;
  if (!cut_frames(bytes, len, chunks, err)) return false;
  return plan_lz4_chunks(bytes, len, chunks.data(), chunks.size(), block_size, 0, table, total, err);
}

}  // namespace orcg
