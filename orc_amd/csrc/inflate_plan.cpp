#include "inflate_plan.hh"

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

bool plan_snappy_framed(const uint8_t* bytes, uint64_t len, uint64_t block_size,
                        std::vector<orcg_snappy_chunk>& table, uint64_t* total, const char** err) {
  std::vector<PlanChunk> chunks;
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
  return plan_snappy_chunks(bytes, len, chunks.data(), chunks.size(), block_size, 0, table, total, err);
}

}  // namespace orcg
