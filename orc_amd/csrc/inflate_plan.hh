// The host half of the device Snappy path (inflate_kernels.hip): a stream's
// chunks laid out from their preambles alone. A byte walk over untrusted
// input; no HIP (tests/cxx/inflate_plan_test.cpp builds it on its own).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/orcg.h"

namespace orcg {

// The kernel's shape (orcg_snappy_device_info): bytes of history in LDS and
// threads (one wavefront) per chunk.
constexpr uint32_t kSnappyRing = 65536;
constexpr uint32_t kSnappyThreads = 64;
// A chunk's length field has 23 bits; the kernel's offsets are 32-bit.
constexpr uint64_t kSnappyMaxBytes = 1ull << 31;

// One chunk body in `file`: [src_off, src_off + src_len), stored or compressed.
struct PlanChunk {
  uint64_t src_off, src_len;
  bool original;
};

// The chunks of one stream -> table entries appended to `table`, destinations
// consecutive from dst_base; *total = their decompressed bytes. A compressed
// chunk's preamble varint is read with snappy_decompress's two checks and
// texts (orc_file.cpp); a stored chunk's dst_bytes = src_bytes. A chunk outside
// [0, file_len) is "Read past EOF in DecompressionStream::readBuffer". False:
// err holds the text, the table is as it was.
bool plan_snappy_chunks(const uint8_t* file, uint64_t file_len, const PlanChunk* chunks, size_t nchunks,
                        uint64_t block_size, uint64_t dst_base, std::vector<orcg_snappy_chunk>& table,
                        uint64_t* total, const char** err);

// [0, len) of `bytes` cut at ORC's 3-byte chunk headers (split_chunks,
// orc_file.cpp), then planned as above.
bool plan_snappy_framed(const uint8_t* bytes, uint64_t len, uint64_t block_size,
                        std::vector<orcg_snappy_chunk>& table, uint64_t* total, const char** err);

}  // namespace orcg
