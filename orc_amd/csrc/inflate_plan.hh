// The host half of the device Snappy and LZ4 paths (inflate_kernels.hip): a
// stream's chunks laid out without inflating them, Snappy from the preambles,
// LZ4 from a walk over the sequence tokens. Byte walks over untrusted input;
// no HIP (tests/cxx/inflate_plan_test.cpp and lz4_plan_test.cpp build it on
// its own).
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

// ---- LZ4 (raw blocks) --------------------------------------------------------
// The same kernel shape (orcg_lz4_device_info). Every LZ4 offset (<= 65,535)
// lies inside the ring.
constexpr uint32_t kLz4Ring = kSnappyRing;
constexpr uint32_t kLz4Threads = kSnappyThreads;

// The decompressed size of one raw LZ4 block in[0, n), at most cap, without
// copying a byte. These are the decoder's rules in this project (the kernel
// repeats them), per sequence and in this order:
//   - no token left (n == 0 included) fails;
//   - a literal length of 15 is extended by bytes until one is not 255; the
//     input ending inside the extension fails;
//   - the literal lies inside the input, and o + literal <= cap;
//   - the input ending exactly after the literal ends the block, *out_len = o;
//   - fewer than 2 bytes left for the offset fails;
//   - a match length of 15 is extended the same way, then 4 is added;
//   - offset == 0, offset > o and o + match > cap fail;
//   - a length stops accumulating once it exceeds what can still fit
//     (min(n - p, cap - o) for a literal, cap - o for a match): no sum wraps
//     and a lost block's run of 0xFF bytes is not walked to its end.
// False = the host path's "Corrupt lz4 compressed block" (decompress_chunk).
//
// These are the format's safety rules and nothing more. Every block a writer
// produces is accepted, with liblz4's bytes. On crafted blocks liblz4
// (LZ4_decompress_safe, which the host path calls) differs in two ways only:
// 1.9.3 does not check a zero offset (it emits zeros), and it refuses blocks
// that break its compressor's end-of-block margins (a last literal run shorter
// than 5 bytes after a match, a match within 12 bytes of the end), which vary
// by version and with the destination's capacity.
bool lz4_block_size(const uint8_t* in, uint64_t n, uint64_t cap, uint64_t* out_len);

// As the Snappy pair. A compressed chunk's dst_bytes is its walked size under
// cap = min(block_size, 2^31 - 1); a block that fails the walk is "Corrupt lz4
// compressed block".
bool plan_lz4_chunks(const uint8_t* file, uint64_t file_len, const PlanChunk* chunks, size_t nchunks,
                     uint64_t block_size, uint64_t dst_base, std::vector<orcg_lz4_chunk>& table, uint64_t* total,
                     const char** err);
bool plan_lz4_framed(const uint8_t* bytes, uint64_t len, uint64_t block_size, std::vector<orcg_lz4_chunk>& table,
                     uint64_t* total, const char** err);

}  // namespace orcg
