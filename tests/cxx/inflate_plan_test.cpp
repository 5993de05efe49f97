// The Snappy chunk planner (orc_amd/csrc/inflate_plan.hh) over truncated and
// corrupted input, for the host sanitizers: every stream lies in a heap buffer
// of exactly its length, so a read one past its end is caught. Built with
// inflate_plan.cpp alone; no HIP.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../orc_amd/csrc/inflate_plan.hh"

using namespace orcg;

namespace {

int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      ++failures;                              \
      fprintf(stderr, "FAILED %s: ", #cond);   \
      fprintf(stderr, __VA_ARGS__);            \
      fprintf(stderr, "\n");                   \
    }                                          \
  } while (0)

void frame(std::vector<uint8_t>& out, const std::vector<uint8_t>& body, bool original) {
  const uint32_t h = ((uint32_t)body.size() << 1) | (original ? 1u : 0u);
  out.push_back((uint8_t)h);
  out.push_back((uint8_t)(h >> 8));
  out.push_back((uint8_t)(h >> 16));
  out.insert(out.end(), body.begin(), body.end());
}

// A raw block: the preamble varint of `ulen`, then one literal of n bytes.
std::vector<uint8_t> block(uint64_t ulen, uint32_t n) {
  std::vector<uint8_t> b;
  for (; ulen >= 0x80; ulen >>= 7) b.push_back((uint8_t)(ulen | 0x80));
  b.push_back((uint8_t)ulen);
  b.push_back((uint8_t)((n - 1) << 2));
  for (uint32_t i = 0; i < n; ++i) b.push_back((uint8_t)('a' + i % 26));
  return b;
}

const char* const kTexts[] = {"snappy: bad length", "snappy: output exceeds the compression block size",
                              "Read past EOF in DecompressionStream::readBuffer"};

// Plans `bytes` (copied to a buffer of exactly its length) under several
// block sizes and checks the table's invariants.
void run(const std::vector<uint8_t>& bytes, const char* what, size_t at) {
  const uint64_t len = bytes.size();
  uint8_t* s = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(s, bytes.data(), len);
  for (uint64_t bs : {(uint64_t)0, (uint64_t)20, (uint64_t)300, (uint64_t)1 << 18, ~(uint64_t)0}) {
    std::vector<orcg_snappy_chunk> table(1);  // an entry of the caller's stays
    table[0].flags = 77;
    uint64_t total = ~0ull;
    const char* err = nullptr;
    const bool ok = plan_snappy_framed(s, len, bs, table, &total, &err);
    CHECK(table.size() >= 1 && table[0].flags == 77, "%s %zu: the caller's entry", what, at);
    if (!ok) {
      bool known = false;
      for (const char* t : kTexts) known = known || (err && !strcmp(err, t));
      CHECK(known, "%s %zu: text %s", what, at, err ? err : "(null)");
      CHECK(table.size() == 1, "%s %zu: a failed plan left %zu entries", what, at, table.size());
      continue;
    }
    uint64_t src = 0, dst = 0;
    for (size_t k = 1; k < table.size(); ++k) {
      const orcg_snappy_chunk& c = table[k];
      CHECK(c.src_offset == src + 3, "%s %zu: chunk %zu source", what, at, k);
      CHECK(c.src_offset <= len && c.src_bytes <= len - c.src_offset, "%s %zu: chunk %zu outside", what, at, k);
      CHECK(c.dst_offset == dst, "%s %zu: chunk %zu destination", what, at, k);
      if (c.flags & ORCG_SNAPPY_STORED) CHECK(c.dst_bytes == c.src_bytes, "%s %zu: stored chunk %zu", what, at, k);
      else CHECK(c.dst_bytes <= bs && c.src_bytes >= 1, "%s %zu: chunk %zu size", what, at, k);
      CHECK((c.flags & ~(uint64_t)ORCG_SNAPPY_STORED) == 0, "%s %zu: chunk %zu flags", what, at, k);
      src = c.src_offset + c.src_bytes;
      dst += c.dst_bytes;
    }
    CHECK(src == len && total == dst, "%s %zu: the table covers the input", what, at);
  }
  // the chunk-list entry point with chunks that lie about the file
  const PlanChunk lies[] = {{len, 1, false}, {len + 1, 0, true}, {0, len + 1, false}, {~0ull, 2, false},
                            {1, ~0ull, true}, {len / 2, len - len / 2, false}};
  for (const PlanChunk& c : lies) {
    std::vector<orcg_snappy_chunk> table;
    uint64_t total = 0;
    const char* err = nullptr;
    if (plan_snappy_chunks(s, len, &c, 1, 1 << 18, 0, table, &total, &err))
      CHECK(table.size() == 1 && table[0].src_offset + table[0].src_bytes <= len, "%s %zu: a lying chunk", what, at);
    else
      CHECK(err && table.empty(), "%s %zu: a lying chunk's error", what, at);
  }
  free(s);
}

}  // namespace

int main() {
  // compressed, stored, empty stored, a two-byte preamble, a compressed chunk of one byte
  std::vector<uint8_t> stream;
  frame(stream, block(12, 12), false);
  frame(stream, {'s', 't', 'o', 'r', 'e', 'd'}, true);
  frame(stream, {}, true);
  frame(stream, block(200, 30), false);
  frame(stream, {0x05}, false);
  {
    std::vector<orcg_snappy_chunk> t;
    uint64_t total = 0;
    const char* err = nullptr;
    CHECK(plan_snappy_framed(stream.data(), stream.size(), 256, t, &total, &err), "the whole stream plans");
    CHECK(t.size() == 5 && total == 12 + 6 + 0 + 200 + 5, "chunks %zu total %llu", t.size(), (unsigned long long)total);
    CHECK(!plan_snappy_framed(stream.data(), stream.size(), 199, t, &total, &err) && !strcmp(err, kTexts[1]),
          "a block size below a preamble");
    CHECK(t.size() == 5, "a failed plan appends nothing");
  }
  for (size_t cut = 0; cut <= stream.size(); ++cut)
    run(std::vector<uint8_t>(stream.begin(), stream.begin() + cut), "truncation", cut);
  for (size_t at = 0; at < stream.size(); ++at)
    for (int v = 0; v < 256; ++v) {
      if ((uint8_t)v == stream[at]) continue;
      std::vector<uint8_t> b = stream;
      b[at] = (uint8_t)v;
      run(b, "corruption", at);
    }
  // preambles: five continuation bytes, a sixth, the largest value
  for (std::vector<uint8_t> pre : {std::vector<uint8_t>{0x80, 0x80, 0x80, 0x80, 0x80},
                                   std::vector<uint8_t>{0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x01},
                                   std::vector<uint8_t>{0xff, 0xff, 0xff, 0xff, 0xff, 0x7f},
                                   std::vector<uint8_t>{0xff, 0xff, 0xff, 0xff, 0xff, 0xff}}) {
    std::vector<uint8_t> b;
    frame(b, pre, false);
    run(b, "preamble", pre.size());
  }
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("inflate plans ok\n");
  return 0;
}
