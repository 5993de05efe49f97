// The LZ4 size walk and chunk planner (orc_amd/csrc/inflate_plan.hh) over
// truncated and corrupted input, for the host sanitizers: every stream lies in
// a heap buffer of exactly its length, so a read one past its end is caught.
// Every chunk the plan accepts is then decoded by a plain decoder that follows
// the walk, into a buffer of exactly dst_bytes: it must fill it and leave
// neither buffer. Built with inflate_plan.cpp alone; no HIP.
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

typedef std::vector<uint8_t> Bytes;

void frame(Bytes& out, const Bytes& body, bool original) {
  const uint32_t h = ((uint32_t)body.size() << 1) | (original ? 1u : 0u);
  out.push_back((uint8_t)h);
  out.push_back((uint8_t)(h >> 8));
  out.push_back((uint8_t)(h >> 16));
  out.insert(out.end(), body.begin(), body.end());
}

void length(Bytes& b, uint32_t v) {  // the extension bytes of a nibble of 15
  for (v -= 15; v >= 255; v -= 255) b.push_back(255);
  b.push_back((uint8_t)v);
}

// One sequence: `lit` literal bytes, then (match > 0) a match; match == 0 ends the block.
void sequence(Bytes& b, uint32_t lit, uint32_t match, uint32_t off) {
  const uint32_t ml = match ? match - 4 : 0;
  b.push_back((uint8_t)(((lit < 15 ? lit : 15) << 4) | (ml < 15 ? ml : 15)));
  if (lit >= 15) length(b, lit);
  for (uint32_t i = 0; i < lit; ++i) b.push_back((uint8_t)('a' + i % 26));
  if (!match) return;
  b.push_back((uint8_t)off);
  b.push_back((uint8_t)(off >> 8));
  if (ml >= 15) length(b, ml);
}

// The decoder the walk implies, with no check of its own beyond an assert-like
// count of steps outside the buffers (which the walk's acceptance rules out):
// in[0, n) -> out[0, want). Returns the bytes produced.
uint64_t decode(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t want, int* outside) {
  uint64_t p = 0, o = 0;
  for (;;) {
    if (p >= n) return ++*outside, o;
    const uint8_t token = in[p++];
    uint64_t lit = token >> 4;
    if (lit == 15) {
      uint8_t b;
      do {
        if (p >= n) return ++*outside, o;
        lit += b = in[p++];
      } while (b == 255);
    }
    if (lit > n - p || lit > want - o) return ++*outside, o;
    memcpy(out + o, in + p, lit);
    p += lit;
    o += lit;
    if (p == n) return o;
    if (n - p < 2) return ++*outside, o;
    const uint32_t off = in[p] | (in[p + 1] << 8);
    p += 2;
    uint64_t ml = token & 15;
    if (ml == 15) {
      uint8_t b;
      do {
        if (p >= n) return ++*outside, o;
        ml += b = in[p++];
      } while (b == 255);
    }
    ml += 4;
    if (off == 0 || off > o || ml > want - o) return ++*outside, o;
    for (uint64_t i = 0; i < ml; ++i) out[o + i] = out[o + i - off];
    o += ml;
  }
}

const char* const kTexts[] = {"Corrupt lz4 compressed block", "Read past EOF in DecompressionStream::readBuffer"};

// Plans `bytes` (copied to a buffer of exactly its length) under several
// block sizes, checks the table's invariants and decodes what it accepts.
void run(const Bytes& bytes, const char* what, size_t at) {
  const uint64_t len = bytes.size();
  uint8_t* s = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(s, bytes.data(), len);
  for (uint64_t bs : {(uint64_t)0, (uint64_t)20, (uint64_t)300, (uint64_t)1 << 18, ~(uint64_t)0}) {
    const uint64_t cap = bs < ((uint64_t)1 << 31) ? bs : ((uint64_t)1 << 31) - 1;
    std::vector<orcg_lz4_chunk> table(1);  // an entry of the caller's stays
    table[0].flags = 77;
    uint64_t total = ~0ull;
    const char* err = nullptr;
    const bool ok = plan_lz4_framed(s, len, bs, table, &total, &err);
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
      const orcg_lz4_chunk& c = table[k];
      CHECK(c.src_offset == src + 3, "%s %zu: chunk %zu source", what, at, k);
      CHECK(c.src_offset <= len && c.src_bytes <= len - c.src_offset, "%s %zu: chunk %zu outside", what, at, k);
      CHECK(c.dst_offset == dst, "%s %zu: chunk %zu destination", what, at, k);
      CHECK((c.flags & ~(uint64_t)ORCG_LZ4_STORED) == 0, "%s %zu: chunk %zu flags", what, at, k);
      src = c.src_offset + c.src_bytes;
      dst += c.dst_bytes;
      if (c.flags & ORCG_LZ4_STORED) {
        CHECK(c.dst_bytes == c.src_bytes, "%s %zu: stored chunk %zu", what, at, k);
        continue;
      }
      CHECK(c.dst_bytes <= cap && c.src_bytes >= 1, "%s %zu: chunk %zu size", what, at, k);
      if (c.src_offset > len || c.src_bytes > len - c.src_offset || c.dst_bytes > ((uint64_t)1 << 24)) continue;
      // the walk accepted it: the decoder fills exactly dst_bytes from a buffer of exactly src_bytes
      uint8_t* in = (uint8_t*)malloc(c.src_bytes ? c.src_bytes : 1);
      memcpy(in, s + c.src_offset, c.src_bytes);
      uint8_t* out = (uint8_t*)malloc(c.dst_bytes ? c.dst_bytes : 1);
      int outside = 0;
      const uint64_t made = decode(in, c.src_bytes, out, c.dst_bytes, &outside);
      CHECK(made == c.dst_bytes && outside == 0, "%s %zu: chunk %zu decodes to %llu of %llu bytes", what, at, k,
            (unsigned long long)made, (unsigned long long)c.dst_bytes);
      uint64_t again = ~0ull;
      CHECK(lz4_block_size(in, c.src_bytes, c.dst_bytes, &again) && again == c.dst_bytes,
            "%s %zu: chunk %zu walks the same under its own size", what, at, k);
      if (c.dst_bytes)
        CHECK(!lz4_block_size(in, c.src_bytes, c.dst_bytes - 1, &again), "%s %zu: chunk %zu under a smaller cap", what,
              at, k);
      free(out);
      free(in);
    }
    CHECK(src == len && total == dst, "%s %zu: the table covers the input", what, at);
  }
  // the chunk-list entry point with chunks that lie about the file
  const PlanChunk lies[] = {{len, 1, false}, {len + 1, 0, true}, {0, len + 1, false}, {~0ull, 2, false},
                            {1, ~0ull, true}, {len / 2, len - len / 2, false}, {len, 0, false}};
  for (const PlanChunk& c : lies) {
    std::vector<orcg_lz4_chunk> table;
    uint64_t total = 0;
    const char* err = nullptr;
    if (plan_lz4_chunks(s, len, &c, 1, 1 << 18, 0, table, &total, &err))
      CHECK(table.size() == 1 && table[0].src_offset + table[0].src_bytes <= len, "%s %zu: a lying chunk", what, at);
    else
      CHECK(err && table.empty(), "%s %zu: a lying chunk's error", what, at);
  }
  free(s);
}

}  // namespace

int main() {
  // compressed (literals, an overlapping and an extended match, an extended literal), stored, empty stored,
  // the one-byte block, a literal-only block
  Bytes a, b, c, stream;
  sequence(a, 12, 7, 3);
  sequence(a, 0, 40, 19);
  sequence(a, 20, 4, 1);
  sequence(a, 5, 0, 0);
  sequence(b, 30, 300, 30);
  sequence(b, 0, 0, 0);
  sequence(c, 9, 0, 0);
  frame(stream, a, false);
  frame(stream, {'s', 't', 'o', 'r', 'e', 'd'}, true);
  frame(stream, {}, true);
  frame(stream, b, false);
  frame(stream, {0x00}, false);
  frame(stream, c, false);
  {
    std::vector<orcg_lz4_chunk> t;
    uint64_t total = 0;
    const char* err = nullptr;
    CHECK(plan_lz4_framed(stream.data(), stream.size(), 330, t, &total, &err), "the whole stream plans");
    CHECK(t.size() == 6 && total == 88 + 6 + 0 + 330 + 0 + 9, "chunks %zu total %llu", t.size(),
          (unsigned long long)total);
    CHECK(!plan_lz4_framed(stream.data(), stream.size(), 329, t, &total, &err) && !strcmp(err, kTexts[0]),
          "a block size below a block");
    CHECK(t.size() == 6, "a failed plan appends nothing");
  }
  for (size_t cut = 0; cut <= stream.size(); ++cut)
    run(Bytes(stream.begin(), stream.begin() + cut), "truncation", cut);
  for (size_t at = 0; at < stream.size(); ++at)
    for (int v = 0; v < 256; ++v) {
      if ((uint8_t)v == stream[at]) continue;
      Bytes m = stream;
      m[at] = (uint8_t)v;
      run(m, "corruption", at);
    }
  // length runs: all 0xFF to the end, a run that passes 2^31, a run ended past the capacity
  for (size_t ff : {(size_t)1, (size_t)300, (size_t)70000}) {
    for (uint8_t token : {(uint8_t)0xF0, (uint8_t)0x0F}) {
      Bytes body;
      if (token == 0x0F) sequence(body, 4, 4, 1);
      body.push_back(token);
      if (token == 0x0F) body.push_back(1), body.push_back(0);
      body.insert(body.end(), ff, 0xFF);
      Bytes f1, f2;
      frame(f1, body, false);
      run(f1, "run to the end", ff);
      body.push_back(0);
      body.push_back(0);
      frame(f2, body, false);
      run(f2, "run ended", ff);
    }
  }
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("lz4 plans ok\n");
  return 0;
}
