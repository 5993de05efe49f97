// The host stream planners and the seek lookup (orc_amd/csrc/host_plan.hh)
// over truncated and corrupted streams, for the host sanitizers: every stream
// lies in a heap buffer of exactly its length, so a read one past its end is
// caught. Built with host_plan.cpp alone; no HIP.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../orc_amd/csrc/host_plan.hh"

using namespace orcg;

namespace {

typedef orcg_rlev2_plan* (*Planner)(const uint8_t*, uint64_t, uint64_t, uint64_t);
orcg_rlev2_plan* plan_v2(const uint8_t* s, uint64_t n, uint64_t mb, uint64_t mv) { return make_plan(s, n, mb, mv); }
orcg_rlev2_plan* plan_v2_java(const uint8_t* s, uint64_t n, uint64_t mb, uint64_t mv) {
  return make_plan(s, n, mb, mv, 2);
}

struct Format {
  const char* name;
  Planner plan;
  GroupParser parse;
  std::vector<uint8_t> stream;  // short, mixed, whole
};

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

// Plans `bytes` (copied to a buffer of exactly its length) under several cut
// limits, checks the plan's invariants and looks every byte offset up.
void run(const Format& f, const std::vector<uint8_t>& bytes, const char* what, size_t at) {
  const uint64_t len = bytes.size();
  uint8_t* s = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(s, bytes.data(), len);
  const uint64_t limits[][2] = {{16u << 10, 8192}, {1, 1ull << 40}, {1ull << 30, 1}, {7, 5}};
  for (const auto& lim : limits) {
    std::unique_ptr<orcg_rlev2_plan> p(f.plan(s, len, lim[0], lim[1]));
    for (size_t k = 0; k < p->segs.size(); ++k) {
      CHECK(p->segs[k].byte_offset < len, "%s %s %zu: cut %zu at %llu of %llu", f.name, what, at, k,
            (unsigned long long)p->segs[k].byte_offset, (unsigned long long)len);
      if (k)
        CHECK(p->segs[k].byte_offset > p->segs[k - 1].byte_offset && p->segs[k].value_index >= p->segs[k - 1].value_index,
              "%s %s %zu: cut %zu does not ascend", f.name, what, at, k);
    }
    if (!p->segs.empty()) {
      CHECK(p->segs[0].byte_offset == 0 && p->segs[0].value_index == 0, "%s %s %zu: first cut", f.name, what, at);
      CHECK(p->values >= p->segs.back().value_index, "%s %s %zu: values below the last cut", f.name, what, at);
    }
    if (p->err != kErrNone) CHECK(p->err_at <= p->values, "%s %s %zu: err_at past values", f.name, what, at);
    if (p->err == kErrNone && len) CHECK(!p->segs.empty(), "%s %s %zu: a whole stream without a cut", f.name, what, at);
    // every cut is found again at its value index; every other offset gives a
    // value index within the plan or kNotFound
    for (const orcg_segment& g : p->segs)
      CHECK(locate(*p, s, len, g.byte_offset, f.parse) == g.value_index, "%s %s %zu: cut not located", f.name, what, at);
    for (uint64_t rel = 0; rel <= len; ++rel) {
      const uint64_t v = locate(*p, s, len, rel, f.parse);
      CHECK(v == kNotFound || v <= p->values, "%s %s %zu: located past values", f.name, what, at);
    }
    // (the lookup walks by the C++ rules: a stream only Java's accept may not be walked to its end)
    if (p->err == kErrNone && !p->segs.empty() && f.plan != plan_v2_java)
      CHECK(locate(*p, s, len, len, f.parse) == p->values, "%s %s %zu: the stream's end", f.name, what, at);
  }
  free(s);
}

void put(std::vector<uint8_t>& v, std::initializer_list<int> b) {
  for (int x : b) v.push_back((uint8_t)x);
}

std::vector<uint8_t> v2_stream() {
  std::vector<uint8_t> v;
  put(v, {0x0a, 0x27, 0x10});                                      // SHORT_REPEAT: 5 x 10000
  put(v, {0x5e, 0x03, 0x5c, 0xa1, 0xab, 0x1e, 0xde, 0xad, 0xbe, 0xef});  // DIRECT: 4 x 16 bits
  put(v, {0xc6, 0x09, 0x02, 0x02, 0x22, 0x42, 0x42, 0x46});        // DELTA: 10 values, 4-bit deltas
  put(v, {0xc0, 0x04, 0x90, 0x4e, 0x81, 0x01});                    // DELTA: fixed delta, two-byte varints
  // PATCHED_BASE: 20 x 8 bits, a 1-byte base, one patch entry (pw 12 + pgw 2 -> 14 bits)
  put(v, {0x8e, 0x13, 0x0b, 0x21, 0x64});
  for (int i = 0; i < 20; ++i) v.push_back((uint8_t)(i * 7));
  put(v, {0x40, 0x04});
  put(v, {0x12, 0x01, 0x02, 0x03});                                // SHORT_REPEAT of 3 bytes
  put(v, {0x44, 0x07, 0x12, 0x34, 0x56});                          // DIRECT: 8 x 3 bits
  return v;
}

std::vector<uint8_t> v1_stream() {
  std::vector<uint8_t> v;
  put(v, {0x05, 0x01, 0x07});                          // run of 8
  put(v, {0xfc, 0x01, 0xac, 0x02, 0x80, 0x80, 0x01, 0x7f});  // 4 literals of 1 to 3 bytes
  put(v, {0x7f, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0x01});  // run of 130, 9-byte base
  put(v, {0xff, 0x00});                                // 1 literal
  put(v, {0x00, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x00});  // padded base
  put(v, {0xfe, 0x85, 0x01, 0x02});                    // 2 literals
  return v;
}

std::vector<uint8_t> byte_stream() {
  std::vector<uint8_t> v;
  put(v, {0x00, 0x11});                    // run of 3
  put(v, {0xfd, 0x01, 0x02, 0x03});        // 3 literals
  put(v, {0x7f, 0x22});                    // run of 130
  put(v, {0xff, 0x09});                    // 1 literal
  v.push_back(0x80);                       // 128 literals
  for (int i = 0; i < 128; ++i) v.push_back((uint8_t)(i + 1));
  put(v, {0x05, 0x33, 0xfe, 0x44, 0x55});  // run of 8, 2 literals
  return v;
}

}  // namespace

int main() {
  std::vector<Format> formats = {{"rlev2", plan_v2, host_parse_run, v2_stream()},
                                 {"rlev2-java", plan_v2_java, host_parse_run, v2_stream()},
                                 {"rlev1", make_v1_plan, host_parse_v1_group, v1_stream()},
                                 {"byterle", make_byte_plan, host_parse_byte_group, byte_stream()}};
  for (const Format& f : formats) {
    // the stream is whole: the plan has no error and ends at the stream's end
    {
      std::unique_ptr<orcg_rlev2_plan> p(f.plan(f.stream.data(), f.stream.size(), 16u << 10, 8192));
      CHECK(p->err == kErrNone && p->values > 50, "%s: the test stream does not parse", f.name);
    }
    for (size_t cut = 0; cut <= f.stream.size(); ++cut)
      run(f, std::vector<uint8_t>(f.stream.begin(), f.stream.begin() + cut), "cut", cut);
    for (size_t at = 0; at < 64 && at < f.stream.size(); ++at)
      for (int b = 0; b < 256; ++b) {
        if (b == f.stream[at]) continue;
        std::vector<uint8_t> bad = f.stream;
        bad[at] = (uint8_t)b;
        run(f, bad, "corrupt", at);
      }
  }
  if (failures) return 1;
  printf("host plans ok\n");
  return 0;
}
