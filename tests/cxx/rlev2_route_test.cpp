// The RLEv2 launch routing (orc_amd/csrc/rlev2_route.hh): the density rule at
// its edges, the segments-per-CU test, the two-pass shape and its addressing
// limits, and the grouping of multi-stream launches. Built with
// rlev2_route.cpp alone; no HIP.
//   rlev2_route_test           the checks; prints "rlev2 routes ok"
//   rlev2_route_test streams   stdin: "src_len values nsegs" a line; stdout:
//                              "instance bound spg slice" a line (the grouped
//                              density class, seg_value_bound and its shape),
//                              for tests/test_cxx_rlev2_route.py
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../orc_amd/csrc/rlev2_route.hh"

using namespace orcg;

namespace {

int failures = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      ++failures;                            \
      fprintf(stderr, "FAILED %s: ", #cond); \
      fprintf(stderr, __VA_ARGS__);          \
      fprintf(stderr, "\n");                 \
    }                                        \
  } while (0)

constexpr int kCus = 256;

int single(uint64_t src_len, uint64_t values, uint64_t nsegs = 1, int pinned = 0) {
  return route_rlev2(Rlev2Route{src_len, values, nsegs, kCus, pinned, false});
}
int grouped(uint64_t src_len, uint64_t values, uint64_t nsegs = 1, int pinned = 0) {
  return route_rlev2(Rlev2Route{src_len, values, nsegs, kCus, pinned, true});
}

void ids() {
  CHECK(kRlev2Default == 0 && kRlev2WaveWalk == 1 && kRlev2Wide == 2 && kRlev2SerialDrain == 3 && kRlev2Dense8 == 4 &&
            kRlev2Dense12 == 5 && kRlev2UnionTwoPass == 6 && kRlev2WideDrain == 7 && kRlev2UnionOnePass == 8 &&
            kRlev2WideNoFlat == 9 && kRlev2WideFlat8 == 10 && kMaxRlev2Variant == 10 && kRlev2FirstTiled == 2,
        "the public numbers");
  for (int v = -2; v <= 12; ++v) {
    CHECK(rlev2_variant_valid(v) == (v >= 0 && v <= 10), "valid %d", v);
    CHECK(rlev2_multi_capable(v) == (v == 0 || (v >= 2 && v <= 10)), "multi %d", v);
  }
}

void density() {
  // 5 B/value and 1.25 B/value, at equality and one off
  CHECK(single(5, 1) == 2 && grouped(5, 1) == 2, "5 B/value");
  CHECK(single(4, 1) == 3 && grouped(4, 1) == 3, "just under 5 B/value");
  CHECK(single(5, 4) == 3 && grouped(5, 4) == 3, "1.25 B/value");
  CHECK(single(4, 4) == 6 && grouped(4, 4) == 6, "1 B/value");
  CHECK(single(4999, 4000) == 6 && single(5000, 4000) == 3, "1.25 B/value, scaled");
  // 8.1 B/value: single streams only
  CHECK(single(81, 10) == 2, "8.1 B/value stays");
  CHECK(single(82, 10) == 6, "8.2 B/value: two passes");
  CHECK(grouped(81, 10) == 2 && grouped(82, 10) == 2, "grouped: no 8.1 rule");
  CHECK(single(800390626ull, 100000000ull, 12208) == 2, "512-value W=64 runs: the serial walk");
  CHECK(grouped(800390626ull, 100000000ull, 12208) == 2, "the same, grouped");
  // segments per CU: 12 x 256
  CHECK(single(100, 1000, 3072) == 6 && single(100, 1000, 3073) == 8, "12 segments per CU");
  CHECK(union_variant(3072, kCus) == 6 && union_variant(3073, kCus) == 8 && union_variant(0, kCus) == 6, "union_variant");
  CHECK(union_variant(12, 1) == 6 && union_variant(13, 1) == 8, "one CU");
  CHECK(single(8200, 1000, 3072) == 6 && single(8200, 1000, 3073) == 6, "the 8.1 rule skips the segment test");
  CHECK(grouped(100, 1000, 3073) == 6, "a job's class: the segment test is its group's");
  // a pin is a pin
  for (int v = 1; v <= 10; ++v) {
    CHECK(single(100, 1000, 3073, v) == v && single(8200, 1000, 1, v) == v, "pinned %d", v);
    CHECK(grouped(100, 1000, 3073, v) == v, "pinned %d, grouped", v);
  }
}

void shapes() {
  const struct {
    uint64_t bound;
    uint32_t spg, slice;
  } want[] = {{0, 1, 256},     {1, 1, 256},      {256, 1, 256},       {257, 1, 512},       {1024, 1, 1024},
              {1025, 2, 768},  {2048, 2, 1024},  {2049, 3, 768},      {262144, 256, 1024}, {262145, 256, 1024},
              {8950, 9, 1024}, {30512, 30, 1024}, {~0ull >> 1, 256, 1024}};
  for (const auto& w : want) {
    uint32_t spg = 0, slice = 0;
    two_pass_shape(w.bound, &spg, &slice);
    CHECK(spg == w.spg && slice == w.slice, "shape of %" PRIu64 ": (%u, %u)", w.bound, spg, slice);
    CHECK(slice % 256 == 0 && slice <= kSliceMax && spg >= 1 && spg <= 256, "shape limits of %" PRIu64, w.bound);
  }
  CHECK(seg_value_bound(80000, 3) == 30512 && seg_value_bound(30001, 4) == 8950, "seg_value_bound");
  CHECK(seg_value_bound(8, 1) == 8 + 1 + 512 && seg_value_bound(9, 2) == 5 + 512, "rounding");
}

void addressing() {
  CHECK(kTabEntryLim == 0xffff0000ull && kTabSegLim == 0x7fff0000ull && kTabSliceLim == 0x7fffffffull, "the limits");
  CHECK(!two_pass_fits(10, 10, 0), "no shape: one pass");
  CHECK(two_pass_fits(0xfffeffffull, 1, 1) && !two_pass_fits(0xffff0000ull, 1, 1), "run-table entries");
  CHECK(two_pass_fits(1, 0x7ffffffeull, 1) && !two_pass_fits(1, 0x7fffffffull, 1), "slices, one a segment");
  CHECK(two_pass_fits(1, 0x7fffffull, 256) && !two_pass_fits(1, 0x800000ull, 256), "slices, 256 a segment");
  // a single stream: its bytes and segments too
  TwoPass t = stream_two_pass(0xfffeffffull, 1, 1000);
  CHECK(t.spg == 1 && t.slice == 1024 && t.entries == 0xfffeffffull / 2 + 2, "the longest stream");
  t = stream_two_pass(0xffff0000ull, 1, 1000);
  CHECK(t.spg == 0 && t.slice == 0, "a stream too long");
  t = stream_two_pass(100, 0x7ffeffffull, 1000);
  CHECK(t.spg == 1 && t.entries == 50 + 0x7ffeffffull + 1, "the most segments");
  t = stream_two_pass(100, 0x7fff0000ull, 1000);
  CHECK(t.spg == 0, "too many segments");
  t = stream_two_pass(100, 0x7fffffull, 262144);
  CHECK(t.spg == 256 && t.slice == 1024, "the most slices");
  t = stream_two_pass(100, 0x800000ull, 262144);
  CHECK(t.spg == 0, "too many slices");
  t = stream_two_pass(20, 3, 8950);
  CHECK(t.entries == 14 && t.spg == 9 && t.slice == 1024, "a small stream");
}

RleJob job(uintptr_t tag, uint64_t src_len, uint64_t nvalues, uint64_t nsegs) {
  RleJob j{};
  j.dst = (void*)tag;
  j.src_len = src_len;
  j.nvalues = nvalues;
  j.nsegs = nsegs;
  j.seg_base = 99;
  j.tab_base = 99;
  return j;
}
std::vector<uintptr_t> tags(const Rlev2Group& g) {
  std::vector<uintptr_t> t;
  for (const RleJob& j : g.jobs) t.push_back((uintptr_t)j.dst);
  return t;
}

void grouping() {
  CHECK(group_rlev2_jobs(nullptr, 0, 0, kCus).empty(), "no jobs");
  const std::vector<RleJob> jobs = {
      job(0, 1000, 1000, 4),   // 1 B/value: union
      job(1, 0, 0, 0),         // empty
      job(2, 8000, 1000, 2),   // wide
      job(3, 2000, 1000, 3),   // serial + drain
      job(4, 500, 1000, 0),    // no segments
      job(5, 500, 500, 5),     // union, the density of job 0: stays behind it
      job(6, 1100, 1000, 1),   // union, denser: first
      job(7, 9000, 1000, 7),   // wide, denser than job 2: first (no 8.1 rule in a group)
      job(8, 500, 0, 3),       // no values
      job(9, 3000, 3000, 2),   // union, the density of jobs 0 and 5
  };
  for (size_t j = 0; j < jobs.size(); ++j) {
    const int want[] = {6, -1, 2, 3, -1, 6, 6, 2, -1, 6};
    CHECK(rlev2_job_instance(jobs[j], 0, kCus) == want[j], "job %zu", j);
    CHECK(rlev2_job_instance(jobs[j], 4, kCus) == (want[j] < 0 ? -1 : 4), "job %zu, pinned", j);
  }
  std::vector<Rlev2Group> gs = group_rlev2_jobs(jobs.data(), (uint32_t)jobs.size(), 0, kCus);
  CHECK(gs.size() == 3, "%zu groups", gs.size());
  if (gs.size() == 3) {
    CHECK(gs[0].variant == 2 && gs[0].launch_variant == 2 && tags(gs[0]) == (std::vector<uintptr_t>{7, 2}), "wide");
    CHECK(gs[0].segs == 9 && gs[0].values == 2000 && gs[0].spg == 0 && gs[0].slice == 0, "wide totals");
    CHECK(gs[0].jobs[0].seg_base == 0 && gs[0].jobs[1].seg_base == 7, "wide seg_base");
    CHECK(gs[0].jobs[0].tab_base == 0 && gs[0].jobs[1].tab_base == 4500 + 7 + 1, "wide tab_base");
    CHECK(gs[1].variant == 3 && gs[1].launch_variant == 3 && tags(gs[1]) == (std::vector<uintptr_t>{3}), "serial");
    CHECK(gs[1].jobs[0].seg_base == 0 && gs[1].jobs[0].tab_base == 0 && gs[1].segs == 3, "serial bases");
    const Rlev2Group& u = gs[2];
    CHECK(u.variant == 6 && u.launch_variant == 6 && tags(u) == (std::vector<uintptr_t>{6, 0, 5, 9}), "union order");
    uint64_t segs = 0, entries = 0, bound = 0;
    for (const RleJob& j : u.jobs) {
      CHECK(j.seg_base == segs && j.tab_base == entries, "prefix sums at job %zu", (size_t)(uintptr_t)j.dst);
      segs += j.nsegs;
      entries += j.src_len / 2 + j.nsegs + 1;
      if (seg_value_bound(j.nvalues, j.nsegs) > bound) bound = seg_value_bound(j.nvalues, j.nsegs);
    }
    CHECK(u.segs == segs && segs == 12 && u.entries == entries && u.values == 5500, "union totals");
    CHECK(u.bound == bound && bound == 1500 + 187 + 512, "union bound %" PRIu64, u.bound);
    CHECK(u.spg == 3 && u.slice == 768, "union shape (%u, %u)", u.spg, u.slice);
  }
  // a pinned variant: every job in that one group, launched as pinned
  for (int pin = 2; pin <= 10; ++pin) {
    gs = group_rlev2_jobs(jobs.data(), (uint32_t)jobs.size(), pin, kCus);
    CHECK(gs.size() == 1 && gs[0].variant == pin && gs[0].launch_variant == pin, "pinned %d", pin);
    if (gs.size() != 1) continue;
    CHECK(tags(gs[0]) == (std::vector<uintptr_t>{7, 2, 3, 6, 0, 5, 9}), "pinned %d: one order", pin);
    CHECK(gs[0].segs == 24 && gs[0].values == 8500, "pinned %d: totals", pin);
    CHECK((gs[0].spg != 0) == (pin == 6) && (gs[0].slice != 0) == (pin == 6), "pinned %d: shape", pin);
  }
  CHECK(group_rlev2_jobs(jobs.data(), (uint32_t)jobs.size(), 1, kCus).empty(), "the wave walk takes no job tables");
  // the union group's passes go by its total segments; a pinned 6 stays 6
  std::vector<RleJob> many = {job(0, 100, 1000, 3000), job(1, 100, 1000, 72)};
  gs = group_rlev2_jobs(many.data(), 2, 0, kCus);
  CHECK(gs.size() == 1 && gs[0].segs == 3072 && gs[0].launch_variant == 6 && gs[0].spg == 1, "3,072 segments");
  many[1].nsegs = 73;
  gs = group_rlev2_jobs(many.data(), 2, 0, kCus);
  CHECK(gs.size() == 1 && gs[0].variant == 6 && gs[0].launch_variant == 8 && gs[0].spg == 0, "3,073 segments");
  gs = group_rlev2_jobs(many.data(), 2, 6, kCus);
  CHECK(gs.size() == 1 && gs[0].launch_variant == 6 && gs[0].spg == 1 && gs[0].slice == 768, "3,073 segments, pinned");
  // tab_base saturates; a group past the entry limit is not shaped
  const uint64_t big = 1ull << 33;
  std::vector<RleJob> huge = {job(0, big, big, 1), job(1, big, big, 1), job(2, big, big, 1)};
  gs = group_rlev2_jobs(huge.data(), 3, 6, kCus);
  CHECK(gs.size() == 1 && gs[0].entries == 3 * ((1ull << 32) + 2), "huge entries");
  if (gs.size() == 1) {
    CHECK(gs[0].jobs[0].tab_base == 0 && gs[0].jobs[1].tab_base == 0xffffffffu && gs[0].jobs[2].tab_base == 0xffffffffu,
          "tab_base saturates");
    CHECK(gs[0].launch_variant == 6 && gs[0].spg == 0 && gs[0].slice == 0, "too many entries: no shape");
  }
  // the entry limit of a group, at its edge: entries = src_len / 2 + nsegs + 1
  std::vector<RleJob> edge = {job(0, 2 * (0xffff0000ull - 3), 1ull << 40, 1)};
  gs = group_rlev2_jobs(edge.data(), 1, 6, kCus);
  CHECK(gs.size() == 1 && gs[0].entries == 0xfffeffffull && gs[0].spg == 256, "the last shaped group");
  edge[0].src_len += 2;
  gs = group_rlev2_jobs(edge.data(), 1, 6, kCus);
  CHECK(gs.size() == 1 && gs[0].entries == 0xffff0000ull && gs[0].spg == 0, "the first unshaped group");
}

int streams() {
  uint64_t src_len, values, nsegs;
  while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &src_len, &values, &nsegs) == 3) {
    const uint64_t bound = seg_value_bound(values, nsegs);
    uint32_t spg = 0, slice = 0;
    two_pass_shape(bound, &spg, &slice);
    printf("%d %" PRIu64 " %u %u\n", route_rlev2(Rlev2Route{src_len, values, nsegs, kCus, 0, true}), bound, spg, slice);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "streams")) return streams();
  ids();
  density();
  shapes();
  addressing();
  grouping();
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("rlev2 routes ok\n");
  return 0;
}
