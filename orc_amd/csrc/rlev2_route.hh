// RLEv2 launch routing: which tiled instance a stream or a group of streams
// gets, whether the union instance runs in one pass or two, and how the jobs
// of a multi-stream launch are grouped and ordered. Host arithmetic only:
// nothing here needs HIP (the launcher, rlev2_tiled.cpp, supplies the CU
// count), and tests/cxx/rlev2_route_test.cpp pins every rule and edge under
// the host sanitizers.
#pragma once

#include <stdint.h>

#include <vector>

namespace orcg {

// The instances by their public numbers (ctx->rlev2_variant, include/orcg.h):
// 0 = the density-adaptive default, 1 = the wave-walk kernel
// (rlev2_kernels.hip), kRlev2FirstTiled .. kMaxRlev2Variant pin one tiled
// instance (rlev2_tiled.cpp kInstances holds their parameters; the parity
// tests run each).
constexpr int kRlev2Default = 0;
constexpr int kRlev2WaveWalk = 1;
constexpr int kRlev2Wide = 2;          // 33 KB serial windows, flat DIRECT prologue: the default's at >= 5 B/value
constexpr int kRlev2SerialDrain = 3;   // 21 KB serial windows + the dense drain: the default's at 1.25 - 5 B/value
constexpr int kRlev2Dense8 = 4;        // dense-capable, 8.5 KB
constexpr int kRlev2Dense12 = 5;       // dense-capable, 12.5 KB
constexpr int kRlev2UnionTwoPass = 6;  // the union instance in two passes: the default's below 1.25 B/value
constexpr int kRlev2WideDrain = 7;     // 33 KB serial windows + the dense drain (round-3 default, A/B)
constexpr int kRlev2UnionOnePass = 8;  // the union instance in one pass
constexpr int kRlev2WideNoFlat = 9;    // kRlev2Wide without the flat DIRECT prologue, its in-binary A/B control
constexpr int kRlev2WideFlat8 = 10;    // kRlev2Wide with the prologue's 8-byte form at every width (A/B control
                                       // and parity cover of flat_expand at W=64)
constexpr int kRlev2FirstTiled = 2;
constexpr int kMaxRlev2Variant = 10;
// Variants a context accepts (orcg_rlev2_variants).
inline bool rlev2_variant_valid(int v) { return v >= kRlev2Default && v <= kMaxRlev2Variant; }
// Variants whose instances take job tables with row-index segments (RleJob::trip).
inline bool rlev2_multi_capable(int v) {
  return v == kRlev2Default || (v >= kRlev2FirstTiled && v <= kMaxRlev2Variant);
}

// One RLEv2 stream of a multi-stream launch: its bytes, segments, output
// (int64) and value count; seg_base = the launch-wide index of its first
// segment (set by group_rlev2_jobs). Segments are either a table ({byte offset,
// value index} per segment) or, for row-index streams of a column without
// nulls, the row index itself: {byte offset, values to skip, bits} triplets
// (trip) and the first row of each row group (rows): value index = rows[g] -
// skip, clamped at 0, as rg_segtab_kernel computes it.
struct RleJob {
  const uint8_t* src;
  uint64_t src_len;
  const uint64_t* segtab;
  const int64_t* trip;
  const int64_t* rows;
  uint64_t nsegs;
  void* dst;
  uint64_t nvalues;
  uint64_t seg_base;
  uint32_t is_signed;
  uint32_t tab_base;  // two-pass launches: the job's first run-table entry (set by group_rlev2_jobs)
  unsigned long long* err;  // the job's device error record (the reader's per-column word), or null = the launch's
  const uint64_t* dcount;   // non-null: the value count on the device (nvalues is then the output's capacity)
};

// What the routing rule sees of a launch under the default.
struct Rlev2Route {
  uint64_t src_len;  // stream bytes
  uint64_t values;   // values, or an estimate (row-index launches: segments x rows per group)
  uint64_t nsegs;
  int cus;      // compute units of the device
  int pinned;   // ctx->rlev2_variant: non-zero pins the instance
  bool grouped; // one job of a multi-stream launch (group_rlev2_jobs), not a launch of its own
};
// The instance of a launch (kRlev2FirstTiled .. kMaxRlev2Variant, or `pinned`).
int route_rlev2(const Rlev2Route& r);
// The union instance in two passes or one, by its launch's segments per CU.
int union_variant(uint64_t nsegs, int cus);

// Two-pass launches (DESIGN.md §3.1 "Two passes"). Values per slice of the
// second pass: at most kSliceMax, a multiple of 256.
constexpr uint32_t kSliceMax = 1024;
// A segment's value bound for the two-pass shape: its share of the values,
// + 1/8 and one run (row-index segments start up to 511 values early).
uint64_t seg_value_bound(uint64_t values, uint64_t nsegs);
// Two-pass shape for segments of at most `seg_values` values (a bound: a
// segment that turns out longer has its later passes expanded by the first
// kernel): slices of <= kSliceMax values, a multiple of 256, spg per segment.
void two_pass_shape(uint64_t seg_values, uint32_t* spg, uint32_t* slice);
// What the run table can address: u32 entry indices and stream offsets with
// room for the kernels' sentinels, and a grid of nsegs x spg slices.
constexpr uint64_t kTabEntryLim = 0xffff0000ull;  // run-table entries of a launch, and stream bytes of a single stream
constexpr uint64_t kTabSegLim = 0x7fff0000ull;    // segments of a single-stream launch
constexpr uint64_t kTabSliceLim = 0x7fffffffull;  // slices of a launch (the second pass's grid)
// Two passes (true) or fall back to one: a shaped launch (spg > 0) of
// `entries` run-table entries over nsegs segments.
bool two_pass_fits(uint64_t entries, uint64_t nsegs, uint32_t spg);
// A single stream's two-pass launch: its entry bound (a run is >= 2 bytes)
// and shape for segments of at most `seg_values` values; spg = 0 where the
// table cannot address the stream (one pass then).
struct TwoPass {
  uint64_t entries;
  uint32_t spg, slice;
};
TwoPass stream_two_pass(uint64_t src_len, uint64_t nsegs, uint64_t seg_values);

// One launch of a multi-stream plan: the jobs one instance gets, in launch
// order with seg_base and tab_base set, and the launch's totals.
struct Rlev2Group {
  int variant = 0;         // the instance the jobs were routed to
  int launch_variant = 0;  // the one to launch: the union instance's passes go by the group's total segments
  std::vector<RleJob> jobs;
  uint64_t segs = 0, values = 0;
  uint64_t entries = 0;  // run-table entries the jobs' ranges add up to
  uint64_t bound = 0;    // the largest seg_value_bound of a job
  uint32_t spg = 0, slice = 0;  // the two-pass shape; 0 = not a two-pass launch
};
// The instance job J joins (route_rlev2, grouped), or -1: nothing to decode.
int rlev2_job_instance(const RleJob& J, int pinned, int cus);
// The launches of `jobs` under a multi-capable `pinned`, by ascending instance.
std::vector<Rlev2Group> group_rlev2_jobs(const RleJob* jobs, uint32_t njobs, int pinned, int cus);

}  // namespace orcg
