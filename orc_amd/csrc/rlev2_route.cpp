// RLEv2 launch routing (rlev2_route.hh): the default's density rule, the
// one-pass / two-pass decisions and the grouping of multi-stream launches.
#include "rlev2_route.hh"

#include <algorithm>

namespace orcg {

// The default's instance for a stream, by its stream bytes per value
// (profiles/r03/sweep.md):
//  * >= 5 B/value (wide values, W >= 40): 33 KB windows (4 WG/CU) filled
//    through registers, one walking wave, no queue (writers emit wide random
//    values in long DIRECT runs; the empty queue drain cost 4 us of C2's 290);
//    a segment's leading chain of equal full DIRECT runs skips the windows
//    altogether (kOptFlat);
//  * 1.25 - 5 B/value: 21 KB serial windows (6 WG/CU), queueing segments whose
//    first runs are short by values for the dense drain (long DIRECT / DELTA /
//    PATCHED_BASE runs of 10-40-bit values: 5.3-6.1 TB/s; short runs of wide
//    values 20 % slower than the union instance, the price of the rule);
//  * < 1.25 B/value (low-cardinality columns, SHORT_REPEAT 0.2-1 B/value): the
//    union instance, which routes each window by its own runs (8.5 KB dense
//    windows with parallel run discovery, 16.75 KB serial windows once a
//    segment's runs are long).
// The dense-capable instances walk long runs 15-20 % slower than the serial
// ones (at 6 WG/CU they carry 56 B/lane of scratch, the serial ones none), so long-run
// streams above 1.25 B/value stay on the serial instance.
static int density_variant(uint64_t src_len, uint64_t values) {
  return src_len >= 5 * values ? kRlev2Wide : (4 * src_len >= 5 * values ? kRlev2SerialDrain : kRlev2UnionTwoPass);
}

// The union instance runs in two passes (kOptTable + rlev2_expand_kernel)
// when its launch has at most this many segments per CU: a launch of a few
// segments per CU lasts as long as its slowest segments' discovery +
// expansion, and balancing the expansion by values pays (configs[3]'s
// multi-stream launch, 1,336 segments: 297 -> 150 + 86 us; configs[4]'s
// child streams, 264: 93 -> 57 + 20 us); with many more segments than the
// chip holds at once, the one-pass instance's expansion already overlaps
// other workgroups' discovery and the second pass only adds its own latency
// and the run table's traffic (the stream sweep's 10,000-segment launches:
// SHORT_REPEAT 12-bit 2,016 GB/s in one pass, 1,267 in two; profiles/r06/
// sweep_*).
constexpr uint64_t kTwoPassSegsPerCu = 12;
int union_variant(uint64_t nsegs, int cus) {
  return nsegs <= kTwoPassSegsPerCu * (uint64_t)cus ? kRlev2UnionTwoPass : kRlev2UnionOnePass;
}

int route_rlev2(const Rlev2Route& r) {
  if (r.pinned) return r.pinned;
  const int v = density_variant(r.src_len, r.values);
  // A job of a multi-stream launch gets its density class and nothing else:
  // the segments-per-CU test is its group's, on the group's total segments
  // (group_rlev2_jobs), and the 8.1 B/value rule below is not applied.
  if (r.grouped) return v;
  if (v == kRlev2UnionTwoPass) return union_variant(r.nsegs, r.cus);
  // Single streams only: more than 8.1 stream bytes a value is more than any
  // 64-bit payload: the excess is run headers, i.e. runs of ~20 values or
  // fewer of wide values (short DIRECT / PATCHED_BASE), whose expansion the
  // two-pass union balances by values at any segment count, so this route
  // skips the segments-per-CU test (sweep short DIRECT 64-bit, 10,000
  // segments: 217 GB/s in the serial walk, 270 in one union pass, 379 in two;
  // profiles/r06/sweep_shortdirect_64_548c478.jsonl). 512-value W=64 runs
  // (configs[1]) are 8.004 B/value: the serial walk.
  if (v == kRlev2Wide && 10 * r.src_len > 81 * r.values) return kRlev2UnionTwoPass;
  return v;
}

uint64_t seg_value_bound(uint64_t values, uint64_t nsegs) {
  const uint64_t avg = (values + nsegs - 1) / std::max<uint64_t>(nsegs, 1);
  return avg + avg / 8 + 512;
}

void two_pass_shape(uint64_t seg_values, uint32_t* spg, uint32_t* slice) {
  const uint64_t n = std::max<uint64_t>(seg_values, 1);
  const uint64_t smax = kSliceMax;
  const uint64_t k = std::min<uint64_t>((n + smax - 1) / smax, 256);
  uint64_t s = (n + k - 1) / k;
  s = std::min<uint64_t>((s + 255) & ~255ull, smax);
  *spg = (uint32_t)k;
  *slice = (uint32_t)s;
}

bool two_pass_fits(uint64_t entries, uint64_t nsegs, uint32_t spg) {
  return spg && entries < kTabEntryLim && nsegs * spg < kTabSliceLim;
}

TwoPass stream_two_pass(uint64_t src_len, uint64_t nsegs, uint64_t seg_values) {
  TwoPass t{0, 0, 0};
  if (src_len >= kTabEntryLim || nsegs >= kTabSegLim) return t;
  t.entries = src_len / 2 + nsegs + 1;
  two_pass_shape(seg_values, &t.spg, &t.slice);
  if (!two_pass_fits(t.entries, nsegs, t.spg)) t.spg = t.slice = 0;
  return t;
}

int rlev2_job_instance(const RleJob& J, int pinned, int cus) {
  if (J.nsegs == 0 || J.nvalues == 0) return -1;
  return route_rlev2(Rlev2Route{J.src_len, J.nvalues, J.nsegs, cus, pinned, true});
}

std::vector<Rlev2Group> group_rlev2_jobs(const RleJob* jobs, uint32_t njobs, int pinned, int cus) {
  std::vector<Rlev2Group> out;
  if (!rlev2_multi_capable(pinned)) return out;
  // one launch per instance: group the streams by the instance they get
  std::vector<Rlev2Group> by_instance(kMaxRlev2Variant + 1);
  for (uint32_t j = 0; j < njobs; ++j) {
    const int v = rlev2_job_instance(jobs[j], pinned, cus);
    if (v >= 0) by_instance[v].jobs.push_back(jobs[j]);
  }
  for (int v = kRlev2FirstTiled; v <= kMaxRlev2Variant; ++v) {
    if (by_instance[v].jobs.empty()) continue;
    out.push_back(std::move(by_instance[v]));
    Rlev2Group& g = out.back();
    g.variant = v;
    // workgroups start in index order: the streams with the most stream
    // bytes per value (the most runs per segment, the slowest segments) first,
    // so the launch does not end on a tail of slow segments
    std::stable_sort(g.jobs.begin(), g.jobs.end(), [](const RleJob& a, const RleJob& b) {
      return (double)a.src_len * (double)b.nvalues > (double)b.src_len * (double)a.nvalues;
    });
    for (RleJob& J : g.jobs) {
      J.seg_base = g.segs;
      g.segs += J.nsegs;
      g.values += J.nvalues;
      // two-pass (the union instance): the job's run-table range
      J.tab_base = (uint32_t)std::min<uint64_t>(g.entries, 0xffffffffull);
      g.entries += J.src_len / 2 + J.nsegs + 1;
      g.bound = std::max(g.bound, seg_value_bound(J.nvalues, J.nsegs));
    }
    // the default's union group: one pass or two by the group's total
    // segments per CU (a pinned instance launches as pinned)
    g.launch_variant = (v == kRlev2UnionTwoPass && !pinned) ? union_variant(g.segs, cus) : v;
    // shaped for two passes while the table's entry indices hold; the
    // launcher falls back to one pass if the shaped launch does not fit
    // (two_pass_fits)
    if (g.launch_variant == kRlev2UnionTwoPass && g.entries < kTabEntryLim) two_pass_shape(g.bound, &g.spg, &g.slice);
  }
  return out;
}

}  // namespace orcg
