// Host stream planning: the walk over a host stream's group headers that cuts
// it into header-aligned segments for the kernels, for RLEv2, RLEv1 and byte
// RLE. The input is untrusted (truncated and corrupt streams are its job) and
// nothing here needs HIP: tests/cxx/host_plan_test.cpp runs it under the host
// sanitizers.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/orcg.h"
#include "dev_error.hh"

// A planned stream (the C ABI keeps the name for all three formats): segment
// cuts, the values the reference can produce, and the first group it cannot
// read with the index of the first value it fails at.
struct orcg_rlev2_plan {
  std::vector<orcg_segment> segs;
  uint64_t values = 0;
  uint32_t err = orcg::kErrNone;
  uint64_t err_at = 0;
};

namespace orcg {

// The group at `pos` < len: kErrNone with its value count and end (<= len), or
// a DevErr with *count = the values the cut group still delivers. Only header
// bytes (and varint terminators) are read, none at or past `len`.
// java: the RLEv2 rules of launch_rlev2_decode's `java`; the others ignore it.
using GroupParser = uint32_t (*)(const uint8_t* s, uint64_t len, uint64_t pos, uint64_t* count, uint64_t* end,
                                 int java);
// RLEv2 (RleDecoderV2::next*, c++/src/RleDecoderV2.cc:184-435): a run the
// stream cuts or a corrupt header fails before any of its values. A DELTA
// run's two varints end inside the run's first kRlev2HdrLim bytes (every
// writer's take <= 22), or the run is a bad read: the device kernels' limit
// (rlev2_tiled_common.hh kHdrLim, parse_run's `lim`), kept here so that a plan and
// the kernels agree on every stream.
constexpr uint32_t kRlev2HdrLim = 64;
uint32_t host_parse_run(const uint8_t* s, uint64_t len, uint64_t pos, uint64_t* run_len, uint64_t* run_end,
                        int java = 0);
// RLEv1 (RleDecoderV1::readHeader / readLong, c++/src/RLEv1.cc:154-191): a
// run needs its base varint whole; a cut literal delivers its whole varints
// (next reads them one by one, :234-300).
uint32_t host_parse_v1_group(const uint8_t* s, uint64_t len, uint64_t pos, uint64_t* count, uint64_t* end, int = 0);
// Byte RLE (ByteRleDecoderImpl::readHeader, c++/src/ByteRLE.cc:378-388): a
// run needs its value byte (readHeader reads it); a cut literal hands out the
// bytes that are there and fails at the first missing one (nextInternal,
// :484-494).
uint32_t host_parse_byte_group(const uint8_t* s, uint64_t len, uint64_t pos, uint64_t* count, uint64_t* end,
                               int = 0);

// The one cut rule: a group opens a segment when none is open yet or the open
// one has reached max_bytes or max_values. The walk ends at the first group
// that fails; the values it still delivers count, and err_at = values. What
// differs between the formats is that group's own cut:
enum class CutAtBad {
  // only if it delivers values: a segment is a workgroup's start, and one
  // whose first group yields nothing has nothing to decode. Byte RLE (a cut
  // literal's bytes that are there: ByteRLE.cc:484-494) and RLEv2, where a bad
  // run never delivers any (RleDecoderV2 reads a whole run before it hands out
  // its first value), so RLEv2 cuts only after a run has parsed.
  kIfItDelivers,
  // like any other group, values or not (RLEv1 cuts before it parses). A cut
  // literal delivers its whole varints and RleDecoderV1 fails with "bad read
  // in readByte" at the next value; rlev1_kernel reports that from the
  // segment the group lies in, so a stream whose first group is bad keeps its
  // segment at 0: a launch over it has a workgroup to report from.
  kAlways,
};
orcg_rlev2_plan* cut_stream(const uint8_t* src, uint64_t len, uint64_t max_bytes, uint64_t max_values,
                            GroupParser parse, CutAtBad at_bad, int java = 0);

}  // namespace orcg

inline orcg_rlev2_plan* make_plan(const uint8_t* src, uint64_t len, uint64_t max_bytes, uint64_t max_values,
                                  int java = 0) {
  return orcg::cut_stream(src, len, max_bytes, max_values, orcg::host_parse_run, orcg::CutAtBad::kIfItDelivers, java);
}
inline orcg_rlev2_plan* make_v1_plan(const uint8_t* src, uint64_t len, uint64_t max_bytes, uint64_t max_values) {
  return orcg::cut_stream(src, len, max_bytes, max_values, orcg::host_parse_v1_group, orcg::CutAtBad::kAlways);
}
inline orcg_rlev2_plan* make_byte_plan(const uint8_t* src, uint64_t len, uint64_t max_bytes, uint64_t max_values) {
  return orcg::cut_stream(src, len, max_bytes, max_values, orcg::host_parse_byte_group,
                          orcg::CutAtBad::kIfItDelivers);
}

namespace orcg {

// The value index of the group that starts at byte `rel` <= len of the planned
// stream, if the walk over group headers from the nearest segment cut at or
// before `rel` lands on it and the plan holds that many values; else kNotFound.
constexpr uint64_t kNotFound = ~0ull;
uint64_t locate(const orcg_rlev2_plan& plan, const uint8_t* s, uint64_t len, uint64_t rel, GroupParser parse);

}  // namespace orcg
