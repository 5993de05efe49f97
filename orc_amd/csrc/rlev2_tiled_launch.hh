// What the launcher (rlev2_tiled.cpp) and the instance units
// (rlev2_tiled_inst_*.hip) share: an instance's option bits, one launch's
// arguments and the declaration of enqueue<...>, which the units instantiate
// (rlev2_tiled_kernel.hh holds its definition). Host code only.
#pragma once

#include "orcg_internal.hh"

namespace orcg {

// kOpt bits: what an instance adds to the common code. (Output stores are
// non-temporal, the window's tail is carried over in LDS, full runs inside the
// output range take predicate-free paths and dense discovery probes inline in
// every instance; the alternatives measured and rejected are in DESIGN.md §4.)
// The values keep the positions they had among the retired bits (gaps): the
// kernels' symbols carry them, and the profiling build's data section is laid
// out by those symbols.
constexpr int kOptRegFill = 16;    // fill windows through registers (16 B buffer loads, then LDS writes), not LDS-DMA
constexpr int kOptUnion = 1024;    // dense instance whose serial (long-run) windows also cover the dense stage and
                                   // marks: one instance routes each window by its runs (dense or serial), no queue
constexpr int kOptTable = 16384;   // two-pass (RunTab): dense passes write their runs to the run table for
                                   // rlev2_expand_kernel instead of expanding them
constexpr int kOptFlat = 32768;    // a segment's leading chain of equal full DIRECT runs of >= 40 bits (int64
                                   // output): one header probe, then expanded straight from memory (flat_*),
                                   // no LDS window, no walk, no barrier
constexpr int kOptFlat16 = 65536;  // kOptFlat's W=64 runs: aligned 16-byte chunk loads shifted in registers, two
                                   // values per lane, ORCG_FLAT16_RUNS runs in flight (flat_expand16)
constexpr int kSer = 0;             // LDS-DMA windows
constexpr int kWide = kOptRegFill;  // register-filled windows

// One launch of an instance: a stream's arguments, or (jobs) the launch-wide
// segments a.nsegs and values a.nvalues of a device job table; the queue of a
// serial + drain pair and the run table of a two-pass launch.
struct TiledLaunch {
  Rlev2Args a;
  const RleJob* jobs;
  uint32_t njobs;
  unsigned long long* dq;
  uint32_t dpar;
  RunTab rtab;
};
using Enqueue = void (*)(Ctx*, const TiledLaunch&);

// An instance, K = (options, window KB, min waves, kDense, kDefer): defined
// in rlev2_tiled_kernel.hh, instantiated once per distinct K over the units.
template <int... K>
void enqueue(Ctx* ctx, const TiledLaunch& l);

// The instance units. Each is a code object of its own with its own no-op
// warm kernel (warm_rlev2_tiled launches them all) and, in the profiling
// build, its own copy of the counters: prof_phase_<unit> reads (and resets)
// its 16 phase counters, prof_wgdur_<unit> its first n workgroup durations.
#define ORCG_TILED_UNITS(X) X(serial) X(dense) X(union)
#define ORCG_TILED_UNIT_DECL(u)                         \
  void warm_rlev2_tiled_##u(hipStream_t s);             \
  int prof_phase_##u(unsigned long long* h, int reset); \
  int prof_wgdur_##u(unsigned long long* out, int n);
ORCG_TILED_UNITS(ORCG_TILED_UNIT_DECL)
#undef ORCG_TILED_UNIT_DECL

}  // namespace orcg
