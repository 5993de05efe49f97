// RLEv2 decode, tiled through LDS (the default kernels).
//
// One 256-thread workgroup per segment. The segment's bytes stream through an
// LDS window filled by buffer_load ... lds (LDS-DMA, 1 KB per wave
// instruction, range-checked so reads past the stream return zeros), or, in
// the wide-value instance, by 16-byte buffer loads into registers that are
// all in flight before the LDS writes (kOptRegFill). The run
// headers are walked in LDS (RleDecoderV2::next's run loop,
// c++/src/RleDecoderV2.cc:132-170) into a run table, and waves expand runs
// round-robin straight out of LDS:
//   SHORT_REPEAT  broadcast                                      (:184-222)
//   DIRECT        per-lane big-endian W-bit extract + zigzag     (:224-248)
//   PATCHED_BASE  extract + base, patches applied in registers   (:250-370)
//   DELTA         wavefront int64 inclusive scan                 (:372-435)
// A window holds every run that STARTS in its first (kWin - kMaxRun) bytes;
// runs are at most kMaxRun bytes, so they end inside it. The next window
// starts at the first unprocessed run.
//
// All 4 waves fill the window; wave 0 walks it and publishes work items as
// they close, and every wave (wave 0 once its walk is done) claims and
// expands them, so the walk overlaps the expansion. Dense-capable instances
// discover the runs of short-run windows in parallel instead (dense mode,
// below), and the wide-value instance takes a segment's leading chain of
// equal full DIRECT runs straight from memory (the flat path, flat_*).
#include <algorithm>
#include <type_traits>
#include <vector>

#include "rlev2_device.hh"

namespace orcg {
namespace {
using namespace dev;

// Phase profiling (build with -DORCG_PHASE_PROF, scripts/phase_prof.py):
// thread 0 adds the cycles between consecutive phase marks to g_phase[k].
#ifdef ORCG_PHASE_PROF
__device__ unsigned long long g_phase[16];
// union instances: per workgroup {wall-clock ticks, dense passes | serial passes << 32}
constexpr uint32_t kWgDurMax = 16384;
__device__ unsigned long long g_wgdur[2 * kWgDurMax];
#define PROF_MARK(k)                                                        \
  do {                                                                      \
    if (threadIdx.x == 0) {                                                 \
      const uint64_t now_ = wall_clock64();                                 \
      atomicAdd(&g_phase[k], (unsigned long long)(now_ - prof_last_));      \
      prof_last_ = now_;                                                    \
    }                                                                       \
  } while (0)
#define PROF_DECL uint64_t prof_last_ = wall_clock64()
#else
#define PROF_MARK(k) \
  do {               \
  } while (0)
#define PROF_DECL
#endif

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kMaxRun = 4608;  // >= 4356, the longest legal run

// Dense (short-run) mode. A stream of short runs (SHORT_REPEAT-heavy
// low-cardinality columns: 2-9 bytes per run) makes the one-wave serial header
// walk the bottleneck. Dense mode discovers run starts in parallel over a slab
// of kSlab bytes: thread t owns bytes [t*kBlk, (t+1)*kBlk) and computes, for
// every position of its block, the chain exit "first run start past the block
// if a run started here" and the values in between (a backward scan, since a
// run ending inside the block continues from a later position of the same
// block); one lane then chains the 256 blocks (one LDS read per block instead
// of one header parse per run), and every thread re-walks its own block from
// its true entry to emit the run table. Short runs are then expanded one lane
// per run into a per-wave LDS stage, flushed with coalesced stores.
constexpr uint32_t kSlab = 2048;
constexpr uint32_t kBlk = kSlab / kThreads;  // 8 bytes per thread
constexpr uint32_t kDenseRuns = kSlab / 2;   // every run is >= 2 bytes
constexpr uint32_t kStage = 256;             // values staged per wave
constexpr uint32_t kShortL = 16;             // runs of <= kShortL values go lane-per-run
constexpr uint32_t kVparL = 256;             // dense expansion: runs of kVparMin+1 .. kVparL values go
#ifndef ORCG_VPAR_MIN                         // value-parallel
#define ORCG_VPAR_MIN 16
#endif
constexpr uint32_t kVparMin = ORCG_VPAR_MIN;
#ifndef ORCG_VPAR_FRAG
#define ORCG_VPAR_FRAG 2
#endif
constexpr uint32_t kVparFrag = ORCG_VPAR_FRAG;  // short-run groups per 64 runs before all go value-parallel
#ifndef ORCG_FLAT_RUNS  // flat DIRECT path (kOptFlat): runs in flight per wave, 1 or 2
#define ORCG_FLAT_RUNS 2
#endif
// its 16-byte form for W=64 runs (kOptFlat16): runs in flight per wave, 2, 3
// or 5 (a wave's share of a 10,000-row segment: measured 1.1 % faster than 2 on
// C2, 3 within noise of 2). DESIGN.md §4.
#ifndef ORCG_FLAT16_RUNS
#define ORCG_FLAT16_RUNS 5
#endif
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint16_t kSink = 0xffffu;          // chain successor: none
constexpr uint32_t kWalkDone = 0x80000000u;  // published-runs flag: the walk has finished
// density hysteresis (stream bytes per run of the last pass)
constexpr uint32_t kToDense = 24, kToSerial = 64;
// two-pass (kOptTable) instances: dense discovery no longer pays for the
// expansion, and a serial walk over medium runs (DELTA / DIRECT runs of tens
// of bytes) was the launch's tail (one wave walking a whole row group while
// co-resident workgroups share the CU): dense up to far longer runs
#ifndef ORCG_TAB_TO_DENSE
#define ORCG_TAB_TO_DENSE 128
#endif
#ifndef ORCG_TAB_TO_SERIAL
#define ORCG_TAB_TO_SERIAL 512
#endif
constexpr uint32_t kTabToDense = ORCG_TAB_TO_DENSE, kTabToSerial = ORCG_TAB_TO_SERIAL;

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

// Debug build only (ORCG_AB_FLAGS=-DORCG_DEBUG_COVER): every expansion path
// counts the values of the runs it expands; each pass checks the count
// against the values its discovery consumed.
#ifdef ORCG_DEBUG_COVER
#define ORCG_COVER_ADD(x) atomicAdd(s_cover_ptr(), (uint32_t)(x))
__device__ __forceinline__ uint32_t* s_cover_ptr() {
  __shared__ uint32_t s_cover;
  return &s_cover;
}
#else
#define ORCG_COVER_ADD(x) \
  do {                    \
  } while (0)
#endif

// output stores are non-temporal: streamed, never re-read
template <typename T>
__device__ __forceinline__ void store1(T* p, uint64_t v) {
  __builtin_nontemporal_store((T)(int64_t)v, p);
}

__device__ __forceinline__ uint32_t lds_byte(const uint32_t* w, uint32_t o) {
  return (w[o >> 2] >> ((o & 3u) * 8)) & 0xffu;
}

__device__ __forceinline__ u32x3 lds12(const uint32_t* w, uint32_t o) {
  const uint32_t i = o >> 2;
  u32x3 r;
  r.x = w[i];
  r.y = w[i + 1];
  r.z = w[i + 2];
  return r;
}

// Run headers are parsed from a 256-byte slice of the LDS window held one
// dword per lane and read back with v_readlane: one LDS round trip per slice
// instead of one per header byte. kHdrLim bounds how far a header may reach
// (DELTA's two varints take <= 22 bytes; longer ones are corrupt).
constexpr uint32_t kHdrLim = kRlev2HdrLim;  // host_plan.hh: the one limit of every RLEv2 decoder

// terminator bits of a dword's bytes (bit i = byte i < 0x80)
__device__ __forceinline__ uint32_t term4(uint32_t w) {
  const uint32_t m = (~w >> 7) & 0x01010101u;
  return (m * 0x10204080u) >> 28;
}

struct LaneWin {
  uint32_t word = 0, base = 0xffffffffu;
  uint32_t t4 = 0;  // term4(word): the walk's varint ends, computed once per slice on the VALU
  __device__ __forceinline__ void load(const uint32_t* win, uint32_t hoff, uint32_t nwords, int lane) {
    base = hoff & ~3u;
    uint32_t idx = (base >> 2) + (uint32_t)lane;
    if (idx >= nwords) idx = nwords - 1;
    word = win[idx];
    t4 = term4(word);
  }
  // make sure [hoff, hoff + kHdrLim) is inside the slice
  __device__ __forceinline__ void cover(const uint32_t* win, uint32_t hoff, uint32_t nwords, int lane) {
    if (base == 0xffffffffu || hoff < base || hoff + kHdrLim > base + 256) load(win, hoff, nwords, lane);
  }
  __device__ __forceinline__ uint32_t byte(uint32_t o) const {
    o -= base;
    return (rdlane(word, o >> 2) >> ((o & 3u) * 8)) & 0xffu;
  }
};

// Expand one run (already validated by the walk) with one wave.
template <typename T>
__device__ __forceinline__ void expand_run(const uint32_t* win, uint32_t nwords, uint32_t hoff, uint64_t v0,
                                           int is_signed, uint64_t value_begin, uint64_t value_end, T* dst,
                                           int lane) {
  LaneWin hw;
  hw.load(win, hoff, nwords, lane);
  Run r;
  if ((hw.byte(hoff) >> 6) == 3) {
    // DELTA header of a run the walk validated, one header byte per lane: varint
    // ends from a ballot of the terminator bytes, values OR-reduced in the
    // DPP rows, instead of a
    // scalar byte loop (the kernel's scalar unit is its busiest on DELTA
    // streams)
    const uint32_t fb = hw.byte(hoff);
    r.kind = 3;
    r.pbs = r.pl = r.cfb = 0;
    r.err = kErrNone;
    r.L = ((fb & 1u) << 8 | hw.byte(hoff + 1)) + 1u;
    const uint32_t fbo = (fb >> 1) & 0x1fu;
    r.W = fbo ? fbs_width(fbo) : 0u;
    const uint32_t hb = lds_byte(win, hoff + 2u + (uint32_t)lane);
    const uint64_t term = __ballot(hb < 0x80u);
    const uint32_t n1 = (uint32_t)__builtin_ctzll(term) + 1u;
    const uint32_t n2 = (uint32_t)__builtin_ctzll(term >> n1) + 1u;
    const uint32_t b7 = hb & 0x7fu, k2 = (uint32_t)lane - n1;
    uint64_t ca = ((uint32_t)lane < n1 && lane < 10) ? (uint64_t)b7 << (7 * lane) : 0ull;
    uint64_t cb = ((uint32_t)lane >= n1 && k2 < n2 && k2 < 10u) ? (uint64_t)b7 << (7 * k2) : 0ull;
#define ORCG_OR_ROWS(x)                  \
  x |= dpp0_64<0x111, 0xf>(x);           \
  x |= dpp0_64<0x112, 0xf>(x);           \
  x |= dpp0_64<0x114, 0xf>(x);           \
  x |= dpp0_64<0x118, 0xf>(x)
    ORCG_OR_ROWS(ca);
    ORCG_OR_ROWS(cb);
#undef ORCG_OR_ROWS
    // the row totals sit in lanes 15 / 31 / 47 / 63 (a header reaches 64 bytes)
    auto rows_or = [](uint64_t x) -> uint64_t {
      const uint32_t lo = rdlane((uint32_t)x, 15) | rdlane((uint32_t)x, 31) | rdlane((uint32_t)x, 47) |
                          rdlane((uint32_t)x, 63);
      const uint32_t hi = rdlane((uint32_t)(x >> 32), 15) | rdlane((uint32_t)(x >> 32), 31) |
                          rdlane((uint32_t)(x >> 32), 47) | rdlane((uint32_t)(x >> 32), 63);
      return ((uint64_t)hi << 32) | lo;
    };
    const uint64_t a_raw = rows_or(ca), b_raw = rows_or(cb);
    r.a = is_signed ? unzigzag(a_raw) : a_raw;
    r.b = unzigzag(b_raw);
    r.data = 2u + n1 + n2;
    r.bytes = r.data + (r.W ? (r.W * (r.L - 2u) + 7u) / 8u : 0u);
  } else {
    r = parse_run([&](uint32_t i) { return hw.byte(hoff + i); }, ~0ull, kHdrLim, is_signed);
  }
  const uint32_t L = r.L;
  if (v0 + L <= value_begin || v0 >= value_end) return;  // outside the requested rows
  const uint32_t d = hoff + r.data;  // LDS offset of the packed data
  const uint32_t niter = (L + kWave - 1) / kWave;

  if (r.kind == 0) {
    const uint64_t o = v0 + (uint64_t)lane;
    if ((uint32_t)lane < L && o >= value_begin && o < value_end) store1(dst + (o - value_begin), r.a);
    return;
  }
  if (r.kind == 1) {
    const uint32_t W = r.W;
    if (L == 512 && v0 >= value_begin && v0 + 512 <= value_end) {
      // Full run entirely inside the output range: no per-value predicates.
      T* out = dst + (v0 - value_begin);
      if (W == 64) {
        // 8 bytes per value at d + 8j: one uniform byte alignment per run
        const uint32_t r4 = d & 3u;
#pragma unroll
        for (int it = 0; it < kMaxRunUnroll; ++it) {
          const uint32_t j = it * kWave + lane;
          const u32x3 w = lds12(win, d + 8 * j);
          const uint32_t lo = __builtin_amdgcn_alignbyte(w.y, w.x, r4);
          const uint32_t hi = __builtin_amdgcn_alignbyte(w.z, w.y, r4);
          uint64_t v = ((uint64_t)__builtin_bswap32(lo) << 32) | __builtin_bswap32(hi);
          if (is_signed) v = unzigzag(v);
          store1(out + j, v);
        }
      } else {
#pragma unroll
        for (int it = 0; it < kMaxRunUnroll; ++it) {
          const uint32_t j = it * kWave + lane;
          const uint32_t bit = j * W;
          const uint32_t br = d + (bit >> 3);
          uint64_t v = field(lds12(win, br), br, bit & 7u, W);
          if (is_signed) v = unzigzag(v);
          store1(out + j, v);
        }
      }
      return;
    }
#pragma unroll
    for (int it = 0; it < kMaxRunUnroll; ++it) {
      if ((uint32_t)it < niter) {
        const uint32_t j = it * kWave + lane;
        const uint32_t bit = j * W;
        const uint32_t br = d + (bit >> 3);
        uint64_t v = field(lds12(win, br), br, bit & 7u, W);
        if (is_signed) v = unzigzag(v);
        const uint64_t o = v0 + j;
        if (j < L && o >= value_begin && o < value_end) store1(dst + (o - value_begin), v);
      }
    }
    return;
  }
  if (r.kind == 2) {
    // PATCHED_BASE. The patch list (<= 31 entries of cfb bits) is held one
    // entry per lane; positions are the inclusive prefix sum of the gap
    // fields (an escape entry, gap 255 / patch 0, contributes its 255), and
    // the entries are applied in order exactly like nextPatched's loop
    // (:340-366) with adjustGapAndPatch (:250-271): escapes only advance, a
    // patch that does not move past the previous one stalls the walk, and
    // positions >= L are never reached. Low register footprint: one 64-value
    // chunk of literals at a time, patches consumed with a scalar cursor.
    const uint32_t W = r.W;
    const uint32_t p0 = d + (W * L + 7) / 8;  // patch list
    uint64_t entry = 0;
    if ((uint32_t)lane < r.pl) {
      const uint32_t bit = lane * r.cfb;
      const uint32_t br = p0 + (bit >> 3);
      entry = field(lds12(win, br), br, bit & 7u, r.cfb);
    }
    const uint64_t pmask = (1ull << r.pbs) - 1;  // pbs <= 63 (checked by the walk)
    const uint32_t gap = (uint32_t)lane < r.pl ? (uint32_t)(entry >> r.pbs) : 0u;  // <= 255
    const uint32_t cum = wave_scan_u32(gap);  // positions (<= 31 * 255)
    const uint64_t patch = entry & pmask;
    const uint32_t p_lo = (uint32_t)patch, p_hi = (uint32_t)(patch >> 32);
    // scalar pass: which entries apply (bitmask over entries)
    uint64_t applied = 0;
    {
      uint32_t prev = 0;
      bool first = true;
      for (uint32_t k = 0; k < r.pl; ++k) {
        const uint32_t c = rdlane(cum, k), g = rdlane(gap, k);
        const bool esc = g == 255 && rdlane(p_lo, k) == 0 && rdlane(p_hi, k) == 0;
        if (esc) continue;
        if ((!first && c == prev) || c >= L) break;
        applied |= 1ull << k;
        prev = c;
        first = false;
      }
    }
    if (L == 512 && v0 >= value_begin && v0 + 512 <= value_end) {
      // full run inside the output range: all 8 chunks' literals in
      // registers, the (few) patches OR-ed into the lane that owns their
      // position, then predicate-free stores
      T* out = dst + (v0 - value_begin);
      uint64_t lit[kMaxRunUnroll];
#pragma unroll
      for (int it = 0; it < kMaxRunUnroll; ++it) {
        const uint32_t bit = (uint32_t)(it * kWave + lane) * W;
        const uint32_t br = d + (bit >> 3);
        lit[it] = field(lds12(win, br), br, bit & 7u, W);
      }
      for (uint64_t t = applied; t; t &= t - 1) {
        const uint32_t k = (uint32_t)__builtin_ctzll(t);
        const uint32_t c = rdlane(cum, k);
        const uint64_t add = (((uint64_t)rdlane(p_hi, k) << 32) | rdlane(p_lo, k)) << (W & 63u);
#pragma unroll
        for (int it = 0; it < kMaxRunUnroll; ++it)
          if (c == (uint32_t)(it * kWave + lane)) lit[it] |= add;
      }
#pragma unroll
      for (int it = 0; it < kMaxRunUnroll; ++it) store1(out + it * kWave + lane, r.a + lit[it]);
      return;
    }
    uint64_t todo = applied;
#pragma unroll 1
    for (uint32_t it = 0; it < niter; ++it) {
      const uint32_t j = it * kWave + lane;
      const uint32_t bit = j * W;
      const uint32_t br = d + (bit >> 3);
      uint64_t lit = field(lds12(win, br), br, bit & 7u, W);
      // patches whose position falls in this chunk (positions increase)
      while (todo) {
        const uint32_t k = (uint32_t)__builtin_ctzll(todo);
        const uint32_t c = rdlane(cum, k);
        if (c / kWave != it) break;
        const uint64_t pv = ((uint64_t)rdlane(p_hi, k) << 32) | rdlane(p_lo, k);
        if ((uint32_t)lane == c % kWave) lit |= pv << (W & 63u);
        todo &= todo - 1;
      }
      const uint64_t o = v0 + j;
      if (j < L && o >= value_begin && o < value_end) store1(dst + (o - value_begin), r.a + lit);
    }
    return;
  }
  // DELTA
  if (r.W == 0) {
#pragma unroll
    for (int it = 0; it < kMaxRunUnroll; ++it) {
      const uint32_t j = it * kWave + lane;
      const uint64_t o = v0 + j;
      if ((uint32_t)it < niter && j < L && o >= value_begin && o < value_end)
        store1(dst + (o - value_begin), r.a + (uint64_t)j * r.b);
    }
    return;
  }
  const uint32_t W = r.W;
  const uint64_t v1 = r.a + r.b;
  const bool neg = (int64_t)r.b < 0;
  uint64_t carry = 0;  // wave-uniform running |delta| total
  if (W <= 26 && L == 512 && v0 >= value_begin && v0 + 512 <= value_end) {
    // full run inside the output range: all 8 chunks' deltas loaded up
    // front, no per-value predicates, one 32-bit wave scan per chunk
    T* out = dst + (v0 - value_begin);
    uint32_t dl[kMaxRunUnroll];
#pragma unroll
    for (int it = 0; it < kMaxRunUnroll; ++it) {
      const uint32_t j = it * kWave + lane;
      const uint32_t k = j >= 2 ? j - 2 : 0u;  // j < 2: a dummy in-range read, masked below
      const uint32_t bit = k * W;
      const uint32_t br = d + (bit >> 3);
      dl[it] = (uint32_t)field(lds12(win, br), br, bit & 7u, W);
    }
    if (lane < 2) dl[0] = 0;
#pragma unroll
    for (int it = 0; it < kMaxRunUnroll; ++it) {
      const uint32_t j = it * kWave + lane;
      const uint32_t s32 = wave_scan_u32(dl[it]);
      const uint64_t sum = carry + s32;
      carry += (uint32_t)__builtin_amdgcn_readlane((int)s32, 63);
      const uint64_t v = j == 0 ? r.a : (j == 1 ? v1 : (neg ? v1 - sum : v1 + sum));
      store1(out + j, v);
    }
    return;
  }
  if (W <= 26) {
    // 64 deltas of <= 26 bits sum below 2^32: scan in 32 bits
#pragma unroll 1
    for (uint32_t it = 0; it < niter; ++it) {
      const uint32_t j = it * kWave + lane;
      const int32_t k = (int32_t)j - 2;
      uint32_t dlt = 0;
      if (k >= 0 && j < L) {
        const uint32_t bit = (uint32_t)k * W;
        const uint32_t br = d + (bit >> 3);
        dlt = (uint32_t)field(lds12(win, br), br, bit & 7u, W);
      }
      const uint32_t s32 = wave_scan_u32(dlt);
      const uint64_t sum = carry + s32;
      carry += (uint32_t)__builtin_amdgcn_readlane((int)s32, 63);
      const uint64_t v = j == 0 ? r.a : (j == 1 ? v1 : (neg ? v1 - sum : v1 + sum));
      const uint64_t o = v0 + j;
      if (j < L && o >= value_begin && o < value_end) store1(dst + (o - value_begin), v);
    }
    return;
  }
#pragma unroll 1
  for (uint32_t it = 0; it < niter; ++it) {
    const uint32_t j = it * kWave + lane;
    const int32_t k = (int32_t)j - 2;
    uint64_t dlt = 0;
    if (k >= 0 && j < L) {
      const uint32_t bit = (uint32_t)k * W;
      const uint32_t br = d + (bit >> 3);
      dlt = field(lds12(win, br), br, bit & 7u, W);
    }
    const uint64_t sum = wave_inclusive_scan(dlt) + carry;
    carry = last_lane(sum);
    const uint64_t v = j == 0 ? r.a : (j == 1 ? v1 : (neg ? v1 - sum : v1 + sum));
    const uint64_t o = v0 + j;
    if (j < L && o >= value_begin && o < value_end) store1(dst + (o - value_begin), v);
  }
}

// The flat DIRECT path (kOptFlat). A writer emits a wide random column as
// back-to-back DIRECT runs of 512 values at one width: every such run has the
// same two header bytes and the same byte length B = 2 + 512 * nb (nb = W / 8
// bytes per value), and a run's extent depends on its own header only. So if
// the header at pos + k * B equals the one at pos for k = 1 .. m - 1, those m
// runs start exactly there (by induction): one memory round trip validates
// the chain, and each lane then loads its values' bytes straight from memory,
// as a flat copy does. Every wave probes for itself (the same few cache
// lines), so the path needs no LDS, no barrier and no walk.
//
// flat_probe: lane k reads the two bytes at descriptor offset prel + k * B,
// for the B of each of the four widths (40, 48, 56, 64 bits) at once; the
// first header then picks the width, so the probe is a single round trip.
// Only lanes k < kmax whose run would end at or before descriptor offset
// `lim` (W=64 runs: `lim64`, the 16-byte form's reach) take part; the others
// hold zeros, which is no eligible header.
// Returns m, the number of leading runs whose header equals the first one
// (not the number of matches: the chain ends at the first mismatch), 0 when
// the first run is not eligible: DIRECT, 512 values, W >= 40.
__device__ __forceinline__ uint32_t flat_probe(__amdgpu_buffer_rsrc_t rs, uint32_t prel, uint32_t lim,
                                               uint32_t lim64, uint32_t kmax, int lane, uint32_t* nb) {
  uint32_t h[4];
#pragma unroll
  for (uint32_t wi = 0; wi < 4; ++wi) {
    const uint32_t B = 2u + 512u * (5u + wi);
    const uint64_t off = (uint64_t)prel + (uint32_t)lane * B;
    uint32_t x = 0;
    if ((uint32_t)lane < kmax && off + B <= (wi == 3 ? lim64 : lim)) {
      // the aligned-down dword pair around the two bytes
      const auto q = __builtin_amdgcn_raw_buffer_load_b64(rs, (uint32_t)off & ~3u, 0, 0);
      const uint64_t qq = ((uint64_t)q[1] << 32) | q[0];
      x = (uint32_t)(qq >> (((uint32_t)off & 3u) * 8u)) & 0xffffu;
    }
    h[wi] = x;
  }
  const uint32_t hdr = uni(h[0]);  // lane 0: the first header, whatever the width
  // 01 wwwww 1 | 11111111: DIRECT, L - 1 = 0x1ff, width code 28 .. 31
  if ((hdr & 0xfff9u) != 0xff79u) return 0;
  const uint32_t wi = (hdr >> 1) & 3u;
  const uint32_t mine = wi == 0 ? h[0] : (wi == 1 ? h[1] : (wi == 2 ? h[2] : h[3]));
  const uint64_t differ = ~__ballot(mine == hdr);
  *nb = 5u + wi;
  return differ ? (uint32_t)__builtin_ctzll(differ) : 64u;
}

// flat_expand: kRuns full runs of 512 values of nb bytes each with one wave,
// run q's packed data at descriptor offset d + q * dstep, its values at
// out + q * ostep. Each lane loads the three dwords at the aligned-down
// address of its value (expand_run's extract, from memory instead of LDS);
// all of the loads are issued before the first store.
template <int kRuns, typename T>
__device__ __forceinline__ void flat_expand(__amdgpu_buffer_rsrc_t rs, uint32_t d, uint32_t dstep, uint32_t nb,
                                            int is_signed, T* out, uint32_t ostep, int lane) {
  u32x3 w[kRuns][kMaxRunUnroll];
#pragma unroll
  for (int q = 0; q < kRuns; ++q) {
#pragma unroll
    for (int it = 0; it < kMaxRunUnroll; ++it) {
      const uint32_t rel = d + (uint32_t)q * dstep + (uint32_t)(it * kWave + lane) * nb;
      const auto t = __builtin_amdgcn_raw_buffer_load_b96(rs, rel & ~3u, 0, 2);
      w[q][it].x = t[0];
      w[q][it].y = t[1];
      w[q][it].z = t[2];
    }
  }
#pragma unroll
  for (int q = 0; q < kRuns; ++q) {
#pragma unroll
    for (int it = 0; it < kMaxRunUnroll; ++it) {
      const uint32_t j = (uint32_t)(it * kWave + lane);
      const uint32_t rel = d + (uint32_t)q * dstep + j * nb;
      uint64_t v = field(w[q][it], rel, 0, 8u * nb);
      if (is_signed) v = unzigzag(v);
      store1(out + (uint32_t)q * ostep + j, v);
    }
  }
}

// flat_expand16 (kOptFlat16): flat_expand for W=64 runs, two values per lane.
// A run's payload starts at descriptor offset d = a + s, a = d & ~15: the
// shift s (0-15) is the same for the whole run, so the wave loads the payload
// as aligned 16-byte chunks (chunk it * 64 + lane in iteration it, 0-3, and
// chunk 256 one dword per lane: lane e0 + k holds its dword k) and lane l's value pair 2 * (it * 64 + l) is bytes
// [s, s + 16) of its own chunk followed by its right neighbour's: the
// neighbour's dwords come by a one-lane DPP shift (lane 63 takes lane 0 of
// the next iteration's chunk, or chunk 256), the dword offset s >> 2 picks
// the code (flat16_run<K>, a wave-uniform branch), v_alignbyte shifts by
// s & 3. The chunks reach up to 15 bytes past the payload (chunk 256 is
// loaded whatever s is) and their addresses are not left to the descriptor's
// range check (the run's start is the scalar offset): the caller takes a run this way only if it ends 16
// bytes or more before the descriptor's end. cnt <= kRuns runs (q-th at
// d + q * dstep, values at out + q * ostep), all loads before the first
// store; a pair is two 8-byte stores.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// lane i takes lane i + 1's x (wave_shl:1), lane 63 takes `last`
__device__ __forceinline__ uint32_t next_lane(uint32_t x, uint32_t last) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)last, (int)x, 0x130, 0xf, 0xf, false);
}

template <int K>
__device__ __forceinline__ void flat16_run(const u32x4 (&c)[4], uint32_t e, int e0, uint32_t r, int is_signed,
                                           int64_t* out, int lane) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    uint32_t D[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) D[k] = c[it][k];
#pragma unroll
    for (int k = 0; k <= K; ++k) D[4 + k] = next_lane(c[it][k], it < 3 ? uni(c[it < 3 ? it + 1 : 3][k]) : rdlane(e, e0 + k));
    uint64_t v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t lo = __builtin_amdgcn_alignbyte(D[K + 2 * h + 1], D[K + 2 * h], r);
      const uint32_t hi = __builtin_amdgcn_alignbyte(D[K + 2 * h + 2], D[K + 2 * h + 1], r);
      v[h] = ((uint64_t)__builtin_bswap32(lo) << 32) | __builtin_bswap32(hi);
      if (is_signed) v[h] = unzigzag(v[h]);
    }
    // the lane's 16 bytes + a constant: the loads' vector offset serves the stores too
    int64_t* const o = (int64_t*)((char*)out + 16u * (uint32_t)lane) + 2 * kWave * it;
    store1(o, v[0]);
    store1(o + 1, v[1]);
  }
}

template <int kRuns>
__device__ __forceinline__ void flat_expand16(__amdgpu_buffer_rsrc_t rs, uint32_t d, uint32_t dstep, uint32_t cnt,
                                              int is_signed, int64_t* out, uint32_t ostep, int lane) {
  cnt = uni(cnt);
  d = uni(d);
  u32x4 c[kRuns][4];
  // the chunks' addresses: the lane's 16 bytes as the vector offset, the
  // run's (wave-uniform) aligned start as the scalar one
  const uint32_t l16 = 16u * (uint32_t)lane;
#pragma unroll
  for (int q = 0; q < kRuns; ++q) {
    if ((uint32_t)q < cnt) {
      const uint32_t a = (d + (uint32_t)q * dstep) & ~15u;
#pragma unroll
      for (int it = 0; it < 4; ++it)
        c[q][it] = __builtin_amdgcn_raw_buffer_load_b128(rs, l16, a + 1024u * (uint32_t)it, 2);
    }
  }
  // chunk 256 of every run in one register: lane 4 * q + k holds dword k of
  // run q's (the lanes past the last run load the last run's again)
  static_assert(4 * kRuns <= kWave, "one lane per dword of the runs' last chunks");
  const uint32_t eq = (uint32_t)lane >> 2 < cnt ? (uint32_t)lane >> 2 : cnt - 1u;
  const uint32_t e =
      __builtin_amdgcn_raw_buffer_load_b32(rs, ((d + eq * dstep) & ~15u) + 4096u + 4u * ((uint32_t)lane & 3u), 0, 2);
#pragma unroll
  for (int q = 0; q < kRuns; ++q) {
    if ((uint32_t)q < cnt) {
      const uint32_t s = (d + (uint32_t)q * dstep) & 15u;
      int64_t* const o = out + (uint32_t)q * ostep;
      switch (s >> 2) {
        case 0: flat16_run<0>(c[q], e, 4 * q, s & 3u, is_signed, o, lane); break;
        case 1: flat16_run<1>(c[q], e, 4 * q, s & 3u, is_signed, o, lane); break;
        case 2: flat16_run<2>(c[q], e, 4 * q, s & 3u, is_signed, o, lane); break;
        default: flat16_run<3>(c[q], e, 4 * q, s & 3u, is_signed, o, lane); break;
      }
    }
  }
}

struct WalkResult {
  uint32_t n, stop, dpos, dval, items, shrt;  // shrt: stopped by the probe (short runs)
};

// Work items of a serial pass (the walk publishes item ends): a group of up
// to 64 consecutive short runs, expanded one lane per run, or one long /
// PATCHED_BASE run (flag kItemLong), expanded by a whole wave.
constexpr uint16_t kItemLong = 0x8000;
#ifndef ORCG_ITEM_MAX
#define ORCG_ITEM_MAX 64
#endif
constexpr uint32_t kItemMax = ORCG_ITEM_MAX;  // short runs per group (<= 64)

// The serial walk's view of a run: bytes, values and the error parse_run
// would report, in its order. SHORT_REPEAT / DIRECT from the first two
// bytes, DELTA from a terminator mask of the 24 bytes after its header
// (two varints of <= 11 bytes: every writer's); PATCHED_BASE and longer
// varints through parse_run.
__device__ __forceinline__ void walk_extent(const LaneWin& hw, uint32_t lp, uint32_t avail, int is_signed,
                                            uint32_t* bytes, uint32_t* L, uint32_t* err, uint32_t* rkind) {
  const uint32_t fb = hw.byte(lp), kind = fb >> 6;
  *err = kErrNone;
  *rkind = kind;
  if (kind < 2) {
    // SHORT_REPEAT / DIRECT, straight-line scalar code (a DIRECT run short
    // of its second header byte has >= 2 bytes > avail: the same bad read)
    const uint32_t L2 = ((fb & 1u) << 8 | hw.byte(lp + 1)) + 1u;
    const uint32_t db = 2u + (fbs_width((fb >> 1) & 0x1fu) * L2 + 7u) / 8u;
    *bytes = kind ? db : 2u + ((fb >> 3) & 7u);
    *L = kind ? L2 : (fb & 7u) + 3u;
    if (*bytes > avail) *err = kErrBadRead;
    return;
  }
  if (kind != 2) {
    if (avail < 2) {
      *err = kErrBadRead;
      *bytes = 0;
      *L = 0;
      return;
    }
    const uint32_t L2 = ((fb & 1u) << 8 | hw.byte(lp + 1)) + 1u;
    const uint32_t code = (fb >> 1) & 0x1fu;
    // DELTA: varint lengths from the terminator mask of bytes lp+2 .. lp+25
    // (the slice's per-dword terminator nibbles, gathered and realigned)
    const uint32_t o = lp + 2u - hw.base, i0 = o >> 2, sh = o & 3u;
    uint32_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < 7; ++k) t |= rdlane(hw.t4, i0 + k) << (4 * k);
    t = (t >> sh) & 0xffffffu;
    const uint32_t n1 = t ? (uint32_t)__builtin_ctz(t) + 1u : 32u;
    const uint32_t t2 = n1 < 24 ? t >> n1 : 0u;
    const uint32_t n2 = t2 ? (uint32_t)__builtin_ctz(t2) + 1u : 32u;
    if (n1 <= 11 && n2 <= 11) {
      const uint32_t W = code ? fbs_width(code) : 0u;
      *L = L2;
      if (2u + n1 + n2 > avail) {
        *err = kErrBadRead;
        return;
      }
      if (W != 0 && L2 < 2) {
        *err = kErrDeltaLength;
        return;
      }
      *bytes = 2u + n1 + n2 + (W ? (W * (L2 - 2u) + 7u) / 8u : 0u);
      if (*bytes > avail) *err = kErrBadRead;
      return;
    }
  }
  const Run r = parse_run([&](uint32_t i) { return hw.byte(lp + i); }, avail, kHdrLim, is_signed);
  *bytes = r.bytes;
  *L = r.L;
  *err = r.err;
}

// Wave-uniform header walk over the window [wpos, wpos + kWin): records runs
// starting at pos.. into (run_off, run_val) until the next run starts past
// kWin - kMaxRun and does not end inside the loaded bytes (`lim`), leaves the
// segment, or the table is full. With `pub` the
// walk also cuts the runs into work items (`items`, ends by run index) and
// publishes the item count as items close, so expanding waves start early.
// (`cap` is kCap at every call; it stays a run-time argument because the
// compiler lays the walk's loop out differently for a literal bound.)
template <uint32_t kWin, uint32_t kCap, typename OffT>
__device__ __forceinline__ WalkResult walk(const uint32_t* win, OffT* run_off, uint32_t* run_val,
                                           uint64_t wpos, uint64_t pos, uint64_t vi, uint64_t seg_end,
                                           uint64_t src_len, uint64_t value_end, int is_signed,
                                           unsigned long long* err, int lane, uint32_t lim, uint32_t cap,
                                           uint32_t* pub, uint16_t* items, uint32_t probe_n, bool probe_values) {
  static_assert(kCap < kItemLong, "run indices must leave the item flag free");
  constexpr uint32_t kChunk = kWin - kMaxRun;
  // everything wave-uniform and 32-bit, relative to the window / the first
  // value: the loop stays on the scalar unit (no 64-bit VALU compares)
  const uint32_t sp = (uint32_t)(pos - wpos);
  const uint32_t a_seg = seg_end - wpos < 0xfffff000ull ? (uint32_t)(seg_end - wpos) : 0xfffff000u;
  const uint32_t a_src = src_len - wpos < 0xfffff000ull ? (uint32_t)(src_len - wpos) : 0xfffff000u;
  const uint32_t v_lim = value_end - vi < 0xffffffffull ? (uint32_t)(value_end - vi) : 0xffffffffu;
  uint32_t lp = sp, vr = 0;
  uint32_t n = 0, stop = 0, shrt = 0;
  LaneWin hw;
  hw.load(win, sp, kWin / 4 + 8, lane);
  // run k waits in lane k % 64 (r_off, r_val) until the table write of its
  // batch: one LDS round trip (and one release store) per item or per 64
  // runs instead of one per run
  uint32_t r_off = 0, r_val = 0, flushed = 0, gstart = 0, nitems = 0;
  auto flush = [&]() {
    const uint32_t r = flushed + (((uint32_t)lane - flushed) & (kWave - 1));
    if (r < n) {
      run_off[r] = (OffT)r_off;
      run_val[r] = r_val;
    }
    flushed = n;
  };
  const uint32_t lim_all = uni(min(min(a_src, a_seg), lim));
  const bool items_on = uni(pub != nullptr ? 1u : 0u) != 0;
  while (lp < a_seg && vr < v_lim && n < cap) {
    // a run starting past the chunk is taken only when all of its bytes are
    // loaded (its extent depends on its own bytes only); otherwise it starts
    // the next window
    const bool past = lp >= kChunk && n > 0;
    if (past && lp + 2u > lim) break;
    if (lp + kHdrLim > hw.base + 256) hw.load(win, lp, kWin / 4 + 8, lane);
    // the two header bytes from two lanes of the slice, realigned on the
    // scalar unit; SHORT_REPEAT / DIRECT sized inline (branch-free selects),
    // DELTA / PATCHED_BASE through walk_extent
    const uint32_t o = lp - hw.base, wi = o >> 2;
    const uint64_t w2 = ((uint64_t)rdlane(hw.word, wi + 1) << 32) | rdlane(hw.word, wi);
    const uint32_t hdr = (uint32_t)(w2 >> ((o & 3u) * 8u));
    const uint32_t fb = hdr & 0xffu, kind = fb >> 6;
    uint32_t rbytes, rL, e = kErrNone;
    if (kind < 2) {
      const uint32_t L2 = ((fb & 1u) << 8 | ((hdr >> 8) & 0xffu)) + 1u;
      const uint32_t code = (fb >> 1) & 0x1fu;
      const uint32_t wt = (uint32_t)(0x40383028201E1C1Aull >> (((code - 24u) & 7u) * 8u)) & 0xffu;
      const uint32_t W = code < 24 ? code + 1u : wt;  // fbs_width
      uint32_t bits;
      asm("s_mul_i32 %0, %1, %2" : "=s"(bits) : "s"(uni(W)), "s"(uni(L2)));
      rbytes = kind ? 2u + ((bits + 7u) >> 3) : 2u + ((fb >> 3) & 7u);
      rL = kind ? L2 : (fb & 7u) + 3u;
    } else {
      uint32_t kd;
      walk_extent(hw, lp, a_src - lp, is_signed, &rbytes, &rL, &e, &kd);
      rbytes = uni(rbytes);  // keep the merged values scalar
      rL = uni(rL);
      e = uni(e);
    }
    if (past && (e != kErrNone || lp + rbytes > lim)) break;  // the next window decides
    if (e != kErrNone || lp + rbytes > lim_all) {
      // the first failing check, in the order parse / segment / window
      if (e == kErrNone)
        e = lp + rbytes > a_src ? kErrBadRead : (lp + rbytes > a_seg ? kErrBadSegment : kErrBadRead);
      if (lane == 0) report(err, vi + vr, e);
      stop = 1;
      break;
    }
    // a per-lane select, not v_writelane: the compiler may copy r_off /
    // r_val with a partial EXEC inside a branch it cannot prove uniform, which
    // is only safe when no lane's value is written by another lane
    const bool mine = (uint32_t)lane == (n & (kWave - 1));
    r_off = mine ? lp : r_off;
    r_val = mine ? vr : r_val;
    ++n;
    lp += rbytes;
    vr += rL;
    if (items_on) {
      if (rL > kShortL || kind == 2) {
        // close the open group of short runs, then this run as its own item
        flush();
        const uint32_t grp = n - 1 > gstart ? 1u : 0u;
        if (lane == 0) {
          if (grp) items[nitems] = (uint16_t)(n - 1);
          items[nitems + grp] = (uint16_t)(n | kItemLong);
        }
        nitems += grp + 1;
        gstart = n;
        // expanding waves may claim the items as soon as they are published
        if (lane == 0) __hip_atomic_store(pub, nitems, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else if (n - gstart == kItemMax) {
        flush();
        if (lane == 0) items[nitems] = (uint16_t)n;
        ++nitems;
        gstart = n;
        if (lane == 0) __hip_atomic_store(pub, nitems, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    } else if (n - flushed == kWave) {
      flush();
    }
    // the probe: the first probe_n runs of a segment average < kToDense
    // bytes (a short-run segment), the caller switches to dense discovery
    // (probe_values: their values average <= kShortL, whatever their bytes)
    if (n == probe_n && (probe_values ? vr <= probe_n * kShortL : lp - sp < probe_n * kToDense)) {
      shrt = 1;
      break;
    }
  }
  if (n != flushed) flush();
  if (pub && n > gstart) {
    // the last group: published by the caller's final (walk done) store
    if (lane == 0) items[nitems] = (uint16_t)n;
    ++nitems;
  }
  return WalkResult{n, stop, lp - sp, vr, nitems, shrt};
}

// Value j of a short run (kind SHORT_REPEAT / DIRECT / DELTA) parsed at
// window offset `hoff`; `acc` carries a variable-width DELTA run's |delta| sum.
__device__ __forceinline__ uint64_t short_value(const uint32_t* win, const Run& r, uint32_t hoff, uint32_t j,
                                                int is_signed, uint64_t& acc) {
  if (r.kind == 0) return r.a;
  if (r.kind == 1) {
    const uint32_t bit = j * r.W;
    const uint32_t br = hoff + r.data + (bit >> 3);
    uint64_t v = field(lds12(win, br), br, bit & 7u, r.W);
    return is_signed ? unzigzag(v) : v;
  }
  if (r.W == 0) return r.a + (uint64_t)j * r.b;
  if (j == 0) return r.a;
  const uint64_t v1 = r.a + r.b;
  if (j == 1) return v1;
  const uint32_t bit = (j - 2) * r.W;
  const uint32_t br = hoff + r.data + (bit >> 3);
  acc += field(lds12(win, br), br, bit & 7u, r.W);
  return (int64_t)r.b < 0 ? v1 - acc : v1 + acc;
}

// Expand runs [r0, r1) (r1 - r0 <= 64, each SHORT_REPEAT / DIRECT / DELTA of
// <= kShortL values) one lane per run, storing straight to the output.
template <typename T, typename OffT>
__device__ __forceinline__ void group_expand(const uint32_t* win, const OffT* s_off, const uint32_t* s_val,
                                             uint32_t r0, uint32_t r1, uint64_t vi, int is_signed,
                                             uint64_t value_begin, uint64_t value_end, T* dst, int lane) {
  const uint32_t r = r0 + (uint32_t)lane;
  const bool act = r < r1;
  const uint32_t hoff = act ? s_off[r] : s_off[r0];
  const uint64_t o0 = vi + (act ? s_val[r] : 0u);
  const uint32_t w0 = hoff >> 2, sh = hoff & 3u;
  const uint32_t d0 = win[w0], d1 = win[w0 + 1], d2 = win[w0 + 2], d3 = win[w0 + 3];
  const uint32_t b0 = __builtin_amdgcn_alignbyte(d1, d0, sh), b1 = __builtin_amdgcn_alignbyte(d2, d1, sh),
                 b2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
  const uint32_t fb = b0 & 0xffu;
  if (__ballot(act && (fb >> 6) != 0) == 0) {
    // SHORT_REPEAT only: W + 1 value bytes, big endian
    const uint32_t L = act ? (fb & 7u) + 3u : 0u;
    const uint32_t nb = ((fb >> 3) & 7u) + 1u;
    const uint64_t be = ((uint64_t)__builtin_bswap32(__builtin_amdgcn_alignbyte(b1, b0, 1)) << 32) |
                        __builtin_bswap32(__builtin_amdgcn_alignbyte(b2, b1, 1));
    uint64_t a = be >> (64 - 8 * nb);
    if (is_signed) a = unzigzag(a);
    ORCG_COVER_ADD(L);
    for (uint32_t j = 0; __ballot(j < L) != 0; ++j) {
      const uint64_t o = o0 + j;
      if (j < L && o >= value_begin && o < value_end) store1(dst + (o - value_begin), a);
    }
    return;
  }
  const Run run = parse_run([&](uint32_t i) { return lds_byte(win, hoff + i); }, ~0ull, kHdrLim, is_signed);
  const uint32_t L = act ? run.L : 0u;
  ORCG_COVER_ADD(L);
  uint64_t acc = 0;
  for (uint32_t j = 0; __ballot(j < L) != 0; ++j) {
    const uint64_t o = o0 + j;
    if (j < L) {
      const uint64_t x = short_value(win, run, hoff, j, is_signed, acc);
      if (o >= value_begin && o < value_end) store1(dst + (o - value_begin), x);
    }
  }
}

// ---- dense mode -----------------------------------------------------------

struct DenseResult {
  uint32_t n, stop, dpos, dval;
};

// Header of the run at window offset lq, with every check the serial walk
// applies (same order): truncated stream, run past the segment, run past the
// loaded bytes. Returns the error code (kErrNone when the run is good).
__device__ __forceinline__ uint32_t checked_run(const uint32_t* win, uint32_t lq, uint64_t wpos, uint64_t seg_end,
                                                uint64_t src_len, uint32_t need, int is_signed, Run* out) {
  const uint64_t pabs = wpos + lq;
  const uint64_t avail = pabs < src_len ? src_len - pabs : 0;
  const Run r = parse_run([&](uint32_t i) { return lds_byte(win, lq + i); }, avail, kHdrLim, is_signed);
  uint32_t e = r.err;
  if (e == kErrNone && pabs + r.bytes > seg_end) e = kErrBadSegment;
  if (e == kErrNone && lq + r.bytes > need) e = kErrBadRead;
  *out = r;
  return e;
}

// ---- dense discovery ---------------------------------------------------
// Shaped for the CDNA issue model (divergent branches cost SALU exec-mask
// bookkeeping per decoded value):
//  * the speculative header parse at every position is branch-free (all
//    kinds computed, selected by kind) and the in-block DP lives in
//    registers, indexed at compile time (select chains), not through LDS;
//  * PATCHED_BASE headers and DELTA varints over 10 bytes are "unknown" to
//    the DP: a block whose path meets one re-walks exactly (checked_run);
//    such a block also ends the pass;
//  * the chain goes by hops over two u16 LDS tables (block exits, 64-byte
//    super-block exits), three barriers;
//  * a block's runs come from a forward pass over the DP registers (no
//    header re-parse), appended to the run table with predicated writes.
constexpr uint32_t kDpUnknown = 0x80000000u;

// FBSToBitWidthMap without a branch (RLEV2Util.cc:24-26)
__device__ __forceinline__ uint32_t fbs_width_nb(uint32_t code) {
  const uint32_t hi = (uint32_t)((0x40383028201E1C1Aull >> (8 * ((code - 24u) & 7u))) & 0xffu);
  return code < 24 ? code + 1 : hi;
}

template <typename OffT>
__device__ __forceinline__ DenseResult dense2_discover(const uint32_t* win, OffT* s_off, uint32_t* s_val,
                                                       uint16_t* s_nxt, uint32_t* s_mark, uint32_t* s_ctl,
                                                       uint64_t wpos, uint32_t sb, uint32_t lim, uint64_t vi,
                                                       uint64_t seg_end, uint64_t src_len, uint64_t value_end,
                                                       uint32_t need, int is_signed, unsigned long long* err,
                                                       int tid
#ifdef ORCG_PHASE_PROF
                                                       , uint64_t& prof_last_
#endif
) {
  const int wave = tid / kWave, lane = tid % kWave;
  const uint32_t lo = (uint32_t)tid * kBlk, hi = lo + kBlk;
  __builtin_amdgcn_s_setprio(2);
  // runs may not start at or past the segment end
  {
    const uint64_t sa = wpos + sb;
    const uint64_t seg_room = seg_end > sa ? seg_end - sa : 0;
    if (seg_room < lim) lim = (uint32_t)seg_room;
  }
  // (1) per position e of the block: ent[e] = exit (first run start past the
  // block on the path from e) | values on the path << 15, or kDpUnknown;
  // info (two positions per register): in-block successor (e + run bytes,
  // 15 = past the block) | L << 4
  uint32_t ent[kBlk], info2[kBlk / 2];
  {
    const uint32_t a0 = sb + lo, sh = a0 & 3u, w0 = a0 >> 2;
    uint32_t b4[kBlk / 4 + 8];
    {
      uint32_t prev = win[w0];
#pragma unroll
      for (int i = 0; i < (int)kBlk / 4 + 8; ++i) {
        const uint32_t nx = win[w0 + i + 1];
        b4[i] = __builtin_amdgcn_alignbyte(nx, prev, sh);
        prev = nx;
      }
    }
    uint64_t term = 0;  // bit i: byte i < 0x80 (varint terminators)
#pragma unroll
    for (int i = 0; i < (int)kBlk / 4 + 8 && i < 16; ++i) {
      const uint32_t m = (~b4[i] >> 7) & 0x01010101u;
      term |= (uint64_t)((m * 0x10204080u) >> 28) << (4 * i);
    }
    auto B = [&](int i) -> uint32_t { return (b4[i >> 2] >> ((i & 3) * 8)) & 0xffu; };
    // bytes from block byte 0 that a run may use: inside the stream, the
    // segment and the loaded window
    const uint64_t pblk = wpos + sb + lo;
    const uint64_t lim_abs = src_len < seg_end ? src_len : seg_end;
    const uint64_t r1 = lim_abs > pblk ? lim_abs - pblk : 0;
    const uint32_t r2 = need > sb + lo ? need - (sb + lo) : 0u;
    const uint32_t room0 = r1 < (uint64_t)r2 ? (uint32_t)r1 : r2;
#pragma unroll
    for (int e = (int)kBlk - 1; e >= 0; --e) {
      const uint32_t fb = B(e), b1 = B(e + 1);
      const uint32_t kind = fb >> 6, code = (fb >> 1) & 0x1fu;
      const uint32_t W = fbs_width_nb(code);
      const uint32_t L2 = ((fb & 1u) << 8 | b1) + 1u;
      const uint32_t sr_bytes = 2u + ((fb >> 3) & 7u), sr_L = (fb & 7u) + 3u;
      const uint32_t di_bytes = 2u + (W * L2 + 7u) / 8u;
      const uint32_t Wd = code ? W : 0u;
      const uint64_t t1 = term >> (e + 2);
      const uint32_t n1 = t1 ? (uint32_t)__builtin_ctzll(t1) + 1u : 64u;
      const uint64_t t2 = n1 < 32 ? t1 >> n1 : 0ull;
      const uint32_t n2 = t2 ? (uint32_t)__builtin_ctzll(t2) + 1u : 64u;
      const bool de_ok = n1 <= 10 && n2 <= 10 && !(Wd != 0 && L2 < 2);
      const uint32_t de_bytes = 2u + n1 + n2 + (Wd ? (Wd * (L2 - 2u) + 7u) / 8u : 0u);
      const uint32_t bytes = kind == 0 ? sr_bytes : (kind == 1 ? di_bytes : de_bytes);
      const uint32_t L = kind == 0 ? sr_L : L2;
      const uint32_t room = room0 > (uint32_t)e ? room0 - (uint32_t)e : 0u;
      const bool ok = kind != 2 && (kind != 3 || de_ok) && bytes <= room;
      const uint32_t nx = (uint32_t)e + bytes;
      const uint32_t inf = (nx < 15u ? nx : 15u) | (L << 4);
      if (e & 1) info2[e >> 1] = inf << 16;
      else info2[e >> 1] |= inf;
      uint32_t sel = lo + nx;  // the exit when the run leaves the block
      bool past = true;
#pragma unroll
      for (int k = e + 2; k < (int)kBlk; ++k) {
        if (nx == (uint32_t)k) {
          sel = ent[k];
          past = false;
        }
      }
      const bool path_ok = past || !(sel & kDpUnknown);
      ent[e] = (ok && path_ok) ? (past ? sel | (L << 15) : sel + (L << 15)) : kDpUnknown;
    }
  }
  PROF_MARK(3);
  // (2) every block's entry on the chain from slab position 0, by hops:
  // O(slab) work in three barriers. ta = each position's block exit; tb = its
  // 64-byte super-block exit (<= 7 hops over ta, every thread for its 8
  // positions); one lane hops the <= 32 super-blocks from position 0 and
  // records each one's first chain position; every thread hops from its
  // super-block's entry to its own block (<= 7 hops).
  bool has = false;
  uint32_t eb = 0;
  {
    uint32_t na[kBlk];
  #pragma unroll
    for (int e = 0; e < (int)kBlk; ++e) {
      const uint32_t x = ent[e] & 0x7fffu;
      na[e] = ((ent[e] & kDpUnknown) || x >= lim) ? (uint32_t)kSink : x;
    }
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    auto put8 = [&](uint16_t* t) {
      u4 w;
      w.x = na[0] | na[1] << 16;
      w.y = na[2] | na[3] << 16;
      w.z = na[4] | na[5] << 16;
      w.w = na[6] | na[7] << 16;
      *(u4*)(t + lo) = w;
    };
    uint16_t* ta = s_nxt;
    uint16_t* tb = s_nxt + kSlab;
    put8(ta);
    constexpr uint32_t kSup = 8u * kBlk;
    __syncthreads();
    {
      const uint32_t send = (lo / kSup + 1u) * kSup;
      uint32_t q[kBlk];
  #pragma unroll
      for (int e = 0; e < (int)kBlk; ++e) q[e] = na[e];
  #pragma unroll
      for (int h = 0; h < 7; ++h) {
  #pragma unroll
        for (int e = 0; e < (int)kBlk; ++e) {
          const bool in = q[e] != kSink && q[e] < send;
          const uint32_t v = ta[in ? q[e] : lo + (uint32_t)e];
          q[e] = in ? v : q[e];
        }
      }
      typedef uint32_t u4h __attribute__((ext_vector_type(4)));
      u4h w;
      w.x = q[0] | q[1] << 16;
      w.y = q[2] | q[3] << 16;
      w.z = q[4] | q[5] << 16;
      w.w = q[6] | q[7] << 16;
      *(u4h*)(tb + lo) = w;
    }
    if (tid < (int)(kSlab / kSup)) s_mark[tid] = kSink;  // the super-blocks' chain entries
    __syncthreads();
    if (tid == 0) {
      uint32_t p = 0;
      while (p != kSink && p < lim) {
        s_mark[p / kSup] = p;
        p = tb[p];
      }
    }
    __syncthreads();
    {
      uint32_t p = s_mark[lo / kSup];
      for (int h = 0; h < 7 && p != kSink && p < lo; ++h) p = ta[p];
      has = p != kSink && p >= lo && p < hi && p < lim;
      eb = has ? p - lo : 0u;
    }
    static_assert(kSlab / kSup <= kSlab / 32, "super-block entries fit the marks");
  }
  PROF_MARK(4);
  // (3) the block's entry, its runs (a forward pass over the DP registers),
  // one combined scan of the values and run counts
  uint32_t ee = ent[0];
#pragma unroll
  for (int k = 1; k < (int)kBlk; ++k) ee = eb == (uint32_t)k ? ent[k] : ee;
  const bool exact = has && (ee & kDpUnknown);
  uint32_t cnt = 0, pk_off = 0, cum = 0, p_end = ee & 0x7fffu;
  uint64_t pk_val = 0;
  bool stopped = false;
  if (has && !exact) {
    uint32_t reach = 1u << eb;
#pragma unroll
    for (int e = 0; e < (int)kBlk; ++e) {
      const bool on = ((reach >> e) & 1u) && !stopped;
      const bool st = on && lo + (uint32_t)e >= lim;
      p_end = st ? lo + (uint32_t)e : p_end;
      stopped = stopped || st;
      const bool em = on && !st;
      const uint32_t inf = (info2[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
      const uint32_t nx = inf & 15u, Le = inf >> 4;
      pk_off |= em ? (uint32_t)e << (3 * cnt) : 0u;
      pk_val |= em ? (uint64_t)cum << (16 * cnt) : 0ull;
      cnt += em ? 1u : 0u;
      reach |= (em && nx < kBlk) ? 1u << nx : 0u;
      cum += em ? Le : 0u;
    }
  }
  uint32_t* s_wsum = s_ctl + 4;  // [0..3] value totals, [4..7] run-count totals of the waves
  const uint32_t vincl = wave_scan_u32(cum), cincl = wave_scan_u32(cnt);
  if (lane == kWave - 1) {
    s_wsum[wave] = vincl;
    s_wsum[4 + wave] = cincl;
  }
  if (tid == 0) {
    s_ctl[3] = 0;       // stop (corrupt run)
    s_ctl[12] = kNone;  // first block whose walk stopped inside it
    s_ctl[13] = 0;      // last block with an entry
    s_ctl[14] = 0;      // runs of the exact-walk block
  }
  __syncthreads();
  uint32_t vb = vincl - cum, base = cincl - cnt;
  for (int w = 0; w < wave; ++w) {
    vb += s_wsum[w];
    base += s_wsum[4 + w];
  }
  uint32_t total = s_wsum[4] + s_wsum[5] + s_wsum[6] + s_wsum[7];
  uint32_t v_end = vb + cum;
  if (exact) {
    // the path meets a run the DP cannot vouch for (it is the pass's last
    // block with an entry): walk it exactly
    uint32_t p = lo + eb, v = vb;
    while (p < hi && p < lim && vi + v < value_end) {
      Run r;
      const uint32_t e = checked_run(win, sb + p, wpos, seg_end, src_len, need, is_signed, &r);
      if (e != kErrNone) {
        report(err, vi + v, e);
        s_ctl[3] = 1;
        break;
      }
      pk_off |= (p - lo) << (3 * cnt);
      pk_val |= (uint64_t)(v - vb) << (16 * cnt);
      ++cnt;
      p += r.bytes;
      v += r.L;
    }
    stopped = p < hi;
    p_end = p;
    v_end = v;
    s_ctl[14] = cnt;
  }
  {
    // one atomic per wave: its first stopped lane, its last lane with an entry
    const uint64_t bs = __ballot(has && stopped), bh = __ballot(has);
    if (bs && lane == __builtin_ctzll(bs)) atomicMin(&s_ctl[12], (uint32_t)tid);
    if (bh && lane == 63 - __builtin_clzll(bh)) atomicMax(&s_ctl[13], (uint32_t)tid);
  }
  // the successor tables are dead: the run table may overwrite them
  __syncthreads();
  {
    const uint32_t fin = s_ctl[12] != kNone ? s_ctl[12] : s_ctl[13];
    if ((uint32_t)tid == fin) {
      s_ctl[1] = p_end;
      s_ctl[2] = v_end;
    }
  }
  total += s_ctl[14];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k)
    if (k < cnt) {
      s_off[base + k] = (OffT)(sb + lo + ((pk_off >> (3 * k)) & 7u));
      s_val[base + k] = vb + (uint32_t)((pk_val >> (16 * k)) & 0xffffu);
    }
  __syncthreads();
  PROF_MARK(5);
  __builtin_amdgcn_s_setprio(0);
  return DenseResult{uni(total), uni(s_ctl[3]), uni(s_ctl[1]), uni(s_ctl[2])};
}

// Expand runs [r0, r1) of the run table with one wave: maximal groups of
// consecutive short runs (<= kStage values) are decoded one lane per run into
// the wave's LDS stage and flushed with coalesced stores; any other run
// (long, PATCHED_BASE) goes through expand_run.
template <typename T, typename OffT>
__device__ __forceinline__ void dense_expand(const uint32_t* win, uint32_t nwords, const OffT* s_off,
                                             const uint32_t* s_val, uint64_t* stage, uint32_t r0, uint32_t r1,
                                             uint64_t vi, int is_signed, uint64_t value_begin, uint64_t value_end,
                                             T* dst, int lane) {
  uint32_t c = r0;
  while (c < r1) {
    const uint32_t r = c + (uint32_t)lane;
    const bool act = r < r1;
    const uint32_t hoff = act ? s_off[r] : s_off[c];
    const uint32_t val = act ? s_val[r] : 0u;
    // the run's first 12 bytes in registers (one LDS round trip)
    const uint32_t w0 = hoff >> 2, sh = hoff & 3u;
    const uint32_t d0 = win[w0], d1 = win[w0 + 1], d2 = win[w0 + 2], d3 = win[w0 + 3];
    const uint32_t b0 = __builtin_amdgcn_alignbyte(d1, d0, sh), b1 = __builtin_amdgcn_alignbyte(d2, d1, sh),
                   b2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
    const uint32_t fb = b0 & 0xffu;
    Run run;
    if (__ballot(act && (fb >> 6) != 0) == 0) {
      // SHORT_REPEAT only (low-cardinality streams): W + 1 value bytes, big endian
      run.kind = 0;
      run.L = (fb & 7u) + 3u;
      const uint32_t nb = ((fb >> 3) & 7u) + 1u;
      const uint64_t be = ((uint64_t)__builtin_bswap32(__builtin_amdgcn_alignbyte(b1, b0, 1)) << 32) |
                          __builtin_bswap32(__builtin_amdgcn_alignbyte(b2, b1, 1));
      const uint64_t v = be >> (64 - 8 * nb);
      run.a = is_signed ? unzigzag(v) : v;
      run.W = 8 * nb;
      run.data = 1;
      run.b = 0;
    } else {
      run = parse_run([&](uint32_t i) { return lds_byte(win, hoff + i); }, ~0ull, kHdrLim, is_signed);
    }
    // SHORT_REPEAT, DIRECT and constant-step DELTA runs of kVparMin + 1 ..
    // kVparL values are expanded value-parallel (below); short runs (<=
    // kShortL) one lane per run through the stage; the rest (long runs,
    // PATCHED_BASE) by the whole wave each
    // Short runs stay one lane per run (their stage flush needs them
    // consecutive) unless the longer runs between them cut them into more
    // than kVparFrag groups (low-cardinality dictionary indices: a flush per
    // group of a few runs); then every eligible run goes value-parallel
    const bool elig = act && run.L <= kVparL && (run.kind <= 1 || (run.kind == 3 && run.W == 0));
    const bool sh0 = act && run.kind != 2 && run.L <= kShortL;
    const uint64_t shm = __ballot(sh0);
    const bool frag = (uint32_t)__builtin_popcountll(shm & ~(shm << 1)) > kVparFrag;
    const bool vpr = elig && (run.L > kVparMin || frag);
    const bool shortr = sh0 && !vpr;
    const uint32_t Ls = shortr ? run.L : 0u;
    const uint32_t incl = wave_scan_u32(Ls);
    // every run parsed here is expanded before the next 64 are parsed
    // (a mix of short and long runs, e.g. low-cardinality dictionary
    // indices, used to parse its 64 headers again after every long run):
    // first the runs of consecutive short runs, through the stage,
    // then each long / PATCHED_BASE run by the whole wave, once
    // the parsed runs are dead (fewer live registers around expand_run)
    const uint32_t nact = r1 - c < (uint32_t)kWave ? r1 - c : (uint32_t)kWave;
    const uint64_t longm = __ballot(act && !vpr && !shortr);
    {
      // value-parallel: lane o of each step takes value o of the runs'
      // concatenation, finds its run by a binary search over the runs' first
      // values (ds_bpermute, 6 steps), and decodes it by random access (a
      // lane per run left most lanes idle behind the longest run of the 64,
      // and runs of 17-256 values went one whole-wave expansion each: the
      // low-cardinality dictionary indices of C4 spent 120 us a workgroup
      // here)
      const uint32_t Lv = vpr ? run.L : 0u;
      const uint32_t inclv = wave_scan_u32(Lv);
      const uint32_t exclv = inclv - Lv;
      const uint32_t Tv = rdlane(inclv, kWave - 1);
      if (Tv) {
        const uint32_t pk = (hoff + run.data) | (run.W << 16) | (run.kind << 24);
        const uint32_t a_lo = (uint32_t)run.a, a_hi = (uint32_t)(run.a >> 32);
        const bool anyd = __ballot(vpr && run.kind == 3) != 0;
        for (uint32_t o = (uint32_t)lane; __ballot(o < Tv) != 0; o += kWave) {
          uint32_t lo = 0, hi = kWave;
#pragma unroll
          for (int st = 0; st < 6; ++st) {
            const uint32_t mid = (lo + hi) >> 1;
            const uint32_t e = (uint32_t)__shfl((int)exclv, (int)mid);
            if (e <= o) lo = mid;
            else hi = mid;
          }
          const uint32_t k = lo;
          const uint32_t p = (uint32_t)__shfl((int)pk, (int)k), e = (uint32_t)__shfl((int)exclv, (int)k);
          const uint32_t vk = (uint32_t)__shfl((int)val, (int)k);
          const uint64_t ak = (uint64_t)(uint32_t)__shfl((int)a_lo, (int)k) |
                              (uint64_t)(uint32_t)__shfl((int)a_hi, (int)k) << 32;
          const uint32_t j = o - e, kind = p >> 24;
          uint64_t x = ak;
          if (kind == 1) {
            const uint32_t W = (p >> 16) & 0xffu, bit = j * W, br = (p & 0xffffu) + (bit >> 3);
            const uint64_t v = field(lds12(win, br), br, bit & 7u, W);
            x = is_signed ? unzigzag(v) : v;
          }
          if (anyd) {
            const uint64_t bk = (uint64_t)(uint32_t)__shfl((int)(uint32_t)run.b, (int)k) |
                                (uint64_t)(uint32_t)__shfl((int)(uint32_t)(run.b >> 32), (int)k) << 32;
            if (kind == 3) x = ak + (uint64_t)j * bk;
          }
          const uint64_t g = vi + vk + j;
          if (o < Tv && g >= value_begin && g < value_end) store1(dst + (g - value_begin), x);
        }
        ORCG_COVER_ADD(vpr ? run.L : 0u);
      }
    }
    for (uint64_t rem = __ballot(shortr); rem;) {
      const uint32_t a = (uint32_t)__builtin_ctzll(rem);
      // short runs [a, b): consecutive in the output; a stage-full at most
      const uint32_t base = a ? rdlane(incl, a - 1) : 0u;
      const uint64_t stop_m = __ballot((uint32_t)lane >= a && (!shortr || incl - base > kStage));
      uint32_t b = stop_m ? (uint32_t)__builtin_ctzll(stop_m) : (uint32_t)kWave;
      if (b > nact) b = nact;
      rem &= b >= (uint32_t)kWave ? 0ull : ~((1ull << b) - 1ull);
      const bool mine = (uint32_t)lane >= a && (uint32_t)lane < b;
      const uint32_t myl = mine ? Ls : 0u;
      ORCG_COVER_ADD(myl);
      const uint32_t st0 = incl - Ls - base;
      if (__ballot(mine && run.kind != 0) == 0) {
        for (uint32_t j = 0; __ballot(j < myl) != 0; ++j)
          if (j < myl) stage[st0 + j] = run.a;
      } else {
        uint64_t acc = 0;
        for (uint32_t j = 0; __ballot(j < myl) != 0; ++j)
          if (j < myl) stage[st0 + j] = short_value(win, run, hoff, j, is_signed, acc);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint32_t tot = rdlane(incl, b - 1) - base;
      const uint64_t g0 = vi + rdlane(val, a);
      for (uint32_t o = (uint32_t)lane; o < tot; o += kWave) {
        const uint64_t g = g0 + o;
        if (g >= value_begin && g < value_end) store1(dst + (g - value_begin), stage[o]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    for (uint64_t m = longm; m; m &= m - 1) {
      const uint32_t a = (uint32_t)__builtin_ctzll(m);
#ifdef ORCG_DEBUG_COVER
      if (lane == 0) ORCG_COVER_ADD(parse_run([&](uint32_t i) { return lds_byte(win, uni(s_off[c + a]) + i); }, ~0ull,
                                              kHdrLim, is_signed).L);
#endif
      expand_run(win, nwords, uni(s_off[c + a]), vi + uni(s_val[c + a]), is_signed, value_begin, value_end, dst, lane);
    }
    c += nact;
  }
}

// Dense LDS: the run table (u16 window offsets, u32 value offsets) shares
// its bytes with the chain's two exit tables (dead once the runs are
// emitted); per-wave value stages; the super-blocks' chain entries (mark).
struct Dense2Lds {
  union {
    struct {
      uint16_t off[kDenseRuns];
      uint32_t val[kDenseRuns];
      uint16_t items[kDenseRuns];  // serial passes: work item ends
    } tab;
    uint16_t nxt[2 * kSlab];
  };
  uint64_t stage[kThreads / kWave][kStage];
  uint32_t mark[kSlab / 32];
};

// Union instances (kOptUnion): the run table / successor tables only; the
// value stages and the marks live past the dense window inside s_win, which a
// serial window covers whole.
struct Dense2TabLds {
  union {
    struct {
      uint16_t off[kDenseRuns];
      uint32_t val[kDenseRuns];
      uint16_t items[kDenseRuns];
    } tab;
    uint16_t nxt[2 * kSlab];
  };
};

// Deferral (kDefer): a serial-walk instance (kDefer = 1) whose probe pass
// finds short runs stops at the end of that pass and records {stamp, byte
// offset, value index} in the segment's own entry of `defer_q` (3 words per
// launch-wide segment; stamp = the launch pair's sequence number
// `defer_par`); the dense instance launched right after it (kDefer = 2)
// decodes the stamped segments with a persistent grid, each workgroup a
// static share, so a short-run segment never runs the one-wave header walk,
// whatever the stream's overall density. Entries of older launches carry
// older stamps: nothing is ever reset.
template <typename T, bool kPositions, int kOpt, int kWinKB, int kMinWaves, int kDense, int kDefer, bool kMulti>
__global__ __launch_bounds__(kThreads, kMinWaves) void rlev2_tiled_kernel(
    const uint8_t* __restrict__ p_src, uint64_t p_src_len, int p_is_signed,
    const uint64_t* __restrict__ p_segtab, uint64_t p_nsegs, uint64_t rows_per_group,
    uint64_t p_value_begin, uint64_t p_nvalues, T* __restrict__ p_dst, unsigned long long* p_err,
    unsigned long long* __restrict__ defer_q, uint32_t defer_par, const RleJob* __restrict__ jobs,
    uint32_t njobs, const uint64_t* __restrict__ p_dcount, const RunTab rtab) {
  // dense instances get 512 B more so the window's run-start chunk is a
  // whole number of 2 KB slabs (no partially occupied discovery pass)
  constexpr uint32_t kWin = kWinKB * 1024u + (kDense ? 512u : 0u);
  constexpr uint32_t kChunk = kWin - kMaxRun;
  // union instances: serial windows of kWinS bytes = the dense window, its
  // 32-byte slack, the value stages and the marks
  constexpr bool kUnion = kDense == 2 && (kOpt & kOptUnion) != 0;
  // density hysteresis (stream bytes per run)
  constexpr uint32_t kDenseB = (kOpt & kOptTable) ? kTabToDense : kToDense;
  constexpr uint32_t kSerialB = (kOpt & kOptTable) ? kTabToSerial : kToSerial;
  constexpr uint32_t kWinS = kUnion ? kWin + (uint32_t)(kWaves * kStage * 8 + kSlab / 8) : kWin;
  constexpr uint32_t kChunkS = kWinS - kMaxRun;
  static_assert(!kUnion || (kWin + 32) % 8 == 0, "stage alignment");
  static_assert(!kDense || kChunk % kSlab == 0, "dense window chunk must be whole slabs");
  static_assert(kDense == 0 || kDense == 2, "kDense: 0 serial only, 2 dense-capable");
  constexpr uint32_t kCap = kDense ? kDenseRuns : 512u;  // run table capacity
  static_assert(!kDense || kChunk >= kSlab, "window too small for a slab");
  using OffT = typename std::conditional<kDense == 2, uint16_t, uint32_t>::type;
  __shared__ __attribute__((aligned(16))) uint32_t s_win[kWinS / 4 + 8];  // + 32 B: the 12-byte extract may read past a run
  __shared__ uint32_t s_ctl[16];
  __shared__ uint32_t s_sync[2][2];  // serial passes: {published runs, claimed runs}, by pass parity
  OffT* s_off = nullptr;
  uint32_t* s_val = nullptr;
  uint16_t* s_nxt2 = nullptr;   // dense: successor tables, marks, stages
  uint32_t* s_mark2 = nullptr;
  uint64_t* s_stage2 = nullptr;
  uint16_t* s_items = nullptr;  // serial passes: work item ends
  if constexpr (kUnion) {
    __shared__ __attribute__((aligned(16))) Dense2TabLds s_d2;
    s_items = s_d2.tab.items;
    s_off = s_d2.tab.off;
    s_val = s_d2.tab.val;
    s_nxt2 = s_d2.nxt;
    s_stage2 = (uint64_t*)((char*)s_win + kWin + 32);
    s_mark2 = (uint32_t*)((char*)s_win + kWin + 32 + kWaves * kStage * 8);
  } else if constexpr (kDense == 2) {
    __shared__ __attribute__((aligned(16))) Dense2Lds s_d2;
    s_items = s_d2.tab.items;
    s_off = s_d2.tab.off;
    s_val = s_d2.tab.val;
    s_nxt2 = s_d2.nxt;
    s_mark2 = s_d2.mark;
    s_stage2 = &s_d2.stage[0][0];
  } else {
    __shared__ uint32_t s_tab[2 * kCap];
    __shared__ uint16_t s_itm[kCap];
    s_off = s_tab;
    s_val = s_tab + kCap;
    s_items = s_itm;
  }

  const int tid = (int)threadIdx.x;
  const int wave = tid / kWave, lane = tid % kWave;
#ifdef ORCG_PHASE_PROF
  const uint64_t wg_t0 = wall_clock64();
  uint32_t wg_dense = 0, wg_serial = 0;
#endif
  // the stream of the segment being decoded: the launch's, or (multi-stream
  // instances, kMulti) the job of `jobs` that owns the launch-wide segment
  // index (single-stream instances never rebind: the arguments stay as they
  // are, scalar and rematerialisable)
  const uint8_t* src = p_src;
  uint64_t src_len = p_src_len;
  int is_signed = p_is_signed;
  const uint64_t* segtab = p_segtab;
  const int64_t* trip = nullptr;  // multi-stream row-index jobs (RleJob::trip)
  const int64_t* rows = nullptr;
  uint64_t nsegs = p_nsegs;
  uint64_t value_begin = p_value_begin;
  // (p_dcount: the value count lives on the device, e.g. a nullable
  // column's non-null rows counted by its PRESENT decode; p_nvalues is then
  // only the output's capacity)
  uint64_t value_end = p_value_begin + (p_dcount ? uni64(*p_dcount) : p_nvalues);
  T* dst = p_dst;
  unsigned long long* err = p_err;
  uint32_t tab_base = 0;  // kOptTable: the stream's first run-table entry
  uint32_t job_idx = 0;   // kMulti: the segment's job
  auto bind = [&](const uint64_t gg) -> uint64_t {
    if constexpr (!kMulti) return gg;
    uint32_t lo = 0, hi = njobs - 1;
    while (lo < hi) {  // last job whose first segment is <= gg
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (uni64(jobs[mid].seg_base) <= gg) lo = mid;
      else hi = mid - 1;
    }
    const RleJob* J = jobs + lo;
    src = (const uint8_t*)uni64((uint64_t)(uintptr_t)J->src);
    src_len = uni64(J->src_len);
    is_signed = (int)uni(J->is_signed);
    segtab = (const uint64_t*)uni64((uint64_t)(uintptr_t)J->segtab);
    trip = (const int64_t*)uni64((uint64_t)(uintptr_t)J->trip);
    rows = (const int64_t*)uni64((uint64_t)(uintptr_t)J->rows);
    nsegs = uni64(J->nsegs);
    value_begin = 0;
    const uint64_t jdc = uni64((uint64_t)(uintptr_t)J->dcount);
    value_end = jdc ? uni64(*(const uint64_t*)(uintptr_t)jdc) : uni64(J->nvalues);
    dst = (T*)uni64((uint64_t)(uintptr_t)J->dst);
    const uint64_t je = uni64((uint64_t)(uintptr_t)J->err);
    err = je ? (unsigned long long*)(uintptr_t)je : p_err;
    tab_base = uni(J->tab_base);
    job_idx = lo;
    return gg - uni64(J->seg_base);
  };

  // one segment, from its start or (queued) from a byte offset / value index
  auto run_segment = [&](const uint64_t gg, const bool queued, const uint64_t q_pos, const uint64_t q_vi) {
  const uint64_t g = bind(gg);
  // segment g: {first byte, index of its first value}
  auto seg_at = [&](const uint64_t s, uint64_t* off) -> uint64_t {
    if (kMulti && trip) {
      const int64_t v = rows[s] - trip[3 * s + 1];
      *off = (uint64_t)trip[3 * s];
      return v < 0 ? 0ull : (uint64_t)v;
    }
    *off = segtab[2 * s];
    return kPositions ? s * rows_per_group - segtab[2 * s + 1] : segtab[2 * s + 1];
  };
  uint64_t seg_first = 0;
  const uint64_t vi0 = queued ? 0ull : seg_at(g, &seg_first);
  const uint64_t seg_start = queued ? q_pos : seg_first;
  uint64_t vi = queued ? q_vi : vi0;
  uint64_t seg_end = src_len;
  uint64_t v_next = ~0ull;
  if (g + 1 < nsegs) v_next = seg_at(g + 1, &seg_end);
  if (seg_end > src_len) seg_end = src_len;
  // kOptTable: the segment's header and run table (RunTab). Its runs lie in
  // [seg_first, next segment's first byte) and are >= 2 bytes each, so
  // seg_first / 2 + g leaves every earlier segment room for its runs.
  constexpr bool kTable = (kOpt & kOptTable) != 0;
  uint32_t* thdr = nullptr;
  uint64_t* ttab = nullptr;
  uint32_t tcnt = 0;                                     // entries written
  const uint64_t tlim = (uint64_t)rtab.spg * rtab.slice;  // values the slices cover
  if constexpr (kTable) {
    thdr = rtab.hdr + gg * (kRtHdr + rtab.spg);
    const uint32_t tb = tab_base + (uint32_t)(seg_first >> 1) + (uint32_t)g;
    ttab = rtab.tab + tb;
    if (tid == 0) {
      thdr[0] = 0;
      thdr[1] = 0;
      thdr[2] = (uint32_t)vi0;
      thdr[3] = (uint32_t)(vi0 >> 32);
      thdr[4] = tb;
      thdr[5] = job_idx;
    }
  }
  if (vi >= value_end || v_next <= value_begin) return;
  if (seg_start >= seg_end) {
    if (tid == 0 && v_next != ~0ull && v_next != vi && seg_start < src_len) report(err, vi, kErrBadSegment);
    if (tid == 0 && v_next == ~0ull) report(err, vi, kErrBadRead);  // no stream left for the requested values
    return;
  }

  // Range-checked descriptor over [seg_start & ~15, end of stream).
  const uintptr_t base_abs = ((uintptr_t)src + seg_start) & ~(uintptr_t)15;
  const uintptr_t end_abs = ((uintptr_t)src + src_len + 3) & ~(uintptr_t)3;
  const uint64_t span = (uint64_t)(end_abs - base_abs);
  const uint32_t nrec = span > 0xfffff000ull ? 0xfffff000u : (uint32_t)span;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)base_abs, (short)0, (int)nrec, 0x00020000);
  const uint64_t bias = (uint64_t)(base_abs - (uintptr_t)src);  // stream offset of descriptor byte 0

  uint64_t pos = seg_start;
  uint32_t sync_par = 0;
  if (tid < 4) s_sync[tid >> 1][tid & 1] = 0;  // ordered before use by the first window's barrier
  PROF_DECL;
  if constexpr ((kOpt & kOptFlat) != 0 && sizeof(T) == 8 && kDense == 0 && kDefer == 0) {
    // The flat prologue (flat_probe / flat_expand above): the segment's
    // leading chain of equal full DIRECT runs of >= 40 bits, taken only while
    // the runs lie wholly inside the requested values and end at or before
    // the segment's end. Whatever comes next (another header, a shorter or
    // narrower run, another kind, a partial or truncated run, a run that
    // straddles the segment's end) is left to the window loop below with
    // the advanced pos / vi, with its checks and reports as they are; a
    // segment that has gone there stays there.
    if (!queued) {
      // no flat run ends past the segment, nor closer than 4 bytes to the
      // descriptor's end (a value's 12-byte extract reads up to 4 bytes past it)
      const uint64_t flat_end = seg_end < bias + nrec - 4u ? seg_end : bias + nrec - 4u;
      const uint64_t vstop = v_next < value_end ? v_next : value_end;
      const uint32_t wv = uni((uint32_t)wave);
      // runs in flight per wave (ORCG_AB_FLAGS=-DORCG_FLAT_RUNS=1 for the
      // A/B): two measured 1 % faster than one on C2
      constexpr int kRuns = ORCG_FLAT_RUNS;
      static_assert(kRuns == 1 || kRuns == 2, "flat runs in flight");
      uint32_t flat_runs = 0;
      // kOptFlat16: W=64 runs go through flat_expand16, whose chunk loads
      // read up to 15 bytes past the run: no such run ends closer than 16
      // bytes to the descriptor's end (a run the margin excludes is left to
      // the window loop, like any other end of the chain)
      constexpr bool kF16 = (kOpt & kOptFlat16) != 0;
      constexpr int kRuns16 = ORCG_FLAT16_RUNS;
      static_assert(kRuns16 == 2 || kRuns16 == 3 || kRuns16 == 5, "flat 16-byte runs in flight");
      uint32_t lim64 = (uint32_t)(flat_end - bias);
      if constexpr (kF16) {
        const uint64_t rel_end = seg_end - bias;
        lim64 = nrec < 16u ? 0u : (uint32_t)(rel_end < nrec - 16u ? rel_end : nrec - 16u);
      }
      while (vi >= value_begin && vi < vstop && pos < flat_end) {
        const uint64_t kv = (vstop - vi) / 512u;  // whole runs before the next segment's / the last value
        uint32_t nb = 0;
        const uint32_t m = flat_probe(rs, (uint32_t)(pos - bias), (uint32_t)(flat_end - bias), lim64,
                                      kv < 64u ? (uint32_t)kv : 64u, lane, &nb);
        if (m == 0) break;
        const uint32_t B = 2u + 512u * nb;
        const uint32_t d0 = (uint32_t)(pos - bias) + 2u;
        T* const out = dst + (vi - value_begin);
        // wave w takes runs w, w + 4, ...
        bool wide16 = false;
        if constexpr (kF16) {
          if (nb == 8u) {
            wide16 = true;
            for (uint32_t r = wv; r < m; r += kWaves * kRuns16) {
              const uint32_t left = (m - r + kWaves - 1) / kWaves;  // this wave's runs from r on
              flat_expand16<kRuns16>(rs, d0 + r * B, kWaves * B, left < (uint32_t)kRuns16 ? left : kRuns16, is_signed,
                                     (int64_t*)out + 512u * r, kWaves * 512u, lane);
            }
          }
        }
        for (uint32_t r = wv; !wide16 && r < m; r += kWaves * kRuns) {
          if constexpr (kRuns == 2) {
            if (r + kWaves < m) {
              flat_expand<2>(rs, d0 + r * B, kWaves * B, nb, is_signed, out + 512u * r, kWaves * 512u, lane);
              continue;
            }
          }
          flat_expand<1>(rs, d0 + r * B, 0, nb, is_signed, out + 512u * r, 0, lane);
        }
        pos += (uint64_t)m * B;
        vi += 512ull * m;
        flat_runs += m;
        if (m < 64u) break;  // the chain ended; 64 runs: there may be more, probe again
      }
      PROF_MARK(7);
#ifdef ORCG_PHASE_PROF
      if (tid == 0) atomicAdd(&g_phase[10], (unsigned long long)flat_runs);  // runs expanded flat
#else
      (void)flat_runs;
#endif
    }
  }
  uint64_t pwpos = ~0ull;  // previous window (stream offset) and its valid bytes
  uint32_t pneed = 0;
  // wave-uniform mode of the next pass (dense instances only): the bytes per
  // run of the segment's first runs pick it (the inline probe below; queued
  // segments, short runs by values, are sized by it too: dense discovery for
  // short runs in bytes, the serial walk with staged group expansion for wide
  // ones)
  bool dense = false;
  bool probe = true;
  while (pos < seg_end && vi < value_end) {
    const uint32_t wrel = (uint32_t)(pos - bias) & ~15u;
    const uint64_t wpos = bias + wrel;
    // union instances: a window whose runs are known to be long (the probe
    // is done and the mode is serial) is a serial window of kWinS bytes:
    // serial passes only, short-run groups expanded without the stage
    const bool big = kUnion && !dense && !probe;
    uint32_t need = big ? kWinS : kWin, keep = 0;
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    // never load past the segment: its runs end at seg_end
    const uint64_t end_rel = (seg_end - bias + 15) & ~15ull;
    if (end_rel - wrel < need) need = (uint32_t)(end_rel - wrel);
    // the previous window's tail [wpos, pwpos + pneed) is already in LDS:
    // move it to the front instead of re-reading it (source and
    // destination must not overlap: the shift is at least the length;
    // otherwise reload)
    if (pwpos != ~0ull && pwpos + pneed > wpos && wpos - pwpos >= pwpos + pneed - wpos) {
      keep = (uint32_t)(pwpos + pneed - wpos);
      if (keep > need) keep = need;
      const uint32_t so = (uint32_t)(wpos - pwpos);
      for (uint32_t o = tid * 16u; o < keep; o += kThreads * 16u)
        *(u4*)((char*)s_win + o) = *(const u4*)((const char*)s_win + so + o);
      __syncthreads();  // reads of the tail finish before the DMA below lands
    }
    if constexpr ((kOpt & kOptRegFill) != 0) {
      // every lane issues all of its 16-byte loads before the first LDS
      // write (measured: +4 % over LDS-DMA on a pure window copy)
      constexpr int kPer = (kWinS + kThreads * 16 - 1) / (kThreads * 16);
      u4 v[kPer];
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const uint32_t off = keep + (uint32_t)(i * kThreads + tid) * 16u;
        if (off < need) v[i] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rs, wrel + off, 0, 2));
      }
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const uint32_t off = keep + (uint32_t)(i * kThreads + tid) * 16u;
        if (off < need) *(u4*)((char*)s_win + off) = v[i];
      }
    } else {
      // LDS-DMA: 1 KB per wave instruction
      for (uint32_t off = keep + wave * 1024u; off < need; off += kWaves * 1024u)
        if (off + lane * 16u < need)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)((char*)s_win + off),
                                                   16, wrel + off + lane * 16u, 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    PROF_MARK(0);
    if constexpr (kDense == 2) {
      // inline probe (no serial pass): one lane sizes the segment's first
      // runs; short ones (< kToDense stream bytes each) start it dense
      if (probe) {
        if (tid == 0) {
          uint32_t p = (uint32_t)(pos - wpos), nb = 0, nr = 0;
          while (nr < 4 && nb < 4 * kDenseB && p + kHdrLim < need) {
            const Run r = parse_run([&](uint32_t i) { return lds_byte(s_win, p + i); }, ~0ull, kHdrLim, is_signed);
            if (r.err != kErrNone || r.kind == 2) break;
            nb += r.bytes;
            p += r.bytes;
            ++nr;
          }
          s_ctl[15] = (nr == 4 && nb < 4 * kDenseB) ? 1u : 0u;
        }
        __syncthreads();
        dense = uni(s_ctl[15]) != 0;
        probe = false;
      }
    }
    // every run that starts in the window's first kChunk bytes ends inside
    // it: consume them all (several passes) before moving the window
    do {
      uint32_t n, stop, dpos, dval, shrt = 0;
#ifdef ORCG_DEBUG_COVER
      if (tid == 0) *s_cover_ptr() = 0;
      __syncthreads();
#endif
      bool was_dense = false;
      bool tabled = false;  // kOptTable: this pass's runs went to the run table
      if constexpr (kDense) was_dense = dense;
      if (was_dense) {
        const uint32_t sb = (uint32_t)(pos - wpos);
        const uint32_t lim = min(kSlab, kChunk - sb);
        DenseResult d;
        if constexpr (kDense == 2) {
          d = dense2_discover(s_win, s_off, s_val, s_nxt2, s_mark2, s_ctl, wpos, sb, lim, vi, seg_end, src_len,
                              value_end, need, is_signed, err, tid
#ifdef ORCG_PHASE_PROF
                              , prof_last_
#endif
          );
        }
        n = d.n;
        stop = d.stop;
        dpos = d.dpos;
        dval = d.dval;
        if constexpr (kTable) {
          // the runs go to the run table (entry: stream byte offset | first
          // value in the segment << 32); a run holding slice boundary k * S
          // is where slice k starts (runs are <= 512 < S values: one each)
          const uint64_t vrel = vi - vi0;
          if (vrel + dval <= tlim) {
            tabled = true;
            const uint32_t vr = (uint32_t)vrel, S = rtab.slice;
            for (uint32_t r = (uint32_t)tid; r < n; r += kThreads) {
              const uint32_t v = vr + s_val[r];
              const uint32_t ve = vr + (r + 1 < n ? s_val[r + 1] : dval);
              ttab[tcnt + r] = (wpos + s_off[r]) | ((uint64_t)v << 32);
              const uint32_t kb = (v + S - 1) / S;
              if (kb >= 1 && kb * S < ve) thdr[kRtHdr + kb] = tcnt + r;
            }
            tcnt += n;
          }
        }
        if constexpr (kDense != 0) {
          if (!tabled) {
            uint64_t* const stage = s_stage2 + wave * kStage;
            const uint32_t r0 = (uint32_t)(((uint64_t)n * wave) / kWaves),
                           r1 = (uint32_t)(((uint64_t)n * (wave + 1)) / kWaves);
            dense_expand(s_win, kWin / 4 + 8, s_off, s_val, stage, r0, r1, vi, is_signed, value_begin, value_end,
                         dst, lane);
          }
        }
      } else {
        // Wave 0 walks and publishes work items (a group of short runs or
        // one long run) as they close; every wave (wave 0 once its walk is
        // done) claims published items from an LDS counter and expands
        // them, so the walk overlaps the expansion.
        uint32_t* s_pub = &s_sync[sync_par][0];
        uint32_t* s_claim = &s_sync[sync_par][1];
        if (wave == 0) {
          // the walk is the workgroup's critical path: raise its issue
          // priority over co-resident waves that are expanding
          __builtin_amdgcn_s_setprio(3);
          // a segment's first walk probes its first runs (4 in dense
          // instances, 8 in queueing serial ones) and stops there when
          // they are short; a long-run segment just walks on
          const uint32_t probe_n = (probe && (kDense == 2 || kDefer == 1)) ? (kDense == 2 ? 4u : 8u) : 0u;
          constexpr bool kProbeValues = kDefer == 1;
          const WalkResult w =
              big ? walk<kWinS, kCap, OffT>(s_win, s_off, s_val, wpos, pos, vi, seg_end, src_len, value_end, is_signed,
                                            err, lane, need, kCap, s_pub, s_items, probe_n, kProbeValues)
                  : walk<kWin, kCap, OffT>(s_win, s_off, s_val, wpos, pos, vi, seg_end, src_len, value_end, is_signed,
                                           err, lane, need, kCap, s_pub, s_items, probe_n, kProbeValues);
          if (lane == 0) {
            s_ctl[0] = w.n;
            s_ctl[1] = w.stop;
            s_ctl[2] = w.dpos;
            s_ctl[3] = w.dval;
            s_ctl[4] = w.shrt;
            __hip_atomic_store(s_pub, w.items | kWalkDone, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
          PROF_MARK(1);  // wave 0's walk of this pass
#ifdef ORCG_PHASE_PROF
          if (tid == 0) {
            atomicAdd(&g_phase[8], (unsigned long long)w.n);  // runs walked
            atomicAdd(&g_phase[9], 1ull);                     // serial passes
          }
#endif
          __builtin_amdgcn_s_setprio(0);
        }
        for (;;) {
          uint32_t k = 0;
          if (lane == 0) k = atomicAdd(s_claim, 1u);
          k = uni(k);
          uint32_t pub;
          // waiting waves back off: polling shares the CU's scalar unit with
          // the walk (a short-run walk publishes an item every ~64 runs)
          for (uint32_t spin = 0;; ++spin) {
            pub = uni(__hip_atomic_load(s_pub, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
            if (k < (pub & ~kWalkDone) || (pub & kWalkDone)) break;
            if (spin < 2) __builtin_amdgcn_s_sleep(2);
            else __builtin_amdgcn_s_sleep(24);
          }
          if (k >= (pub & ~kWalkDone)) break;  // the walk is done and every item is claimed
          const uint32_t e = uni(s_items[k]);
          const uint32_t r0 = k ? (uni(s_items[k - 1]) & ~(uint32_t)kItemLong) : 0u;
          if (e & kItemLong) {
#ifdef ORCG_DEBUG_COVER
            if (lane == 0) {
              const uint32_t h = uni(s_off[r0]);
              ORCG_COVER_ADD(parse_run([&](uint32_t i) { return lds_byte(s_win, h + i); }, ~0ull, kHdrLim,
                                       is_signed).L);
            }
#endif
            expand_run(s_win, kWinS / 4 + 8, uni(s_off[r0]), vi + uni(s_val[r0]), is_signed, value_begin, value_end,
                       dst, lane);
          } else if (kDense == 2 && !big) {
            // coalesced stores through the wave's value stage
            dense_expand(s_win, kWin / 4 + 8, s_off, s_val, s_stage2 + wave * kStage, r0, e, vi, is_signed,
                         value_begin, value_end, dst, lane);
          } else {
            group_expand(s_win, s_off, s_val, r0, e, vi, is_signed, value_begin, value_end, dst, lane);
          }
        }
        // the other parity's counters are idle: clear them for the next serial pass
        if (tid == 0) {
          s_sync[sync_par ^ 1][0] = 0;
          s_sync[sync_par ^ 1][1] = 0;
        }
        sync_par ^= 1;
        __syncthreads();
        n = uni(s_ctl[0]);
        stop = uni(s_ctl[1]);
        dpos = uni(s_ctl[2]);
        dval = uni(s_ctl[3]);
        shrt = uni(s_ctl[4]);
      }
      __syncthreads();  // the run table (and the window) are rewritten next
#ifdef ORCG_DEBUG_COVER
      if (tid == 0 && !stop && *s_cover_ptr() != dval) report(err, vi, was_dense ? 0x71u : 0x70u);
      __syncthreads();
#endif
      PROF_MARK(was_dense ? 6 : 2);
#ifdef ORCG_PHASE_PROF
      if (was_dense) ++wg_dense;
      else ++wg_serial;
#endif
      if constexpr (kTable) {
        // a pass expanded here: slices starting inside it start at the next
        // table entry; then the segment header (read by the second pass)
        const uint64_t vrel = vi - vi0, vend = vrel + dval;
        if (!tabled) {
          const uint64_t S = rtab.slice, ve = vend < tlim ? vend : tlim;
          const uint64_t kb0 = vrel == 0 ? 1u : (vrel + S - 1) / S;
          for (uint64_t kb = kb0 + (uint64_t)tid; kb * S < ve; kb += kThreads) thdr[kRtHdr + kb] = tcnt;
        }
        if (tid == 0) {
          thdr[0] = tcnt;
          thdr[1] = vend < 0xffffffffull ? (uint32_t)vend : 0xffffffffu;
        }
      }
      if (stop) return;
      pos += dpos;
      vi += dval;
      const bool was_probe = probe;
      probe = false;
      if constexpr (kDefer == 1) {
        // a short-run segment: queue the rest for the dense instance
        if (shrt && pos < seg_end && vi < value_end) {
          if (tid == 0) {
            // the segment's own entry, stamped with this launch pair's
            // sequence number (no shared counter: one atomic per queued
            // segment on one word serialised whole launches)
            defer_q[3 * gg + 1] = pos;
            defer_q[3 * gg + 2] = vi;
            __hip_atomic_store(&defer_q[3 * gg], (unsigned long long)defer_par, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            // the launch-wide "something was queued" word (after the
            // launch's last segment entry): written once per launch pair
            // in the common case (a load first, so a stream whose every
            // segment queues does not serialise on one address)
            unsigned long long* any = &defer_q[3 * p_nsegs];
            if (__hip_atomic_load(any, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (unsigned long long)defer_par)
              __hip_atomic_store(any, (unsigned long long)defer_par, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          return;
        }
      }
      if constexpr (kDense) {
        // hysteresis on the stream bytes per run of this pass
        if (n > 0) {
          const uint32_t bpr = dpos / n;
          if (shrt || (!dense && (n >= 8 || (was_probe && n >= 4)) && bpr < kDenseB)) dense = true;
          else if (dense && bpr >= kSerialB) dense = false;
        }
      }
      if (n == 0 && dpos == 0) break;  // nothing consumed (cannot happen for a good window)
      // a union instance leaves a serial window as soon as its runs turn
      // short: the next window is a dense one
      if (big && dense) break;
    } while (pos < wpos + (big ? kChunkS : kChunk) && pos < seg_end && vi < value_end);
    pwpos = wpos;
    pneed = need;
  }
  if (tid == 0 && v_next != ~0ull && vi < value_end && vi != v_next) report(err, vi, kErrBadSegment);
  if (tid == 0 && v_next == ~0ull && vi < value_end) report(err, vi, kErrBadRead);  // stream ended early
  };

  if constexpr (kDefer == 2) {
    // the drain: one workgroup per launch-wide segment; a segment the serial
    // launch stamped with this pair's sequence number is decoded from its
    // queued byte offset / value index, any other exits after one load (the
    // hardware hands out the queued segments as workgroups free up: the
    // earlier persistent grid of 6 workgroups per CU, each a static share,
    // ran 19 % slower on all-short-run streams)
    // nothing queued by the serial launch (long-run streams): one load, exit
    if (uni64(__hip_atomic_load(&defer_q[3 * p_nsegs], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) !=
        (unsigned long long)defer_par)
      return;
    const uint64_t q = blockIdx.x;
    if (q >= p_nsegs || uni64(defer_q[3 * q]) != (unsigned long long)defer_par) return;
    run_segment(q, true, uni64(defer_q[3 * q + 1]), uni64(defer_q[3 * q + 2]));
  } else {
    // (one call site per instance: a second one makes the compiler outline
    // run_segment into a call with a ~700-byte stack frame)
    run_segment(blockIdx.x, false, 0, 0);
  }
#ifdef ORCG_PHASE_PROF
  if (kUnion && tid == 0 && blockIdx.x < kWgDurMax) {
    g_wgdur[2 * blockIdx.x] = wall_clock64() - wg_t0;
    g_wgdur[2 * blockIdx.x + 1] = wg_dense | ((uint64_t)wg_serial << 32);
  }
#endif
}

}  // namespace

// The host half: the instance table and the launchers. Which instance a
// stream gets (ctx->rlev2_variant, include/orcg.h: 0 = the density-adaptive
// default, kRlev2FirstTiled .. kMaxRlev2Variant pin one instance, 1 = the
// wave-walk kernel of rlev2_kernels.hip), one pass or two, and the grouping
// of multi-stream launches are rlev2_route.hh's; what needs the device (the
// CU count, the queue, the run table, the launches) is here.

static int defer_queue(Ctx* ctx, uint64_t nsegs, unsigned long long** out) {
  // {stamp, byte offset, value index} per launch-wide segment, stamps zeroed
  // at allocation (launch sequence numbers start at 1); word 3 * nsegs is
  // the launch's "something was queued" stamp
  if (ctx->defer_cap < nsegs + 1) {
    if (ctx->d_defer) {
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipFree(ctx->d_defer);
      ctx->d_defer = nullptr;
      ctx->defer_cap = 0;
    }
    const uint64_t cap = std::max<uint64_t>(nsegs + nsegs / 4, 4096);
    int rc = hip_check(ctx, hipMalloc(&ctx->d_defer, 3 * cap * 8), "hipMalloc defer queue");
    if (!rc) rc = hip_check(ctx, hipMemsetAsync(ctx->d_defer, 0, 3 * cap * 8, ctx->stream), "defer queue reset");
    if (rc) return rc;
    ctx->defer_cap = cap;
  }
  *out = (unsigned long long*)ctx->d_defer;
  return ORCG_OK;
}

static int cu_count(Ctx* ctx) {
  if (ctx->num_cus == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0)
      cus = 256;
    ctx->num_cus = cus;
  }
  return ctx->num_cus;
}

// ORCG_DEBUG_DEFER: after a serial launch, how many of its segments it
// queued for the dense drain (stderr; synchronises the stream)
static void debug_defer(Ctx* ctx, const unsigned long long* dq, uint64_t nsegs, uint32_t dpar) {
  if (!debug_on("defer")) return;
  std::vector<unsigned long long> h(3 * nsegs + 1);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
      hipMemcpy(h.data(), dq, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return;
  uint64_t q = 0;
  for (uint64_t g = 0; g < nsegs; ++g) q += h[3 * g] == dpar ? 1 : 0;
  fprintf(stderr, "defer: %llu of %llu segments queued (any %d)\n", (unsigned long long)q,
          (unsigned long long)nsegs, h[3 * nsegs] == dpar ? 1 : 0);
}

// The context's run table (entries) and segment headers (nsegs x (kRtHdr +
// spg) words), grow-only; nothing needs clearing (the first kernel writes
// every segment's header before the second reads it).
static int runtab_buffers(Ctx* ctx, uint64_t entries, uint64_t nsegs, uint32_t spg, uint32_t slice, RunTab* rt) {
  const uint64_t tb = std::max<uint64_t>(entries, 1) * 8, hb = nsegs * (kRtHdr + spg) * 4;
  if (ctx->rtab_cap < tb || ctx->rhdr_cap < hb) {
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->rtab_cap < tb) {
      if (ctx->d_rtab) (void)hipFree(ctx->d_rtab);
      ctx->d_rtab = nullptr;
      ctx->rtab_cap = 0;
      const uint64_t cap = std::max<uint64_t>(tb + tb / 4, 1u << 20);
      int rc = hip_check(ctx, hipMalloc(&ctx->d_rtab, cap), "hipMalloc run table");
      if (rc) return rc;
      ctx->rtab_cap = cap;
    }
    if (ctx->rhdr_cap < hb) {
      if (ctx->d_rhdr) (void)hipFree(ctx->d_rhdr);
      ctx->d_rhdr = nullptr;
      ctx->rhdr_cap = 0;
      const uint64_t cap = std::max<uint64_t>(hb + hb / 4, 256u << 10);
      int rc = hip_check(ctx, hipMalloc(&ctx->d_rhdr, cap), "hipMalloc run-table headers");
      if (rc) return rc;
      ctx->rhdr_cap = cap;
    }
  }
  *rt = RunTab{(uint64_t*)ctx->d_rtab, (uint32_t*)ctx->d_rhdr, spg, slice};
  return ORCG_OK;
}

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

template <typename T, typename Kernel>
static void enqueue_kernel(Ctx* ctx, const TiledLaunch& l, Kernel kernel) {
  const Rlev2Args& a = l.a;
  hipLaunchKernelGGL(kernel, dim3((unsigned)a.nsegs), dim3(kThreads), 0, ctx->stream, a.src, a.src_len,
                     a.is_signed ? 1 : 0, a.segtab, a.nsegs, a.rows_per_group, a.value_begin, a.nvalues, (T*)a.dst,
                     ctx->d_err, l.dq, l.dpar, l.jobs, l.njobs, a.dcount, l.rtab);
}
// An instance, K = (options, window KB, min waves, kDense, kDefer): its
// multi-stream kernel and its single-stream ones. (All seven are named in
// this one body, so the code object holds the kernels instance by instance in
// kInstances' order: scripts/isa_diff.py compares its metadata as one piece.)
template <int... K>
static void enqueue(Ctx* ctx, const TiledLaunch& l) {
  const bool pos = l.a.positions;
  if (l.jobs) {
    enqueue_kernel<int64_t>(ctx, l, rlev2_tiled_kernel<int64_t, false, K..., true>);
  } else if (l.a.dst_bytes == 8) {
    if (pos) enqueue_kernel<int64_t>(ctx, l, rlev2_tiled_kernel<int64_t, true, K..., false>);
    else enqueue_kernel<int64_t>(ctx, l, rlev2_tiled_kernel<int64_t, false, K..., false>);
  } else if (l.a.dst_bytes == 4) {
    if (pos) enqueue_kernel<int32_t>(ctx, l, rlev2_tiled_kernel<int32_t, true, K..., false>);
    else enqueue_kernel<int32_t>(ctx, l, rlev2_tiled_kernel<int32_t, false, K..., false>);
  } else {
    if (pos) enqueue_kernel<int16_t>(ctx, l, rlev2_tiled_kernel<int16_t, true, K..., false>);
    else enqueue_kernel<int16_t>(ctx, l, rlev2_tiled_kernel<int16_t, false, K..., false>);
  }
}

constexpr int kSer = 0;             // LDS-DMA windows
constexpr int kWide = kOptRegFill;  // register-filled windows
// The instances: enqueue<options, window KB, min waves, kDense, kDefer>, and
// for a serial instance that queues short-run segments (kDefer 1) the dense
// instance that drains the queue (kDefer 2).
struct Instance {
  int id;
  Enqueue launch, drain;
};
constexpr Instance kInstances[] = {
    // 33 KB register-filled serial, no queue, flat DIRECT prologue (W=64 runs in 16-byte chunks)
    {kRlev2Wide, enqueue<kWide | kOptFlat | kOptFlat16, 33, 1, 0, 0>, nullptr},
    // 21 KB serial + dense drain
    {kRlev2SerialDrain, enqueue<kSer, 21, 6, 0, 1>, enqueue<kSer, 8, 6, 2, 2>},
    {kRlev2Dense8, enqueue<kSer, 8, 6, 2, 0>, nullptr},    // dense-capable, 8.5 KB
    {kRlev2Dense12, enqueue<kSer, 12, 5, 2, 0>, nullptr},  // dense-capable, 12.5 KB
    // union, two passes: dense passes table their runs, rlev2_expand_kernel expands them in value slices
    {kRlev2UnionTwoPass, enqueue<kSer | kOptUnion | kOptTable, 8, 6, 2, 0>, nullptr},
    // 33 KB serial + dense drain (round-3 default, A/B)
    {kRlev2WideDrain, enqueue<kWide, 33, 1, 0, 1>, enqueue<kSer, 8, 6, 2, 2>},
    {kRlev2UnionOnePass, enqueue<kSer | kOptUnion, 8, 6, 2, 0>, nullptr},  // union in one pass (round-5 default)
    {kRlev2WideNoFlat, enqueue<kWide, 33, 1, 0, 0>, nullptr},            // kRlev2Wide without the flat prologue (A/B control)
    {kRlev2WideFlat8, enqueue<kWide | kOptFlat, 33, 1, 0, 0>, nullptr},  // kRlev2Wide without kOptFlat16 (A/B control)
};

// A serial instance that queues its short-run segments, then the dense
// instance that drains the queue.
static int launch_deferring(Ctx* ctx, TiledLaunch& l, const Instance& in) {
  const int rc = defer_queue(ctx, l.a.nsegs, &l.dq);
  if (rc) return rc;
  l.dpar = (uint32_t)(ctx->defer_seq++ % 0xffffffffull) + 1u;  // never 0
  in.launch(ctx, l);
  debug_defer(ctx, l.dq, l.a.nsegs, l.dpar);
  in.drain(ctx, l);
  return ORCG_OK;
}

// One launch (or serial + drain pair, or two passes) of instance `variant`
// over the segments of one stream, or (ml) over the launch-wide segments of a
// planned launch's device job table.
static int launch_tiled(Ctx* ctx, int variant, const Rlev2Args& a, const MultiLaunch* ml = nullptr) {
  if (a.nsegs == 0 || a.nvalues == 0) return ORCG_OK;
  TiledLaunch l{a, nullptr, 0, nullptr, 0, RunTab{nullptr, nullptr, 0, 0}};
  if (ml) {
    l.jobs = (const RleJob*)ml->d_jobs;
    l.njobs = ml->njobs;
  }
  if (variant == kRlev2UnionTwoPass) {
    // two passes when the run table can address the launch, else one
    const uint64_t bound = a.positions ? a.rows_per_group + 512 : seg_value_bound(a.nvalues, a.nsegs);
    const TwoPass tp = ml ? TwoPass{ml->tab_entries, ml->spg, ml->slice} : stream_two_pass(a.src_len, a.nsegs, bound);
    if (two_pass_fits(tp.entries, a.nsegs, tp.spg)) {
      const int rc = runtab_buffers(ctx, tp.entries, a.nsegs, tp.spg, tp.slice, &l.rtab);
      if (rc) return rc;
    } else {
      variant = kRlev2UnionOnePass;
    }
  }
  if (a.nsegs > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many segments");
  if (a.dst_bytes != 8 && a.dst_bytes != 4 && a.dst_bytes != 2)
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "dst_bytes must be 8, 4 or 2");
  const Instance* in = std::find_if(std::begin(kInstances), std::end(kInstances),
                                    [&](const Instance& i) { return i.id == variant; });
  if (in == std::end(kInstances)) return set_error(ctx, ORCG_INVALID_ARGUMENT, "unknown RLEv2 kernel variant");
  if (in->drain) {
    const int rc = launch_deferring(ctx, l, *in);
    if (rc) return rc;
  } else {
    in->launch(ctx, l);
  }
  const int rc = hip_check(ctx, hipGetLastError(), "rlev2_tiled_kernel launch");
  if (rc || variant != kRlev2UnionTwoPass) return rc;
  return launch_rlev2_expand(ctx, a, l.jobs, l.njobs, l.rtab);
}

int launch_rlev2_tiled(Ctx* ctx, const Rlev2Args& a) {
  const uint64_t est = a.positions ? a.nsegs * a.rows_per_group : a.nvalues;
  return launch_tiled(ctx, route_rlev2(Rlev2Route{a.src_len, est, a.nsegs, cu_count(ctx), ctx->rlev2_variant, false}), a);
}

int launch_rlev2_tiled_jobs(Ctx* ctx, const MultiLaunch& m) {
  Rlev2Args a{};  // the streams are the job table's
  a.nsegs = m.grid;
  a.nvalues = m.values;
  a.dst_bytes = 8;
  return launch_tiled(ctx, m.variant, a, &m);
}

int plan_rlev2_multi(Ctx* ctx, const RleJob* jobs, uint32_t njobs, std::vector<MultiLaunch>& out) {
  const int pinned = ctx->rlev2_variant;
  if (!rlev2_multi_capable(pinned)) {
    // not a multi-stream instance: one launch per stream (the reader queues
    // only segment-table jobs for these variants, rlev2_multi_capable)
    for (uint32_t j = 0; j < njobs; ++j) {
      if (!jobs[j].segtab) return set_error(ctx, ORCG_INVALID_ARGUMENT, "row-index job needs a multi-stream instance");
      out.push_back(MultiLaunch{MultiLaunch::kRlev2Pinned, pinned, jobs + j, 1, jobs[j].nsegs, jobs[j].nvalues});
    }
    return ORCG_OK;
  }
  const int cus = cu_count(ctx);
  const std::vector<Rlev2Group> groups = group_rlev2_jobs(jobs, njobs, pinned, cus);
  if (debug_on("jobs"))
    for (const Rlev2Group& g : groups)
      for (uint32_t j = 0; j < njobs; ++j)
        if (rlev2_job_instance(jobs[j], pinned, cus) == g.variant)
          fprintf(stderr, "rle job: instance %d bytes %llu values %llu segments %llu (%.3f B/value)\n", g.variant,
                  (unsigned long long)jobs[j].src_len, (unsigned long long)jobs[j].nvalues,
                  (unsigned long long)jobs[j].nsegs, (double)jobs[j].src_len / (double)jobs[j].nvalues);
  for (const Rlev2Group& g : groups) {
    if (g.segs > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many segments");
    const RleJob* d = nullptr;
    const int rc = stage_rle_jobs(ctx, g.jobs.data(), (uint32_t)g.jobs.size(), &d);
    if (rc) return rc;
    MultiLaunch m{MultiLaunch::kRlev2, g.launch_variant, d, (uint32_t)g.jobs.size(), g.segs, g.values};
    if (g.spg) {
      m.tab_entries = g.entries;
      m.spg = g.spg;
      m.slice = g.slice;
    }
    out.push_back(m);
  }
  return ORCG_OK;
}

int launch_rlev2_multi(Ctx* ctx, const RleJob* jobs, uint32_t njobs) {
  std::vector<MultiLaunch> ls;
  const int rc = plan_rlev2_multi(ctx, jobs, njobs, ls);
  return rc ? rc : run_multi(ctx, ls);
}

}  // namespace orcg

#ifdef ORCG_PHASE_PROF
extern "C" int orcg_debug_wg_durations(unsigned long long* out, int n) {
  if (n > (int)(2 * orcg::kWgDurMax)) n = 2 * orcg::kWgDurMax;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(orcg::g_wgdur), (size_t)n * 8) == hipSuccess ? 0 : -1;
}

extern "C" int orcg_debug_phase_counters(unsigned long long* out, int n, int reset) {
  unsigned long long h[16];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(orcg::g_phase), sizeof(h)) != hipSuccess) return -1;
  for (int i = 0; i < n && i < 16; ++i) out[i] = h[i];
  if (reset) {
    unsigned long long z[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(orcg::g_phase), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// A no-op launch that makes HIP load this file's code object (warm_modules).
namespace orcg {
namespace {
__global__ void warm_rlev2_tiled_kernel() {}
}  // namespace
void warm_rlev2_tiled(hipStream_t s) { hipLaunchKernelGGL(warm_rlev2_tiled_kernel, dim3(1), dim3(64), 0, s); }
}  // namespace orcg
