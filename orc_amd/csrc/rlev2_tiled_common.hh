// What every phase of rlev2_tiled_kernel (rlev2_tiled_kernel.hh) shares: the
// geometry, the profiling and coverage macros, the LDS window primitives and
// the one-wave expansion of a run.
#pragma once

#include "rlev2_device.hh"

namespace orcg {
namespace {
using namespace dev;

// Phase profiling (build with -DORCG_PHASE_PROF, scripts/phase_prof.py):
// thread 0 adds the cycles between consecutive phase marks to g_phase[k]
// (one copy of the counters per instance unit, summed by rlev2_tiled.cpp).
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
// thread 0 adds x to the count g_phase[k]
#define PROF_COUNT(k, x) \
  if (tid == 0) atomicAdd(&g_phase[k], (unsigned long long)(x))
// dense2_discover marks phases too: the caller's clock, as a last parameter / argument
#define PROF_PARAM , uint64_t& prof_last_
#define PROF_ARG , prof_last_
// a workgroup's wall-clock time and passes, written to g_wgdur by the instances `on`
#define PROF_WG_DECL                    \
  const uint64_t wg_t0 = wall_clock64(); \
  uint32_t wg_dense = 0, wg_serial = 0
#define PROF_WG_PASS(was_dense) \
  if (was_dense) ++wg_dense;    \
  else ++wg_serial
#define PROF_WG_END(on)                                                    \
  if ((on) && tid == 0 && blockIdx.x < kWgDurMax) {                        \
    g_wgdur[2 * blockIdx.x] = wall_clock64() - wg_t0;                      \
    g_wgdur[2 * blockIdx.x + 1] = wg_dense | ((uint64_t)wg_serial << 32); \
  }
#else
#define PROF_MARK(k) \
  do {               \
  } while (0)
#define PROF_DECL
#define PROF_COUNT(k, x) (void)(x)
#define PROF_PARAM
#define PROF_ARG
#define PROF_WG_DECL
#define PROF_WG_PASS(was_dense)
#define PROF_WG_END(on)
#endif

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kMaxRun = 4608;  // >= 4356, the longest legal run

// dense (short-run) mode, rlev2_tiled_dense.hh
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

// Debug build only (ORCG_AB_FLAGS=-DORCG_DEBUG_COVER): every expansion path
// counts the values of the runs it expands; each pass checks the count
// against the values its discovery consumed.
#ifdef ORCG_DEBUG_COVER
#define ORCG_COVER_ADD(x) atomicAdd(s_cover_ptr(), (uint32_t)(x))
__device__ __forceinline__ uint32_t* s_cover_ptr() {
  __shared__ uint32_t s_cover;
  return &s_cover;
}
// a pass starts its count at zero ...
#define COVER_RESET()                   \
  if (tid == 0) *s_cover_ptr() = 0; \
  __syncthreads()
// ... and ends by comparing it with `dval`, the values its discovery consumed
#define COVER_CHECK(stop, dval, code)                                                \
  if (tid == 0 && !(stop) && *s_cover_ptr() != (dval)) report(err, vi, (code)); \
  __syncthreads()
// a long run that a whole wave expands (expand_run) counts through its header at window offset hoff
#define COVER_ADD_RUN(win, hoff)                                                                                \
  if (lane == 0) {                                                                                              \
    const uint32_t h = hoff;                                                                                    \
    ORCG_COVER_ADD(parse_run([&](uint32_t i) { return lds_byte(win, h + i); }, ~0ull, kHdrLim, is_signed).L); \
  }
#else
#define ORCG_COVER_ADD(x) \
  do {                    \
  } while (0)
#define COVER_RESET()
#define COVER_CHECK(stop, dval, code)
#define COVER_ADD_RUN(win, hoff)
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

}  // namespace
}  // namespace orcg
