// The serial walk: wave 0 walks the run headers of an LDS window into the run
// table and cuts the runs into work items (walk), which every wave claims
// and expands: a group of short runs one lane per run (group_expand), a long
// run with the whole wave (expand_run, rlev2_tiled_common.hh).
#pragma once

#include "rlev2_tiled_common.hh"

namespace orcg {
namespace {

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

}  // namespace
}  // namespace orcg
