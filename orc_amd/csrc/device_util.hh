// Device building blocks shared by every kernel unit, whatever it decodes:
// wave-uniform reads, wavefront scans and sums, the error record, the
// range-checked stream descriptor and the segment lookup. (What is specific
// to RLEv2 -- width tables, the bit-field extract, the run-header parser --
// is rlev2_device.hh.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orcg {
namespace dev {

constexpr int kWave = 64;

// Values the wave agrees on but the compiler cannot prove uniform (loaded
// from LDS or computed from such loads): readfirstlane puts them in SGPRs, so
// the code that depends on them stays scalar (a v_readlane with a VGPR lane
// index becomes a waterfall loop).
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uni64(uint64_t x) {
  return ((uint64_t)uni((uint32_t)(x >> 32)) << 32) | uni((uint32_t)x);
}

__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

// Wavefront inclusive prefix sums on DPP (no LDS round trips): Kogge-Stone
// inside each 16-lane row with row_shr:1,2,4,8, then row_bcast:15 (rows 1,3)
// and row_bcast:31 (rows 2,3) carry the row totals across. Requires all 64
// lanes active. Invalid source lanes read 0 (bound_ctrl).
template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t dpp0(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, kCtrl, kRowMask, 0xf, true);
}

__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t x) {
  x += dpp0<0x111, 0xf>(x);  // row_shr:1
  x += dpp0<0x112, 0xf>(x);  // row_shr:2
  x += dpp0<0x114, 0xf>(x);  // row_shr:4
  x += dpp0<0x118, 0xf>(x);  // row_shr:8
  x += dpp0<0x142, 0xa>(x);  // row_bcast:15
  x += dpp0<0x143, 0xc>(x);  // row_bcast:31
  return x;
}

template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint64_t dpp0_64(uint64_t x) {
  const uint32_t lo = dpp0<kCtrl, kRowMask>((uint32_t)x), hi = dpp0<kCtrl, kRowMask>((uint32_t)(x >> 32));
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t wave_inclusive_scan(uint64_t x, int /*lane*/ = 0) {
  x += dpp0_64<0x111, 0xf>(x);
  x += dpp0_64<0x112, 0xf>(x);
  x += dpp0_64<0x114, 0xf>(x);
  x += dpp0_64<0x118, 0xf>(x);
  x += dpp0_64<0x142, 0xa>(x);
  x += dpp0_64<0x143, 0xc>(x);
  return x;
}

// Value of lane 63 (wave-uniform, scalar register).
__device__ __forceinline__ uint64_t last_lane(uint64_t x) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(x >> 32), 63) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 63);
}

// unZigZag (c++/src/RLE.hh:32-34): signed RLEv1 and RLEv2 streams alike
__device__ __forceinline__ uint64_t unzigzag(uint64_t v) { return (v >> 1) ^ (0 - (v & 1)); }

// The wave's sum on every lane (a butterfly of cross-lane adds).
template <typename T>
__device__ __forceinline__ T wave_sum(T c) {
  for (int m = kWave / 2; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  return c;
}

__device__ __forceinline__ void report(unsigned long long* err, uint64_t value_index, uint32_t code) {
  atomicMin(err, (unsigned long long)((value_index << 8) | code));
}

template <typename T>
__device__ __forceinline__ void put(T* dst, uint64_t idx, uint64_t v) {
  dst[idx] = (T)(int64_t)v;
}

// Range-checked buffer descriptor over [(src + seg_start) & ~15, end of the
// stream rounded up to a dword): loads past the stream return zeros. The
// record count is clamped to 0xfffff000 bytes (the 32-bit field; a segment
// is far shorter). bias = stream offset of descriptor byte 0.
struct StreamDesc {
  __amdgpu_buffer_rsrc_t rs;
  uint32_t nrec;
  uint64_t bias;
};

__device__ __forceinline__ void stream_desc(const uint8_t* src, uint64_t src_len, uint64_t seg_start, StreamDesc& d) {
  const uintptr_t base_abs = ((uintptr_t)src + seg_start) & ~(uintptr_t)15;
  const uintptr_t end_abs = ((uintptr_t)src + src_len + 3) & ~(uintptr_t)3;
  const uint64_t span = (uint64_t)(end_abs - base_abs);
  d.nrec = span > 0xfffff000ull ? 0xfffff000u : (uint32_t)span;
  d.rs = __builtin_amdgcn_make_buffer_rsrc((void*)base_abs, (short)0, (int)d.nrec, 0x00020000);
  d.bias = (uint64_t)(base_abs - (uintptr_t)src);
}

// Segment g of a stream: its first byte, the index of its first value, its
// end (the next segment's first byte, or the stream's end; clamped to
// src_len) and the next segment's first value (~0: g is the last). An entry
// k is read from
//  * a segment table: {byte offset, first value index};
//  * row-index positions (kPositions): {byte offset, values to skip}, the
//    first value index being k * rows_per_group - skip;
//  * a multi-stream row-index job (trip, rows given): trip[3k] = byte offset,
//    rows[k] - trip[3k + 1] = first value index, clamped at 0 (rg_segtab_kernel).
struct Seg {
  uint64_t seg_start, vi, seg_end, v_next;
};

template <bool kPositions>
__device__ __forceinline__ void seg_lookup(const uint64_t* segtab, uint64_t nsegs, uint64_t g, uint64_t src_len, Seg& s,
                                           uint64_t rows_per_group = 0, const int64_t* trip = nullptr,
                                           const int64_t* rows = nullptr) {
  auto at = [&](const uint64_t k, uint64_t* off) -> uint64_t {
    if (trip) {
      const int64_t v = rows[k] - trip[3 * k + 1];
      *off = (uint64_t)trip[3 * k];
      return v < 0 ? 0ull : (uint64_t)v;
    }
    *off = segtab[2 * k];
    return kPositions ? k * rows_per_group - segtab[2 * k + 1] : segtab[2 * k + 1];
  };
  s.vi = at(g, &s.seg_start);
  s.seg_end = src_len;
  s.v_next = ~0ull;
  if (g + 1 < nsegs) s.v_next = at(g + 1, &s.seg_end);
  if (s.seg_end > src_len) s.seg_end = src_len;
}

}  // namespace dev
}  // namespace orcg
