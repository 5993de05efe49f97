// The flat DIRECT path (kOptFlat). A writer emits a wide random column as
// back-to-back DIRECT runs of 512 values at one width: every such run has the
// same two header bytes and the same byte length B = 2 + 512 * nb (nb = W / 8
// bytes per value), and a run's extent depends on its own header only. So if
// the header at pos + k * B equals the one at pos for k = 1 .. m - 1, those m
// runs start exactly there (by induction): one memory round trip validates
// the chain, and each lane then loads its values' bytes straight from memory,
// as a flat copy does. Every wave probes for itself (the same few cache
// lines), so the path needs no LDS, no barrier and no walk.
#pragma once

#include "rlev2_tiled_common.hh"

namespace orcg {
namespace {

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

}  // namespace
}  // namespace orcg
