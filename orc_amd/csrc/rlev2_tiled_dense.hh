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
#pragma once

#include "rlev2_tiled_walk.hh"  // short_value

namespace orcg {
namespace {

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
                                                       int tid PROF_PARAM) {
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
      // (the coverage build's count of the run; nothing in any other build)
      if (lane == 0) ORCG_COVER_ADD(parse_run([&](uint32_t i) { return lds_byte(win, uni(s_off[c + a]) + i); }, ~0ull,
                                              kHdrLim, is_signed).L);
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

}  // namespace
}  // namespace orcg
