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
//
// The phases are rlev2_tiled_{common,flat,walk,dense}.hh; the instance units
// (rlev2_tiled_inst_*.hip) include this file and instantiate enqueue<...>,
// rlev2_tiled.cpp holds the instance table and the launchers.
#pragma once

#include <type_traits>

#include "rlev2_tiled_dense.hh"
#include "rlev2_tiled_flat.hh"
#include "rlev2_tiled_launch.hh"
#include "rlev2_tiled_walk.hh"

namespace orcg {
namespace {

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
  PROF_WG_DECL;
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
        PROF_COUNT(10, flat_runs);  // runs expanded flat
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
        COVER_RESET();
        bool was_dense = false;
        bool tabled = false;  // kOptTable: this pass's runs went to the run table
        if constexpr (kDense) was_dense = dense;
        if (was_dense) {
          const uint32_t sb = (uint32_t)(pos - wpos);
          const uint32_t lim = min(kSlab, kChunk - sb);
          DenseResult d;
          if constexpr (kDense == 2) {
            d = dense2_discover(s_win, s_off, s_val, s_nxt2, s_mark2, s_ctl, wpos, sb, lim, vi, seg_end, src_len,
                                value_end, need, is_signed, err, tid PROF_ARG);
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
                big ? walk<kWinS, kCap, OffT>(s_win, s_off, s_val, wpos, pos, vi, seg_end, src_len, value_end,
                                              is_signed, err, lane, need, kCap, s_pub, s_items, probe_n, kProbeValues)
                    : walk<kWin, kCap, OffT>(s_win, s_off, s_val, wpos, pos, vi, seg_end, src_len, value_end,
                                             is_signed, err, lane, need, kCap, s_pub, s_items, probe_n, kProbeValues);
            if (lane == 0) {
              s_ctl[0] = w.n;
              s_ctl[1] = w.stop;
              s_ctl[2] = w.dpos;
              s_ctl[3] = w.dval;
              s_ctl[4] = w.shrt;
              __hip_atomic_store(s_pub, w.items | kWalkDone, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            PROF_MARK(1);  // wave 0's walk of this pass
            PROF_COUNT(8, w.n);   // runs walked
            PROF_COUNT(9, 1ull);  // serial passes
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
              COVER_ADD_RUN(s_win, uni(s_off[r0]));
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
        COVER_CHECK(stop, dval, was_dense ? 0x71u : 0x70u);
        PROF_MARK(was_dense ? 6 : 2);
        PROF_WG_PASS(was_dense);
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
  PROF_WG_END(kUnion);
}

}  // namespace

template <typename T, typename Kernel>
static void enqueue_kernel(Ctx* ctx, const TiledLaunch& l, Kernel kernel) {
  const Rlev2Args& a = l.a;
  hipLaunchKernelGGL(kernel, dim3((unsigned)a.nsegs), dim3(kThreads), 0, ctx->stream, a.src, a.src_len,
                     a.is_signed ? 1 : 0, a.segtab, a.nsegs, a.rows_per_group, a.value_begin, a.nvalues, (T*)a.dst,
                     ctx->d_err, l.dq, l.dpar, l.jobs, l.njobs, a.dcount, l.rtab);
}
// An instance, K = (options, window KB, min waves, kDense, kDefer): its
// multi-stream kernel and its single-stream ones. Declared in
// rlev2_tiled_launch.hh; each K of kInstances is instantiated in one unit.
template <int... K>
void enqueue(Ctx* ctx, const TiledLaunch& l) {
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

// What a unit holds besides its instances: a no-op kernel whose launch makes
// HIP load the unit's code object (warm_rlev2_tiled), and in the profiling
// build the accessors of its copy of the counters (g_phase, g_wgdur).
#ifdef ORCG_PHASE_PROF
#define ORCG_TILED_UNIT_PROF(u)                                                                   \
  int prof_phase_##u(unsigned long long* h, int reset) {                                          \
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase), sizeof(g_phase)) != hipSuccess) return -1;    \
    const unsigned long long z[16] = {};                                                          \
    return !reset || hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z)) == hipSuccess ? 0 : -1; \
  }                                                                                               \
  int prof_wgdur_##u(unsigned long long* out, int n) {                                            \
    if (n > (int)(2 * kWgDurMax)) n = 2 * kWgDurMax;                                              \
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wgdur), (size_t)n * 8) == hipSuccess ? 0 : -1;   \
  }
#else
#define ORCG_TILED_UNIT_PROF(u)
#endif
#define ORCG_TILED_UNIT(u)                                                                                   \
  namespace {                                                                                                \
  __global__ void warm_rlev2_tiled_kernel() {}                                                               \
  }                                                                                                          \
  void warm_rlev2_tiled_##u(hipStream_t s) { hipLaunchKernelGGL(warm_rlev2_tiled_kernel, dim3(1), dim3(64), 0, s); } \
  ORCG_TILED_UNIT_PROF(u)

}  // namespace orcg
