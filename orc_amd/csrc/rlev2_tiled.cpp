// The host half: the instance table and the launchers. Which instance a
// stream gets (ctx->rlev2_variant, include/orcg.h: 0 = the density-adaptive
// default, kRlev2FirstTiled .. kMaxRlev2Variant pin one instance, 1 = the
// wave-walk kernel of rlev2_kernels.hip), one pass or two, and the grouping
// of multi-stream launches are rlev2_route.hh's; what needs the device (the
// CU count, the queue, the run table, the launches) is here. Host code only:
// the kernels are rlev2_tiled_kernel.hh's, compiled by the instance units
// (rlev2_tiled_inst_*.hip), which the linker binds kInstances' rows to.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "rlev2_tiled_launch.hh"

namespace orcg {

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

// A no-op launch per instance unit, which makes HIP load its code object
// (warm_modules).
void warm_rlev2_tiled(hipStream_t s) {
#define ORCG_WARM(u) warm_rlev2_tiled_##u(s);
  ORCG_TILED_UNITS(ORCG_WARM)
#undef ORCG_WARM
}

}  // namespace orcg

#ifdef ORCG_PHASE_PROF
// the union unit's table (only union instances write one)
extern "C" int orcg_debug_wg_durations(unsigned long long* out, int n) { return orcg::prof_wgdur_union(out, n); }

// the sum of the units' counters
extern "C" int orcg_debug_phase_counters(unsigned long long* out, int n, int reset) {
  unsigned long long sum[16] = {}, h[16];
#define ORCG_SUM(u)                                 \
  if (orcg::prof_phase_##u(h, reset)) return -1;    \
  for (int i = 0; i < 16; ++i) sum[i] += h[i];
  ORCG_TILED_UNITS(ORCG_SUM)
#undef ORCG_SUM
  for (int i = 0; i < n && i < 16; ++i) out[i] = sum[i];
  return 0;
}
#endif
