// The stripe scheduler's host side: the job-table ring / arena (stage_table)
// and run_multi, which enqueues a batch's planned launches (RLEv2 instances,
// RLEv1, varint counts, dictionaries, decimals, length scans) over the
// context's stream and its side lanes (forked and joined by LaneFork).
#include <cstdio>
#include <cstring>

#include "orcg_internal.hh"

namespace orcg {

// Job tables go through a pinned ring mirrored on the device (entries are
// reused only after the stream has drained: a wrap synchronises first), or
// into the caller's arena (Ctx::arena_*), which the caller uploads itself.
int stage_table(Ctx* ctx, const void* src, size_t bytes, const void** out) {
  const uint64_t need = (bytes + 255) & ~(uint64_t)255;
  if (ctx->arena_h) {
    if (ctx->arena_used + need > ctx->arena_cap) return set_error(ctx, ORCG_INVALID_ARGUMENT, "job arena full");
    memcpy(ctx->arena_h + ctx->arena_used, src, bytes);
    *out = ctx->arena_d + ctx->arena_used;
    ctx->arena_used += need;
    return ORCG_OK;
  }
  if (ctx->jobs_cap < need) {
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->d_jobs) (void)hipFree(ctx->d_jobs);
    if (ctx->h_jobs) (void)hipHostFree(ctx->h_jobs);
    ctx->d_jobs = ctx->h_jobs = nullptr;
    ctx->jobs_cap = ctx->jobs_used = 0;
    const uint64_t cap = std::max<uint64_t>(4 * need, 256u << 10);
    int rc = hip_check(ctx, hipMalloc(&ctx->d_jobs, cap), "hipMalloc job table");
    if (!rc) rc = hip_check(ctx, hipHostMalloc(&ctx->h_jobs, cap, hipHostMallocDefault), "hipHostMalloc job table");
    if (rc) return rc;
    ctx->jobs_cap = cap;
  }
  if (ctx->jobs_used + need > ctx->jobs_cap) {
    int rc = hip_check(ctx, hipStreamSynchronize(ctx->stream), "job ring wrap");
    if (rc) return rc;
    ctx->jobs_used = 0;
  }
  uint8_t* h = (uint8_t*)ctx->h_jobs + ctx->jobs_used;
  uint8_t* d = (uint8_t*)ctx->d_jobs + ctx->jobs_used;
  memcpy(h, src, bytes);
  ctx->jobs_used += need;
  *out = d;
  return hip_check(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream), "H2D jobs");
}

// The planned launches, in order. The work before the join runs side by
// side: the critical RLEv2 instance (the two-pass one, else the one with the
// most values) on this stream, every other instance on a side lane of its
// own, and the varint tile counts and RLEv1 segments (on_aux_lane) on one
// more lane; then this stream waits for the lanes and runs what reads their
// outputs (dictionaries, decimals, length scans: joins_first) itself. The
// critical path never changes queues: a dependency across HIP queues costs
// 12-30 us a hop on the MI355X (configs[3] timelines), so the lanes, done
// long before the critical instance, are the ones waited on, and the
// post-join kernels follow the critical instance on its own queue.
int run_multi(Ctx* ctx, const std::vector<MultiLaunch>& ls) {
  int ninst = 0, crit = -1;
  bool aux = false;
  for (size_t i = 0; i < ls.size(); ++i) {
    const MultiLaunch& m = ls[i];
    if (on_aux_lane(m.kind)) aux = true;
    if (m.kind != MultiLaunch::kRlev2) continue;
    ++ninst;
    const bool two = m.spg > 0, ctwo = crit >= 0 && ls[crit].spg > 0;
    if (crit < 0 || (two && !ctwo) || (two == ctwo && m.values > ls[crit].values)) crit = (int)i;
  }
  const int nlanes = (ninst > 0 ? ninst - 1 : 0) + (aux && ninst > 0 ? 1 : 0);
  const bool par = nlanes > 0 && side_lanes() > 1 && (size_t)nlanes <= side_lanes() &&
                   ctx_lane(ctx, (size_t)nlanes - 1) != nullptr;
  Ctx* const base = ctx;
  LaneFork lf(base);
  size_t next = 0;         // lanes handed out so far, in launch order
  Ctx* aux_ctx = nullptr;  // the auxiliary lane
  bool joined = false;     // past the join: everything runs on base
  int rc = par ? lf.begin() : ORCG_OK;
  auto join = [&]() -> int {
    joined = true;
    return lf.join();
  };
  for (size_t i = 0; i < ls.size() && !rc; ++i) {
    const MultiLaunch& m = ls[i];
    if (joins_first(m.kind) && !joined && (rc = join())) break;
    debug_stale("run_multi: before a launch");
    if (m.kind == MultiLaunch::kRlev2) {
      Ctx* c = base;
      if (par && (int)i != crit && (rc = lf.lane(next++, &c))) break;
      // jobs without a record of their own report into the base's (the
      // lane's own record is the lane's: it frees it)
      const ErrRecordScope err(c, base->d_err);
      rc = launch_rlev2_tiled_jobs(c, m);
      if (rc) {
        char b[160];
        snprintf(b, sizeof b, " (instance %d, %u streams, %llu segments%s)", m.variant, m.njobs,
                 (unsigned long long)m.grid, c == base ? "" : ", side lane");
        base->last_error = c->last_error + b;
      }
    } else if (on_aux_lane(m.kind)) {
      Ctx* c = base;
      if (par && !joined) {
        if (!aux_ctx && (rc = lf.lane(next++, &aux_ctx))) break;
        c = aux_ctx;
      }
      const ErrRecordScope err(c, base->d_err);
      if (m.kind == MultiLaunch::kRlev1) {
        rc = launch_rlev1_jobs(c, (const V1SegDesc*)m.d_jobs, m.grid, m.variant);
      } else {
        const VarintJob& J = *(const VarintJob*)m.d_jobs;
        uint64_t ntiles = 0;
        rc = launch_varint_tile_counts(c, J.src, J.len, J.counts, &ntiles);
        if (!rc) rc = launch_exclusive_scan(c, J.counts, ntiles, J.base, nullptr, J.total);
      }
      if (rc && c != base) base->last_error = c->last_error;
    } else if (m.kind == MultiLaunch::kDict) {
      rc = launch_dict_jobs(base, (const DictJob*)m.d_jobs, m.njobs, m.grid);
    } else if (m.kind == MultiLaunch::kDecimal) {
      rc = launch_decimal_jobs(base, (const DecJob*)m.d_jobs, m.njobs, m.grid, m.variant);
    } else if (m.kind == MultiLaunch::kLengthScan) {
      const ScanJob& J = *(const ScanJob*)m.d_jobs;
      rc = launch_exclusive_scan(base, J.in, J.n, J.out, J.flags, J.total);
    } else {
      // kRlev2Pinned, a pinned single-stream variant: host job (d_jobs is a host pointer)
      const RleJob& J = *(const RleJob*)m.d_jobs;
      const ErrRecordScope err(base, J.err ? J.err : base->d_err);  // the job's own error record
      Rlev2Args a{};
      a.src = J.src;
      a.src_len = J.src_len;
      a.is_signed = (int)J.is_signed;
      a.segtab = J.segtab;
      a.nsegs = J.nsegs;
      a.nvalues = J.nvalues;
      a.dst = J.dst;
      a.dst_bytes = 8;
      rc = launch_rlev2(base, a);
    }
  }
  if (!joined) {  // join what was forked (also after a failure)
    const int jr = join();
    if (jr && !rc) rc = jr;
  }
  return rc;
}

}  // namespace orcg
