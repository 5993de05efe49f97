// Device half of a stripe read: issue (upload, batched launches, per-column
// decodes), finish (the first error in column order, the column views), the
// pipelined read of several stripes.
#include "reader_internal.hh"

int orcg_reader::poll_counts(const std::vector<CountSrc>& srcs, uint64_t* out) {
  if (!h_pub) {
    void* h = nullptr;
    if (hipHostMalloc(&h, kPubSlots * kPubStride * 8, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
      (void)hipGetLastError();
      return 1;
    }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipHostFree(h);
      return 1;
    }
    memset(h, 0, kPubSlots * kPubStride * 8);
    h_pub = (uint64_t*)h;
    d_pub = (uint64_t*)d;
  }
  std::vector<Ctx*> order;  // one slot per stream, in first-use order
  std::vector<PublishArgs> args;
  std::vector<std::vector<size_t>> where;
  for (size_t i = 0; i < srcs.size(); ++i) {
    size_t g = 0;
    while (g < order.size() && order[g] != srcs[i].lane) ++g;
    if (g == order.size()) {
      if (g == kPubSlots) return 1;
      order.push_back(srcs[i].lane);
      args.push_back(PublishArgs{});
      where.emplace_back();
    }
    if (args[g].n == kPublishMax) return 1;
    args[g].src[args[g].n++] = (const int64_t*)srcs[i].src;
    where[g].push_back(i);
  }
  const uint64_t gen = ++pub_gen;
  for (size_t g = 0; g < order.size(); ++g) {
    const int rc = launch_publish(order[g], args[g], d_pub + g * kPubStride, d_pub + g * kPubStride + kPublishMax,
                                  gen);
    if (rc) return fail(rc, order[g]->last_error);
  }
  for (size_t g = 0; g < order.size(); ++g) {
    const uint64_t* flag = h_pub + g * kPubStride + kPublishMax;
    const double t0 = now_s();
    for (uint32_t spin = 1; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != gen; ++spin) {
      if ((spin & 1023) != 0) continue;
      // a failed stream never sets the flag; a long wait gives the core back
      const hipError_t q = hipStreamQuery(order[g]->stream);
      if (q != hipSuccess && q != hipErrorNotReady) {
        const int rc = hip_check(order[g], q, "publish wait");
        return fail(rc, order[g]->last_error);
      }
      if (q == hipSuccess || now_s() - t0 > 2e-3) {
        const int rc = hip_check(order[g], hipStreamSynchronize(order[g]->stream), "hipStreamSynchronize");
        if (rc) return fail(rc, order[g]->last_error);
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != gen)
          return fail(ORCG_DEVICE_ERROR, "mid-stripe counts were not published");
        break;
      }
    }
    for (size_t k = 0; k < where[g].size(); ++k) out[where[g][k]] = h_pub[g * kPubStride + k];
  }
  return ORCG_OK;
}

// The stripe's first error, in column order (type ids are pre-order, the
// order decode() visits the columns): for each column up to the one that
// failed inline (`inline_rc`, detected on the host while launching), its
// deferred F->checks, then its device error record (the first bad value of its
// kernels), as the reference raises them while reading that column; then the
// inline failure itself; then the context's own record.
int orcg_reader::first_error(int inline_rc) {
  const std::string inline_msg = last_error;
  const uint32_t inline_col = err_col;
  cur_col = kNoCol;
  // the stripe's read-back copy (error records, non-null counts, summary
  // slots) and its deferred copies were queued by issue(): wait for them
  const size_t nc = H->cols.size();
  if (hipEventSynchronize(F->done) != hipSuccess) return fail(ORCG_DEVICE_ERROR, "stream synchronize failed");
  std::vector<unsigned long long> rec(F->h_rb, F->h_rb + nc);
  const uint32_t last = inline_rc ? (inline_col == kNoCol ? 0u : inline_col) : (uint32_t)nc;
  // checks grouped by column once (stable: a column's checks keep their
  // order), then one walk over columns and checks together
  std::stable_sort(F->checks.begin(), F->checks.end(),
                   [](const std::pair<uint32_t, std::function<int()>>& a,
                      const std::pair<uint32_t, std::function<int()>>& b) { return a.first < b.first; });
  // a chunk the device could not inflate: ahead of any column's error (the
  // host's inflate fails the stripe in prepare(), before any column decodes)
  if (F->inflate_word && F->h_rb[F->inflate_word] != kNoError) {
    const unsigned long long r = F->h_rb[F->inflate_word];
    act.ctx->last_error_value = r >> 8;
    return fail(dev_error_status((uint32_t)(r & 0xff)), dev_error_message((uint32_t)(r & 0xff)));
  }
  size_t ci = 0;
  for (uint32_t col = 0; col < nc && col <= last; ++col) {
    for (; ci < F->checks.size() && F->checks[ci].first <= col; ++ci) {
      const int rc = F->checks[ci].second();
      if (rc) return rc;
    }
    if (rec[col] != kNoError) {
      const uint32_t code = (uint32_t)(rec[col] & 0xff);
      act.ctx->last_error_value = rec[col] >> 8;
      std::string m = dev_error_message(code);
      if (m == "unknown device error") {
        char b[96];
        snprintf(b, sizeof b, " (column %u, record 0x%llx)", col, (unsigned long long)rec[col]);
        m += b;
      }
      return fail(dev_error_status(code), m);
    }
  }
  if (inline_rc) return fail(inline_rc, inline_msg);
  for (auto& ch : F->checks)
    if (ch.first >= nc) {
      const int rc = ch.second();
      if (rc) return rc;
    }
  // the context's own record (launches outside a column's scope)
  const unsigned long long own = F->h_rb[2 * nc];
  if (own != kNoError) {
    const uint32_t code = (uint32_t)(own & 0xff);
    act.ctx->last_error_value = own >> 8;
    return fail(dev_error_status(code), dev_error_message(code));
  }
  return ORCG_OK;
}

// Device half, launch side: one H2D of the staging buffer (streams, the
// initialised read-back block, the batched launches' job tables), the
// batched launches, every selected column's launches, the read-back copy and
// the flight's event. Host checks wait for finish().
void orcg_reader::issue(HostStage& hs, DevSlot& ds, Flight& fl) {
  const Bound bound(this, fl, &hs, &ds);
  fl.hs = &hs;
  fl.ds = &ds;
  fl.t0 = now_s();
  fl.rc = ORCG_OK;
  fl.enqueued = false;
  // Launch checks read hipGetLastError (per host thread): drop a failure a
  // call whose result was already checked or deliberately ignored (frees in
  // destructors, a retried allocation) left behind, so it cannot surface as
  // this stripe's first launch error.
  {
    const hipError_t stale = hipGetLastError();
    if (debug_on("stale") && stale != hipSuccess) fprintf(stderr, "orcg: stale HIP error before upload: %s\n", hipGetErrorString(stale));
  }
  cur_col = err_col = kNoCol;
  auto early = [&](int rc) {  // a failure before anything was enqueued
    fl.rc = rc;
    fl.err_col = err_col;
    fl.err_msg = last_error;
    fl.t1 = now_s();
  };
  ds.stripe = hs.stripe;
  ds.pool.release_all();
  ds.f_valid = false;
  // a fresh slot's first chunk: the staging plus ~16 bytes per row and
  // selected column (outputs and scratch); later stripes use what it took
  {
    size_t nsel = 0;
    for (size_t i = 0; i < hs.cols.size(); ++i) nsel += act.selected[i] && hs.cols[i].supported ? 1 : 0;
    ds.pool.hint = hs.used + hs.slack + hs.tail_bytes + 256 + 16 * nsel * footer.stripes[hs.stripe].num_rows + (1u << 20);
  }
  const size_t nc = hs.cols.size();
  const uint64_t nrows_stripe = footer.stripes[hs.stripe].num_rows;
  // after the streams: the read-back block (error records 0xff.., non-null
  // counts and summary slots 0) and the job arena (the batched launches'
  // tables): one upload carries the stripe, its initialised counters and
  // its job tables
  const uint64_t rb_off = (hs.used + 255) & ~(uint64_t)255;
  fl.rb_words = rb_words_for(nc);
  fl.rb_used = 2 * nc + 1;  // word 2 nc: the context's own record during this stripe
  // then the device inflate's record ((chunk index << 8) | code)
  fl.inflate_word = hs.inflate.empty() ? 0 : fl.rb_used++;
  const uint64_t arena_off = (rb_off + 8 * fl.rb_words + 255) & ~(uint64_t)255;
  const uint64_t arena_cap = arena_bytes_for(nc, v1_segments(hs), (nrows_stripe + 2047) / 2048 + 1);
  const uint64_t total = arena_off + arena_cap;
  // the device-only tail (streams the device inflates) lies past the upload
  if (!hs.inflate.empty() && total + 64 > hs.tail_off)
    return early(fail(ORCG_DEVICE_ERROR, "stripe upload overlaps its device-inflated streams"));
  if (!hs.ensure(total + 64, hs.used)) return early(fail(ORCG_OUT_OF_MEMORY, "pinned staging allocation failed"));
  memset(hs.h + rb_off, 0xff, 8 * nc);
  memset(hs.h + rb_off + 8 * nc, 0, 8 * (fl.rb_words - nc));
  memset(hs.h + rb_off + 8 * (2 * nc), 0xff, 8 * (fl.inflate_word ? 2 : 1));
  ds.d_stage = (uint8_t*)ds.pool.get(std::max(total, hs.tail_off + hs.tail_bytes) + 64);
  if (!ds.d_stage) return early(fail_oom(__FILE_NAME__, __LINE__));
  ds.d_rb = (uint64_t*)(ds.d_stage + rb_off);
  ds.d_errs = (unsigned long long*)ds.d_rb;
  ds.d_ones = ds.d_rb + nc;
  if (fl.h_rb_cap < fl.rb_words) {
    if (fl.h_rb) (void)hipHostFree(fl.h_rb);
    fl.h_rb = nullptr;
    fl.h_rb_cap = 0;
    if (hipHostMalloc((void**)&fl.h_rb, fl.rb_words * 8, hipHostMallocDefault) != hipSuccess)
      return early(fail(ORCG_OUT_OF_MEMORY, "pinned allocation failed"));
    fl.h_rb_cap = fl.rb_words;
  }
  if (!fl.done && hipEventCreateWithFlags(&fl.done, hipEventDisableTiming) != hipSuccess) {
    fl.done = nullptr;
    return early(fail(ORCG_DEVICE_ERROR, "event creation failed"));
  }
  for (hipEvent_t* e : {&fl.ev_up0, &fl.ev_up1, &fl.ev_dec})
    if (!*e && hipEventCreate(e) != hipSuccess) *e = nullptr;
  fl.ev_split = fl.ev_up0 && fl.ev_up1 && fl.ev_dec;
  const size_t need_defer = 4 * nc + 16;
  if (fl.defer_cap < need_defer) {
    if (fl.h_defer) (void)hipHostFree(fl.h_defer);
    fl.h_defer = nullptr;
    fl.defer_cap = 0;
    if (hipHostMalloc((void**)&fl.h_defer, need_defer * 8, hipHostMallocDefault) != hipSuccess)
      return early(fail(ORCG_OUT_OF_MEMORY, "pinned allocation failed"));
    fl.defer_cap = need_defer;
  }
  fl.defer_used = 0;
  fl.checks.clear();
  // the context's own record for this stripe rides the read-back block (the
  // stripe's one copy back replaces sync_ctx's synchronous record read)
  const ErrRecordScope own_rec(act.ctx, (unsigned long long*)(ds.d_rb + 2 * nc));
  B.reset();
  const uint64_t nrows = nrows_stripe;
  const int64_t* rg_rows = hs.ngroups ? (const int64_t*)(ds.d_stage + hs.rows_off) : nullptr;
  // the batch: streams (and dictionaries) whose counts the host knows, their
  // job tables staged into the arena before the upload
  int rc = ORCG_OK;
  if (batch_on) {
    act.ctx->arena_h = hs.h + arena_off;
    act.ctx->arena_d = ds.d_stage + arena_off;
    act.ctx->arena_cap = arena_cap;
    act.ctx->arena_used = 0;
    rc = collect(0, nrows, rg_rows);
    if (!rc) rc = plan_batch();
    act.ctx->arena_h = act.ctx->arena_d = nullptr;
    act.ctx->arena_cap = 0;
  }
  const uint64_t up = arena_off + act.ctx->arena_used;
  stage_bytes += up;
  // (uploaded even after a failure above: finish() reads the records back);
  // a small stripe (configs[0]: ~60 KB) is pulled by a kernel from the
  // pinned staging, a large one copied by the DMA engine
  constexpr uint64_t pull_max = 256u << 10;
  if (fl.ev_split && hipEventRecord(fl.ev_up0, act.ctx->stream) != hipSuccess) fl.ev_split = false;
  const int urc = up <= pull_max && hs.pinned_mapped
                      ? launch_pull(act.ctx, ds.d_stage, hs.h, up)
                      : hip_check(act.ctx, hipMemcpyAsync(ds.d_stage, hs.h, up, hipMemcpyHostToDevice, act.ctx->stream),
                                  "H2D stripe");
  if (urc && !rc) rc = fail_ctx(urc);
  if (fl.ev_split && hipEventRecord(fl.ev_up1, act.ctx->stream) != hipSuccess) fl.ev_split = false;
  fl.t1 = now_s();
  // the stripe's Snappy or LZ4 chunks, ahead of every decode: compressed bytes
  // and the chunk table rode the upload, the streams land in the tail
  if (!rc && !hs.inflate.empty()) {
    const auto launch = ps.compression == file::kLz4 ? launch_lz4_inflate : launch_snappy_inflate;
    if ((rc = launch(act.ctx, ds.d_stage, (const orcg_snappy_chunk*)(ds.d_stage + hs.inflate_off), hs.inflate.size(),
                     ds.d_stage, (unsigned long long*)(ds.d_rb + fl.inflate_word))))
      rc = fail_ctx(rc);
    last_dev_inflate[0] += hs.inflate.size();
    for (const orcg_snappy_chunk& k : hs.inflate) last_dev_inflate[1] += k.dst_bytes;
  }
  // A batch of nested or nullable columns' dictionaries only (collect_dicts;
  // configs[4]'s map keys): nothing reads its offsets before the fork's next
  // level, so it runs on side lane 0 beside the stripe's first decodes, not
  // ahead of them on the base stream (4 launches, ~45 us of a C5 stripe)
  Ctx* pre_lane = nullptr;
  if (!rc && !B.launches.empty() && B.only_preloaded_dicts() && side_lanes() > 1 &&
      (B.ev_pre || hipEventCreateWithFlags(&B.ev_pre, hipEventDisableTiming) == hipSuccess))
    pre_lane = ctx_lane(act.ctx, 0);
  if (!rc && pre_lane) {
    // (never joined: the gathers and the stripe's end wait for ev_pre instead)
    LaneFork lf(act.ctx);
    if (!(rc = lf.begin())) rc = lf.lane(0, &pre_lane);
    if (!rc && (rc = run_multi(pre_lane, B.launches))) act.ctx->last_error = pre_lane->last_error;
    if (!rc) rc = hip_check(act.ctx, hipEventRecord(B.ev_pre, pre_lane->stream), "dictionary batch event");
    if (rc) rc = fail_ctx(rc);
    B.pre_on_lane = !rc;
  } else if (!rc && !B.launches.empty() && (rc = timed(0, [&]() -> int { return run_multi(act.ctx, B.launches); }))) {
    rc = fail_ctx(rc);
  }
  if (!rc) rc = decode(0, nrows, nullptr, nrows, rg_rows);
  if (B.pre_on_lane && hipStreamWaitEvent(act.ctx->stream, B.ev_pre, 0) != hipSuccess && !rc)
    rc = fail(ORCG_DEVICE_ERROR, "dictionary batch wait failed");
  batched_streams += B.batched.size();
  fl.rc = rc;
  fl.err_col = err_col;
  fl.err_msg = last_error;
  if (fl.ev_split && hipEventRecord(fl.ev_dec, act.ctx->stream) != hipSuccess) fl.ev_split = false;
  // the read-back copy, then the flight's event (queued copies land before
  // the buffers are reused)
  if (hipMemcpyAsync(fl.h_rb, ds.d_rb, 8 * fl.rb_used, hipMemcpyDeviceToHost, act.ctx->stream) != hipSuccess ||
      hipEventRecord(fl.done, act.ctx->stream) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(act.ctx->stream);
    if (!fl.rc) {
      fl.rc = ORCG_DEVICE_ERROR;
      fl.err_msg = "read error records";
    }
    // (the records are unreadable: finish() reports fl.rc)
    memset(fl.h_rb, 0xff, 8 * fl.rb_used);
    (void)hipEventRecord(fl.done, act.ctx->stream);
  }
  fl.enqueued = true;
}

// Device half, host side: the first error in column order, as the reference
// raises them one column at a time, then the stripe's column views.
int orcg_reader::finish(Flight& fl) {
  const Bound bound(this, fl, fl.hs, fl.ds);
  HostStage& hs = *fl.hs;
  DevSlot& ds = *fl.ds;
  int rc = fl.rc;
  if (!fl.enqueued) return fail(rc, fl.err_msg);  // failed before anything was enqueued
  err_col = fl.err_col;
  last_error = fl.err_msg;
  rc = first_error(rc);
  fl.checks.clear();
  ds.out.clear();
  for (const Col& c : hs.cols) ds.out.emplace_back(c, !rc);
  const double t_end = now_s();
  // the upload's and the decode's GPU time (the flight's events, complete
  // here: first_error waited for `done`); host clocks without them
  float up_ms = 0, dec_ms = 0;
  if (fl.ev_split && hipEventElapsedTime(&up_ms, fl.ev_up0, fl.ev_up1) == hipSuccess &&
      hipEventElapsedTime(&dec_ms, fl.ev_up1, fl.ev_dec) == hipSuccess) {
    timings[3] += up_ms * 1e-3;
    timings[4] += dec_ms * 1e-3;
  } else {
    (void)hipGetLastError();
    timings[3] += fl.t1 - fl.t0;
    timings[4] += t_end - fl.t1;
  }
  // ReaderMetrics (ReaderCall / ReaderInclusiveLatencyUs are counted per
  // caller-facing call: orcg_reader_read_stripe(s), orcg_row_reader_next):
  // the stripe's decompression, I/O and decode work
  madd(kMDecompressCall, hs.n_chunks);
  madd(kMDecompressLatency, (uint64_t)(hs.t_decomp * 1e6));
  madd(kMIOCount, hs.n_io);
  madd(kMIOLatency, (uint64_t)(hs.t_io * 1e6));
  if (metrics_timing) collect_event_times();
  else madd(kMDecodeLatency, (uint64_t)((t_end - fl.t1) * 1e6));
  return rc;
}

int orcg_reader::upload_and_decode(HostStage& hs, DevSlot& ds) {
  issue(hs, ds, flights[0]);
  return finish(flights[0]);
}

// Stripes [first, first + count), pipelined three ways: a host thread
// prepares stripe i + 1 (decompression, plans) while the caller's thread
// issues stripe i (upload, launches) and then finishes stripe i - 1 (its
// synchronisation and host checks) -- so the GPU starts stripe i while the
// host checks stripe i - 1. Stripe i lives in stages[i % 3] and
// flights[i & 1]; the preparer of stripe i waits for stripe i - 3 to be
// finished. One thread for the whole read: a thread per stripe cost more
// than a configs[0] stripe decodes in.
int orcg_reader::read_stripes(uint64_t first, uint64_t count) {
  if (!act.ctx) return fail(ORCG_INVALID_ARGUMENT, "reader has no device context");
  if (first > footer.stripes.size() || count > footer.stripes.size() - first)
    return fail(ORCG_INVALID_ARGUMENT, "stripe index out of range");
  hipSetDevice(act.ctx->device);
  for (auto& t : timings) t = 0;
  stream_stats[0] = stream_stats[1] = 0;
  batched_streams = 0;
  stage_bytes = 0;
  last_dev_inflate[0] = last_dev_inflate[1] = 0;
  while (slots.size() < count) slots.emplace_back(new DevSlot());
  nslots = 0;
  if (count == 0) return ORCG_OK;
  std::mutex pm;
  std::condition_variable pcv;
  uint64_t prepared = 0, released = 0;  // stripes prepared; stripes finished (their stages free)
  bool quit = false;
  std::thread prep([&] {
    for (uint64_t k = 0; k < count; ++k) {
      {
        std::unique_lock<std::mutex> lk(pm);
        pcv.wait(lk, [&] { return quit || k < released + 3; });  // stripe k - 3 released stages[k % 3]
        if (quit) return;
      }
      prepare(first + k, stages[k % 3], act);
      {
        std::lock_guard<std::mutex> lk(pm);
        prepared = k + 1;
      }
      pcv.notify_all();
      if (stages[k % 3].rc) return;  // the decode raises it when it reaches stripe k
    }
  });
  auto release = [&](uint64_t n) {
    {
      std::lock_guard<std::mutex> lk(pm);
      released = n;
    }
    pcv.notify_all();
  };
  int rc = ORCG_OK;
  bool pending = false;  // stripe k - 1 issued, not finished
  for (uint64_t k = 0; k <= count; ++k) {
    bool issued = false;
    if (k < count) {
      {
        std::unique_lock<std::mutex> lk(pm);
        pcv.wait(lk, [&] { return prepared > k; });
      }
      HostStage& cur = stages[k % 3];
      timings[0] += cur.t_parse;
      timings[1] += cur.t_decomp;
      timings[2] += cur.t_plan;
      stream_stats[0] += cur.n_pos;
      stream_stats[1] += cur.n_plan;
      if (cur.rc) {
        if (pending) {
          const int prc = finish(flights[(k - 1) & 1]);
          if (!prc) nslots = k;
          rc = prc ? prc : fail(cur.rc, cur.err);
        } else {
          rc = fail(cur.rc, cur.err);
        }
        pending = false;
        break;
      }
      issue(cur, *slots[k], flights[k & 1]);
      issued = true;
    }
    if (pending) {
      const int prc = finish(flights[(k - 1) & 1]);
      release(k);
      if (prc) {
        rc = prc;
        if (issued) {  // let the issued stripe drain before its buffers go
          (void)hipEventSynchronize(flights[k & 1].done);
          issued = false;
        }
        break;
      }
      nslots = k;
    }
    pending = issued;
  }
  {
    std::lock_guard<std::mutex> lk(pm);
    quit = true;
  }
  pcv.notify_all();
  prep.join();
  return rc;
}
