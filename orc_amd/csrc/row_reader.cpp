#include "reader_internal.hh"

// ---- RowReader: batches of at most `capacity` rows over the stripes of a
// byte range (c++/src/Reader.cc RowReaderImpl: ctor :307-363, next
// :1392-1442, seekToRow :428-499, getRowNumber :424-426, markEndOfFile
// :1128-1139, startNextStripe's prefetch :1336-1360).
//
// The GPU decodes a whole stripe into HBM, which is copied once into a pinned
// host slab; each batch is a row range of that slab (per column an element
// range, through list / map offsets and union tags), so next() touches no
// device and waits for nothing but the slab of a new stripe. A worker thread
// per row reader prepares (host decompression), decodes and copies stripe
// s + 1 (and decompresses s + 2) while the caller consumes stripe s. The
// row reader keeps its own RowReaderOptions (include, lazy decoding), its own
// device slot and slabs; decodes take the reader's lock.

// A decoded stripe in pinned host memory.
struct HostSlab {
  uint64_t stripe = ~0ull;
  uint8_t* h = nullptr;
  size_t cap = 0;
  std::vector<ColOut> out;  // host pointers into h
  int rc = ORCG_OK;
  std::string err;
  ~HostSlab() { pinned_free(h); }
};

// The buffers of a decoded column, in the batch layout of
// include/orcg_reader.h: (field, bytes) pairs; col_field reads / rebinds one.
enum ColField { kFNn, kFData, kFLength, kFOffsets, kFBlob, kFSecondary, kFTags, kFIndex, kFDictOffsets };
static void col_buffers(const ColOut& o, const TypeInfo& t, std::vector<std::pair<int, uint64_t>>& b) {
  const uint64_t n = o.n;
  auto add = [&](int f, const void* p, uint64_t bytes) {
    if (p && bytes) b.push_back({f, bytes});
  };
  if (o.has_nulls) add(kFNn, o.nn, n);
  // a converted column has the layout of its read kind
  const uint32_t k = o.out_kind();
  if (k == ORCG_TYPE_DECIMAL) {
    const uint32_t p = o.out_precision(t.precision);
    add(kFData, o.data, (p > 18 || p == 0 ? 16 : 8) * n);
  } else if (k == ORCG_TYPE_LIST || k == ORCG_TYPE_MAP) {
    add(kFOffsets, o.offsets, 8 * (n + 1));
  } else if (k == ORCG_TYPE_UNION) {
    add(kFTags, o.tags, n);
    add(kFOffsets, o.offsets, 8 * n);
  } else if (k != ORCG_TYPE_STRUCT) {
    add(kFData, o.data, 8 * n);
  }
  add(kFLength, o.length, 8 * n);
  add(kFSecondary, o.secondary, 8 * n);
  add(kFIndex, o.index, 8 * n);
  add(kFDictOffsets, o.dict_offsets, 8 * (o.dict_size + 1));
  add(kFBlob, o.blob, o.blob_len);
}
static const void* col_get(const ColOut& o, int f) {
  switch (f) {
    case kFNn: return o.nn;
    case kFData: return o.data;
    case kFLength: return o.length;
    case kFOffsets: return o.offsets;
    case kFBlob: return o.blob;
    case kFSecondary: return o.secondary;
    case kFTags: return o.tags;
    case kFIndex: return o.index;
    default: return o.dict_offsets;
  }
}
static void col_set(ColOut& o, int f, const void* p) {
  switch (f) {
    case kFNn: o.nn = (const uint8_t*)p; break;
    case kFData: o.data = p; break;
    case kFLength: o.length = (const int64_t*)p; break;
    case kFOffsets: o.offsets = (const int64_t*)p; break;
    case kFBlob: o.blob = (const uint8_t*)p; break;
    case kFSecondary: o.secondary = (const int64_t*)p; break;
    case kFTags: o.tags = (const uint8_t*)p; break;
    case kFIndex: o.index = (const int64_t*)p; break;
    default: o.dict_offsets = (const int64_t*)p; break;
  }
}

struct orcg_row_reader {
  orcg_reader* r = nullptr;
  // This row reader's options: the reader's at its creation, with the
  // RowReaderOptions it was created with on top; immutable from then on.
  // opt.ctx is the worker's own context (stream, error record, scratch,
  // queues), owned here: the caller's context may be driven by its thread
  // while the worker decodes ahead, e.g. by another reader sharing it
  ReadOptions opt;
  uint64_t nstripes = 0, first = 0, last = 0;  // stripes [first, last) are in range
  uint64_t current = 0, row_in_stripe = 0, rows_in_stripe = 0;
  uint64_t previous_row = 0;
  std::vector<uint64_t> first_row;  // firstRowOfStripe_
  uint64_t batch_stripe = ~0ull, batch_row0 = 0, batch_rows = 0;
  std::vector<uint64_t> begin, count;  // per type id: element range of the current batch
  std::vector<uint8_t> in_batch;
  const HostSlab* cur = nullptr;  // the slab of the current batch

  // decode pipeline: host stages, one device slot, two host slabs (stripe
  // s in slab s & 1); slab_state 0 empty, 1 queued / decoding, 2 ready
  HostStage stage[2];
  uint64_t prepared[2] = {~0ull, ~0ull};
  std::unique_ptr<DevSlot> dev{new DevSlot()};
  HostSlab slab[2];
  int slab_state[2] = {0, 0};
  uint64_t slab_want[2] = {~0ull, ~0ull};
  std::thread worker;
  std::mutex m;
  std::condition_variable cv;
  std::string last_error;  // this row reader's last failure (orcg_row_reader_last_error)
  std::deque<uint64_t> jobs;
  bool stop = false;
  // worker seconds: [0] prepare inside a job (host decompression the
  // look-ahead did not do), [1] upload + decode, [2] D2H into the slab,
  // [3] slab (re)allocation, [4] look-ahead prepare; [5] caller waits for a
  // slab (orcg_row_reader_timings)
  std::atomic<uint64_t> prof[6] = {};  // nanoseconds
  uint64_t last_d2h = 0;               // bytes of the last slab copy (debug output)
  // NUMA node of the thread that created the row reader: the caller's
  // batch copies read the slabs, so their pages live there (the copy
  // helpers are placed there too, GpuRowReader.hh CopyPool)
  int node = -1;
  void addp(int i, double sec) { prof[i].fetch_add((uint64_t)(sec * 1e9), std::memory_order_relaxed); }

  ~orcg_row_reader() {
    {
      std::lock_guard<std::mutex> lk(m);
      stop = true;
      jobs.clear();
    }
    cv.notify_all();
    if (worker.joinable()) worker.join();
    if (opt.ctx) orcg_ctx_destroy(static_cast<orcg_ctx*>(opt.ctx));
  }

  void mark_end_of_file() {
    current = last;
    row_in_stripe = 0;
    rows_in_stripe = 0;
    previous_row = last == 0 ? 0 : first_row[last - 1] + r->footer.stripes[last - 1].num_rows;
  }

  // --- worker side -------------------------------------------------------
  // (every decode runs under r->mu with this row reader's options and
  // context as the reader's active ones, orcg_reader::Active; the reader's
  // own options are never touched)
  // D2H of every decoded column of `dev` into the slab: the stripe's
  // buffers sit in one device arena (DevPool), so sorted by address they
  // merge into a few ranges (gaps up to 1 MB copied along), one copy each;
  // then one synchronisation
  int copy_out(HostSlab& sl) {
    sl.out = dev->out;
    struct Buf {
      size_t col;
      int f;
      const uint8_t* d;
      uint64_t bytes;
      size_t range;
    };
    std::vector<Buf> bufs;
    std::vector<std::pair<int, uint64_t>> cb;
    for (size_t i = 0; i < sl.out.size(); ++i) {
      if (!sl.out[i].decoded) continue;
      ColOut& o = sl.out[i];
      if (o.index && o.dict_offsets && o.kind != ORCG_TYPE_DECIMAL) {
        // a dictionary column travels as entry + dictionary (8 B a row
        // instead of 24): the host looks up each row's start and length,
        // as StringDictionaryColumnReader::next does (ColumnReader.cc:561-594)
        o.data = nullptr;
        o.length = nullptr;
      }
      cb.clear();
      col_buffers(o, r->footer.types[i], cb);
      for (auto& x : cb) bufs.push_back(Buf{i, x.first, (const uint8_t*)col_get(sl.out[i], x.first), x.second, 0});
    }
    std::vector<size_t> order(bufs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return bufs[a].d < bufs[b].d; });
    struct Range {
      const uint8_t* d;
      uint64_t bytes, hoff;
    };
    std::vector<Range> rs;
    constexpr uint64_t kGap = 1u << 20;
    for (size_t q : order) {
      Buf& bf = bufs[q];
      if (!rs.empty() && bf.d >= rs.back().d && bf.d <= rs.back().d + rs.back().bytes + kGap) {
        const uint64_t end = (uint64_t)(bf.d - rs.back().d) + bf.bytes;
        rs.back().bytes = std::max(rs.back().bytes, end);
      } else {
        rs.push_back(Range{bf.d, bf.bytes, 0});
      }
      bf.range = rs.size() - 1;
    }
    uint64_t total = 0;
    for (Range& rg : rs) {
      rg.hoff = total;
      total += (rg.bytes + 255) & ~(uint64_t)255;
    }
    if (total > sl.cap) {
      const double ta = now_s();
      pinned_free(sl.h);
      sl.h = nullptr;
      sl.cap = 0;
      const uint64_t ncap = std::max<uint64_t>(total + (total >> 3), 1 << 20);
      if (!(sl.h = (uint8_t*)pinned_alloc(ncap, node)))
        return r->fail(ORCG_OUT_OF_MEMORY, "pinned row batch allocation failed");
      sl.cap = ncap;
      addp(3, now_s() - ta);
    }
    last_d2h = 0;
    for (const Range& rg : rs) last_d2h += rg.bytes;
    for (const Range& rg : rs) {
      const int rc = hip_check(opt.ctx, hipMemcpyAsync(sl.h + rg.hoff, rg.d, rg.bytes, hipMemcpyDeviceToHost,
                                                       opt.ctx->stream), "D2H row batch");
      if (rc) return r->fail_ctx(rc);
    }
    for (const Buf& bf : bufs) {  // the slab's views point at host memory
      const Range& rg = rs[bf.range];
      col_set(sl.out[bf.col], bf.f, sl.h + rg.hoff + (uint64_t)(bf.d - rg.d));
    }
    const int rc = hip_check(opt.ctx, hipStreamSynchronize(opt.ctx->stream), "hipStreamSynchronize");
    return rc ? r->fail_ctx(rc) : ORCG_OK;
  }
  void run_job(uint64_t t) {
    HostSlab& sl = slab[t & 1];
    HostStage& hs = stage[t & 1];
    int rc;
    std::string err;
    const double t0 = now_s();
    // host work ahead, concurrently with this stripe's decode and copies:
    // decompress stripe t + 1 into the other stage (stripe t - 1 is done
    // with it); prepare reads only the file and this row reader's selection
    // (when stripe t itself is not prepared yet, as for the first stripe, its
    // decompression goes first: the two would share the host threads and
    // delay the first batch)
    std::thread ahead;
    const uint64_t u = t + 1;
    auto start_ahead = [&] {
      if (u < last && prepared[u & 1] != u) {
        prepared[u & 1] = u;
        ahead = std::thread([this, u] {
          const double tp = now_s();
          (void)r->prepare(u, stage[u & 1], opt);  // a failure is kept in the stage
          addp(4, now_s() - tp);
        });
      }
    };
    if (prepared[t & 1] == t) start_ahead();
    {
      std::lock_guard<std::mutex> lk(r->mu);
      orcg_reader::Active scope(r, opt);
      (void)hipSetDevice(opt.ctx->device);
      rc = ORCG_OK;
      if (prepared[t & 1] != t) {
        prepared[t & 1] = t;
        rc = r->prepare(t, hs, opt);
        start_ahead();
      } else {
        rc = hs.rc;
      }
      if (rc) err = hs.err;
      const double t1 = now_s();
      if (!rc) {
        const double g3 = r->timings[3], g4 = r->timings[4];
        rc = r->upload_and_decode(hs, *dev);
        const double t2 = now_s();
        if (!rc) rc = copy_out(sl);
        if (rc) err = r->last_error;
        addp(1, t2 - t1);
        addp(2, now_s() - t2);
        if (debug_on("rowreader"))
          fprintf(stderr, "row reader stripe %llu: prepare %.2f ms, upload+decode %.2f ms (GPU upload %.2f, decode %.2f), "
                  "D2H %.2f ms (%.1f MB, %.1f GB/s)\n", (unsigned long long)t, (t1 - t0) * 1e3, (t2 - t1) * 1e3,
                  (r->timings[3] - g3) * 1e3, (r->timings[4] - g4) * 1e3, (now_s() - t2) * 1e3, last_d2h / 1e6,
                  last_d2h / 1e9 / std::max(now_s() - t2, 1e-9));
      }
      addp(0, t1 - t0);
      prepared[t & 1] = ~0ull;  // the stage is reused by stripe t + 2
    }
    {
      std::lock_guard<std::mutex> lk(m);
      sl.stripe = t;
      sl.rc = rc;
      sl.err = err;
      slab_state[t & 1] = 2;
    }
    cv.notify_all();
    if (ahead.joinable()) ahead.join();
  }
  void loop() {
    for (;;) {
      uint64_t t;
      {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return stop || !jobs.empty(); });
        if (stop) return;
        t = jobs.front();
        jobs.pop_front();
      }
      run_job(t);
    }
  }
  // queue stripe t into slab t & 1 (caller holds m)
  void post(std::unique_lock<std::mutex>& lk, uint64_t t) {
    // a queued / running decode into the same slab finishes first
    cv.wait(lk, [&] { return slab_state[t & 1] != 1; });
    slab_state[t & 1] = 1;
    slab_want[t & 1] = t;
    jobs.push_back(t);
    if (!worker.joinable()) worker = std::thread([this] { loop(); });
    cv.notify_all();
  }

  // --- caller side -------------------------------------------------------
  // make stripe s current (decoding it now if it is not already on its way),
  // then start the decode of s + 1
  int load(uint64_t s) {
    std::unique_lock<std::mutex> lk(m);
    HostSlab& sl = slab[s & 1];
    const bool mine = (slab_state[s & 1] == 2 && sl.stripe == s) || (slab_state[s & 1] == 1 && slab_want[s & 1] == s);
    if (!mine) post(lk, s);
    const double tw = now_s();
    cv.wait(lk, [&] { return slab_state[s & 1] == 2; });
    addp(5, now_s() - tw);
    if (sl.rc) {
      const int rc = sl.rc;
      last_error = sl.err;
      lk.unlock();
      r->fail_user(rc, sl.err);  // also the reader's (its workers write it under r->mu)
      lk.lock();
      slab_state[s & 1] = 0;  // a later seek decodes it again
      cur = nullptr;
      return rc;
    }
    cur = &sl;
    const uint64_t u = s + 1;
    if (u < last && !((slab_state[u & 1] == 2 && slab[u & 1].stripe == u) ||
                      (slab_state[u & 1] == 1 && slab_want[u & 1] == u)))
      post(lk, u);
    return ORCG_OK;
  }
  // element range [b, b + c) of column `id` and, recursively, its children
  void ranges(uint32_t id, uint64_t b, uint64_t c) {
    const ColOut& o = cur->out[id];
    if (!o.decoded) return;
    begin[id] = b;
    count[id] = c;
    in_batch[id] = 1;
    const auto& t = r->footer.types[id];
    if (t.kind == ORCG_TYPE_STRUCT) {
      for (uint32_t st : t.subtypes) ranges(st, b, c);
    } else if (t.kind == ORCG_TYPE_LIST || t.kind == ORCG_TYPE_MAP) {
      const int64_t e0 = o.offsets[b], e1 = o.offsets[b + c];
      for (uint32_t st : t.subtypes) ranges(st, (uint64_t)e0, (uint64_t)(e1 - e0));
    } else if (t.kind == ORCG_TYPE_UNION) {
      // child k's rows are the ranks of this batch's non-null tag-k rows
      for (uint32_t k = 0; k < t.subtypes.size(); ++k) {
        uint64_t cb = ~0ull, cc = 0;
        for (uint64_t i = b; i < b + c; ++i)
          if ((!o.has_nulls || o.nn[i]) && o.tags[i] == k) {
            if (cb == ~0ull) cb = (uint64_t)o.offsets[i];
            ++cc;
          }
        if (cb == ~0ull) cb = 0;  // no row of this batch carries tag k: an empty range
        ranges(t.subtypes[k], cb, cc);
      }
    }
  }
};

extern "C" {

int orcg_row_reader_create(orcg_reader* r, const orcg_row_reader_options* o, orcg_row_reader** out) {
  if (!r || !out) return ORCG_INVALID_ARGUMENT;
  *out = nullptr;
  if (!r->own.ctx) return r->fail_user(ORCG_INVALID_ARGUMENT, "reader has no device context");
  const uint64_t off = o ? o->offset : 0;
  const uint64_t len = o ? o->length : ~0ull;
  std::unique_ptr<orcg_row_reader> rr(new orcg_row_reader());
  rr->r = r;
  {
    // the reader's options as they are now
    std::lock_guard<std::mutex> lk(r->mu);
    rr->opt = r->own;
  }
  rr->opt.ctx = nullptr;  // its own, created below
  // then its RowReaderOptions: include, lazy decoding; opts->timezone replaces the reader zone
  int rc = compute_selection(r, o ? o->include : nullptr, o && o->include ? o->include_len : 0, rr->opt.selected);
  if (rc) return rc;
  rr->opt.lazy_dict = o && o->lazy_dictionary != 0;
  if (o && o->timezone) {
    const ZoneEntry* z = r->resolve_zone(o->timezone);
    if (!z || !z->zone)
      return r->fail_user(z ? ORCG_PARSE_ERROR : ORCG_INVALID_ARGUMENT,
                          z ? z->err : std::string("Time zone ") + o->timezone + " not found");
    rr->opt.reader_tz = z;
  }
  rr->node = current_numa_node();
  orcg_ctx* own = nullptr;
  if ((rc = orcg_ctx_create(r->own.ctx->device, &own)) != ORCG_OK)
    return r->fail_user(rc, "row reader context creation failed");
  rr->opt.ctx = own;
  // the caller's kernel choice, snapshotted once: the worker never reads the
  // caller's context
  own->rlev2_variant = r->own.ctx->rlev2_variant;
  // its side lanes (streams, events, error records) now, not in the first
  // stripe's decode
  if (side_lanes() > 1) (void)ctx_lane(own, side_lanes() - 1);
  const uint64_t ns = r->footer.stripes.size();
  rr->nstripes = ns;
  rr->current = ns;
  rr->last = 0;
  rr->first_row.resize(ns);
  uint64_t total = 0;
  for (uint64_t i = 0; i < ns; ++i) {
    rr->first_row[i] = total;
    const StripeInfo& si = r->footer.stripes[i];
    total += si.num_rows;
    // isStripeInRange: offset in [off, off + len), without wrapping
    if (si.offset >= off && si.offset - off < len) {
      if (i < rr->current) rr->current = i;
      if (i >= rr->last) rr->last = i + 1;
    }
  }
  rr->first = rr->current;
  if (rr->current == 0) rr->previous_row = ~0ull;
  else if (rr->current == ns) rr->previous_row = r->footer.num_rows;
  else rr->previous_row = rr->first_row[rr->first] - 1;
  const size_t nt = r->footer.types.size();
  rr->begin.assign(nt, 0);
  rr->count.assign(nt, 0);
  rr->in_batch.assign(nt, 0);
  // the first stripe's decode starts now, on the worker, so the process's
  // first-use costs (code objects, device and pinned allocations: ~40 ms on
  // configs[4]) overlap the caller's setup instead of its first next()
  if (rr->first < rr->last) {
    std::unique_lock<std::mutex> lk(rr->m);
    rr->post(lk, rr->first);
  }
  *out = rr.release();
  return ORCG_OK;
}

void orcg_row_reader_destroy(orcg_row_reader* rr) { delete rr; }

int orcg_row_reader_is_selected(const orcg_row_reader* rr, uint32_t type_id) {
  return rr && type_id < rr->opt.selected.size() && rr->opt.selected[type_id] ? 1 : 0;
}

int orcg_row_reader_next(orcg_row_reader* rr, uint64_t capacity, uint64_t* rows) {
  if (!rr || !rows) return ORCG_INVALID_ARGUMENT;
  ReaderCallScope call(rr->r);
  *rows = 0;
  std::fill(rr->in_batch.begin(), rr->in_batch.end(), 0);
  rr->batch_rows = 0;
  if (rr->current >= rr->last) {
    rr->mark_end_of_file();
    return ORCG_OK;
  }
  int rc;
  if (rr->row_in_stripe == 0 || !rr->cur || rr->cur->stripe != rr->current) {
    // startNextStripe (its slab was decoded ahead while the last one was read)
    if ((rc = rr->load(rr->current))) return rc;
    rr->rows_in_stripe = rr->r->footer.stripes[rr->current].num_rows;
  }
  const uint64_t n = std::min(capacity, rr->rows_in_stripe - rr->row_in_stripe);
  if (n == 0) {
    rr->mark_end_of_file();
    return ORCG_OK;
  }
  rr->batch_stripe = rr->current;
  rr->batch_row0 = rr->row_in_stripe;
  rr->batch_rows = n;
  rr->ranges(0, rr->row_in_stripe, n);
  rr->previous_row = rr->first_row[rr->current] + rr->row_in_stripe;
  rr->row_in_stripe += n;
  if (rr->row_in_stripe >= rr->rows_in_stripe) {
    rr->current += 1;
    rr->row_in_stripe = 0;
  }
  *rows = n;
  return ORCG_OK;
}

int orcg_row_reader_timings(orcg_row_reader* rr, double* out6) {
  if (!rr || !out6) return ORCG_INVALID_ARGUMENT;
  for (int i = 0; i < 6; ++i) out6[i] = rr->prof[i].load(std::memory_order_relaxed) * 1e-9;
  return ORCG_OK;
}

uint64_t orcg_row_reader_row_number(const orcg_row_reader* rr) { return rr ? rr->previous_row : 0; }

const char* orcg_row_reader_last_error(const orcg_row_reader* rr) { return rr ? rr->last_error.c_str() : "null row reader"; }

uint64_t orcg_row_reader_stripe(const orcg_row_reader* rr) { return rr ? rr->batch_stripe : ~0ull; }

int orcg_row_reader_seek_to_row(orcg_row_reader* rr, uint64_t row) {
  if (!rr) return ORCG_INVALID_ARGUMENT;
  if (rr->last == 0) return ORCG_OK;  // empty file / range
  const uint64_t ns = rr->nstripes;
  const uint64_t nrows = rr->r->footer.num_rows;
  if ((rr->last == ns && row >= nrows) || (rr->last < ns && row >= rr->first_row[rr->last])) {
    rr->current = ns;
    rr->previous_row = nrows;
    return ORCG_OK;
  }
  uint64_t s = 0;
  while (s + 1 < rr->last && rr->first_row[s + 1] <= row) ++s;
  if (s < rr->first) {
    rr->current = ns;
    rr->previous_row = nrows;
    return ORCG_OK;
  }
  rr->previous_row = row;
  rr->current = s;
  rr->row_in_stripe = row - rr->first_row[s];
  int rc = rr->load(s);
  if (rc) return rc;
  rr->rows_in_stripe = rr->r->footer.stripes[s].num_rows;
  return ORCG_OK;
}

int orcg_row_reader_column(const orcg_row_reader* rr, uint32_t id, orcg_column_view* view, uint64_t* begin,
                           uint64_t* count) {
  if (!rr || !view || !begin || !count || id >= rr->in_batch.size()) return ORCG_INVALID_ARGUMENT;
  memset(view, 0, sizeof(*view));
  view->type_id = id;
  view->kind = rr->r->footer.types[id].kind;
  *begin = *count = 0;
  if (!rr->in_batch[id] || !rr->cur) return ORCG_OK;  // no batch, or the column is not decoded
  const ColOut& c = rr->cur->out[id];
  fill_view(c, view);
  if (c.converted) view->kind = c.rkind;
  if (!c.decoded) return ORCG_OK;
  *begin = rr->begin[id];
  *count = rr->count[id];
  return ORCG_OK;
}

}  // extern "C"
