// The stripe's multi-stream batch: before the upload, the streams (and what
// hangs off them: dictionaries, varint decimals, string length scans) whose
// counts the host knows are queued for one launch per kernel instance.
#include "reader_internal.hh"

int orcg_reader::queue_stream(uint32_t id, const StreamDesc& desc, const Rows& r, uint64_t count) {
  Col& c = H->cols[id];
  const int slot = desc.slot;
  const bool is_signed = desc.is_signed;
  StreamBuf& sb = c.s[slot];
  // left to decode(): empty or missing streams, RLEv1, a host plan short of
  // values (decode() raises the error in column order)
  if (count == 0 || !sb.present) return ORCG_OK;
  const bool v1 = rle_v1(c.encoding, desc.force_v2);
  if (!sb.pos && count > sb.plan->values) return ORCG_OK;
  // (collect() runs before the stripe's upload: no device work here)
  if (sb.pos && !(r.rg_rows && (v1 || rlev2_multi_capable(act.ctx->rlev2_variant)))) return ORCG_OK;
  if (v1) {
    // RLEv1: one host-built descriptor per segment (the plan's cuts, or the
    // row index with the stripe's row-group starts g * stride)
    int64_t* out = alloc<int64_t>(count);
    if (!out) return fail_oom(__FILE_NAME__, __LINE__);
    const uint8_t* d_src = D->d_stage + sb.host_off;
    const uint64_t stride = footer.row_index_stride;
    const size_t ns = sb.pos ? (size_t)H->ngroups : sb.plan->segs.size();
    auto at = [&](size_t g, uint64_t* off) -> uint64_t {
      if (sb.pos) {
        *off = (uint64_t)sb.trip[3 * g];
        const int64_t v = (int64_t)(g * stride) - sb.trip[3 * g + 1];
        return v < 0 ? 0ull : (uint64_t)v;
      }
      *off = sb.plan->segs[g].byte_offset;
      return sb.plan->segs[g].value_index;
    };
    for (size_t g = 0; g < ns; ++g) {
      V1SegDesc d{};
      d.src = d_src;
      d.src_len = sb.len;
      d.vi = at(g, &d.seg_start);
      d.seg_end = sb.len;
      d.v_next = ~0ull;
      if (g + 1 < ns) d.v_next = at(g + 1, &d.seg_end);
      d.dst = out;
      d.nvalues = count;
      d.err = D->d_errs + id;
      d.is_signed = is_signed ? 1u : 0u;
      B.v1_segs.push_back(d);
    }
    madd(kMDecodeCall, 1);
    B.put(id, slot, out, count);
    return ORCG_OK;
  }
  RleJob j{};
  if (sb.pos) {
    // the row index is the segment table (no rg_segtab launch): collect()
    // only queues columns whose rows are all values (no mask)
    j.trip = (const int64_t*)(D->d_stage + sb.rg_off);
    j.rows = r.rg_rows;
    j.nsegs = H->ngroups;
  } else {
    const uint64_t* d_seg;
    uint64_t nseg;
    int rc = segments(c, slot, false, r, &d_seg, &nseg);
    if (rc) return rc;
    j.segtab = d_seg;
    j.nsegs = nseg;
  }
  int64_t* out = alloc<int64_t>(count);
  if (!out) return fail_oom(__FILE_NAME__, __LINE__);
  j.src = D->d_stage + sb.host_off;
  j.src_len = sb.len;
  j.dst = out;
  j.nvalues = count;
  j.is_signed = is_signed ? 1u : 0u;
  j.err = D->d_errs + id;
  B.rlev2.push_back(j);
  madd(kMDecodeCall, 1);
  B.put(id, slot, out, count);
  return ORCG_OK;
}

// A dictionary column whose streams are both batched: its offsets and row
// gather join the stripe's dictionary launch (decode() then only wires the
// outputs and registers its F->checks).
int orcg_reader::queue_dict(uint32_t id, uint64_t n) {
  Col& c = H->cols[id];
  const uint64_t D_ = c.dict_size;
  if (D_ > kDictLds || !c.s[kSlotData].present) return ORCG_OK;
  if (D_ > 0 && !c.s[kSlotLength].present) return ORCG_OK;  // decode() raises the missing stream
  const StripeBatch::Values* li = B.find(id, kSlotLength);
  const StripeBatch::Values* di = B.find(id, kSlotData);
  if ((D_ > 0 && !li) || (n > 0 && !di)) return ORCG_OK;
  return push_dict(id, D_ ? li->values : nullptr, n ? di->values : nullptr, n, !act.lazy_dict, B.dict_done);
}

int orcg_reader::push_dict(uint32_t id, const int64_t* lengths, const int64_t* idx, uint64_t n, bool gather,
                           std::unordered_map<uint32_t, StripeBatch::DictDone>& done) {
  DictJob j{};
  j.lengths = lengths;
  j.dict_size = H->cols[id].dict_size;
  ORCG_ALLOC_TO(int64_t, j.offsets, j.dict_size + 1);
  const uint64_t* h_summary = nullptr;
  j.summary = rb_alloc(2, &h_summary);
  if (!j.summary) return ORCG_OK;  // no read-back slots: decode() does the dictionary itself
  j.idx = idx;
  j.nn = nullptr;
  j.n = gather ? n : 0;  // 0: offsets and summary only (decode() gathers the rows, or decoding is lazy)
  if (gather) {
    ORCG_ALLOC_TO(int64_t, j.start, n);
    ORCG_ALLOC_TO(int64_t, j.len, n);
  }
  j.err = D->d_errs + id;
  B.dict_jobs.push_back(j);
  done[id] = StripeBatch::DictDone{j.offsets, h_summary, j.start, j.len, const_cast<int64_t*>(j.idx)};
  return ORCG_OK;
}

int orcg_reader::queue_varint(uint32_t id) {
  Col& c = H->cols[id];
  const StreamBuf& sb = c.s[kSlotData];
  if (!sb.present || sb.len == 0) return ORCG_OK;
  VarintJob j{};
  j.src = D->d_stage + sb.host_off;
  j.len = sb.len;
  ORCG_ALLOC_TO(int64_t, j.counts, sb.len / kVarintTile + 2);
  ORCG_ALLOC_TO(int64_t, j.base, sb.len / kVarintTile + 3);
  const uint64_t* h_total = nullptr;
  j.total = rb_alloc(1, &h_total);
  if (!j.total) return ORCG_OK;  // no read-back slot: decode() counts it itself
  B.varint_jobs.push_back(j);
  B.varint_pre[id] = {j.base, h_total};
  B.launches.push_back(MultiLaunch{MultiLaunch::kVarintCounts, 0, &B.varint_jobs.back(), 1, 0, 0});
  return ORCG_OK;
}

int orcg_reader::queue_decimal(uint32_t id, uint64_t n) {
  const file::TypeInfo& t = footer.types[id];
  if (t.precision == 0 || n == 0) return ORCG_OK;  // Hive 0.11: the per-column path (its checks, nulling)
  const auto vp = B.varint_pre.find(id);
  const StripeBatch::Values* sc = B.find(id, kSlotSecondary);
  if (vp == B.varint_pre.end() || !sc || sc->count != n) return ORCG_OK;
  const bool wide = t.precision > 18;
  Col& c = H->cols[id];
  const StreamBuf& sb = c.s[kSlotData];
  DecJob j{};
  j.src = D->d_stage + sb.host_off;
  j.len = sb.len;
  j.tile_base = vp->second.first;
  j.scales = sc->values;
  j.nvalues = n;
  j.err = D->d_errs + id;
  j.scale = (int32_t)t.scale;
  int64_t* out = nullptr;
  ORCG_ALLOC_TO(int64_t, out, wide ? 2 * n : n);
  j.out = out;
  B.dec_jobs[wide ? 1 : 0].push_back(j);
  B.dec_done[id] = out;
  return ORCG_OK;
}

int orcg_reader::queue_scan(uint32_t id, uint64_t n) {
  const StripeBatch::Values* li = B.find(id, kSlotLength);
  if (n == 0 || !li || li->count != n || !H->cols[id].s[kSlotData].present) return ORCG_OK;
  ScanJob j{};
  j.in = li->values;
  j.n = n;
  ORCG_ALLOC_TO(int64_t, j.out, n + 1);
  const uint64_t *h_fl = nullptr, *h_need = nullptr;
  j.flags = rb_alloc(2, &h_fl);
  j.total = j.flags ? rb_alloc(1, &h_need) : nullptr;
  if (!j.total) return ORCG_OK;  // no read-back slots: decode() scans it itself
  B.scan_jobs.push_back(j);
  B.scan_done[id] = StripeBatch::ScanDone{j.out, h_fl, h_need, n};
  return ORCG_OK;
}

// Dictionaries below a column collect() does not descend into (a nullable
// column's subtree, a list's or map's children): a dictionary's size is in
// the stripe footer, so its LENGTH stream and entry offsets join the batch
// instead of being decoded after the parent's counts come back mid-stripe
// (configs[4]: the map keys' dictionary took three dependent launches on an
// idle GPU after the element counts were published, each blocking the host
// ~60-80 us, profiles/r06/inv/hip_api_c5_548c478.txt). LoadStringDictionary
// reads it whole whatever the rows (DictionaryLoader.cc:43-97).
int orcg_reader::collect_dicts(uint32_t id) {
  Col& c = H->cols[id];
  if (!act.selected[id] || !c.supported) return ORCG_OK;
  const uint32_t k = c.kind;
  if (is_string_kind(k) && is_dict(c.encoding)) {
    const uint64_t D_ = c.dict_size;
    if (D_ == 0 || D_ > kDictLds || !c.s[kSlotLength].present) return ORCG_OK;
    // (no row groups: a dictionary's LENGTH stream holds an entry per
    // dictionary entry, count == kDictSize, which reader_layout.hh never
    // positions by the row index, so the rows' row groups are never read)
    const Rows entries{D_, D_, nullptr, nullptr, nullptr, nullptr};
    int rc = queue_stream(id, *layout(id, c).find(kSlotLength), entries, D_);
    if (rc) return rc;
    const StripeBatch::Values* li = B.find(id, kSlotLength);
    if (!li || li->count != D_) return ORCG_OK;
    return push_dict(id, li->values, nullptr, 0, false, B.dict_pre);
  }
  for (uint32_t st : footer.types[id].subtypes) {
    const int rc = collect_dicts(st);
    if (rc) return rc;
  }
  return ORCG_OK;
}

// The integer-RLE streams decode() will read with host-known counts (no
// PRESENT stream here or above: each holds a value per row, or per dictionary
// entry), in the order of the column's layout -- the list decode() takes its
// slots and signedness from; then what the column's kind batches on top.
int orcg_reader::collect(uint32_t id, uint64_t n, const int64_t* rg_rows) {
  Col& c = H->cols[id];
  if (!act.selected[id] || !c.supported) return ORCG_OK;
  if (c.s[kSlotPresent].present) return collect_dicts(id);  // its counts come from the device
  const Rows r{n, n, nullptr, nullptr, rg_rows, nullptr};  // no masks: every row holds a value
  const uint32_t k = c.kind;
  const StreamLayout lay = layout(id, c);
  int rc = ORCG_OK;
  for (const StreamDesc& d : lay)
    if (!rc && d.coding == kIntRle) rc = queue_stream(id, d, r, d.count == kDictSize ? c.dict_size : n);
  if (rc) return rc;
  const StreamDesc* data = lay.find(kSlotData);
  if (data && data->coding == kVarint) {  // decimals
    if (c.s[kSlotSecondary].present) rc = queue_varint(id);
    if (!rc && c.s[kSlotData].present) rc = queue_decimal(id, n);
  } else if (is_string_kind(k)) {
    rc = is_dict(c.encoding) ? queue_dict(id, n) : queue_scan(id, n);
  } else if (k == ORCG_TYPE_LIST || k == ORCG_TYPE_MAP) {
    for (uint32_t st : footer.types[id].subtypes)
      if (!rc) rc = collect_dicts(st);
  } else if (k == ORCG_TYPE_STRUCT) {
    for (uint32_t st : footer.types[id].subtypes)
      if ((rc = collect(st, n, rg_rows))) break;
  }
  return rc;
}

// The queued jobs as launches, their job tables staged into the arena. The
// order the launches are appended in is the one run_multi assigns lanes by:
// the varint counts (as queue_varint queued them), the RLEv2 instances,
// RLEv1, the dictionaries, the decimals of mode 0 then 1, the length scans.
int orcg_reader::plan_batch() {
  Ctx* const ctx = act.ctx;
  int rc = ORCG_OK;
  if (!B.rlev2.empty()) rc = plan_rlev2_multi(ctx, B.rlev2.data(), (uint32_t)B.rlev2.size(), B.launches);
  if (!rc && !B.v1_segs.empty()) rc = plan_rlev1_multi(ctx, B.v1_segs.data(), B.v1_segs.size(), B.launches);
  if (!rc && !B.dict_jobs.empty())
    rc = plan_dict_multi(ctx, B.dict_jobs.data(), (uint32_t)B.dict_jobs.size(), B.launches);
  for (int mode = 0; mode < 2 && !rc; ++mode) {
    std::vector<DecJob>& g = B.dec_jobs[mode];
    if (g.empty()) continue;
    uint64_t tiles = 0;
    for (DecJob& j : g) {
      j.tile0 = tiles;
      tiles += (j.len + kVarintTile - 1) / kVarintTile;
    }
    const void* d = nullptr;
    if (!(rc = stage_table(ctx, g.data(), g.size() * sizeof(DecJob), &d)))
      B.launches.push_back(MultiLaunch{MultiLaunch::kDecimal, mode, d, (uint32_t)g.size(), tiles, 0});
  }
  if (rc) return fail_ctx(rc);
  for (const ScanJob& j : B.scan_jobs) B.launches.push_back(MultiLaunch{MultiLaunch::kLengthScan, 0, &j, 1, 0, 0});
  return ORCG_OK;
}
