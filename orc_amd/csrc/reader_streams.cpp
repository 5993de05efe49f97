// The reader's stream-level device steps: segment tables, integer / byte RLE
// stream decodes, dense values to rows, mid-stripe count reads.
#include "reader_internal.hh"

int orcg_reader::scatter(const void* dense, const uint8_t* nn, uint64_t n, void* out, int width) {
  return launch_scatter(act.ctx, dense, nn, n, out, width, 1, 0);
}

int orcg_reader::place_bytes(const void* dense, int width, const Rows& r, uint64_t pad, void** out) {
  *out = const_cast<void*>(dense);
  if (!r.row_nn) return ORCG_OK;
  ORCG_ALLOC_TO(uint8_t, *out, (r.n + pad) * (uint64_t)width);
  const int rc = scatter(dense, r.row_nn, r.n, *out, width);
  return rc ? fail_ctx(rc) : ORCG_OK;
}

// The stream's segment table: the host plan's, or (row-index streams) built
// on the device from the row groups' positions and the present-row prefix
// at each row group's first row (PRESENT streams count the incoming rows).
int orcg_reader::segments(Col& c, int slot, bool boolean, const Rows& r, const uint64_t** d_seg, uint64_t* nseg) {
  StreamBuf& sb = c.s[slot];
  if (!sb.pos) {
    *d_seg = (const uint64_t*)(D->d_stage + sb.seg_off);
    *nseg = sb.plan->segs.size();
    return ORCG_OK;
  }
  const uint64_t G = H->ngroups;
  if (!r.rg_rows) return fail(ORCG_INVALID_ARGUMENT, "row groups without row starts");
  const uint8_t* mask = slot == kSlotPresent ? r.in_nn : r.row_nn;
  int rc;
  if (mask) {
    // the row groups' set-row prefix and the segment table in one launch
    ORCG_ALLOC(int64_t, pre, G + 1);
    ORCG_ALLOC(uint64_t, seg, 2 * G);
    if ((rc = launch_rg_prefix_segtab(act.ctx, mask, r.n, r.rg_rows, G, (const int64_t*)(D->d_stage + sb.rg_off),
                                      boolean, pre, seg)))
      return fail_ctx(rc);
    *d_seg = seg;
    *nseg = G;
    return ORCG_OK;
  }
  ORCG_ALLOC(uint64_t, seg, 2 * G);
  if ((rc = launch_rg_segtab(act.ctx, (const int64_t*)(D->d_stage + sb.rg_off), r.rg_rows, G, boolean, seg)))
    return fail_ctx(rc);
  *d_seg = seg;
  *nseg = G;
  return ORCG_OK;
}

bool orcg_reader::device_counts(uint32_t id) const {
  const Col& c = H->cols[id];
  if (!rlev2_multi_capable(act.ctx->rlev2_variant)) return false;
  if (c.kind == ORCG_TYPE_DECIMAL) return false;  // Decimal64V2's decode takes its count on the host
  // every per-row value stream is RLEv2 (a struct has none)
  for (const StreamDesc& d : layout(id, c))
    if (d.count == kNonNull && (d.coding != kIntRle || rle_v1(c.encoding, d.force_v2))) return false;
  return true;
}

bool orcg_reader::device_work(uint32_t id) const {
  const Col& c = H->cols[id];
  if (!act.selected[id] || !c.supported) return false;
  if (c.s[kSlotPresent].present) return true;
  const uint32_t k = c.kind;
  auto done = [&](int slot) { return !c.s[slot].present || B.find(id, slot) != nullptr; };
  if (k == ORCG_TYPE_STRUCT) {
    for (uint32_t st : footer.types[id].subtypes)
      if (device_work(st)) return true;
    return false;
  }
  if (is_int_kind(k)) return !done(kSlotData);
  if (k == ORCG_TYPE_DOUBLE) return false;  // the stream bytes are the values
  if (k == ORCG_TYPE_DECIMAL && B.dec_done.count(id)) return false;  // the batch's decimal launch
  if (is_string_kind(k) && is_dict(c.encoding)) return B.dict_done.count(id) == 0;
  return true;
}

int orcg_reader::int_stream(Col& c, const StreamDesc& d, const Rows& r, uint64_t count, int64_t** pout,
                            const uint64_t* dcount) {
  const int slot = d.slot;
  const StripeBatch::Values* done = B.find((uint32_t)(&c - H->cols.data()), slot);
  if (done && done->count == count) {
    *pout = done->values;
    return ORCG_OK;
  }
  int64_t* out = alloc<int64_t>(count);
  if (!out) return fail_oom(__FILE_NAME__, __LINE__);
  *pout = out;
  StreamBuf& sb = c.s[slot];
  if (count == 0) return ORCG_OK;
  if (!sb.present) return fail(ORCG_PARSE_ERROR, "stream not found in column");
  const bool v1 = rle_v1(c.encoding, d.force_v2);
  // (with a device count the kernel reports a stream short of values)
  if (!dcount && !sb.pos && count > sb.plan->values) {
    const uint32_t e = sb.plan->err != kErrNone ? sb.plan->err : (uint32_t)(v1 ? kErrV1BadRead : kErrBadRead);
    return fail(dev_error_status(e), dev_error_message(e));
  }
  const uint8_t* d_src = D->d_stage + sb.host_off;
  const uint64_t* d_seg;
  uint64_t nseg;
  int rc = segments(c, slot, false, r, &d_seg, &nseg);
  if (rc) return rc;
  const int sg = d.is_signed ? 1 : 0;
  madd(kMDecodeCall, 1);
  rc = timed(0, [&]() -> int {
    if (v1) return launch_rlev1(act.ctx, d_src, sb.len, sg, d_seg, nseg, 0, count, out, 8);
    Rlev2Args a{};
    a.src = d_src;
    a.src_len = sb.len;
    a.is_signed = sg;
    a.segtab = d_seg;
    a.nsegs = nseg;
    a.nvalues = count;
    a.dst = out;
    a.dst_bytes = 8;
    a.dcount = dcount;
    return dcount ? launch_rlev2_tiled(act.ctx, a) : launch_rlev2(act.ctx, a);
  });
  return rc ? fail_ctx(rc) : ORCG_OK;
}

int orcg_reader::byte_stream(Col& c, const StreamDesc& d, const Rows& r, uint64_t count, uint8_t* out, uint64_t* d_ones,
                             const uint64_t* d_count) {
  const int slot = d.slot;
  const bool boolean = d.coding == kBoolRle;
  StreamBuf& sb = c.s[slot];
  if (count == 0) return ORCG_OK;
  if (!sb.present) return fail(ORCG_PARSE_ERROR, "stream not found in column");
  if (!sb.pos && !d_count) {  // (with a device count the kernel reports a short stream)
    const uint64_t avail = boolean ? sb.plan->values * 8 : sb.plan->values;
    if (count > avail) {
      const uint32_t e = sb.plan->err != kErrNone ? sb.plan->err : (uint32_t)kErrByteBadRead;
      return fail(dev_error_status(e), dev_error_message(e));
    }
  }
  const uint64_t* d_seg;
  uint64_t nseg;
  int rc = segments(c, slot, boolean, r, &d_seg, &nseg);
  if (rc) return rc;
  madd(kMByteCall, 1);
  rc = timed(1, [&]() -> int {
    return launch_byterle(act.ctx, D->d_stage + sb.host_off, sb.len, d_seg, nseg, boolean, 0, count, out, d_ones,
                          d_count);
  });
  return rc ? fail_ctx(rc) : ORCG_OK;
}

int orcg_reader::read_back(const std::vector<CountSrc>& srcs, uint64_t* out) {
  const int pr = poll_counts(srcs, out);
  if (pr != 1) return pr;
  if (srcs.size() > sync_cap) {
    if (h_sync) (void)hipHostFree(h_sync);
    h_sync = nullptr;
    sync_cap = 0;
    const size_t cap = std::max<size_t>(64, srcs.size());
    if (hipHostMalloc((void**)&h_sync, cap * 8, hipHostMallocDefault) != hipSuccess)
      return fail(ORCG_OUT_OF_MEMORY, "pinned allocation failed");
    sync_cap = cap;
  }
  std::vector<Ctx*> lanes_used;
  for (size_t i = 0; i < srcs.size(); ++i) {
    Ctx* l = srcs[i].lane;
    const int rc = hip_check(l, hipMemcpyAsync(h_sync + i, srcs[i].src, 8, hipMemcpyDeviceToHost, l->stream), "D2H");
    if (rc) return fail(rc, l->last_error);
    if (std::find(lanes_used.begin(), lanes_used.end(), l) == lanes_used.end()) lanes_used.push_back(l);
  }
  for (Ctx* l : lanes_used) {
    const int rc = hip_check(l, hipStreamSynchronize(l->stream), "hipStreamSynchronize");
    if (rc) return fail(rc, l->last_error);
  }
  for (size_t i = 0; i < srcs.size(); ++i) out[i] = h_sync[i];
  return ORCG_OK;
}

// the zone's device table, uploaded at its first use (synchronous copy)
int orcg_reader::zone_table(const ZoneEntry* cz, TzTable* out) {
  ZoneEntry* z = const_cast<ZoneEntry*>(cz);  // decodes are serialised by mu
  if (!z->d_tab) {
    const std::vector<int64_t> t = z->zone->device_table();
    int64_t* d = nullptr;
    if (hipMalloc((void**)&d, t.size() * 8) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ORCG_OUT_OF_MEMORY, "time zone table allocation failed");
    }
    if (hipMemcpy(d, t.data(), t.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(d);
      return fail(ORCG_DEVICE_ERROR, "H2D of the time zone table failed");
    }
    z->d_tab = d;
    z->words = (uint32_t)t.size();
  }
  out->d = z->d_tab;
  out->words = z->words;
  return ORCG_OK;
}
