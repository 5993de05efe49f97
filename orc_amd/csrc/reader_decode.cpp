// Per-column decode: ColumnReader::next's PRESENT handling, then one function
// per column kind. Each takes its streams' slot, signedness and RLE version
// from the column's layout (reader_layout.hh), the list collect() queued the
// stripe's batch from. Struct columns and their side-lane fork:
// reader_fork.cpp.
#include "reader_internal.hh"

int orcg_reader::decode(uint32_t id, uint64_t n, const uint8_t* in_nn, uint64_t in_count, const int64_t* rg_rows,
                        const uint64_t* d_in_count, Col* in_col) {
  Col& c = H->cols[id];
  if (!act.selected[id] || !c.supported) return ORCG_OK;
  // this column's kernels report into its own device error record
  const Restore<uint32_t> col_scope(cur_col, id);
  const ErrRecordScope err_scope(act.ctx, D->d_errs + id);
  c.n = n;
  c.decoded = true;
  if (!c.stream_err.empty()) return fail(ORCG_PARSE_ERROR, c.stream_err);
  Rows r{n, 0, nullptr, nullptr, rg_rows, in_nn};
  const int rc = decode_present(c, in_count, d_in_count, in_col, &r);
  if (rc) return rc;
  const StreamLayout lay = layout(id, c);
  const uint32_t k = c.kind;
  c.converted = false;
  // schema evolution: a numeric or decimal column whose read type differs is
  // converted once its kind's decode has placed its rows
  const bool convert = act.read && id < act.read->conv.size() && act.read->conv[id] == rt::kConvert;
  auto then_convert = [&](int rc) { return rc || !convert ? rc : convert_column(id, c); };
  if (k == ORCG_TYPE_DECIMAL) return then_convert(decode_decimal(id, c, lay, r));
  if (is_timestamp_kind(k)) return decode_timestamp(c, lay, r);
  if (is_int_kind(k)) return then_convert(decode_integer(c, lay, r));
  if (k == ORCG_TYPE_BOOLEAN || k == ORCG_TYPE_BYTE) return then_convert(decode_bytes(c, lay, r));
  if (k == ORCG_TYPE_FLOAT || k == ORCG_TYPE_DOUBLE) return then_convert(decode_double(c, r));
  if (is_string_kind(k)) return is_dict(c.encoding) ? decode_dict_string(id, c, lay, r) : decode_direct_string(id, c, lay, r);
  if (k == ORCG_TYPE_LIST || k == ORCG_TYPE_MAP) return decode_list(id, c, lay, r);
  if (k == ORCG_TYPE_STRUCT) return decode_struct(id, c, r);
  if (k == ORCG_TYPE_UNION) return decode_union(id, c, lay, r);
  return ORCG_OK;
}

// ColumnReader::next: PRESENT bits for the incoming non-null rows
// (d_in: their count is on the device, in_count an upper bound)
int orcg_reader::decode_present(Col& c, uint64_t in_count, const uint64_t* d_in_count, Col* in_col, Rows* rows) {
  const uint32_t id = cur_col;
  const uint64_t n = rows->n;
  const uint8_t* const in_nn = rows->in_nn;
  const bool has_present = c.s[kSlotPresent].present;
  int rc;
  const bool dev = device_counts(id);
  const uint64_t* d_in = in_nn ? d_in_count : nullptr;
  if (d_in && !dev) {  // this column needs the incoming count on the host
    if ((rc = read_back(d_in, &in_count))) return rc;
    d_in = nullptr;
  }
  uint64_t nonnull = in_nn ? in_count : n;  // exact, or (d_nonnull) an upper bound
  const uint64_t* d_nonnull = d_in;
  uint8_t* nn = nullptr;
  if (has_present) {
    ORCG_ALLOC(uint8_t, bits, in_count + 8);
    // the decode counts the set rows it writes: the non-null rows, with or
    // without the parent's mask scattered in
    uint64_t* ones = D->d_ones + id;
    if ((rc = byte_stream(c, *layout(id, c).find(kSlotPresent), *rows, in_nn ? in_count : n, bits, ones, d_in))) return rc;
    if (in_nn) {
      ORCG_ALLOC_TO(uint8_t, nn, n);
      if ((rc = scatter(bits, in_nn, n, nn, 1))) return fail_ctx(rc);
    } else {
      nn = bits;
    }
    if (dev) {
      nonnull = n;
      d_nonnull = ones;
    } else {
      if ((rc = read_back(ones, &nonnull))) return rc;
      d_nonnull = nullptr;
    }
  } else if (in_nn) {
    nn = const_cast<uint8_t*>(in_nn);
  }
  c.has_nulls = nn != nullptr && (d_nonnull != nullptr || nonnull < n);
  if (in_nn && !has_present) c.has_nulls = true;  // incoming mask copied (:97-101)
  c.nn = c.has_nulls ? nn : nullptr;
  // provisional has_nulls: settled by the stripe's F->checks (column order:
  // a parent's before its children's)
  if (has_present && d_nonnull) {
    const uint64_t* h = defer(d_nonnull, 1);
    if (!h) return fail(ORCG_DEVICE_ERROR, "D2H of the non-null count failed");
    c.nulls_deferred = true;
    Col* cp = &c;
    F->checks.emplace_back(cur_col, [cp, h, n]() -> int {
      if (*h >= n) {
        cp->has_nulls = false;
        cp->nn = nullptr;
      }
      return ORCG_OK;
    });
  } else if (in_nn && !has_present && in_col && in_col->nulls_deferred) {
    c.nulls_deferred = true;
    Col* cp = &c;
    F->checks.emplace_back(cur_col, [cp, in_col]() -> int {
      if (!in_col->has_nulls) {  // the parent had no nulls after all: no mask was passed down
        cp->has_nulls = false;
        cp->nn = nullptr;
      }
      return ORCG_OK;
    });
  }
  rows->nonnull = nonnull;
  rows->d_nonnull = d_nonnull;
  rows->row_nn = c.nn;
  return ORCG_OK;
}

int orcg_reader::decode_decimal(uint32_t id, Col& c, const StreamLayout& lay, const Rows& r) {
  const file::TypeInfo& t = footer.types[id];
  const std::string cid = std::to_string(id);
  const uint64_t nonnull = r.nonnull;
  const bool has_data = c.s[kSlotData].present;
  int rc;
  if (decimal64_v2(t, decimal_as_long)) {
    // Decimal64ColumnReaderV2 (ColumnReader.cc:1529-1576): RLEv2 unscaled values
    if (!has_data) return fail(ORCG_PARSE_ERROR, "DATA stream not found in Decimal64V2 column. ColumnId=" + cid);
    int64_t* dense;
    if ((rc = int_stream(c, *lay.find(kSlotData), r, nonnull, &dense))) return rc;
    return place(dense, 8, r, &c.data);
  }
  // Decimal64ColumnReader / Decimal128ColumnReader (:1384-1527): varint
  // DATA, per-value scales in SECONDARY (signed RLE)
  if (!has_data) return fail(ORCG_PARSE_ERROR, "DATA stream not found in Decimal64Column");
  if (!c.s[kSlotSecondary].present) return fail(ORCG_PARSE_ERROR, "SECONDARY stream not found in Decimal64Column");
  // Hive 0.11 (precision 0): Decimal128 at the forced scale (DecimalHive11ColumnReader, :1627-1687)
  const bool hive11 = t.precision == 0;
  const bool wide = hive11 || t.precision > 18;
  int64_t* scales;
  if ((rc = int_stream(c, *lay.find(kSlotSecondary), r, nonnull, &scales))) return rc;
  const StreamBuf& sb = c.s[kSlotData];
  const uint8_t* d_src = D->d_stage + sb.host_off;
  int64_t* base = nullptr;
  const uint64_t* total = nullptr;
  const auto vp = B.varint_pre.find(id);
  if (vp != B.varint_pre.end()) {
    // tile counts + scan ran with the batch (queue_varint)
    base = vp->second.first;
    total = vp->second.second;
  } else {
    uint64_t ntiles = 0;
    ORCG_ALLOC(int64_t, counts, sb.len / kVarintTile + 2);
    ORCG_ALLOC_TO(int64_t, base, sb.len / kVarintTile + 3);
    const uint64_t* h_total = nullptr;
    uint64_t* d_total = rb_alloc(1, &h_total);
    if ((rc = launch_varint_tile_counts(act.ctx, d_src, sb.len, counts, &ntiles))) return fail_ctx(rc);
    if ((rc = launch_exclusive_scan(act.ctx, counts, ntiles, base, nullptr, d_total))) return fail_ctx(rc);
    total = d_total ? h_total : defer(base + ntiles, 1);
    if (!total) return fail(ORCG_DEVICE_ERROR, "D2H of the varint count failed");
  }
  F->checks.emplace_back(cur_col, [this, total, nonnull, cid]() -> int {
    return *total < nonnull ? fail(ORCG_PARSE_ERROR, "Read past end of stream in Decimal64ColumnReader column " +
                                                         cid + " kind DATA")
                            : ORCG_OK;
  });
  const auto dd = B.dec_done.find(id);
  if (dd != B.dec_done.end() && !r.row_nn) {
    // decoded by the batch's decimal launch (queue_decimal)
    c.data = dd->second;
    return ORCG_OK;
  }
  ORCG_ALLOC(int64_t, dense, wide ? 2 * nonnull : nonnull);
  // throwOnHive11DecimalOverflow(false): overflowing values become NULL
  const bool nullify = hive11 && !hive11_throw;
  uint8_t* keep = nullptr;
  if (nullify) {
    ORCG_ALLOC_TO(uint8_t, keep, nonnull + 8);
  }
  if ((rc = launch_varint_decimal(act.ctx, d_src, sb.len, base, scales, nonnull,
                                  hive11 ? hive11_scale : (int32_t)t.scale, hive11 ? (nullify ? 3 : 2) : (wide ? 1 : 0),
                                  dense, keep)))
    return fail_ctx(rc);
  if ((rc = place(dense, wide ? 16 : 8, r, &c.data))) return rc;
  return nullify && nonnull ? decode_hive11_nulls(c, keep, r) : ORCG_OK;
}

// The row mask of a Hive 0.11 column read with overflows nulled: rows present
// in the stream AND kept (the reference clears notNull[i] and sets hasNulls,
// ColumnReader.cc:1650-1677)
int orcg_reader::decode_hive11_nulls(Col& c, const uint8_t* keep, const Rows& r) {
  const uint64_t n = r.n;
  int rc;
  const uint8_t* rnn;
  if ((rc = place(keep, 1, r, &rnn, 8))) return rc;  // (the 8 bytes of padding `keep` has)
  // the column's own count word: sibling decimal columns decode on other
  // side lanes concurrently
  const uint64_t* h_kept = nullptr;
  uint64_t* kept_d = rb_alloc(1, &h_kept);
  if (!kept_d) ORCG_ALLOC_TO(uint64_t, kept_d, 1);
  if ((rc = launch_count_nonzero(act.ctx, rnn, n, kept_d))) return fail_ctx(rc);
  const uint64_t* kept = defer(kept_d, 1);
  if (!kept) return fail(ORCG_DEVICE_ERROR, "D2H of the kept decimal count failed");
  Col* cp = &c;
  F->checks.emplace_back(cur_col, [cp, kept, rnn, n]() -> int {
    if (*kept < n) {
      cp->has_nulls = true;
      cp->nn = rnn;
    }
    return ORCG_OK;
  });
  return ORCG_OK;
}

// ConvertColumnReader::next (ConvertColumnReader.cc:38-48, and the readers
// built on it): the file type's column is read first (c.data, c.nn), then each
// set row is converted to the read type. One launch a converted column; the
// rows it nulled are counted into a read-back slot, and a check after the
// column's own PRESENT check settles has_nulls and the mask. The incoming mask
// may be the parent's buffer: the kernel writes a new one.
int orcg_reader::convert_column(uint32_t id, Col& c) {
  const TypeInfo& ft = footer.types[id];
  const rt::Node& rn = act.read->tree[id];
  c.converted = true;
  c.rkind = rn.kind;
  c.rprecision = rn.precision;
  c.rscale = rn.scale;
  const uint64_t n = c.n;
  if (n == 0) return ORCG_OK;
  int src;
  if (ft.kind == ORCG_TYPE_DECIMAL) src = ft.precision <= 18 ? kConvDec64 : kConvDec128;
  else if (ft.kind == ORCG_TYPE_FLOAT) src = kConvFloat;
  else if (ft.kind == ORCG_TYPE_DOUBLE) src = kConvDouble;
  else src = kConvInt64;
  ConvertArgs a{};
  int dst;
  switch (rn.kind) {
    case ORCG_TYPE_BOOLEAN: dst = kToBool; break;
    case ORCG_TYPE_BYTE: dst = kToInt, a.width = 1; break;
    case ORCG_TYPE_SHORT: dst = kToInt, a.width = 2; break;
    case ORCG_TYPE_INT: dst = kToInt, a.width = 4; break;
    case ORCG_TYPE_LONG: dst = kToInt, a.width = 8; break;
    case ORCG_TYPE_FLOAT: dst = kToFloat; break;
    case ORCG_TYPE_DOUBLE: dst = kToDouble; break;
    default: dst = rn.precision <= 18 ? kToDec64 : kToDec128; break;
  }
  int rc;
  ORCG_ALLOC(int64_t, out, dst == kToDec128 ? 2 * n : n);
  ORCG_ALLOC(uint8_t, out_nn, n + 8);
  // [0] the rows nulled, [1] the first overflowing row (throw mode): a record
  // of its own, so that a decode error of this column, whatever its row, wins
  const uint64_t* h = nullptr;
  uint64_t* slots = rb_alloc(2, &h);
  if (!slots) {
    ORCG_ALLOC_TO(uint64_t, slots, 2);
    if ((rc = hip_check(act.ctx, hipMemsetAsync(slots, 0, 8, act.ctx->stream), "memset"))) return fail_ctx(rc);
  }
  if (act.evo_throw && (rc = hip_check(act.ctx, hipMemsetAsync(slots + 1, 0xff, 8, act.ctx->stream), "memset")))
    return fail_ctx(rc);
  a.src = c.data;
  a.nn = c.has_nulls ? c.nn : nullptr;
  a.out = out;
  a.out_nn = out_nn;
  a.n = n;
  a.err = (unsigned long long*)(slots + 1);
  a.nulled = (unsigned long long*)slots;
  a.src_scale = (int32_t)ft.scale;
  a.precision = (int32_t)rn.precision;
  a.scale = (int32_t)rn.scale;
  a.throw_mode = act.evo_throw ? 1 : 0;
  convert_constants(src, &a);
  if ((rc = launch_convert(act.ctx, src, dst, a))) return fail_ctx(rc);
  if (!h && !(h = defer(slots, 2))) return fail(ORCG_DEVICE_ERROR, "D2H of the conversion's counts failed");
  c.data = out;
  if (c.has_nulls) c.nn = out_nn;  // the incoming nulls and the overflows
  Col* cp = &c;
  const uint64_t* rec = F->h_rb + cur_col;  // the column's own error record, read back with the stripe
  const bool thrown = act.evo_throw;
  const std::shared_ptr<const ReadPlan> plan = act.read;
  F->checks.emplace_back(cur_col, [this, cp, h, out_nn, rec, thrown, id, plan]() -> int {
    if (thrown && h[1] != kNoError && *rec == kNoError) {
      if (act.ctx) act.ctx->last_error_value = h[1] >> 8;
      return fail(ORCG_PARSE_ERROR, std::string(dev_error_message(kErrConvertOverflow)) + " from " +
                                        rt::to_string(file_tree(), id) + " to " + rt::to_string(plan->tree, id));
    }
    if (h[0]) {
      cp->has_nulls = true;
      cp->nn = out_nn;
    }
    return ORCG_OK;
  });
  return ORCG_OK;
}

// TimestampColumnReader (:259-349): seconds (signed RLE), nanos (unsigned RLE)
int orcg_reader::decode_timestamp(Col& c, const StreamLayout& lay, const Rows& r) {
  if (!c.s[kSlotData].present) return fail(ORCG_PARSE_ERROR, "DATA stream not found in Timestamp column");
  if (!c.s[kSlotSecondary].present) return fail(ORCG_PARSE_ERROR, "SECONDARY stream not found in Timestamp column");
  int rc;
  int64_t *secs, *nanos;
  if ((rc = int_stream(c, *lay.find(kSlotData), r, r.nonnull, &secs, r.d_nonnull))) return rc;
  if ((rc = int_stream(c, *lay.find(kSlotSecondary), r, r.nonnull, &nanos, r.d_nonnull))) return rc;
  // TIMESTAMP_INSTANT ignores both zones; the same zone on both sides is
  // sameTimezone_ (:286): no adjustment, with that zone's epoch
  const ZoneEntry* wz = c.kind == ORCG_TYPE_TIMESTAMP ? H->writer_zone : nullptr;
  if (wz && !act.reader_tz) return fail(ORCG_INVALID_ARGUMENT, "reader time zone not found");
  if (wz && !act.reader_tz->zone) return fail(ORCG_PARSE_ERROR, act.reader_tz->err);
  if (!wz || wz == act.reader_tz) {
    if ((rc = launch_timestamp(act.ctx, secs, nanos, r.nonnull, wz ? wz->zone->epoch() : kOrcEpochUtc)))
      return fail_ctx(rc);
  } else {
    TzTable wt, rt;
    if ((rc = zone_table(wz, &wt)) || (rc = zone_table(act.reader_tz, &rt))) return rc;
    if ((rc = launch_timestamp_tz(act.ctx, secs, nanos, r.nonnull, wt, rt))) return fail_ctx(rc);
  }
  if ((rc = place(secs, 8, r, &c.data))) return rc;
  return place(nanos, 8, r, &c.secondary);
}

int orcg_reader::decode_integer(Col& c, const StreamLayout& lay, const Rows& r) {
  if (!c.s[kSlotData].present) return fail(ORCG_PARSE_ERROR, "DATA stream not found in Integer column");
  int64_t* dense;
  const int rc = int_stream(c, *lay.find(kSlotData), r, r.nonnull, &dense, r.d_nonnull);
  return rc ? rc : place(dense, 8, r, &c.data);
}

int orcg_reader::decode_bytes(Col& c, const StreamLayout& lay, const Rows& r) {
  const bool boolean = c.kind == ORCG_TYPE_BOOLEAN;
  if (!c.s[kSlotData].present)
    return fail(ORCG_PARSE_ERROR, boolean ? "DATA stream not found in Boolean column"
                                          : "DATA stream not found in Byte column");
  int rc;
  ORCG_ALLOC(uint8_t, bytes, r.nonnull + 8);
  if ((rc = byte_stream(c, *lay.find(kSlotData), r, r.nonnull, bytes))) return rc;
  ORCG_ALLOC(int64_t, dense, r.nonnull);
  if ((rc = launch_widen(act.ctx, bytes, boolean ? kWidenU8 : kWidenI8, r.nonnull, dense))) return fail_ctx(rc);
  return place(dense, 8, r, &c.data);
}

int orcg_reader::decode_double(Col& c, const Rows& r) {
  if (!c.s[kSlotData].present) return fail(ORCG_PARSE_ERROR, "DATA stream not found in Double column");
  StreamBuf& sb = c.s[kSlotData];
  const uint64_t w = c.kind == ORCG_TYPE_FLOAT ? 4 : 8;
  if (sb.len < w * r.nonnull) return fail(ORCG_PARSE_ERROR, "bad read in DoubleColumnReader::next()");
  const void* raw = D->d_stage + sb.host_off;
  double* dense;
  if (c.kind == ORCG_TYPE_FLOAT) {
    ORCG_ALLOC_TO(double, dense, r.nonnull);
    const int rc = launch_widen(act.ctx, raw, kWidenF32, r.nonnull, dense);
    if (rc) return fail_ctx(rc);
  } else {
    dense = (double*)raw;  // zero copy: the stream bytes are the values
  }
  return place(dense, 8, r, &c.data);
}

void orcg_reader::check_dictionary(uint32_t id, Col& c, const uint64_t* h) {
  const std::string cid = std::to_string(id);
  StreamBuf& db = c.s[kSlotDict];
  Col* cp = &c;
  const bool db_present = db.present;
  const uint64_t db_len = db.present ? db.len : 0;
  F->checks.emplace_back(cur_col, [this, h, cp, db_present, db_len, cid]() -> int {
    if (h[1]) return fail(ORCG_PARSE_ERROR, "Negative dictionary entry length for column " + cid);
    if (h[0] > 0 && !db_present)
      return fail(ORCG_PARSE_ERROR, "DICTIONARY_DATA stream not found in StringDictionaryColumn for column " + cid);
    if (h[0] > db_len) return fail(ORCG_PARSE_ERROR, "bad read in readFully");
    cp->blob_len = h[0];
    return ORCG_OK;
  });
  c.blob = db.present ? D->d_stage + db.host_off : nullptr;
}

int orcg_reader::decode_dict_string(uint32_t id, Col& c, const StreamLayout& lay, const Rows& r) {
  const uint64_t n = r.n;
  const auto dd = B.dict_done.find(id);
  if (dd != B.dict_done.end()) {
    // batched (queue_dict): offsets, summary and gather come from the
    // stripe's dictionary launch; the reference's checks, in its order
    check_dictionary(id, c, dd->second.h_summary);
    c.index = dd->second.idx;
    c.dict_offsets = dd->second.offsets;
    c.data = dd->second.start;
    c.length = dd->second.len;
    return ORCG_OK;
  }
  int rc;
  int64_t* start = nullptr;
  int64_t* len = nullptr;
  if (!act.lazy_dict) {
    ORCG_ALLOC_TO(int64_t, start, n);
    ORCG_ALLOC_TO(int64_t, len, n);
  }
  // loadStringDictionary (DictionaryLoader.cc:43-97), then
  // StringDictionaryColumnReader::next (ColumnReader.cc:561-594)
  const uint64_t dict_size = c.dict_size;
  if (dict_size > 0 && !c.s[kSlotLength].present)
    return fail(ORCG_PARSE_ERROR, "LENGTH stream not found in StringDictionaryColumn for column " + std::to_string(id));
  int64_t* doff;
  const uint64_t* h;
  const auto pre = B.dict_pre.find(id);
  if (pre != B.dict_pre.end()) {
    // offsets and summary from the stripe's dictionary launch (collect_dicts)
    doff = pre->second.offsets;
    h = pre->second.h_summary;
    if (B.pre_on_lane &&
        (rc = hip_check(act.ctx, hipStreamWaitEvent(act.ctx->stream, B.ev_pre, 0), "dictionary batch wait")))
      return fail_ctx(rc);
  } else {
    int64_t* dlen;
    ORCG_ALLOC_TO(int64_t, doff, dict_size + 1);
    if ((rc = int_stream(c, *lay.find(kSlotLength), r, dict_size, &dlen))) return rc;
    const uint64_t* h_sum = nullptr;
    uint64_t* summary = rb_alloc(2, &h_sum);  // blob bytes, negative-length flag
    if (!summary) ORCG_ALLOC_TO(uint64_t, summary, 2);
    if (dict_size <= 65536) {
      // offsets, blob size and the negative-length check in one launch
      if ((rc = launch_dict_offsets(act.ctx, dlen, dict_size, doff, summary))) return fail_ctx(rc);
    } else {
      if ((rc = launch_flag_negative(act.ctx, dlen, dict_size, summary + 1))) return fail_ctx(rc);
      if ((rc = launch_exclusive_scan(act.ctx, dlen, dict_size, doff))) return fail_ctx(rc);
      if ((rc = hip_check(act.ctx,
                          hipMemcpyAsync(summary, doff + dict_size, 8, hipMemcpyDeviceToDevice, act.ctx->stream),
                          "copy")))
        return fail_ctx(rc);
    }
    h = defer(summary, 2);
    if (!h) return fail(ORCG_DEVICE_ERROR, "D2H of the dictionary size failed");
  }
  check_dictionary(id, c, h);
  if (!c.s[kSlotData].present) return fail(ORCG_PARSE_ERROR, "DATA stream not found in StringDictionaryColumn");
  int64_t *idx, *ridx;
  if ((rc = int_stream(c, *lay.find(kSlotData), r, r.nonnull, &idx, r.d_nonnull))) return rc;
  if ((rc = place(idx, 8, r, &ridx))) return rc;
  c.index = ridx;
  c.dict_offsets = doff;
  if (!act.lazy_dict) {
    // StringDictionaryColumnReader::next: bounds-checked gather; nextEncoded
    // (lazy) hands out the indices and the dictionary unchecked (:596-607)
    if (r.row_nn) {
      if ((rc = hip_check(act.ctx, hipMemsetAsync(start, 0, n * 8, act.ctx->stream), "memset"))) return fail_ctx(rc);
      if ((rc = hip_check(act.ctx, hipMemsetAsync(len, 0, n * 8, act.ctx->stream), "memset"))) return fail_ctx(rc);
    }
    if ((rc = launch_dict_gather(act.ctx, ridx, 8, r.row_nn, n, doff, dict_size, start, len))) return fail_ctx(rc);
  }
  c.data = start;
  c.length = len;
  return ORCG_OK;
}

int orcg_reader::decode_direct_string(uint32_t id, Col& c, const StreamLayout& lay, const Rows& r) {
  if (!c.s[kSlotLength].present) return fail(ORCG_PARSE_ERROR, "LENGTH stream not found in StringDirectColumn");
  if (!c.s[kSlotData].present) return fail(ORCG_PARSE_ERROR, "DATA stream not found in StringDirectColumn");
  int rc;
  int64_t* dlen;
  if ((rc = int_stream(c, *lay.find(kSlotLength), r, r.nonnull, &dlen))) return rc;
  const uint64_t ns = r.nonnull;
  // computeSize's checks (ColumnReader.cc:694-710) ride the scan: a
  // negative length, the total's overflow (then the blob's size below),
  // in the reference's order; the flags start at 0 (read-back block).
  // The batch's scan (queue_scan) already ran for a column without nulls.
  const auto sd = B.scan_done.find(id);
  const bool pre = sd != B.scan_done.end() && !r.row_nn && sd->second.n == ns;
  int64_t* dstart = nullptr;
  const uint64_t* h_fl = nullptr;
  const uint64_t* need = nullptr;
  uint64_t* flags = nullptr;
  if (pre) {
    dstart = sd->second.starts;
    h_fl = sd->second.h_flags;
    need = sd->second.h_need;
  } else {
    ORCG_ALLOC_TO(int64_t, dstart, ns + 1);
    flags = rb_alloc(2, &h_fl);
    if (!flags) {
      ORCG_ALLOC_TO(uint64_t, flags, 2);
      if ((rc = hip_check(act.ctx, hipMemsetAsync(flags, 0, 16, act.ctx->stream), "flags memset"))) return fail_ctx(rc);
    }
    uint64_t* d_need = rb_alloc(1, &need);
    if ((rc = launch_exclusive_scan(act.ctx, dlen, ns, dstart, flags, d_need))) return fail_ctx(rc);
  }
  StreamBuf& db = c.s[kSlotData];
  c.blob = D->d_stage + db.host_off;
  c.blob_len = db.len;
  if (!h_fl && !(h_fl = defer(flags, 2))) return fail(ORCG_DEVICE_ERROR, "D2H of the string length checks failed");
  if (!need && !(need = defer(dstart + ns, 1))) return fail(ORCG_DEVICE_ERROR, "D2H of the string bytes failed");
  const uint64_t blob_len = c.blob_len;
  const uint32_t col_id = cur_col;
  F->checks.emplace_back(cur_col, [this, need, blob_len, h_fl, col_id]() -> int {
    if (h_fl[0])
      return fail(ORCG_PARSE_ERROR,
                  "Negative string length in StringDirectColumnReader for column " + std::to_string(col_id));
    if (h_fl[1])
      return fail(ORCG_PARSE_ERROR,
                  "String length overflow in StringDirectColumnReader for column " + std::to_string(col_id));
    return *need > blob_len ? fail(ORCG_PARSE_ERROR, "failed to read in StringDirectColumnReader.next") : ORCG_OK;
  });
  if ((rc = place(dstart, 8, r, &c.data))) return rc;
  return place(dlen, 8, r, &c.length);
}

int orcg_reader::decode_list(uint32_t id, Col& c, const StreamLayout& lay, const Rows& r) {
  const uint64_t n = r.n;
  if (!c.s[kSlotLength].present)
    return fail(ORCG_PARSE_ERROR, c.kind == ORCG_TYPE_LIST ? "LENGTH stream not found in List column"
                                                           : "LENGTH stream not found in Map column");
  int rc;
  int64_t *dlen, *rlen;
  if ((rc = int_stream(c, *lay.find(kSlotLength), r, r.nonnull, &dlen, r.d_nonnull))) return rc;
  if ((rc = place(dlen, 8, r, &rlen))) return rc;
  ORCG_ALLOC(int64_t, off, n + 1);
  if ((rc = launch_exclusive_scan(act.ctx, rlen, n, off))) return fail_ctx(rc);
  c.offsets = off;
  // the children's row groups start at the list offsets of the parent's
  int64_t* child_rows = nullptr;
  if (r.rg_rows && H->ngroups) {
    ORCG_ALLOC_TO(int64_t, child_rows, H->ngroups);
    if ((rc = launch_rg_child_rows(act.ctx, off, r.rg_rows, H->ngroups, child_rows))) return fail_ctx(rc);
  }
  if (pending) {
    // under a fork: the children wait for the fork's next level, whose
    // element counts are read back together (one synchronisation per level
    // instead of one per list / map, which would stall the other lanes)
    pending->push_back(Pending{id, off + n, child_rows, act.ctx});
    return ORCG_OK;
  }
  uint64_t total = 0;
  if ((rc = read_back(off + n, &total))) return rc;
  for (uint32_t st : footer.types[id].subtypes)
    if ((rc = decode(st, total, nullptr, total, child_rows))) return rc;
  return ORCG_OK;
}

// UnionColumnReader (ColumnReader.cc:1158-1274): byte-RLE tags for the
// non-null rows; each row's offset is its rank among the rows of its tag;
// child k reads as many rows as carry tag k
int orcg_reader::decode_union(uint32_t id, Col& c, const StreamLayout& lay, const Rows& r) {
  const uint64_t n = r.n, nonnull = r.nonnull;
  if (!c.s[kSlotData].present) return fail(ORCG_PARSE_ERROR, "LENGTH stream not found in Union column");
  int rc;
  const std::vector<uint32_t> subs = footer.types[id].subtypes;
  const uint32_t nch = (uint32_t)subs.size();
  ORCG_ALLOC(uint8_t, dtags, nonnull + 8);
  if ((rc = byte_stream(c, *lay.find(kSlotData), r, nonnull, dtags))) return rc;
  ORCG_ALLOC(uint64_t, bad, 1);
  if ((rc = launch_union_check(act.ctx, dtags, nonnull, nch, bad))) return fail_ctx(rc);
  ORCG_ALLOC(int64_t, doffs, nonnull);
  ORCG_ALLOC(int64_t, flags, nonnull);
  // dense index of each row group's first row (children's row groups)
  const int64_t* dense_rows = r.rg_rows;
  if (r.rg_rows && H->ngroups && r.row_nn) {
    ORCG_ALLOC(int64_t, cnt, H->ngroups);
    ORCG_ALLOC(int64_t, pre, H->ngroups + 1);
    if ((rc = launch_rg_prefix(act.ctx, r.row_nn, n, r.rg_rows, H->ngroups, cnt, pre))) return fail_ctx(rc);
    dense_rows = pre;
  }
  std::vector<int64_t*> scans(nch, nullptr);
  std::vector<CountSrc> rb;  // per child its row count, then the first bad tag
  for (uint32_t kk = 0; kk < nch; ++kk) {
    ORCG_ALLOC_TO(int64_t, scans[kk], nonnull + 1);
    if ((rc = launch_union_flags(act.ctx, dtags, nonnull, kk, flags)) ||
        (rc = launch_exclusive_scan(act.ctx, flags, nonnull, scans[kk])) ||
        (rc = launch_union_offsets(act.ctx, dtags, nonnull, kk, scans[kk], doffs)))
      return fail_ctx(rc);
    rb.push_back(CountSrc{act.ctx, scans[kk] + nonnull});
  }
  rb.push_back(CountSrc{act.ctx, bad});
  std::vector<uint64_t> counts(nch + 1, 0);
  if ((rc = read_back(rb, counts.data()))) return rc;
  const uint64_t first_bad = counts[nch];
  if (first_bad != ~0ull)
    return fail(ORCG_PARSE_ERROR, "Invalid union tag " + std::to_string(first_bad & 0xff) + " for union with " +
                                      std::to_string(nch) + " children");
  if ((rc = place(dtags, 1, r, &c.tags)) || (rc = place(doffs, 8, r, &c.offsets))) return rc;
  for (uint32_t kk = 0; kk < nch; ++kk) {
    int64_t* child_rows = nullptr;
    if (dense_rows && H->ngroups) {
      ORCG_ALLOC_TO(int64_t, child_rows, H->ngroups);
      if ((rc = launch_rg_child_rows(act.ctx, scans[kk], dense_rows, H->ngroups, child_rows))) return fail_ctx(rc);
    }
    if ((rc = decode(subs[kk], counts[kk], nullptr, counts[kk], child_rows))) return rc;
  }
  return ORCG_OK;
}
