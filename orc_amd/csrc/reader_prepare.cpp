// Host half of a stripe read, no device work: the file tail, then per stripe
// prepare() and its phases.
#include "reader_internal.hh"

int orcg_reader::open_tail() {
  // ReaderImpl tail read (c++/src/Reader.cc:1650-1700, readPostscript :1548-1567)
  if (file_len < 4) return fail(ORCG_PARSE_ERROR, "File size too small");
  const uint64_t ps_len = file[file_len - 1];
  if (ps_len < 3) return fail(ORCG_PARSE_ERROR, "Invalid ORC postscript length");
  if (memcmp(file + file_len - 1 - 3, "ORC", 3) != 0 && memcmp(file, "ORC", 3) != 0)
    return fail(ORCG_PARSE_ERROR, "Not an ORC file");
  if (file_len < 1 + ps_len)
    return fail(ORCG_PARSE_ERROR, "Invalid ORC postscript length: " + std::to_string(ps_len) +
                                      ", file length = " + std::to_string(file_len));
  if (!parse_postscript(file + file_len - 1 - ps_len, ps_len, ps))
    return fail(ORCG_PARSE_ERROR, "Failed to parse the postscript");
  if (ps.block_size == 0) ps.block_size = 256 * 1024;
  decimal_as_long = ps.version.size() == 2 && ps.version[0] == 1 && ps.version[1] == 9999;
  // file_len >= 1 + ps_len here, so the subtraction cannot wrap
  if (ps.footer_length >= file_len - 1 - ps_len)
    return fail(ORCG_PARSE_ERROR, "Invalid tail size: footerSize=" + std::to_string(ps.footer_length) +
                                      ", postscriptLength=" + std::to_string(ps_len) +
                                      ", fileLength=" + std::to_string(file_len));
  if (ps.compression > kZstd) return fail(ORCG_PARSE_ERROR, "Unknown compression type");
  std::vector<uint8_t> fbytes;
  std::string err;
  const uint64_t tail = 1 + ps_len + ps.footer_length;
  if (!read_range(file, file_len - tail, ps.footer_length, ps.compression, ps.block_size, fbytes, err))
    return fail(ORCG_PARSE_ERROR, err);
  if (!parse_footer(fbytes.data(), fbytes.size(), footer)) return fail(ORCG_PARSE_ERROR, "Failed to parse the footer");
  // checkProtoTypes (Reader.cc:1575-1605)
  const size_t nt = footer.types.size();
  if (nt == 0) return fail(ORCG_PARSE_ERROR, "Footer is corrupt: no types found");
  for (size_t i = 0; i < nt; ++i) {
    const auto& t = footer.types[i];
    if (t.kind == ORCG_TYPE_STRUCT && t.subtypes.size() != t.field_names.size())
      return fail(ORCG_PARSE_ERROR, "Footer is corrupt: STRUCT type " + std::to_string(i) + " has " +
                                        std::to_string(t.subtypes.size()) + " subTypes, but has " +
                                        std::to_string(t.field_names.size()) + " fieldNames");
    for (size_t j = 0; j < t.subtypes.size(); ++j) {
      const uint32_t st = t.subtypes[j];
      if (st <= i)
        return fail(ORCG_PARSE_ERROR, "Footer is corrupt: malformed link from type " + std::to_string(i) +
                                          " to " + std::to_string(st));
      if (st >= nt) return fail(ORCG_PARSE_ERROR, "Footer is corrupt: types(" + std::to_string(st) + ") not exists");
      if (j > 0 && t.subtypes[j - 1] >= st)
        return fail(ORCG_PARSE_ERROR, "Footer is corrupt: subType(" + std::to_string(j - 1) + ") >= subType(" +
                                          std::to_string(j) + ") in types(" + std::to_string(i) + ")");
    }
  }
  own.selected.assign(nt, 1);
  return ORCG_OK;
}

// RLEv1 streams up to this size decode in 1 KB host-plan segments
constexpr uint64_t kV1SmallStream = 64u << 10;

// Whether an RLEv2 stream's first runs (up to 32) average >= 96 bytes: a
// stream of long DIRECT / PATCHED_BASE runs (header bytes only are read).
static bool long_runs(const uint8_t* p, uint64_t len) {
  uint64_t pos = 0, runs = 0;
  while (pos < len && runs < 32) {
    uint64_t L = 0, end = 0;
    if (host_parse_run(p, len, pos, &L, &end) != kErrNone) return false;
    pos = end;
    ++runs;
  }
  return runs > 0 && pos >= 96 * runs;
}

const ZoneEntry* orcg_reader::utc_zone_entry() const {
  if (!utc_entry) {
    utc_entry.reset(new ZoneEntry());
    utc_entry->zone = tz::Zone::utc("GMT");
  }
  return utc_entry.get();
}

// registered rules, then the built-in UTC names, then the zone directory
const ZoneEntry* orcg_reader::resolve_zone(const std::string& name) const {
  const std::string canon = tz::canonical_name(name);
  std::lock_guard<std::mutex> lk(tz_mu);
  auto it = zones.find(canon);
  if (it != zones.end()) return it->second.get();
  if (tz::is_utc_name(canon)) return utc_zone_entry();
  std::unique_ptr<ZoneEntry> e(new ZoneEntry());
  try {
    if (!tz::load_zone_file(canon, &e->zone)) return nullptr;  // looked up again by the next read
  } catch (const tz::TimezoneError& x) {
    e->err = x.what();
  }
  return (zones[canon] = std::move(e)).get();
}

// Phase 1: the stripe footer (Reader.cc getStripeFooter :620-640), the stripe's
// writer zone, its columns, and the streams to read with their compression
// chunks (StripeStream.cc:82-125)
int orcg_reader::locate_streams(uint64_t s, HostStage& hs, const std::vector<uint8_t>& selected,
                                const std::string& local_zone, StripeFooter& sf, std::vector<int>& row_index,
                                std::vector<Need>& needs) const {
  const StripeInfo& si = footer.stripes[s];
  std::string err;
  std::vector<uint8_t> fb;
  // stripe = [offset, + index, + data, + footer), every sum checked
  // (RowReaderImpl::startNextStripe, Reader.cc:1257-1268)
  uint64_t foff = 0, total = 0;
  if (__builtin_add_overflow(si.offset, si.index_length, &foff) ||
      __builtin_add_overflow(foff, si.data_length, &foff) ||
      __builtin_add_overflow(foff, si.footer_length, &total) || total >= file_len)
    return hs.fail(ORCG_PARSE_ERROR, "Malformed StripeInformation at stripe index " + std::to_string(s) +
                                         ": fileLength=" + std::to_string(file_len) + ", StripeInfo=(offset=" +
                                         std::to_string(si.offset) + ", indexLength=" +
                                         std::to_string(si.index_length) + ", dataLength=" +
                                         std::to_string(si.data_length) + ", footerLength=" +
                                         std::to_string(si.footer_length) + ")");
  if (!read_range(file, foff, si.footer_length, ps.compression, ps.block_size, fb, err))
    return hs.fail(ORCG_PARSE_ERROR, err);
  if (!parse_stripe_footer(fb.data(), fb.size(), si.offset, sf))
    return hs.fail(ORCG_PARSE_ERROR, std::string("bad StripeFooter from ") + compression_name(ps.compression));
  // Reader.cc:634-640
  const size_t nt = footer.types.size();
  if (sf.encodings.size() != nt)
    return hs.fail(ORCG_PARSE_ERROR, "bad number of ColumnEncodings in StripeFooter: expected=" +
                                         std::to_string(nt) + ", actual=" + std::to_string(sf.encodings.size()));
  hs.cols = std::vector<Col>(nt);
  hs.slack = upload_tail_bytes(nt, 0, (si.num_rows + 2047) / 2048 + 1);
  // The stripe's writer zone (StripeFooter.writerTimezone; the reference
  // assumes the machine's /etc/localtime for a stripe that names none, here
  // the caller names it or the column stays undecoded), resolved only when a
  // TIMESTAMP column is read. Not found: undecoded, nothing raised (the
  // reference throws); found but malformed: the TimezoneError.
  hs.writer_zone = nullptr;
  for (size_t i = 0; i < nt && !hs.writer_zone; ++i) {
    if (footer.types[i].kind != ORCG_TYPE_TIMESTAMP || !selected[i]) continue;
    const std::string& zn = sf.writer_timezone.empty() ? local_zone : sf.writer_timezone;
    if (zn.empty()) break;
    hs.writer_zone = resolve_zone(zn);
    if (!hs.writer_zone) break;
    if (!hs.writer_zone->zone) return hs.fail(ORCG_PARSE_ERROR, hs.writer_zone->err);
  }
  for (size_t i = 0; i < nt; ++i) {
    hs.cols[i].kind = footer.types[i].kind;
    hs.cols[i].encoding = sf.encodings[i].kind;
    hs.cols[i].dict_size = sf.encodings[i].dictionary_size;
    hs.cols[i].supported = is_supported(footer.types[i], hs.writer_zone);
  }
  row_index.assign(nt, -1);  // ROW_INDEX stream of each column (index into sf.streams)
  const uint64_t data_end = foff;  // <= file_len (checked above)
  for (size_t i = 0; i < sf.streams.size(); ++i) {
    const StreamInfo& st = sf.streams[i];
    const bool in_stripe = st.offset >= si.offset && range_ok(st.offset, st.length, data_end);
    if (st.kind == kRowIndex && st.column < nt && selected[st.column] && hs.cols[st.column].supported && in_stripe)
      row_index[st.column] = (int)i;
    const int slot = slot_of(st.kind);
    if (slot < 0 || st.column >= nt) continue;
    if (!selected[st.column] || !hs.cols[st.column].supported) continue;
    if (!in_stripe)
      return hs.fail(ORCG_PARSE_ERROR, "Malformed stream meta at stream index " + std::to_string(i) + " in stripe " +
                                           std::to_string(s));
    Need nd{st.column, slot, {}, st.offset};
    if (!split_chunks(file, st.offset, st.length, ps.compression, nd.chunks, err)) {
      if (hs.cols[st.column].stream_err.empty()) hs.cols[st.column].stream_err = err;
      continue;
    }
    needs.push_back(std::move(nd));
  }
  return ORCG_OK;
}

// Phase 2: page the streams in, inflate their chunks into staging (in
// parallel), compact them. *t_inflate: when the decompression started; *used:
// staging bytes filled.
int orcg_reader::load_streams(HostStage& hs, std::vector<Need>& needs, double* t_inflate, uint64_t* used) const {
  // I/O (ReaderMetrics::IOCount / IOBlockingLatencyUs): the reference preads
  // each stream (SeekableFileInputStream); this reader maps the file, so its
  // blocking I/O is the page-in of the streams' byte ranges: one touch per
  // page, timed (page-cache hits cost ~nothing, cold pages their read)
  {
    const double ti = now_s();
    uint64_t sink = 0;
    for (const Need& nd : needs)
      for (const Chunk& ch : nd.chunks) {
        const uint8_t* b = file + ch.src_off;
        for (uint64_t o = 0; o < ch.src_len; o += 4096) sink += ((const volatile uint8_t*)b)[o];
      }
    hs.io_sink = sink;
    hs.t_io = now_s() - ti;
    hs.n_io = needs.size() + 1;  // + the stripe footer
  }
  // staging: every chunk the host inflates gets a slot of its maximum size,
  // compacted after; a device-inflated stream's chunks are copied compressed
  // behind the compacted streams, with room for the stripe's chunk table
  uint64_t at = 0, comp_bytes = 0, dev_chunks = 0;
  std::vector<std::pair<size_t, size_t>> all;
  for (size_t i = 0; i < needs.size(); ++i) {
    if (!needs[i].device) at = (at + 255) & ~(uint64_t)255;
    for (size_t j = 0; j < needs[i].chunks.size(); ++j) {
      Chunk& ch = needs[i].chunks[j];
      if (needs[i].device) {
        comp_bytes += ch.src_len;
        ++dev_chunks;
      } else {
        ch.dst_off = at;
        at += ch.original ? ch.src_len : ps.block_size;
      }
      all.emplace_back(i, j);
    }
    if (needs[i].device) comp_bytes = (comp_bytes + 255) & ~(uint64_t)255;
  }
  const uint64_t table_bytes = (dev_chunks * sizeof(orcg_snappy_chunk) + 255) & ~(uint64_t)255;
  if (!hs.ensure(at + 256 + comp_bytes + table_bytes + 64, 0))
    return hs.fail(ORCG_OUT_OF_MEMORY, "pinned staging allocation failed");
  *t_inflate = now_s();
  std::vector<std::string> errs(all.size());
  std::atomic<bool> bad{false};
  uint64_t src_bytes = 0;
  for (auto& nd : needs)
    for (auto& ch : nd.chunks) src_bytes += ch.src_len;
  // ~64 KB of compressed input per thread (stored chunks are copies: more)
  parallel_for(all.size(), [&](size_t q) {
    const Need& nd = needs[all[q].first];
    Chunk& ch = needs[all[q].first].chunks[all[q].second];
    if (nd.device) {
      // the chunk's length without inflating it: Snappy's preamble alone,
      // LZ4's size walk (every check of the block runs here)
      const PlanChunk pc{ch.src_off, ch.src_len, ch.original};
      std::vector<orcg_snappy_chunk> one;
      const char* e = "";
      if (!(ps.compression == kLz4 ? plan_lz4_chunks : plan_snappy_chunks)(file, file_len, &pc, 1, ps.block_size, 0,
                                                                           one, &ch.dst_len, &e)) {
        errs[q] = e;
        bad = true;
      }
      return;
    }
    const uint64_t cap = ch.original ? ch.src_len : ps.block_size;
    if (!decompress_chunk(ps.compression, file, ch, hs.h + ch.dst_off, cap, errs[q])) bad = true;
  }, src_bytes, ps.compression == kNone ? (1u << 20) : (64u << 10));
  if (bad)
    for (auto& e : errs)
      if (!e.empty()) return hs.fail(ORCG_PARSE_ERROR, e);
  uint64_t w = 0;  // compact (destinations never pass their sources)
  for (size_t i = 0; i < needs.size(); ++i) {
    if (needs[i].device) continue;
    w = (w + 255) & ~(uint64_t)255;
    const uint64_t s0 = w;
    for (auto& ch : needs[i].chunks) {
      if (ch.dst_off != w) memmove(hs.h + w, hs.h + ch.dst_off, ch.dst_len);
      w += ch.dst_len;
    }
    StreamBuf& sb = hs.cols[needs[i].col].s[needs[i].slot];
    sb.present = true;
    sb.host_off = s0;
    sb.len = w - s0;
  }
  // the device-inflated streams: compressed chunks into staging, their
  // decompressed bytes laid out in the tail (offsets relative to it until
  // prepare() places the tail)
  uint64_t tail = 0;
  for (size_t i = 0; i < needs.size(); ++i) {
    if (!needs[i].device) continue;
    w = (w + 255) & ~(uint64_t)255;
    tail = (tail + 255) & ~(uint64_t)255;
    StreamBuf& sb = hs.cols[needs[i].col].s[needs[i].slot];
    sb.present = true;
    sb.device_only = true;
    sb.host_off = tail;
    for (auto& ch : needs[i].chunks) {
      if (ch.src_len) memcpy(hs.h + w, file + ch.src_off, ch.src_len);
      hs.inflate.push_back({w, ch.src_len, tail, ch.dst_len, ch.original ? (uint64_t)ORCG_SNAPPY_STORED : 0});
      w += ch.src_len;
      tail += ch.dst_len;
    }
    sb.len = tail - sb.host_off;
  }
  if (!hs.inflate.empty()) {
    w = (w + 255) & ~(uint64_t)255;
    hs.inflate_off = w;
    w += hs.inflate.size() * sizeof(orcg_snappy_chunk);
    hs.tail_bytes = tail;
  }
  hs.n_chunks = all.size();
  *used = w;
  return ORCG_OK;
}

// One column's row-index positions mapped to offsets in its decompressed
// streams, in the order of the column's layout (reader_layout.hh). False:
// the column keeps host plans.
bool orcg_reader::column_positions(size_t col, Col& c, const StreamInfo& ri, uint64_t G, const std::vector<int>& need_of,
                                   const std::vector<Need>& needs) const {
  const bool compressed = ps.compression != kNone;
  std::vector<StreamDesc> order;
  for (const StreamDesc& d : layout((uint32_t)col, c))
    if (d.positioned()) order.push_back(d);
  bool ok = !order.empty();
  for (auto& o : order) ok = ok && c.s[o.slot].present && need_of[col * kNumSlots + o.slot] >= 0;
  if (!ok) return false;
  std::vector<uint8_t> ib;
  std::vector<std::vector<uint64_t>> entries;
  std::string e2;
  if (!read_range(file, ri.offset, ri.length, ps.compression, ps.block_size, ib, e2) ||
      !parse_row_index(ib.data(), ib.size(), entries) || entries.size() != G)
    return false;
  // per stream: chunk header offsets (in the stream) -> decompressed starts
  std::vector<std::vector<std::pair<uint64_t, uint64_t>>> cmap(order.size());
  for (size_t o = 0; o < order.size(); ++o) {
    const Need& nd = needs[need_of[col * kNumSlots + order[o].slot]];
    uint64_t d = 0;
    for (const Chunk& ch : nd.chunks) {
      const uint64_t hdr = compressed ? ch.src_off - 3 - nd.file_off : ch.src_off - nd.file_off;
      cmap[o].push_back({hdr, d});
      d += ch.dst_len;
    }
    cmap[o].push_back({nd.file_off + 0, d});  // sentinel: the stream's end
    cmap[o].back().first = ~0ull;
  }
  std::vector<std::vector<int64_t>> trips(order.size());
  for (uint64_t g = 0; g < G && ok; ++g) {
    const std::vector<uint64_t>& pv = entries[g];
    size_t at = 0;
    for (size_t o = 0; o < order.size() && ok; ++o) {
      const size_t need_n = (compressed ? 2 : 1) + order[o].position_extras();
      if (at + need_n > pv.size()) {
        ok = false;
        break;
      }
      uint64_t off;
      const StreamBuf& sb = c.s[order[o].slot];
      if (compressed) {
        const uint64_t chunk = pv[at], in = pv[at + 1];
        auto& m = cmap[o];
        auto it = std::lower_bound(m.begin(), m.end() - 1, std::make_pair(chunk, (uint64_t)0));
        if (it != m.end() - 1 && it->first == chunk) off = it->second + in;
        else if (it == m.end() - 1) off = m.back().second + in;  // position at the stream's end
        else {
          ok = false;
          break;
        }
        at += 2;
      } else {
        off = pv[at++];
      }
      if (off > sb.len) {
        ok = false;
        break;
      }
      if (order[o].position_extras()) {
        const int64_t skip = (int64_t)pv[at++];
        const int64_t bits = order[o].position_extras() == 2 ? (int64_t)pv[at++] : 0;
        auto& t = trips[o];
        if (!t.empty() && (uint64_t)t[t.size() - 3] > off) ok = false;
        t.push_back((int64_t)off);
        t.push_back(skip);
        t.push_back(bits);
      }
    }
  }
  if (!ok) return false;
  for (size_t o = 0; o < order.size(); ++o) {
    if (!order[o].position_extras()) continue;
    StreamBuf& sb = c.s[order[o].slot];
    sb.pos = true;
    sb.trip = std::move(trips[o]);
  }
  return true;
}

// Phase 3, row-index segmentation: the positions every row group records for
// each of the column's streams (ColumnReader::seekToRowGroup order,
// ColumnReader.cc; the writers' recordPosition order, ColumnWriter.cc) give
// run-aligned cut points, so those streams need no host header walk.
void orcg_reader::map_row_index(uint64_t s, const StripeFooter& sf, const std::vector<int>& row_index,
                                const std::vector<Need>& needs, HostStage& hs) const {
  const StripeInfo& si = footer.stripes[s];
  const size_t nt = footer.types.size();
  hs.ngroups = 0;
  // ORCG_NO_ROW_INDEX=1 forces the host plans (A/B and tests)
  const char* no_ri = getenv("ORCG_NO_ROW_INDEX");
  if (footer.row_index_stride == 0 || si.num_rows == 0 || (no_ri && no_ri[0] == '1')) return;
  const uint64_t G = (si.num_rows + footer.row_index_stride - 1) / footer.row_index_stride;
  std::vector<int> need_of(nt * kNumSlots, -1);
  for (size_t i = 0; i < needs.size(); ++i) need_of[needs[i].col * kNumSlots + needs[i].slot] = (int)i;
  // one column per task: decompress + parse its ROW_INDEX, map positions
  std::atomic<bool> any{false};
  uint64_t ri_bytes = 0;
  for (size_t col = 0; col < nt; ++col)
    if (row_index[col] >= 0) ri_bytes += sf.streams[row_index[col]].length;
  parallel_for(nt, [&](size_t col) {
    if (row_index[col] < 0) return;
    if (column_positions(col, hs.cols[col], sf.streams[row_index[col]], G, need_of, needs)) any = true;
  }, ri_bytes, 16u << 10);  // row indexes: ~16 KB of (compressed) entries per thread
  if (any) hs.ngroups = G;
}

// Phase 4: which RLE streams keep their row-index cuts and which get a host
// run plan, of which kind; then the plans, in parallel (header walks only).
void orcg_reader::build_plans(const std::vector<uint8_t>& selected, HostStage& hs, std::vector<StreamBuf*>& rle) const {
  const size_t nt = footer.types.size();
  // columns whose value streams decode in a launch of their own, never in the
  // stripe's multi-stream batch (collect() stops at a PRESENT stream and at a
  // list's or map's children): a column with nulls, or one below a list, a
  // map or a column with nulls (configs[4]'s map keys)
  std::vector<uint8_t> alone(nt, 0);
  for (size_t i = 0; i < nt; ++i) {
    const Col& c = hs.cols[i];
    const bool down = alone[i] || c.s[kSlotPresent].present || c.kind == ORCG_TYPE_LIST || c.kind == ORCG_TYPE_MAP;
    if (c.s[kSlotPresent].present) alone[i] = 1;
    if (down)
      for (uint32_t st : footer.types[i].subtypes)
        if (st < nt && st > i) alone[st] = 1;  // (pre-order ids: children after parents)
  }
  std::vector<int> rle_kind;  // 0 byte RLE, 1 RLEv1, 2 RLEv2, 3 RLEv2 in fine segments
  for (size_t i = 0; i < nt; ++i) {
    Col& c = hs.cols[i];
    if (!selected[i] || !c.supported) continue;
    const StreamLayout lay = layout((uint32_t)i, c);
    for (int sl : {kSlotPresent, kSlotData, kSlotLength, kSlotSecondary}) {
      StreamBuf& sb = c.s[sl];
      if (!sb.present) continue;
      const StreamDesc* d = lay.find(sl);
      if (!d || d->coding == kRaw || d->coding == kVarint) continue;  // raw bytes / varints, or not the kind's stream
      const int kind = d->coding != kIntRle ? 0 : rle_v1(c.encoding, d->force_v2) ? 1 : 2;
      // cut by the row index, unless a byte-RLE stream's row groups are too
      // coarse to fill the GPU: a child column's row groups hold several
      // rows per parent row (C5's list items: ~40k PRESENT bits, 5 KB per
      // row group), one workgroup each while most of the GPU idles; such a
      // stream gets a host plan with 1 KB segments, as streams without a row
      // index do (its walk hops ~129 bytes at a time, in address order: cheap
      // on the host). Integer streams keep the row index: their host walk
      // chases run headers ~2 KB apart through memory (~45 ns a run, 0.9 ms
      // for a 42 MB stream), which lands on the host-bound critical path
      //
      // An RLEv2 stream of long runs (its first runs average >= 96 bytes:
      // DIRECT / PATCHED_BASE runs of hundreds of values) in a launch of its
      // own (`alone`: a nullable column, or one below a list, a map or a
      // nullable column) gets a host plan with 8 KB segments too: a child
      // column's row group holds ~40,000 values in several serial window
      // passes of one workgroup (C5's list items, map keys and map values:
      // 260 workgroups per stream; the keys' launch took 135 us a stripe),
      // while the host walk costs ~45 ns a run, a few thousand runs a
      // stripe. Batched columns keep the row index: their streams
      // share one multi-stream launch with the short-run streams, whose
      // latency sets its length, and the extra host walk lands on the
      // host-bound wall (C4: device 3.46 -> 3.64 ms, host plans 3.4 -> 7.8 ms
      // with fine plans on every long-run stream).
      bool fine = false;
      if (sb.pos) {
        const uint64_t per_group = hs.ngroups ? sb.len / hs.ngroups : 0;
        if (kind == 1 && sb.len <= kV1SmallStream) {
          // a small RLEv1 stream (configs[0]: 5,000-row stripes, <= 5 KB
          // streams, one row group): 1 KB host-plan segments instead of one
          // row-group segment, so the stream's windows decode side by side
          // (rlev1_kernel's narrow instance) -- the host walk is ~1 ns a byte
        } else if (kind == 0) {
          if (per_group <= (2u << 10)) continue;
        } else if (kind == 2 && alone[i] && per_group > (8u << 10) && long_runs(hs.h + sb.host_off, sb.len)) {
          fine = true;
        } else {
          continue;
        }
        sb.pos = false;
        sb.trip.clear();
      }
      rle.push_back(&sb);
      rle_kind.push_back(fine ? 3 : kind);
    }
  }
  uint64_t plan_bytes = 0;
  for (auto* sb : rle) plan_bytes += sb->len;
  parallel_for(rle.size(), [&](size_t q) {
    StreamBuf& sb = *rle[q];
    const uint8_t* p = hs.h + sb.host_off;
    // byte / boolean RLE without row-index segments: 4 KB segments, one
    // byterle_kernel window each (C5's child PRESENT streams: 45.7 -> 32.8 us
    // a launch against 1 KB segments, whose workgroups each paid the
    // window's fixed phase latencies for a quarter of the bytes)
    constexpr uint32_t byte_seg = 4u << 10;
    if (rle_kind[q] == 0) sb.plan.reset(make_byte_plan(p, sb.len, byte_seg, byte_seg));
    else if (rle_kind[q] == 1)
      sb.plan.reset(make_v1_plan(p, sb.len, sb.len <= kV1SmallStream ? (1u << 10) : (16u << 10), 8192));
    else if (rle_kind[q] == 3) sb.plan.reset(make_plan(p, sb.len, 8u << 10, 4096));
    else sb.plan.reset(make_plan(p, sb.len, 16u << 10, 8192));
  }, plan_bytes, 512u << 10);  // header walks: ~512 KB of stream per thread
  hs.n_plan = rle.size();
}

// Phase 5: the plans' segment tables, the row-group start rows and the
// row-index triplets appended to staging (w: bytes used so far)
int orcg_reader::layout_staging(uint64_t s, HostStage& hs, const std::vector<StreamBuf*>& rle, uint64_t w) const {
  const StripeInfo& si = footer.stripes[s];
  const size_t nt = footer.types.size();
  hs.n_pos = 0;
  for (auto& c : hs.cols)
    for (auto& sb : c.s) hs.n_pos += sb.pos ? 1 : 0;
  hs.slack = upload_tail_bytes(nt, v1_segments(hs), (si.num_rows + 2047) / 2048 + 1);
  uint64_t seg_bytes = 0;
  for (auto* sb : rle) seg_bytes += ((sb->plan->segs.size() * sizeof(orcg_segment)) + 255) & ~(uint64_t)255;
  w = (w + 255) & ~(uint64_t)255;
  if (!hs.ensure(w + seg_bytes + 64, w)) return hs.fail(ORCG_OUT_OF_MEMORY, "pinned staging allocation failed");
  for (auto* sb : rle) {
    sb->seg_off = w;
    const size_t nb = sb->plan->segs.size() * sizeof(orcg_segment);
    if (nb) memcpy(hs.h + w, sb->plan->segs.data(), nb);
    w = (w + nb + 255) & ~(uint64_t)255;
  }
  // row-index triplets and the row-group start rows
  uint64_t rg_bytes = hs.ngroups ? ((hs.ngroups * 8 + 255) & ~(uint64_t)255) : 0;
  for (auto& c : hs.cols)
    for (auto& sb : c.s)
      if (sb.pos) rg_bytes += ((sb.trip.size() * 8) + 255) & ~(uint64_t)255;
  if (rg_bytes) {
    if (!hs.ensure(w + rg_bytes + 64, w)) return hs.fail(ORCG_OUT_OF_MEMORY, "pinned staging allocation failed");
    hs.rows_off = w;
    for (uint64_t g = 0; g < hs.ngroups; ++g) ((int64_t*)(hs.h + w))[g] = (int64_t)(g * footer.row_index_stride);
    w = (w + hs.ngroups * 8 + 255) & ~(uint64_t)255;
    for (auto& c : hs.cols)
      for (auto& sb : c.s)
        if (sb.pos) {
          sb.rg_off = w;
          memcpy(hs.h + w, sb.trip.data(), sb.trip.size() * 8);
          w = (w + sb.trip.size() * 8 + 255) & ~(uint64_t)255;
        }
  }
  hs.used = w;
  return ORCG_OK;
}

// Host half of a stripe read (thread-safe w.r.t. the device half of another
// stripe): stripe footer (Reader.cc getStripeFooter :620-640), stream
// location (StripeStream.cc:82-125), decompression of every selected stream
// (Compression.cc) in parallel chunks, run plans + segment tables.
// (Small streams on host plans instead of row-index segment tables were
// measured in round 4, profiles/r04/*small_stream_ab*: no gain, dropped.)
bool orcg_reader::host_never_walks(const HostStage& hs, uint32_t col, int slot) const {
  if (slot == kSlotDict) return true;
  if (slot != kSlotData) return false;
  const StreamLayout lay = stream_layout(footer.types[col], hs.cols[col].encoding, decimal_as_long, false);
  const StreamDesc* d = lay.find(slot);
  return d && (d->coding == kRaw || d->coding == kVarint);
}

int orcg_reader::prepare(uint64_t s, HostStage& hs, const ReadOptions& o) const {
  hs.stripe = s;
  hs.inflate.clear();
  hs.inflate_off = hs.tail_off = hs.tail_bytes = 0;
  hs.rc = ORCG_OK;
  hs.err.clear();
  const double t0 = now_s();
  StripeFooter sf;
  std::vector<int> row_index;
  std::vector<Need> needs;
  int rc = locate_streams(s, hs, o.selected, o.local_tz, sf, row_index, needs);
  if (rc) return rc;
  // Snappy and LZ4 chunks of the streams the host never walks inflate on the
  // device (a block size past the kernel's 32-bit offsets keeps the host path)
  if (o.dev_inflate && (ps.compression == kSnappy || ps.compression == kLz4) && ps.block_size < kSnappyMaxBytes)
    for (Need& nd : needs) nd.device = host_never_walks(hs, nd.col, nd.slot);
  double t1 = 0;
  uint64_t w = 0;
  if ((rc = load_streams(hs, needs, &t1, &w))) return rc;
  const double t15 = now_s();
  map_row_index(s, sf, row_index, needs, hs);
  std::vector<StreamBuf*> rle;
  build_plans(o.selected, hs, rle);
  if ((rc = layout_staging(s, hs, rle, w))) return rc;
  if (!hs.inflate.empty()) {
    // the tail: past everything issue() uploads (used + slack bounds it)
    hs.tail_off = (hs.used + hs.slack + 255) & ~(uint64_t)255;
    for (Col& c : hs.cols)
      for (StreamBuf& sb : c.s)
        if (sb.device_only) sb.host_off += hs.tail_off;
    for (orcg_snappy_chunk& k : hs.inflate) k.dst_offset += hs.tail_off;
    memcpy(hs.h + hs.inflate_off, hs.inflate.data(), hs.inflate.size() * sizeof(orcg_snappy_chunk));
  }
  const double t2 = now_s();
  hs.t_parse = t1 - t0;
  hs.t_decomp = t15 - t1;
  hs.t_plan = t2 - t15;
  return ORCG_OK;
}
