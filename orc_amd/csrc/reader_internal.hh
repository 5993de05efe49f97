// File-level reader (include/orcg_reader.h): ORC tail -> stripe streams ->
// host decompression -> one H2D per stripe -> HIP decode of every selected
// column into device batches.
//
// Column semantics follow the reference's column readers
// (c++/src/ColumnReader.cc): ColumnReader::next's PRESENT handling with the
// parent's incoming mask (:81-104; a child's PRESENT stream has bits only for
// the parent's non-null rows), IntegerColumnReader (:225-258),
// BooleanColumnReader (:131-186), ByteColumnReader (:188-223),
// DoubleColumnReader (:359-450), StringDictionaryColumnReader (:509-607),
// StringDirectColumnReader (:615-793), StructColumnReader (:795-880),
// ListColumnReader / MapColumnReader (:882-1157). Encodings pick RLE v1 or v2
// (createRleDecoder, c++/src/RLE.cc:48-60 via ColumnReader.cc
// convertRleVersion).
//
// Internal to the reader's translation units: its shared structs, in
// orcg::reader (orcg_reader itself is the C API's opaque type and stays
// global). reader_layout.hh says which streams each column kind reads.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>

#include "../../include/orcg_reader.h"
#include "orc_file.hh"
#include "orcg_internal.hh"
#include "inflate_plan.hh"
#include "read_type.hh"
#include "reader_layout.hh"
#include "timezone.hh"

namespace orcg {
namespace reader {

using namespace orcg::file;

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline unsigned host_threads() {
  if (const char* e = getenv("ORCG_HOST_THREADS")) {
    const int v = atoi(e);
    if (v > 0) return (unsigned)v;
  }
  const unsigned hc = std::thread::hardware_concurrency();
  return std::max(1u, std::min(16u, hc ? hc : 1u));
}

// work_bytes / bytes_per_thread caps the thread count: a thread costs tens
// of microseconds to start and join, so a small stripe's few KB of streams
// (configs[0]'s 5,000-row stripes: ~1 KB compressed each) run on the calling
// thread instead of paying for 16 threads three times per stripe.
template <typename F>
void parallel_for(size_t n, F&& f, uint64_t work_bytes = ~0ull, uint64_t bytes_per_thread = 1) {
  const uint64_t by_work = std::max<uint64_t>(1, work_bytes / std::max<uint64_t>(1, bytes_per_thread));
  const unsigned nt = (unsigned)std::min<uint64_t>(std::min<size_t>(host_threads(), n), by_work);
  if (nt <= 1) {
    for (size_t i = 0; i < n; ++i) f(i);
    return;
  }
  std::atomic<size_t> next{0};
  std::vector<std::thread> ts;
  for (unsigned t = 0; t < nt; ++t)
    ts.emplace_back([&] {
      for (size_t i; (i = next.fetch_add(1)) < n;) f(i);
    });
  for (auto& t : ts) t.join();
}

// Zones whose rules are UTC (tz::is_utc_name): TIMESTAMP columns written in
// them decode with no adjustment against the default reader zone, GMT
// (ColumnReader.cc:333-345 is a no-op; epoch 2015-01-01 00:00:00 UTC =
// 1420070400), and no zone file is read for them. Every other zone resolves,
// per stripe, through the rules registered on the reader
// (orcg_reader_set_zone_rules), then the IANA directory (tz::load_zone_file);
// writer and reader zone then differ and the values are adjusted on the
// device (timestamp_tz_kernel).
constexpr int64_t kOrcEpochUtc = tz::kOrcEpochUtc;

// A zone a reader resolved: its rules (or, for a zone file that was found but
// is malformed, the TimezoneError text) and, after the first decode that
// needs it, its flat table in device memory (the reader's own allocation,
// uploaded once).
struct ZoneEntry {
  std::unique_ptr<tz::Zone> zone;
  std::string err;
  int64_t* d_tab = nullptr;
  uint32_t words = 0;
  ~ZoneEntry() {
    if (d_tab) (void)hipFree(d_tab);
  }
};

// [off, off + len) lies inside [0, end), written so that no sum can wrap
// (offsets and lengths come from the file and are untrusted)
inline bool range_ok(uint64_t off, uint64_t len, uint64_t end) { return off <= end && len <= end - off; }

// Columns this reader decodes: every primitive, list / map / struct / union,
// decimals (Hive 0.11 precision-0 decimals at the forced scale), timestamps
// whose stripe's writer zone resolved (writer_zone; NULL: the zone's rules
// were not found, or the stripe names no zone and the caller named none with
// orcg_reader_set_local_timezone, and the column stays undecoded).
inline bool is_supported(const file::TypeInfo& t, const ZoneEntry* writer_zone) {
  const uint32_t k = t.kind;
  if (k == ORCG_TYPE_UNION) return true;
  if (k == ORCG_TYPE_DECIMAL) return true;
  if (k == ORCG_TYPE_TIMESTAMP) return writer_zone != nullptr;
  if (k == ORCG_TYPE_TIMESTAMP_INSTANT) return true;
  return k <= ORCG_TYPE_CHAR || k == ORCG_TYPE_DATE || k == ORCG_TYPE_VARCHAR;
}

// Device arena of a decoded stripe: allocations bump through one hipMalloc'd
// chunk and are all released together when the slot decodes its next stripe,
// so a stripe's buffers are contiguous (the row reader copies them to the
// host in a few large D2H copies). A stripe that outgrows the chunk takes a
// new one; the next stripe then starts from one chunk of the combined size.
struct DevPool {
  int device = 0;
  std::vector<std::pair<uint8_t*, size_t>> chunks;  // the last is the active one
  size_t off = 0;                                   // bump offset in the active chunk
  size_t want = 0;                                  // bytes the last stripe used (all chunks)
  size_t used_now = 0;
  size_t hint = 0;                                  // the caller's estimate for a fresh slot
  ~DevPool() {
    for (auto& c : chunks) (void)hipFree(c.first);
  }
  void release_all() {
    if (chunks.size() > 1 || (!chunks.empty() && chunks.back().second < want)) {
      // consolidate: one chunk for the whole of the last stripe
      for (auto& c : chunks) (void)hipFree(c.first);
      chunks.clear();
    }
    want = std::max(want, used_now);
    off = 0;
    used_now = 0;
  }
  void* get(size_t bytes) {
    bytes = std::max<size_t>(256, (bytes + 255) & ~(size_t)255);
    used_now += bytes;
    if (chunks.empty() || off + bytes > chunks.back().second) {
      const size_t cap = std::max<size_t>({bytes + (bytes >> 2), want + (want >> 3), hint, size_t(1) << 20});
      uint8_t* p = nullptr;
      if (hipMalloc((void**)&p, cap) != hipSuccess) {
        (void)hipGetLastError();  // the failure must not stick to a later launch check
        if (hipMalloc((void**)&p, bytes) != hipSuccess) {
          (void)hipGetLastError();
          if (debug_on("alloc")) fprintf(stderr, "orcg: device allocation of %zu bytes failed\n", bytes);
          return nullptr;
        }
        chunks.push_back({p, bytes});
      } else {
        chunks.push_back({p, cap});
      }
      off = 0;
    }
    void* p = chunks.back().first + off;
    off += bytes;
    return p;
  }
};

struct StreamBuf {
  bool present = false;
  uint64_t host_off = 0;  // offset in staging (== device offset)
  uint64_t len = 0;       // decompressed bytes
  // inflated on the device (orcg_reader_set_device_decompression): host_off
  // lies in the stripe's device-only tail, past everything uploaded; staging
  // holds nothing there, so no host code may read hs.h + host_off
  bool device_only = false;
  std::unique_ptr<orcg_rlev2_plan> plan;
  uint64_t seg_off = 0;   // offset of the plan's segment table in staging
  // row-index segmentation: per row group {byte offset, values to skip, bits
  // to skip} (int64 x 3) in staging at rg_off; no host plan
  bool pos = false;
  std::vector<int64_t> trip;
  uint64_t rg_off = 0;
};

// A column's decoded buffers as the callers see them (device pointers in a
// DevSlot, host pointers in a row reader's slab)
struct ColView {
  bool decoded = false;
  uint32_t kind = 0, encoding = 0;
  uint64_t n = 0;
  bool has_nulls = false;
  const uint8_t* nn = nullptr;
  const void* data = nullptr;
  const int64_t* length = nullptr;
  const int64_t* offsets = nullptr;
  const uint8_t* blob = nullptr;
  uint64_t blob_len = 0;
  const int64_t* secondary = nullptr;     // TIMESTAMP nanoseconds
  const uint8_t* tags = nullptr;          // UNION: child of each row (UnionVectorBatch::tags)
  const int64_t* index = nullptr;         // dictionary strings: entry of each row (EncodedStringVectorBatch::index)
  const int64_t* dict_offsets = nullptr;  // dictionary strings: dict_size + 1 entry offsets (StringDictionary)
  uint64_t dict_size = 0;                 // ColumnEncoding.dictionarySize of this stripe
  // schema evolution: the column was converted to the read type's kind
  // (orcg_reader::convert_column); `kind` stays the file's
  bool converted = false;
  uint32_t rkind = 0, rprecision = 0, rscale = 0;
  // the kind, and for a decimal the precision, the batch layout follows
  uint32_t out_kind() const { return converted ? rkind : kind; }
  uint32_t out_precision(uint32_t file_precision) const { return converted ? rprecision : file_precision; }
};

// A read type set on a reader (RowReaderOptions::setReadType): its tree, the
// conversion of each node against the file type (read_type.hh), its text
struct ReadPlan {
  rt::Tree tree;
  std::vector<rt::Conv> conv;
  std::string text;
};

// What a read is asked for (RowReaderOptions, and this reader's own
// switches): the reader holds its own, changed by the setters; a row reader
// holds the snapshot of its creation, immutable from then on. The decode in
// progress works on a copy (orcg_reader::act, made by Active under the
// reader's mutex) rather than a pointer to the caller's: the copy is what a
// struct's fork points at a side lane (ctx) and where a reader zone left
// unset resolves to GMT, neither of which may touch the caller's options;
// it costs an assignment into members that keep their capacity.
struct ReadOptions {
  Ctx* ctx = nullptr;             // the context the decode launches on
  std::vector<uint8_t> selected;  // RowReaderOptions::include, per type id
  bool lazy_dict = false;         // dictionary strings stay encoded (index + dictionary)
  // Time zones: the reader's (RowReaderOptions::setTimezoneName; nullptr:
  // "GMT"), and the zone assumed for stripes that name none
  const ZoneEntry* reader_tz = nullptr;
  std::string local_tz;
  // Schema evolution (RowReaderOptions::setReadType /
  // throwOnSchemaEvolutionOverflow). A plan is immutable once set; row
  // readers share it.
  std::shared_ptr<const ReadPlan> read;
  bool evo_throw = false;
  // orcg_reader_set_device_decompression: Snappy and LZ4 chunks of raw byte streams
  // ride the upload compressed and inflate on the device
  bool dev_inflate = false;
};

// A column of a stripe being prepared and decoded: its streams, and the view
// the decode fills
struct Col : ColView {
  bool supported = false;  // decoded by this reader (is_supported for this stripe's writer zone)
  // a stream of this column whose compression chunks do not parse: raised
  // when the decode reaches the column, as the reference reads streams
  // column by column (an earlier column's error comes first)
  std::string stream_err;
  StreamBuf s[kNumSlots];  // PRESENT, DATA, LENGTH, DICTIONARY_DATA, SECONDARY
  // has_nulls is provisional until the stripe's checks run: the non-null
  // count stayed on the device (orcg_reader::device_counts)
  bool nulls_deferred = false;
};

// One stripe prepared on the host: stream bytes decompressed into pinned
// staging, run plans and their segment tables appended (no device work).
struct HostStage {
  uint64_t stripe = ~0ull;
  const ZoneEntry* writer_zone = nullptr;  // the stripe's resolved writer zone (TIMESTAMP columns)
  std::vector<Col> cols;  // streams (and, while decoding, the outputs)
  uint8_t* h = nullptr;   // pinned staging
  size_t cap = 0;
  uint64_t used = 0;
  int rc = ORCG_OK;
  std::string err;
  double t_parse = 0, t_decomp = 0, t_plan = 0;
  uint64_t ngroups = 0;    // row groups with row-index positions (0: host plans only)
  uint64_t n_pos = 0, n_plan = 0;  // RLE streams cut by the row index / by a host plan
  uint64_t n_chunks = 0;            // compression chunks inflated (ReaderMetrics::DecompressionCall)
  uint64_t n_io = 0;                // stream reads (ReaderMetrics::IOCount)
  double t_io = 0;                  // their blocking time: page-ins of the mapped stripe (IOBlockingLatencyUs)
  uint64_t io_sink = 0;
  uint64_t rows_off = 0;   // staging offset of int64 rows[g] = g * stride
  // room kept past the prepared bytes for the upload's tail (read-back block
  // and job arena, upload_tail_bytes): upload_and_decode never reallocates
  uint64_t slack = 0;
  // Snappy or LZ4 streams the device inflates: their chunk table (sources: the
  // compressed bytes in staging; destinations in the device-only tail
  // [tail_off, tail_off + tail_bytes) of the stripe's allocation, tail_off >=
  // used + slack), written to staging at inflate_off
  std::vector<orcg_snappy_chunk> inflate;
  uint64_t inflate_off = 0, tail_off = 0, tail_bytes = 0;
  ~HostStage() { pinned_free(h); }
  bool pinned_mapped = false;  // h is hipHostMalloc'd (the device can read it through the same pointer)
  bool ensure(uint64_t bytes, uint64_t keep) {
    if (bytes <= cap) return true;
    const uint64_t ncap = std::max<uint64_t>(bytes + (bytes >> 2), 1 << 20) + slack;
    uint8_t* nh = (uint8_t*)pinned_alloc(ncap);
    if (!nh) return false;
    if (h) {
      if (keep) memcpy(nh, h, keep);
      pinned_free(h);
    }
    h = nh;
    cap = ncap;
    pinned_mapped = ncap < (size_t(8) << 20);  // pinned_alloc's hipHostMalloc range
    return true;
  }
  int fail(int status, const std::string& m) {
    rc = status;
    err = m;
    return status;
  }
};

// The view a finished stripe keeps (ok: the stripe decoded without error)
struct ColOut : ColView {
  ColOut() = default;
  ColOut(const ColView& c, bool ok) : ColView(c) {
    decoded = c.decoded && ok;
    if (!dict_offsets) dict_size = 0;
  }
};

// One decoded stripe in HBM: its device allocations and column views.
struct DevSlot {
  uint64_t stripe = ~0ull;
  DevPool pool;
  uint8_t* d_stage = nullptr;
  // the read-back block, uploaded initialised with the stripe and copied
  // back once after the decode: per column its error record, its PRESENT
  // decode's non-null count, then the summary slots (rb_alloc)
  uint64_t* d_rb = nullptr;
  unsigned long long* d_errs = nullptr;  // device error record per column (the kernels' atomicMin word)
  uint64_t* d_ones = nullptr;            // per column: non-null rows its PRESENT decode wrote
  std::vector<ColOut> out;
  // the stripe's last row-level filter run (orcg_reader_filter_stripe): the
  // selection vector in this slot's arena; dropped with the arena
  const int64_t* f_selected = nullptr;
  uint64_t f_count = 0;
  bool f_valid = false;
};

// A timed pair of events around a stripe's integer-RLE (kind 0) or byte-RLE
// (kind 1) launches (ReaderMetrics with metrics timing)
struct EvPair {
  hipEvent_t a, b;
  int kind;
};

// What upload_and_decode appends to a stripe's staging for nc columns: the
// read-back block (error records, non-null counts, summary slots) and the
// job arena of the batched launches, each 256-byte aligned.
// (+ 1: the stripe's device inflate record)
inline uint64_t rb_words_for(size_t nc) { return 2 * nc + 1 + 4 * nc + 16 + 1; }
inline uint64_t arena_bytes_for(size_t nc, uint64_t v1_segs, uint64_t dict_tiles) {
  // (dictionary jobs: one copy per 2,048-row tile of a column)
  return 5 * (nc + 1) * sizeof(RleJob) + (nc + 1) * sizeof(DictJob) * dict_tiles + v1_segs * sizeof(V1SegDesc) +
         16 * 256;
}
inline uint64_t upload_tail_bytes(size_t nc, uint64_t v1_segs, uint64_t dict_tiles) {
  return 256 + 8 * rb_words_for(nc) + 256 + arena_bytes_for(nc, v1_segs, dict_tiles) + 64;
}
// RLEv1 segments of a prepared stripe (each a descriptor in the arena)
inline uint64_t v1_segments(const HostStage& hs) {
  uint64_t n = 0;
  for (const Col& c : hs.cols) {
    if (!rle_v1(c.encoding, false)) continue;
    for (const StreamBuf& sb : c.s)
      if (sb.present) n += sb.pos ? hs.ngroups : (sb.plan ? sb.plan->segs.size() : 0);
  }
  return n;
}

// A stripe's multi-stream batch: before decode(), the streams whose value
// counts and segments are known without device results (columns with no
// PRESENT stream, under parents with none), and what hangs off them, are
// queued here and decoded by one launch per kernel instance (run_multi);
// decode() then finds their outputs here. One per reader, reused by every
// stripe: a new table is added to reset() and nowhere else.
struct StripeBatch {
  std::vector<RleJob> rlev2;       // RLEv2 streams
  std::vector<V1SegDesc> v1_segs;  // RLEv1 streams' segments
  // batched integer streams by (column, slot): their values and count
  struct Values {
    int64_t* values;
    uint64_t count;
  };
  std::unordered_map<uint64_t, Values> batched;
  const Values* find(uint32_t id, int slot) const {
    const auto it = batched.find(key(id, slot));
    return it == batched.end() ? nullptr : &it->second;
  }
  void put(uint32_t id, int slot, int64_t* values, uint64_t count) { batched[key(id, slot)] = Values{values, count}; }
  // dictionary columns of the batch (no nulls, <= kDictLds entries): their
  // offsets and gathers in one launch after the streams (dict_multi_kernel)
  struct DictDone {
    int64_t* offsets;
    const uint64_t* h_summary;
    int64_t* start;
    int64_t* len;
    int64_t* idx;
  };
  std::vector<DictJob> dict_jobs;
  std::unordered_map<uint32_t, DictDone> dict_done;
  // dictionaries of columns the batch cannot take whole (nullable, under a
  // list / map): their entry offsets and summary only, from the same launch
  std::unordered_map<uint32_t, DictDone> dict_pre;
  // a batch of such dictionaries only runs on side lane 0 (issue()); the
  // gathers reading its offsets and the stripe's read-back wait on ev_pre
  hipEvent_t ev_pre = nullptr;
  bool pre_on_lane = false;
  // varint decimal DATA streams whose tile counts + scan run with the batch
  // (before its join): their tile bases and value-count slots by column.
  // (varint_jobs and scan_jobs are deques: `launches` points at their
  // elements, whose addresses a later push must not move)
  std::deque<VarintJob> varint_jobs;
  std::unordered_map<uint32_t, std::pair<int64_t*, const uint64_t*>> varint_pre;
  // varint decimal columns (no nulls, not Hive 0.11) decoded by one launch
  // per mode after the batch's join (varint_decimal_multi_kernel)
  std::vector<DecJob> dec_jobs[2];
  std::unordered_map<uint32_t, void*> dec_done;
  // direct string columns (no nulls) whose length scan runs after the
  // batch's join, beside the dictionaries and decimals
  struct ScanDone {
    int64_t* starts;
    const uint64_t* h_flags;
    const uint64_t* h_need;
    uint64_t n;
  };
  std::deque<ScanJob> scan_jobs;
  std::unordered_map<uint32_t, ScanDone> scan_done;
  std::vector<MultiLaunch> launches;

  // empties every table for the next stripe and keeps its capacity
  // (configs[0] reads thousands of 5,000-row stripes)
  void reset() {
    rlev2.clear();
    v1_segs.clear();
    batched.clear();
    dict_jobs.clear();
    dict_done.clear();
    dict_pre.clear();
    varint_jobs.clear();
    varint_pre.clear();
    dec_jobs[0].clear();
    dec_jobs[1].clear();
    dec_done.clear();
    scan_jobs.clear();
    scan_done.clear();
    launches.clear();
    pre_on_lane = false;
  }
  // Holds only pre-loaded dictionaries (collect_dicts: every batched stream
  // is such a dictionary's LENGTH): nothing reads the batch's outputs before
  // a fork's next level
  bool only_preloaded_dicts() const {
    return batched.size() == dict_pre.size() && dict_done.empty() && scan_jobs.empty() && dec_jobs[0].empty() &&
           dec_jobs[1].empty() && varint_jobs.empty();
  }

 private:
  static uint64_t key(uint32_t id, int slot) { return (uint64_t)id * 8 + (uint64_t)slot; }
};

}  // namespace reader
}  // namespace orcg

using namespace orcg;
using namespace orcg::file;
using namespace orcg::reader;

struct orcg_reader {
  // serialises decodes: the reader's own reads and the row readers' prefetch
  // workers share its decode state (stages, batch tables, checks)
  std::mutex mu;
  // The reader's own options (changed by the setters under mu; the context
  // is fixed at open). Entry points that run outside a decode (copy_to_host,
  // is_selected, row reader creation, the Arrow export) read only these; a
  // row reader's worker never writes them.
  ReadOptions own;
  // The options of the decode in progress (valid under mu, set by Active):
  // the reader's own for its reads, a row reader's for that row reader's
  // prefetch decodes. act.ctx is the context the decode launches on: null
  // outside a decode, and within a struct's fork a side lane of the caller's.
  ReadOptions act;
  uint64_t last_dev_inflate[2] = {0, 0};  // last read: chunks, decompressed bytes inflated on the device
  // Resolved zones live as long as the reader (zones, under tz_mu: prepare()
  // resolves writer zones on worker threads).
  mutable std::mutex tz_mu;
  mutable std::map<std::string, std::unique_ptr<ZoneEntry>> zones;  // by canonical name
  mutable std::vector<std::unique_ptr<ZoneEntry>> zones_replaced;   // entries set_zone_rules replaced
  mutable std::unique_ptr<ZoneEntry> utc_entry;
  const ZoneEntry* utc_zone_entry() const;                       // caller holds tz_mu
  const ZoneEntry* resolve_zone(const std::string& name) const;  // NULL: not found
  int zone_table(const ZoneEntry* z, TzTable* out);
  rt::Tree file_tree() const;  // the file's types as read_type.hh's tree
  // Makes `o` the options of the decode in progress, for its scope (the
  // caller holds mu). A reader zone left unset resolves to "GMT" here.
  struct Active {
    orcg_reader* r;
    Active(orcg_reader* r_, const ReadOptions& o) : r(r_) {
      r->act = o;
      if (!r->act.reader_tz) r->act.reader_tz = r->resolve_zone("GMT");
    }
    ~Active() { r->act.ctx = nullptr; }
  };
  const uint8_t* file = nullptr;
  uint64_t file_len = 0;
  void* mapped = nullptr;
  PostScript ps;
  Footer footer;
  std::string last_error;
  HostStage stages[3];  // read_stripes: stripe i in stages[i % 3]
  bool decimal_as_long = false;  // PostScript version 1.9999 (UNSTABLE-PRE-2.0): Decimal64V2 columns (Reader.cc:1693-1699)
  int32_t hive11_scale = 6;  // RowReaderOptions::forcedScaleOnHive11Decimal (Reader.cc RowReaderOptionsPrivate: 6)
  bool hive11_throw = true;  // RowReaderOptions::throwOnHive11DecimalOverflow (default true)
  std::string software_version;  // orcg_reader_software_version's buffer
  std::vector<std::unique_ptr<DevSlot>> slots;  // results of the last read, in stripe order
  size_t nslots = 0;
  // decode() state: the host stage and device slot of the stripe being decoded (Bound)
  HostStage* H = nullptr;
  DevSlot* D = nullptr;
  double timings[5] = {0, 0, 0, 0, 0};
  uint64_t stream_stats[2] = {0, 0};  // last read: RLE streams cut by the row index, by host plans
  // ReaderMetrics (Reader.hh:59-76) over the reader's life, in orcg_reader_metrics
  // order; atomics, as the reference's (the caller's thread counts next()
  // calls while a row reader's worker decodes)
  enum {
    kMReaderCall, kMReaderLatency, kMDecompressCall, kMDecompressLatency, kMDecodeCall, kMDecodeLatency,
    kMByteCall, kMByteLatency, kMIOCount, kMIOLatency, kMSelectedRG, kMEvaluatedRG, kMCacheHits, kMCacheMisses
  };
  std::atomic<uint64_t> metrics[14] = {};
  void madd(int i, uint64_t v) { metrics[i].fetch_add(v, std::memory_order_relaxed); }
  // DecodingLatencyUs / ByteDecodingLatencyUs from HIP events around the
  // integer-RLE and byte-RLE launches of a stripe (orcg_reader_set_metrics_timing;
  // off: DecodingLatencyUs is the stripe's device phase, ByteDecoding 0)
  bool metrics_timing = false;
  std::vector<hipEvent_t> ev_pool;
  hipEvent_t ev_get() {
    if (ev_pool.empty()) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      return e;
    }
    hipEvent_t e = ev_pool.back();
    ev_pool.pop_back();
    return e;
  }
  // brackets the launches `f` enqueues on act.ctx->stream with a timed event pair
  template <class Fn>
  int timed(int kind, Fn&& f) {
    if (!metrics_timing) return f();
    hipEvent_t a = ev_get(), b = ev_get();
    if (a) (void)hipEventRecord(a, act.ctx->stream);
    const int rc = f();
    if (b) (void)hipEventRecord(b, act.ctx->stream);
    if (a && b) F->ev_used.push_back(EvPair{a, b, kind});
    else {
      if (a) ev_pool.push_back(a);
      if (b) ev_pool.push_back(b);
    }
    return rc;
  }
  // after the stripe's synchronisation: the pairs' times into the metrics
  void collect_event_times() {
    double us[2] = {0, 0};
    for (const EvPair& p : F->ev_used) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) us[p.kind] += ms * 1e3;
      ev_pool.push_back(p.a);
      ev_pool.push_back(p.b);
    }
    F->ev_used.clear();
    madd(kMDecodeLatency, (uint64_t)us[0]);
    madd(kMByteLatency, (uint64_t)us[1]);
  }
  uint64_t batched_streams = 0;       // last read: RLEv2 streams decoded by multi-stream launches
  uint64_t stage_bytes = 0;           // last read: bytes uploaded (decompressed streams + plans)

  // A stripe between its launches (issue) and its host checks (finish): its
  // stage and slot, the checks whose operands are device scalars (dictionary
  // blob size, varint counts, string bytes: their D2H copies are queued on
  // the stream and the checks run, in column order, after the stripe's one
  // synchronisation instead of a synchronisation each; the reference makes
  // them inline), the pinned read-back mirror, the inline failure, and the
  // event after the stripe's last copy. read_stripes keeps two in flight:
  // stripe i + 1 is issued before stripe i is finished.
  struct Flight {
    HostStage* hs = nullptr;
    DevSlot* ds = nullptr;
    uint64_t* h_defer = nullptr;
    size_t defer_cap = 0, defer_used = 0;
    // (column, check): run in column order with the columns' device errors
    std::vector<std::pair<uint32_t, std::function<int()>>> checks;
    // the read-back block's pinned mirror (valid after the stripe's copy)
    uint64_t* h_rb = nullptr;
    size_t h_rb_cap = 0, rb_words = 0, rb_used = 0;
    size_t inflate_word = 0;  // the device inflate's error record in the read-back block (0: none)
    std::vector<EvPair> ev_used;  // metrics timing events
    hipEvent_t done = nullptr;    // recorded after the read-back copy
    // GPU-time split of the flight (timings[3] / [4]): before and after the
    // stripe's upload, and after its last decode launch
    hipEvent_t ev_up0 = nullptr, ev_up1 = nullptr, ev_dec = nullptr;
    bool ev_split = false;
    bool enqueued = false;        // done / the read-back copy belong to this issue
    int rc = ORCG_OK;             // the inline (host-detected) failure of the issue
    uint32_t err_col = 0;
    std::string err_msg;
    double t0 = 0, t1 = 0;
  };
  Flight flights[2];
  Flight* F = &flights[0];
  // a member set for a scope, then put back
  template <typename T>
  struct Restore {
    T& ref;
    const T old;
    Restore(T& v, T now) : ref(v), old(v) { ref = now; }
    ~Restore() { ref = old; }
  };
  // issue() and finish(): the flight, and for their scope its stage and slot
  struct Bound {
    Restore<HostStage*> h;
    Restore<DevSlot*> d;
    Bound(orcg_reader* r, Flight& fl, HostStage* hs, DevSlot* ds) : h(r->H, hs), d(r->D, ds) { r->F = &fl; }
  };
  // the column decode() is working on, and the column of the first inline
  // (host-detected) failure of this stripe
  static constexpr uint32_t kNoCol = 0xffffffffu;
  uint32_t cur_col = kNoCol, err_col = kNoCol;
  int first_error(int inline_rc);
  // `count` words of the read-back block: the device address a kernel writes,
  // and (*host) where the host reads it after the stripe's synchronisation
  uint64_t* rb_alloc(size_t count, const uint64_t** host) {
    if (!D->d_rb || F->rb_used + count > F->rb_words) return nullptr;
    uint64_t* d = D->d_rb + F->rb_used;
    *host = F->h_rb + F->rb_used;
    F->rb_used += count;
    return d;
  }
  const uint64_t* defer(const void* d_src, size_t count) {
    // a value in the read-back block rides its one copy
    if (D && D->d_rb && (const uint64_t*)d_src >= D->d_rb && (const uint64_t*)d_src + count <= D->d_rb + F->rb_words)
      return F->h_rb + ((const uint64_t*)d_src - D->d_rb);
    if (F->defer_used + count > F->defer_cap) return nullptr;
    uint64_t* h = F->h_defer + F->defer_used;
    F->defer_used += count;
    if (hipMemcpyAsync(h, d_src, count * 8, hipMemcpyDeviceToHost, act.ctx->stream) != hipSuccess) return nullptr;
    return h;
  }

  // Mid-stripe reads the host must wait for (list / map totals, union
  // counts). Up to kPublishMax counts per stream: publish_kernel writes them
  // and a generation flag into coherent pinned memory and the host polls the
  // flag (launch_publish); more: 8-byte D2H copies into pinned memory (one
  // DMA each), then one stream synchronisation.
  uint64_t* h_pub = nullptr;  // kPubSlots slots of kPubStride words: counts, then the flag
  uint64_t* d_pub = nullptr;
  uint64_t pub_gen = 0;
  static constexpr size_t kPubSlots = 32, kPubStride = 32;
  // a count on the device and the context whose stream produced it
  struct CountSrc {
    Ctx* lane;
    const void* src;
  };
  // 1 = more counts on one stream than a slot holds, or no pinned slots (the
  // caller copies them instead)
  int poll_counts(const std::vector<CountSrc>& srcs, uint64_t* out);
  uint64_t* h_sync = nullptr;
  size_t sync_cap = 0;
  // poll_counts, else the D2H copies on each source's stream and one
  // synchronisation per stream used
  int read_back(const std::vector<CountSrc>& srcs, uint64_t* out);
  int read_back(const void* src, uint64_t* out) { return read_back({CountSrc{act.ctx, src}}, out); }

  ~orcg_reader();  // reader_api.cpp
  int fail(int status, const std::string& m) {
    if (err_col == kNoCol) err_col = cur_col;
    last_error = m;
    if (act.ctx) act.ctx->last_error = m;
    return status;
  }
  int fail_ctx(int rc) { return fail(rc, act.ctx ? act.ctx->last_error : std::string("device error")); }
  // a failure outside a decode (argument F->checks of the caller's thread):
  // last_error is shared with the row readers' workers, so under mu
  int fail_user(int status, const std::string& m) {
    std::lock_guard<std::mutex> lk(mu);
    last_error = m;
    if (own.ctx) own.ctx->last_error = m;
    return status;
  }
  int fail_oom(const char* file, int line) {
    if (debug_on("alloc")) fprintf(stderr, "orcg: reader device allocation failed at %s:%d (column %u)\n", file, line, cur_col);
    return fail(ORCG_OUT_OF_MEMORY, "device allocation failed");
  }

  int open_tail();
  // (o: the options of the read it prepares for, of which it reads only the
  // selection, the local zone and the device-inflate flag, and nothing else
  // the decodes change: it runs without mu, beside a decode)
  int prepare(uint64_t s, HostStage& hs, const ReadOptions& o) const;
  // whether the stripe's stream (col, slot) is one the host never walks: raw
  // bytes or varints, which a Snappy or LZ4 file's chunks can inflate on the device
  bool host_never_walks(const HostStage& hs, uint32_t col, int slot) const;
  // prepare()'s phases (reader_prepare.cpp). A stream the stripe reads:
  struct Need {
    uint32_t col;
    int slot;
    std::vector<Chunk> chunks;
    uint64_t file_off = 0;  // stream start in the file
    bool device = false;    // inflated on the device: staging takes its compressed chunks
  };
  int locate_streams(uint64_t s, HostStage& hs, const std::vector<uint8_t>& sel, const std::string& local_zone,
                     StripeFooter& sf, std::vector<int>& row_index, std::vector<Need>& needs) const;
  int load_streams(HostStage& hs, std::vector<Need>& needs, double* t_inflate, uint64_t* used) const;
  void map_row_index(uint64_t s, const StripeFooter& sf, const std::vector<int>& row_index,
                     const std::vector<Need>& needs, HostStage& hs) const;
  bool column_positions(size_t col, Col& c, const StreamInfo& ri, uint64_t G, const std::vector<int>& need_of,
                        const std::vector<Need>& needs) const;
  void build_plans(const std::vector<uint8_t>& sel, HostStage& hs, std::vector<StreamBuf*>& rle) const;
  int layout_staging(uint64_t s, HostStage& hs, const std::vector<StreamBuf*>& rle, uint64_t w) const;
  int read_stripes(uint64_t first, uint64_t count);
  int upload_and_decode(HostStage& hs, DevSlot& ds);  // issue + finish
  void issue(HostStage& hs, DevSlot& ds, Flight& fl);
  int finish(Flight& fl);
  // d_in_count (may be null): in_count is on the device (the parent's
  // non-null rows), in_count is then an upper bound; in_col: the column whose
  // mask in_nn is
  int decode(uint32_t id, uint64_t n, const uint8_t* in_nn, uint64_t in_count, const int64_t* rg_rows,
             const uint64_t* d_in_count = nullptr, Col* in_col = nullptr);
  // The column a decode works on, handed down to every step that needs it:
  // n rows under the parent's mask in_nn (null: none), of which, after the
  // column's PRESENT stream, nonnull hold a value (exact, or with d_nonnull
  // an upper bound whose exact count is on the device); row_nn: the column's
  // own mask (null: every row holds a value); rg_rows (device, may be null):
  // the first row of each row group, in the column's rows
  struct Rows {
    uint64_t n, nonnull;
    const uint64_t* d_nonnull;
    const uint8_t* row_nn;
    const int64_t* rg_rows;
    const uint8_t* in_nn;
  };
  // fills nonnull, d_nonnull and row_nn (in_count: the rows set in in_nn)
  int decode_present(Col& c, uint64_t in_count, const uint64_t* d_in_count, Col* in_col, Rows* rows);
  StreamLayout layout(uint32_t id, const Col& c) const {
    return stream_layout(footer.types[id], c.encoding, decimal_as_long, c.s[kSlotPresent].present);
  }
  // one per column kind (reader_decode.cpp; the struct's fork: reader_fork.cpp)
  int decode_decimal(uint32_t id, Col& c, const StreamLayout& lay, const Rows& r);
  int decode_hive11_nulls(Col& c, const uint8_t* keep, const Rows& r);
  // schema evolution: the decoded column `id` converted to its read type
  // (convert_kernels.hip), right after its kind's decode placed its rows
  int convert_column(uint32_t id, Col& c);
  int decode_timestamp(Col& c, const StreamLayout& lay, const Rows& r);
  int decode_integer(Col& c, const StreamLayout& lay, const Rows& r);
  int decode_bytes(Col& c, const StreamLayout& lay, const Rows& r);
  int decode_double(Col& c, const Rows& r);
  int decode_dict_string(uint32_t id, Col& c, const StreamLayout& lay, const Rows& r);
  int decode_direct_string(uint32_t id, Col& c, const StreamLayout& lay, const Rows& r);
  int decode_list(uint32_t id, Col& c, const StreamLayout& lay, const Rows& r);
  int decode_struct(uint32_t id, Col& c, const Rows& r);
  int decode_union(uint32_t id, Col& c, const StreamLayout& lay, const Rows& r);
  // the dictionary's deferred checks, in the reference's order (h: blob bytes,
  // negative-length flag); sets the column's blob
  void check_dictionary(uint32_t id, Col& c, const uint64_t* h);
  int fork_struct(Col& c, const std::vector<uint32_t>& kids, unsigned nl, const Rows& r);
  // Columns whose value streams take a device-resident value count (RLEv2
  // through the tiled instances): their PRESENT decode's non-null count is
  // not read back mid-stripe (one stream synchronisation per nullable column
  // saved); has_nulls is settled with the stripe's F->checks.
  bool device_counts(uint32_t id) const;
  // Whether decode(id) launches device work: false when everything it needs
  // came from the stripe's batched launches (streams, dictionaries)
  bool device_work(uint32_t id) const;
  // Side streams for sibling subtrees (ORCG_LANES, default 4; 1 = one
  // stream). in_lane: decode() runs on a side context (no nested forks).
  bool in_lane = false;
  // decode() on side context `lane` for a scope
  struct OnLane {
    Restore<Ctx*> ctx;
    Restore<bool> lane;
    OnLane(orcg_reader* r, Ctx* l) : ctx(r->act.ctx, l), lane(r->in_lane, true) {}
  };
  // A list / map decoded under a fork whose children wait for its element
  // count (offsets[n] on the device), decoded on the same side context.
  struct Pending {
    uint32_t id;
    const int64_t* d_total;
    int64_t* child_rows;
    Ctx* lane;
  };
  std::vector<Pending>* pending = nullptr;
  int fork_levels(LaneFork& lf, Ctx* base, unsigned nl, std::vector<Pending>& level, int rc);
  static unsigned num_lanes() { return side_lanes(); }
  int segments(Col& c, int slot, bool boolean, const Rows& r, const uint64_t** d_seg, uint64_t* nseg);
  // RLE integer stream (slot, signedness and RLE version from the column's
  // layout, rle_v1)
  // (*out: the stream's values, decoded by this stripe's multi-stream batch
  // when collect() queued it, else allocated and decoded now)
  // (dcount: the value count on the device, `count` then only sizes the output)
  int int_stream(Col& c, const StreamDesc& d, const Rows& r, uint64_t count, int64_t** out,
                 const uint64_t* dcount = nullptr);
  // The stripe's multi-stream batch (StripeBatch): collect() queues what
  // the host can count before the upload, plan_batch() turns the queues into
  // launches, and decode() then finds the outputs in B.
  bool batch_on = true;
  StripeBatch B;
  int collect(uint32_t id, uint64_t n, const int64_t* rg_rows);
  int collect_dicts(uint32_t id);
  int queue_stream(uint32_t id, const StreamDesc& d, const Rows& r, uint64_t count);
  int queue_dict(uint32_t id, uint64_t n);
  int queue_varint(uint32_t id);
  int queue_decimal(uint32_t id, uint64_t n);
  int queue_scan(uint32_t id, uint64_t n);
  // the job queue_dict and collect_dicts both queue: column id's dictionary
  // (entry offsets and summary; with `gather`, the n rows' starts and
  // lengths too), recorded in `done` (B.dict_done or B.dict_pre)
  int push_dict(uint32_t id, const int64_t* lengths, const int64_t* idx, uint64_t n, bool gather,
                std::unordered_map<uint32_t, StripeBatch::DictDone>& done);
  int plan_batch();
  int byte_stream(Col& c, const StreamDesc& d, const Rows& r, uint64_t count, uint8_t* out, uint64_t* d_ones = nullptr,
                  const uint64_t* d_count = nullptr);
  int scatter(const void* dense, const uint8_t* nn, uint64_t n, void* out, int width);
  // Dense values to rows: `dense` itself when the column has no mask, else
  // r.n (+ pad) elements of `width` bytes with the values scattered to the
  // column's non-null rows
  int place_bytes(const void* dense, int width, const Rows& r, uint64_t pad, void** out);
  template <typename T, typename U>
  int place(T* dense, int width, const Rows& r, U** out, uint64_t pad = 0) {
    void* p = nullptr;
    const int rc = place_bytes(dense, width, r, pad, &p);
    *out = (U*)p;
    return rc;
  }
  template <typename T>
  T* alloc(uint64_t count) {
    return (T*)D->pool.get(std::max<uint64_t>(count, 1) * sizeof(T));
  }
};

// ReaderMetrics::ReaderCall / ReaderInclusiveLatencyUs around a caller-facing
// call (the reference's SCOPED_STOPWATCH in RowReaderImpl::next, Reader.cc:1393)
struct ReaderCallScope {
  orcg_reader* r;
  double t0 = now_s();
  explicit ReaderCallScope(orcg_reader* rr) : r(rr) {}
  ~ReaderCallScope() {
    r->madd(orcg_reader::kMReaderCall, 1);
    r->madd(orcg_reader::kMReaderLatency, (uint64_t)((now_s() - t0) * 1e6));
  }
};

namespace orcg {
namespace reader {
// RowReaderOptions::include by type id: the columns, their subtrees and
// their ancestors (NULL = every column)
int compute_selection(orcg_reader* r, const uint8_t* include, uint32_t ntypes, std::vector<uint8_t>& sel);
// a decoded column as the C API's view (type_id and kind are the caller's)
void fill_view(const ColView& c, orcg_column_view* out);
}  // namespace reader
}  // namespace orcg

#define ORCG_ALLOC(T, v, count)                                                  \
  T* v = alloc<T>(count);                                                         \
  if (!v) return fail_oom(__FILE_NAME__, __LINE__)
#define ORCG_ALLOC_TO(T, v, count)                                                \
  do {                                                                            \
    v = alloc<T>(count);                                                          \
    if (!v) return fail_oom(__FILE_NAME__, __LINE__);                                            \
  } while (0)
