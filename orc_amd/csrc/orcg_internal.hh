// Internal declarations shared by the liborcgpu translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/orcg.h"
#include "host_plan.hh"
#include "rlev2_route.hh"

namespace orcg {

// The device error record: min over (value_index << 8 | code). ~0 = none.
constexpr unsigned long long kNoError = ~0ull;

// The roles of a context's scratch buffers (scratch()). A buffer holds one
// thing at a time: a caller must not hold a slot across a launcher that takes
// it. Launchers that take slots themselves (every other one takes none):
//   launch_scatter, launch_count_nonzero   kScratchTileCounts, kScratchTileOffsets
// Callers: the host round trip (host_decode.hh) kScratchStream, kScratchSegments,
// kScratchDense; the decimal decode kScratchTileCounts, kScratchTileOffsets
// (its own tiles; it calls neither launcher above); the Arrow export
// kScratchNotNull (its entry block), kScratchDense, kScratchColumn; the convert
// entry points kScratchMisc; the debug hooks kScratchDense, kScratchColumn,
// kScratchMisc; orcg_snappy_decompress_device and orcg_lz4_decompress_device kScratchSegments (the chunk table).
enum ScratchSlot {
  kScratchStream = 0,       // a host stream's bytes
  kScratchSegments = 1,     // its segment table
  kScratchDense = 2,        // dense decoded values
  kScratchNotNull = 3,      // not-null bytes
  kScratchColumn = 4,       // column output
  kScratchTileCounts = 5,   // per-tile counts
  kScratchTileOffsets = 6,  // their scan
  kScratchMisc = 7,
  kScratchSlots
};

struct Ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  unsigned long long* d_err = nullptr;  // device error record
  std::string last_error;
  uint64_t last_error_value = 0;
  // grow-only device scratch, one buffer per ScratchSlot
  void* d_scratch[kScratchSlots] = {};
  size_t scratch_cap[kScratchSlots] = {};
  int rlev2_variant = ORCG_RLEV2_TILED;  // which RLEv2 kernel to launch
  void* d_defer = nullptr;  // RLEv2 short-run segment queue (rlev2_tiled.cpp defer_queue)
  uint64_t defer_cap = 0;
  uint64_t defer_seq = 0;  // serial + drain launch pairs so far (their entries' stamps)
  int num_cus = 0;         // compute units of `device` (0 = not queried yet)
  // decoupled look-back status words (column_kernels.hip lb_status): one
  // buffer per context (its launches are ordered), a 16-bit epoch per launch
  void* d_lb = nullptr;
  uint64_t lb_cap = 0;
  uint32_t lb_epoch = 0;
  // two-pass RLEv2 run table and segment headers (RunTab), grow-only
  void* d_rtab = nullptr;
  uint64_t rtab_cap = 0;
  void* d_rhdr = nullptr;
  uint64_t rhdr_cap = 0;
  // job tables of multi-stream launches: a pinned host ring and its device
  // mirror, in bytes (stage_table)
  void* h_jobs = nullptr;
  void* d_jobs = nullptr;
  uint64_t jobs_cap = 0, jobs_used = 0;
  // or an arena the caller uploads itself (the file reader's stripe staging):
  // stage_table writes a table to arena_h and hands out arena_d; the caller
  // orders the arena's upload before the launches (plan_* / run_multi)
  uint8_t* arena_h = nullptr;
  uint8_t* arena_d = nullptr;
  uint64_t arena_cap = 0, arena_used = 0;
  // side contexts (own stream, scratch, queues) the file reader decodes
  // sibling column subtrees on concurrently, forked from and joined back into
  // this context's stream with events (LaneFork); created on first use
  // (ctx_lane)
  std::vector<Ctx*> lanes;
  hipEvent_t ev_fork = nullptr;
  std::vector<hipEvent_t> ev_join;
};

// Side context k of `base` (created on first use, settings copied from base);
// nullptr if it cannot be created.
Ctx* ctx_lane(Ctx* base, size_t k);

// One fork of `base`'s stream over its side lanes: which lanes were started
// from the fork point and have to be joined back. The callers (run_multi, the
// struct's fork, the pre-loaded dictionaries' lane) decide what runs where.
// Every member returns a hip_check status, its message in base->last_error.
struct LaneFork {
  explicit LaneFork(Ctx* b) : base(b) {}
  // the fork point: base->ev_fork on base's stream
  int begin();
  // *out = side lane k, made to wait for the fork point the first time k is
  // handed out (ORCG_DEVICE_ERROR: the lane could not be created)
  int lane(size_t k, Ctx** out);
  // lane `to` continues after what lane `from` holds now (and is joined too)
  int chain(size_t from, size_t to);
  // base's stream waits for every lane handed out since the last join: all
  // of them are tried, the first failure is returned; a second call is a no-op
  int join();

 private:
  Ctx* const base;
  std::vector<uint8_t> used;  // per lane: started from the fork point, not joined yet
};

// Redirects a context's device error record for a scope (a column's own
// record, a job's, the base's for a lane that runs the base's jobs)
struct ErrRecordScope {
  Ctx* const ctx;
  unsigned long long* const saved;
  ErrRecordScope(Ctx* c, unsigned long long* rec) : ctx(c), saved(c->d_err) { c->d_err = rec; }
  ~ErrRecordScope() { ctx->d_err = saved; }
};

// One no-op launch per kernel file on `s`: HIP loads a file's code object at
// its first launch (tens of ms for all of them), so the first context of a
// process pays it at creation instead of inside its first decode
// (ORCG_WARMUP=0: lazily).
void warm_rlev2_walk(hipStream_t s);
void warm_rlev2_tiled(hipStream_t s);
void warm_byterle(hipStream_t s);
void warm_columns(hipStream_t s);
void warm_rlev1(hipStream_t s);
void warm_decimal(hipStream_t s);

// Side streams the file reader may use (ORCG_LANES, default 4; 1 = none).
unsigned side_lanes();

// One RLEv1 segment of a multi-stream launch, built on the host from the
// stream's plan or row index: a workgroup reads its whole description in one
// load (no job search through the table on the device).
struct V1SegDesc {
  const uint8_t* src;
  uint64_t src_len;
  uint64_t seg_start, vi;  // first byte (a group header) and its first value
  uint64_t seg_end, v_next;  // the next segment's, or (src_len, ~0) for the last
  void* dst;               // int64 values [0, nvalues)
  uint64_t nvalues;
  unsigned long long* err;
  uint32_t is_signed, pad;
};

int set_error(Ctx* ctx, int status, const std::string& msg);
// ORCG_DEBUG=topic[,topic...]: stderr diagnostics of that topic (alloc,
// stale, rowreader, defer, jobs)
bool debug_on(const char* topic);
// ORCG_DEBUG_STALE=1: report (and clear) a HIP error left pending on this
// host thread at `where` (launch checks read hipGetLastError).
void debug_stale(const char* where);
// page-locked host memory (transparent huge pages + hipHostRegister for large
// buffers, hipHostMalloc otherwise); pinned_free takes either kind
// node >= 0: large buffers prefer that NUMA node's memory (the node of the
// thread that will read them)
void* pinned_alloc(size_t bytes, int node = -1);
// the NUMA node the calling thread runs on (-1 if unknown)
int current_numa_node();
void pinned_free(void* p);
int hip_check(Ctx* ctx, hipError_t e, const char* what);
int scratch(Ctx* ctx, ScratchSlot slot, size_t bytes, void** out);
// Wait for the context stream and fold the device error record into a status.
int sync_ctx(Ctx* ctx);

// One RLEv2 stream's launch: values [value_begin, value_begin + nvalues) of
// the stream at `src` (device) into dst, as integers of dst_bytes (8, 4 or 2).
// segtab is either orcg_segment[] or the row-index positions array
// (`positions`, with rows_per_group). dcount (may be null; the tiled
// instances only): the value count on the device, nvalues then bounds the
// output only.
struct Rlev2Args {
  const uint8_t* src;
  uint64_t src_len;
  int is_signed;
  const uint64_t* segtab;
  uint64_t nsegs;
  bool positions;
  uint64_t rows_per_group;
  uint64_t value_begin;
  uint64_t nvalues;
  void* dst;
  int dst_bytes;
  const uint64_t* dcount;
};

// The wave-walk kernel (rlev2_kernels.hip).
// java: 0 = the C++ reader's rules; 1 = Java's RunLengthIntegerReaderV2
// (DELTA runs of one value with a bit width decode two values, PATCHED_BASE
// with pl == 0 fails as Java's array index, pw + pgw > 64 fails with Java's
// IOException); 2 = Java with skipCorrupt (pw + pgw > 64 decodes, :196-202).
int launch_rlev2_decode(Ctx* ctx, const Rlev2Args& a, int java = 0);


// Two-pass short-run RLEv2 decode (DESIGN.md §3.1 "Two passes"): the union
// instance's dense (short-run) passes write their run starts to `tab` instead
// of expanding them, and rlev2_expand_kernel then expands every segment's
// tabled runs in value slices of `slice` values (spg slices per segment), a
// workgroup per slice. Per launch-wide segment g, hdr[g * (kRtHdr + spg) + i]:
// [0] table entries, [1] values the passes reached (segment-relative), [2..3]
// the segment's first value index, [4] its first table entry, [kRtHdr + k]
// the entry to start slice k from (k >= 1), [5] the segment's job (multi-
// stream launches). An entry is the run's stream byte
// offset | its first value (segment-relative) << 32. Runs of passes the first
// kernel expands itself (long runs, values past spg * slice) are not tabled.
constexpr uint32_t kRtHdr = 6;
struct RunTab {
  uint64_t* tab;
  uint32_t* hdr;
  uint32_t spg;
  uint32_t slice;
};
// The second pass over a.nsegs launch-wide segments (single stream: `a` as
// launch_rlev2_tiled took it; multi-stream: jobs_d, int64 output).
int launch_rlev2_expand(Ctx* ctx, const Rlev2Args& a, const RleJob* jobs_d, uint32_t njobs, const RunTab& rt);
void warm_rlev2_expand(hipStream_t s);

// A tiled instance (rlev2_tiled.cpp): the pinned one, or the one the default
// routes the stream to (rlev2_route.hh, which also lists the variants).
int launch_rlev2_tiled(Ctx* ctx, const Rlev2Args& a);

// Every stream of `jobs` (segment-table mode, int64 output) in one launch per
// instance the default's density rule picks (or the pinned variant);
// variant 1 falls back to one launch per stream.
int launch_rlev2_multi(Ctx* ctx, const RleJob* jobs, uint32_t njobs);
// Copies a job table into the context's arena (no copy enqueued) or its
// pinned ring and device mirror (an H2D ordered on ctx->stream); *out = the
// device copy.
int stage_table(Ctx* ctx, const void* src, size_t bytes, const void** out);
inline int stage_rle_jobs(Ctx* ctx, const RleJob* jobs, uint32_t n, const RleJob** out) {
  return stage_table(ctx, jobs, (size_t)n * sizeof(RleJob), (const void**)out);
}

// A multi-stream launch planned ahead of the upload that carries its job
// table (stage_table in arena mode): plan_* group, order and stage the
// jobs; run_multi enqueues the kernels (RLEv2 instances on side lanes).
struct MultiLaunch {
  enum Kind : int {
    kRlev2,         // RLEv2 instance `variant`
    kRlev1,         // RLEv1 segments, `variant` = the chunk width
    kDict,          // dictionaries
    kRlev2Pinned,   // pinned single-stream RLEv2 (host job)
    kVarintCounts,  // varint tile counts + scan (host VarintJob)
    kDecimal,       // decimal columns (DecJob table, `variant` = the decimal mode)
    kLengthScan,    // a direct string column's length scan (host ScanJob)
  };
  Kind kind;
  int variant;
  const void* d_jobs;
  uint32_t njobs;
  uint64_t grid;      // segments / tiles
  uint64_t values;
  // two-pass RLEv2 launch (kRlev2, spg > 0): run-table entries, slices per
  // segment and values per slice (RunTab)
  uint64_t tab_entries = 0;
  uint32_t spg = 0, slice = 0;
};
// The scheduler's rule (run_multi): the RLEv2 instances run side by side
// from the fork; these need only stream bytes and share one auxiliary lane
// before the join ...
inline bool on_aux_lane(MultiLaunch::Kind k) { return k == MultiLaunch::kRlev1 || k == MultiLaunch::kVarintCounts; }
// ... and these read the lanes' outputs, so the join comes first
inline bool joins_first(MultiLaunch::Kind k) {
  return k == MultiLaunch::kDict || k == MultiLaunch::kDecimal || k == MultiLaunch::kLengthScan;
}
int plan_rlev2_multi(Ctx* ctx, const RleJob* jobs, uint32_t njobs, std::vector<MultiLaunch>& out);
// One planned RLEv2 launch (kRlev2) over its staged job table, on ctx's stream:
// run_multi's entry into the tiled instances (rlev2_tiled.cpp).
int launch_rlev2_tiled_jobs(Ctx* ctx, const MultiLaunch& m);
// A varint DATA stream's tile counts and their scan (the first value of each
// kVarintTile-byte tile) ahead of its decode: the decimal columns' first two
// launches, run before the batch's join (they need only the stream bytes).
struct VarintJob {
  const uint8_t* src;
  uint64_t len;
  int64_t* counts;
  int64_t* base;    // ntiles + 1
  uint64_t* total;  // the values in the stream (read-back slot)
};
// A direct string column's starts: the exclusive scan of its batched LENGTH
// stream with computeSize's checks (launch_exclusive_scan's flags / total),
// run after the join beside the dictionaries and decimals.
struct ScanJob {
  const int64_t* in;
  uint64_t n;
  int64_t* out;     // n + 1
  uint64_t* flags;  // 2 (read-back slots)
  uint64_t* total;  // read-back slot
};
int plan_rlev1_multi(Ctx* ctx, const V1SegDesc* segs, uint64_t nsegs, std::vector<MultiLaunch>& out);
int run_multi(Ctx* ctx, const std::vector<MultiLaunch>& launches);

// d_ones (boolean mode, may be null): += the set rows written (a PRESENT
// stream's non-null rows), one atomic per wave. d_nout (may be null): the
// output count on the device (nout then bounds the output only).
int launch_byterle(Ctx* ctx, const uint8_t* d_src, uint64_t src_len, const uint64_t* d_segtab, uint64_t nsegs,
                   bool boolean, uint64_t begin, uint64_t nout, uint8_t* d_dst, uint64_t* d_ones = nullptr,
                   const uint64_t* d_nout = nullptr);
int launch_rlev1(Ctx* ctx, const uint8_t* d_src, uint64_t src_len, int is_signed, const uint64_t* d_segtab,
                 uint64_t nsegs, uint64_t value_begin, uint64_t nvalues, void* d_dst, int dst_bytes);
// The segments of several RLEv1 streams (int64 output) in one launch per
// chunk width (rlev1_kernel's narrow instance for short segments).
int launch_rlev1_multi(Ctx* ctx, const V1SegDesc* segs, uint64_t nsegs);
int launch_rlev1_jobs(Ctx* ctx, const V1SegDesc* d_segs, uint64_t nsegs, int chunk);
int launch_scatter(Ctx* ctx, const void* d_dense, const uint8_t* d_nn, uint64_t n, void* d_out, int width,
                   int fill_mode, int64_t fill);
// (d_summary, may be null: [0] blob bytes, [1] any negative length)
int launch_dict_offsets(Ctx* ctx, const int64_t* d_lengths, uint64_t dict_size, int64_t* d_offsets,
                        uint64_t* d_summary = nullptr);
int launch_dict_gather(Ctx* ctx, const void* d_idx, int idx_width, const uint8_t* d_nn, uint64_t n,
                       const int64_t* d_offsets, uint64_t dict_size, int64_t* d_start, int64_t* d_len);
// One dictionary column of a batched launch (dict_multi_kernel): entry
// lengths -> offsets + {blob bytes, negative-length flag} summary, and the
// bounds-checked gather of n rows (n = 0: offsets only, lazy decoding).
constexpr uint32_t kDictLds = 4096;  // largest dictionary a batch takes
struct DictJob {
  const int64_t* lengths;
  uint64_t dict_size;
  int64_t* offsets;   // dict_size + 1
  uint64_t* summary;  // [0] blob bytes, [1] any negative length
  const int64_t* idx;
  const uint8_t* nn;  // row not-null mask, or null
  uint64_t n;
  int64_t* start;
  int64_t* len;
  unsigned long long* err;
  uint64_t tile_base;  // set by the launcher
};
int launch_dict_multi(Ctx* ctx, const DictJob* jobs, uint32_t njobs);
int plan_dict_multi(Ctx* ctx, const DictJob* jobs, uint32_t njobs, std::vector<MultiLaunch>& out);
int launch_dict_jobs(Ctx* ctx, const DictJob* d_jobs, uint32_t njobs, uint64_t tiles);

// Varint decimals (decimal_kernels.hip): per-tile (kVarintTile bytes) terminator counts,
// then (after an exclusive scan of the counts) the decode + rescale into
// int64 (Decimal64) or [hi, lo] int64 pairs (Decimal128, orc::Int128 layout).
int launch_varint_tile_counts(Ctx* ctx, const uint8_t* d_src, uint64_t len, int64_t* d_counts, uint64_t* ntiles);
constexpr uint64_t kVarintTile = 4096;
// mode: 0 Decimal64, 1 Decimal128, 2 Hive 0.11 (overflow raises), 3 Hive 0.11
// with overflowing values nulled (d_keep[k] = 0; 1 otherwise)
int launch_varint_decimal(Ctx* ctx, const uint8_t* d_src, uint64_t len, const int64_t* d_tile_base,
                          const int64_t* d_scales, uint64_t nvalues, int32_t scale, int mode, void* d_out,
                          uint8_t* d_keep = nullptr);
// One decimal column of a batched launch (mode 0 Decimal64 / 1 Decimal128,
// no nulls): varint DATA, its tile bases, the decoded SECONDARY scales;
// tile0 = its first launch-wide tile (set by the planner).
struct DecJob {
  const uint8_t* src;
  uint64_t len;
  const int64_t* tile_base;
  const int64_t* scales;
  uint64_t nvalues;
  void* out;
  unsigned long long* err;
  uint64_t tile0;
  int32_t scale;
  int32_t pad;
};
int launch_decimal_jobs(Ctx* ctx, const DecJob* d_jobs, uint32_t njobs, uint64_t tiles, int mode);
// TimestampColumnReader value construction, in place.
int launch_timestamp(Ctx* ctx, int64_t* d_secs, int64_t* d_nanos, uint64_t n, int64_t epoch);
// A zone's flat table in device memory (tz::Zone::device_table, timezone.hh)
struct TzTable {
  const int64_t* d = nullptr;
  uint32_t words = 0;  // int64 words
};
// TimestampColumnReader::next for writer zone != reader zone, in place (the
// writer zone's epoch is in its table)
int launch_timestamp_tz(Ctx* ctx, int64_t* d_secs, int64_t* d_nanos, uint64_t n, const TzTable& writer,
                        const TzTable& reader);

// Schema evolution (convert_kernels.hip): n decoded values of class `src`
// (ConvSrc) converted to class `dst` (ConvDst) by the reference's rules
// (ConvertColumnReader.cc). nn (may be null = every row set) is read only;
// out_nn[i] = the row is set and its value fits; a row that does not fit holds
// 0 and adds one to *nulled (device; the caller zeroes it). throw_mode: the
// first such row is also reported into err as kErrConvertOverflow.
enum ConvSrc { kConvInt64 = 0, kConvFloat = 1, kConvDouble = 2, kConvDec64 = 3, kConvDec128 = 4 };
enum ConvDst { kToBool = 0, kToInt = 1, kToFloat = 2, kToDouble = 3, kToDec64 = 4, kToDec128 = 5 };
struct ConvertArgs {
  const void* src;
  const uint8_t* nn;
  void* out;
  uint8_t* out_nn;
  uint64_t n;
  unsigned long long* err;
  unsigned long long* nulled;
  int32_t src_scale;         // decimal sources
  int32_t width;             // kToInt: bytes of the read type (1, 2, 4, 8)
  int32_t precision, scale;  // decimal targets
  int32_t throw_mode;
  // host-computed constants (convert_constants): 10^src_scale as the double and
  // the float the reference divides by, and (T)pow(10, scale) for a float or
  // double source (a float's held in a double)
  float factor_f;
  double factor_d;
  double pow_t;
};
void convert_constants(int src, ConvertArgs* a);
int launch_convert(Ctx* ctx, int src, int dst, const ConvertArgs& a);

// Row-index segmentation (column_kernels.hip): prefix[g] = non-zero bytes of
// mask before row rows[g] (counts: scratch of G entries; prefix: G + 1);
// segment table from {offset, skip, bit skip} triplets; list / map child row
// group starts.
int launch_rg_prefix(Ctx* ctx, const uint8_t* d_mask, uint64_t n, const int64_t* d_rows, uint64_t G,
                     int64_t* d_counts, int64_t* d_prefix);
int launch_rg_segtab(Ctx* ctx, const int64_t* d_trip, const int64_t* d_prefix, uint64_t G, bool boolean,
                     uint64_t* d_seg);
int launch_rg_child_rows(Ctx* ctx, const int64_t* d_offsets, const int64_t* d_rows, uint64_t G, int64_t* d_out);
// rg_prefix + rg_segtab in one launch (decoupled look-back over the row
// groups' counts): d_prefix (G + 1 entries) and the segment table.
int launch_rg_prefix_segtab(Ctx* ctx, const uint8_t* d_mask, uint64_t n, const int64_t* d_rows, uint64_t G,
                            const int64_t* d_trip, bool boolean, int64_t* d_prefix, uint64_t* d_seg);

// UNION tags (UnionColumnReader): flags[j] = tags[j] == k; the first tag >=
// nchildren as (index << 8 | tag), ~0 when none; offsets[j] = scan_k[j] for
// the rows with tag k.
int launch_union_flags(Ctx* ctx, const uint8_t* d_tags, uint64_t n, uint32_t k, int64_t* d_flags);
int launch_union_check(Ctx* ctx, const uint8_t* d_tags, uint64_t n, uint32_t nchildren, uint64_t* d_first_bad);
int launch_union_offsets(Ctx* ctx, const uint8_t* d_tags, uint64_t n, uint32_t k, const int64_t* d_scan_k,
                         int64_t* d_offsets);

// Multi-workgroup exclusive scan: d_out[0..n] (n + 1 entries). Takes no scratch slot.
// d_flags (may be null; zero on entry): StringDirect length checks fused into
// the scan, [0] |= 1 for a negative input, [1] |= 1 when the total wraps.
// d_total (may be null): the total (d_out[n]) also written there (e.g. a
// slot of the reader's read-back block: no separate copy).
int launch_exclusive_scan(Ctx* ctx, const int64_t* d_in, uint64_t n, int64_t* d_out, uint64_t* d_flags = nullptr,
                          uint64_t* d_total = nullptr);
// Number of non-zero bytes of d_nn[0..n) into *d_total (device).
// kScratchTileCounts, kScratchTileOffsets.
int launch_count_nonzero(Ctx* ctx, const uint8_t* d_nn, uint64_t n, uint64_t* d_total);
// *d_flag = 1 if any d_v[i] < 0, else 0.
int launch_flag_negative(Ctx* ctx, const int64_t* d_v, uint64_t n, uint64_t* d_flag);
enum WidenKind { kWidenI8 = 0, kWidenU8 = 1, kWidenF32 = 2 };
int launch_widen(Ctx* ctx, const void* d_in, int kind, uint64_t n, void* d_out);
// Host (pinned, device-mapped) -> device copy by a kernel on ctx->stream;
// both buffers 16-byte aligned, rounded up to whole 16-byte words.
int launch_pull(Ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes);
// up to kPublishMax device int64 counts -> d_dst (coherent pinned memory),
// then *d_flag = gen (system-scope release): the host polls the flag
constexpr uint32_t kPublishMax = 16;
struct PublishArgs {
  const int64_t* src[kPublishMax];
  uint32_t n;
};
int launch_publish(Ctx* ctx, const PublishArgs& a, uint64_t* d_dst, uint64_t* d_flag, uint64_t gen);

// Snappy chunks (inflate_kernels.hip): chunk i of d_table (device) inflates
// d_src + src_offset into d_dst + dst_offset, a wavefront per chunk; the
// caller has bounded every entry by the buffers. d_err: the launch's error
// record ((chunk index << 8) | code), null = the context's.
int launch_snappy_inflate(Ctx* ctx, const uint8_t* d_src, const orcg_snappy_chunk* d_table, uint64_t nchunks,
                          uint8_t* d_dst, unsigned long long* d_err);
// The same launch for LZ4 chunks (raw blocks; dst_bytes = the host walk's size).
int launch_lz4_inflate(Ctx* ctx, const uint8_t* d_src, const orcg_lz4_chunk* d_table, uint64_t nchunks,
                       uint8_t* d_dst, unsigned long long* d_err);

// Dispatch on ctx->rlev2_variant.
static_assert(kRlev2Default == ORCG_RLEV2_TILED && kRlev2WaveWalk == ORCG_RLEV2_WAVE_WALK, "the public numbers");
inline int launch_rlev2(Ctx* ctx, const Rlev2Args& a) {
  return ctx->rlev2_variant == kRlev2WaveWalk ? launch_rlev2_decode(ctx, a) : launch_rlev2_tiled(ctx, a);
}

}  // namespace orcg

struct orcg_ctx : orcg::Ctx {};
