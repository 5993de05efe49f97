// Column-level kernels around the stream decoders:
//  * null scatter: dense decoded values -> row positions of a nullable column
//    (RleDecoderV2::copyDataFromBuffer with notNull, c++/src/RleDecoderV2.cc:
//    437-453; ColumnReader::next's PRESENT handling, c++/src/ColumnReader.cc:
//    81-104). C++ leaves null slots untouched; the Java face writes 1
//    (java/core/.../RunLengthIntegerReaderV2.java:371-396).
//  * dictionary offsets: lengths -> exclusive prefix sum
//    (loadStringDictionary, c++/src/DictionaryLoader.cc:69-80).
//  * dictionary gather: index -> (blob offset, length) with the reference's
//    bounds check (StringDictionaryColumnReader::next, c++/src/
//    ColumnReader.cc:561-594).
#include "device_util.hh"
#include "orcg_internal.hh"

namespace orcg {
namespace {
using namespace dev;

constexpr int kTile = 4096;  // rows per scatter tile (256 threads x 16 rows)
constexpr int kThreads = 256;

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t nn_bytes_count(u4 v) {
  // each byte is 0 or non-zero; count non-zero bytes
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = v[k];
    c += ((x & 0xffu) != 0) + ((x & 0xff00u) != 0) + ((x & 0xff0000u) != 0) + ((x & 0xff000000u) != 0);
  }
  return c;
}

__device__ __forceinline__ u4 load16(const uint8_t* nn, uint64_t row0, uint64_t n) {
  if (row0 + 16 <= n && (((uintptr_t)(nn + row0)) & 15u) == 0) return *(const u4*)(nn + row0);
  u4 v = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (row0 + k < n) v[k >> 2] |= (uint32_t)nn[row0 + k] << (8 * (k & 3));
  return v;
}

// ---- decoupled look-back (single-pass scans; no reset launch) ----------
// A tile's status is two words, each epoch << 48 | flag << 46 | 46 bits: the
// value's low 46 bits in word 2t, its high 18 bits in word 2t + 1 (the full
// 64-bit value: sums wrap mod 2^64 exactly like the reference's int64 sums,
// ColumnReader.cc:960-993, and a corrupt length cannot silently lose its high
// bits). Flag 1 = the tile's aggregate, 2 = its inclusive prefix; a tile
// publishes each flag once per epoch, so two words carrying the same epoch
// and flag belong to the same publication (no ordering between the two
// stores or loads is needed; a reader that sees different flags retries). A
// word of another epoch is unpublished, so the context's buffer is never
// cleared between launches (lb_status hands out a new 16-bit epoch per
// launch). The word before the status words counts tickets: tiles take them
// in the order they start (so a tile only waits on tiles already running),
// and the tile that takes the launch's last ticket sets the counter back to 0
// for the next launch on the stream (a compare-and-swap ticket on an
// epoch-tagged word instead cost 40x: thousands of workgroups retrying on one
// address).
constexpr uint64_t kLbMask = (1ull << 46) - 1;
constexpr uint32_t kLbWords = 2;  // status words per tile

__device__ __forceinline__ uint32_t lb_ticket(unsigned long long* status, uint32_t ntiles) {
  unsigned int* ctr = (unsigned int*)(status - 1);
  const uint32_t t = atomicAdd(ctr, 1u);
  if (t == ntiles - 1) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return t;
}

__device__ __forceinline__ void lb_publish(unsigned long long* status, uint32_t t, uint32_t flag, uint64_t v,
                                           uint32_t epoch) {
  const unsigned long long tag = ((unsigned long long)epoch << 48) | ((unsigned long long)flag << 46);
  __hip_atomic_store(&status[kLbWords * t], tag | (v & kLbMask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&status[kLbWords * t + 1], tag | (v >> 46), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Tile k's status: its flag (0 = not published in this epoch, or the two
// words from different publications) and value.
__device__ __forceinline__ uint32_t lb_read(unsigned long long* status, int64_t k, uint32_t epoch, uint64_t* v) {
  const unsigned long long lo = __hip_atomic_load(&status[kLbWords * k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long hi =
      __hip_atomic_load(&status[kLbWords * k + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  *v = (uint64_t)(lo & kLbMask) | ((uint64_t)(hi & kLbMask) << 46);
  const bool same = (lo >> 46) == (hi >> 46) && (uint32_t)(lo >> 48) == epoch;
  return same ? (uint32_t)((lo >> 46) & 3u) : 0u;
}

// One wave of tile t > 0 (after it published its aggregate): the sum over
// tiles [0, t), 64 predecessors a round back to the nearest inclusive prefix.
__device__ uint64_t lb_lookback(unsigned long long* status, uint32_t t, uint32_t epoch, int lane) {
  uint64_t excl = 0;
  for (int64_t j = (int64_t)t - 1;; j -= kWave) {
    const int64_t k = j - lane;
    uint64_t v = 0;
    uint32_t fl = 2;  // before tile 0: an inclusive prefix of 0
    if (k >= 0) fl = lb_read(status, k, epoch, &v);
    while (__ballot(fl == 0) != 0) {
      if (fl == 0) {
        __builtin_amdgcn_s_sleep(1);
        fl = lb_read(status, k, epoch, &v);
      }
    }
    const uint64_t pm = __ballot(fl == 2);
    const int first = pm ? __builtin_ctzll(pm) : kWave;
    excl += wave_sum<uint64_t>((k >= 0 && lane <= first) ? v : 0ull);
    if (pm) break;
  }
  return excl;
}

// StringDirectColumnReader::computeSize's checks (ColumnReader.cc:694-710),
// fused into the scan of the lengths: flags[0] |= 1 if a length is negative,
// flags[1] |= 1 if the running total wraps (a start plus its length below
// the start: with non-negative lengths, the size_t total overflowed). The
// flags are zero before the scan (the reader's read-back block).
__device__ __forceinline__ void strlen_flags(unsigned long long* flags, bool neg, bool wrap) {
  if (__any(neg) && (threadIdx.x % kWave) == 0) atomicOr(flags, 1ull);
  if (__any(wrap) && (threadIdx.x % kWave) == 0) atomicOr(flags + 1, 1ull);
}

__global__ __launch_bounds__(kThreads) void tile_count_kernel(const uint8_t* __restrict__ nn, uint64_t n,
                                                               uint32_t* __restrict__ counts) {
  __shared__ uint32_t red[kThreads / kWave];
  const uint64_t row0 = (uint64_t)blockIdx.x * kTile + threadIdx.x * 16u;
  uint32_t c = row0 < n ? nn_bytes_count(load16(nn, row0, n)) : 0;
  for (int d = kWave / 2; d > 0; d >>= 1) c += __shfl_down(c, d, kWave);
  if ((threadIdx.x % kWave) == 0) red[threadIdx.x / kWave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kThreads / kWave; ++w) t += red[w];
    counts[blockIdx.x] = t;
  }
}

// The one-workgroup exclusive scan: `n` values of Tin into offsets[0 .. n]
// (Tout; offsets[n] = the total, sums wrapping mod 2^64), 1,024 values a trip
// with the carry in LDS. What else it reports:
//  * kScanCounts: nothing (tile counts -> tile offsets, uint32 -> uint64);
//  * kScanDict: dictionary entry lengths -> offsets (int64). With `aux`:
//    aux[0] = the blob bytes (offsets[n]), aux[1] = 1 if an entry length is
//    negative (loadStringDictionary's check, DictionaryLoader.cc:71-77), both
//    stored -- the file reader's whole dictionary preparation in one launch;
//  * kScanFlags: uint64 -> uint64. With `aux`: the negative / wrap flags
//    OR-ed into aux[0], aux[1] (strlen_flags above); with `total`: *total =
//    offsets[n].
enum ScanReport { kScanCounts, kScanDict, kScanFlags };

template <typename Tin, typename Tout, int kReport>
__global__ __launch_bounds__(1024) void wg_scan_kernel(const Tin* __restrict__ in, uint64_t n,
                                                        Tout* __restrict__ offsets,
                                                        unsigned long long* __restrict__ aux,
                                                        uint64_t* __restrict__ total) {
  __shared__ uint64_t wsum[1024 / kWave];
  __shared__ uint64_t carry_s;
  __shared__ uint32_t neg_s;  // kScanDict
  const int lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
  if (threadIdx.x == 0) {
    carry_s = 0;
    if constexpr (kReport == kScanDict) neg_s = 0;
  }
  __syncthreads();
  bool neg = false, wrap = false;
  for (uint64_t b = 0; b < n; b += 1024) {
    const uint64_t i = b + threadIdx.x;
    const uint64_t x = i < n ? (uint64_t)in[i] : 0;  // (0 past n: neither negative nor a wrap)
    const uint64_t inc = wave_inclusive_scan(x);
    if (lane == kWave - 1) wsum[wv] = inc;
    __syncthreads();
    uint64_t before = carry_s;
    for (int w = 0; w < wv; ++w) before += wsum[w];
    const uint64_t st = before + inc - x;
    if (i < n) offsets[i] = (Tout)st;
    if constexpr (kReport != kScanCounts) neg |= (int64_t)x < 0;
    if constexpr (kReport == kScanFlags) wrap |= st + x < st;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = before + inc;
    __syncthreads();
  }
  if constexpr (kReport == kScanDict) {
    if (aux && __any(neg) && lane == 0) atomicOr(&neg_s, 1u);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    offsets[n] = (Tout)carry_s;
    if constexpr (kReport == kScanDict) {
      if (aux) {
        aux[0] = carry_s;
        aux[1] = neg_s;
      }
    }
    if constexpr (kReport == kScanFlags) {
      if (total) *total = carry_s;
    }
  }
  if constexpr (kReport == kScanFlags) {
    if (aux) strlen_flags(aux, neg, wrap);
  }
}

// One workgroup per kTile rows; row r = tile + 256 k + tid (k < 16), so the
// not-null bytes, the dense values (consecutive ranks) and the output rows
// are all read and written coalesced. A row's rank: the tile's first rank +
// the non-null rows of the earlier 256-row chunks + those of the lower waves
// of its chunk + a ballot popcount inside its wave.
template <typename T, bool kFill>
__global__ __launch_bounds__(kThreads) void scatter_kernel(const T* __restrict__ dense, const uint8_t* __restrict__ nn,
                                                            uint64_t n, const uint64_t* __restrict__ tile_off,
                                                            T* __restrict__ out, T fill) {
  constexpr int kChunks = kTile / kThreads;
  static_assert(kChunks * kThreads == kTile, "tile = whole 256-row chunks");
  __shared__ uint32_t s_cnt[kChunks][kThreads / kWave];
  const int lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
  const uint64_t t0 = (uint64_t)blockIdx.x * kTile;
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t flags = 0;  // bit k: my row of chunk k is not null
  uint32_t below_cnt[kChunks];
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const uint64_t r = t0 + (uint64_t)k * kThreads + threadIdx.x;
    const bool f = r < n && nn[r] != 0;
    const uint64_t b = __ballot(f);
    flags |= (f ? 1u : 0u) << k;
    below_cnt[k] = (uint32_t)__builtin_popcountll(b & below);
    if (lane == 0) s_cnt[k][wv] = (uint32_t)__builtin_popcountll(b);
  }
  __syncthreads();
  uint64_t base = tile_off[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const uint64_t r = t0 + (uint64_t)k * kThreads + threadIdx.x;
    uint32_t lower = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / kWave; ++w) {
      const uint32_t c = s_cnt[k][w];
      lower += w < wv ? c : 0u;
      all += c;
    }
    if (r < n) {
      if ((flags >> k) & 1u) out[r] = dense[base + lower + below_cnt[k]];
      else if (kFill) out[r] = fill;
    }
    base += all;
  }
}

template <typename T>
__global__ void dict_gather_kernel(const T* __restrict__ idx, const uint8_t* __restrict__ nn, uint64_t n,
                                   const int64_t* __restrict__ offsets, uint64_t dict_size,
                                   int64_t* __restrict__ out_start, int64_t* __restrict__ out_len,
                                   unsigned long long* err) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (nn && !nn[i]) continue;
    const uint64_t e = (uint64_t)(int64_t)idx[i];
    if (e >= dict_size) {
      report(err, i, kErrDictIndex);
      continue;
    }
    const int64_t s = offsets[e];
    out_start[i] = s;
    out_len[i] = offsets[e + 1] - s;
  }
}

// A stripe's dictionary string columns in one launch: per column the entry
// offsets (loadStringDictionary's prefix sum and negative-length check,
// DictionaryLoader.cc:69-80) and the row gather (StringDictionaryColumnReader::
// next, ColumnReader.cc:561-594). Every workgroup scans its column's entry
// lengths into LDS (dictionaries of <= kDictLds entries: a few KB) and
// gathers one tile of rows from there; the column's first tile also writes
// the offsets and the {blob bytes, negative length} summary. Null rows get
// (0, 0), as the per-column path's memset leaves them.
constexpr uint32_t kDictTile = 2048;  // rows per workgroup (256 threads x 8)

// One workgroup per (column, tile): jobs[blockIdx.x] is the column's job with
// tile_base = the tile's index in the column (the host writes one copy per
// tile: a workgroup reads its whole description in one load). The tile's
// indices are loaded before the dictionary's lengths so both latencies
// overlap.
__global__ __launch_bounds__(kThreads) void dict_multi_kernel(const DictJob* __restrict__ jobs, uint32_t njobs) {
  __shared__ int64_t s_off[kDictLds + 1];
  __shared__ uint64_t s_wsum[kThreads / kWave];
  __shared__ uint32_t s_neg;
  constexpr int kRows = kDictTile / kThreads;
  const int tid = (int)threadIdx.x, lane = tid % kWave, wv = tid / kWave;
  const DictJob& J = jobs[blockIdx.x];
  const uint64_t tile = uni64(J.tile_base);
  const uint64_t D = uni64(J.dict_size);
  const uint64_t n = uni64(J.n);
  const int64_t* lengths = (const int64_t*)uni64((uint64_t)(uintptr_t)J.lengths);
  const int64_t* idx = (const int64_t*)uni64((uint64_t)(uintptr_t)J.idx);
  const uint8_t* nn = (const uint8_t*)uni64((uint64_t)(uintptr_t)J.nn);
  const uint64_t r0 = tile * kDictTile;
  // my rows' entries (and not-null bytes) first
  int64_t e_[kRows];
  uint32_t present = 0;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const uint64_t i = r0 + (uint64_t)k * kThreads + (uint64_t)tid;
    const bool in = i < n;
    const bool p = in && (!nn || nn[i] != 0);
    present |= (p ? 1u : 0u) << k;
    e_[k] = p ? idx[i] : 0;
  }
  if (tid == 0) s_neg = 0;
  // offsets: thread t sums entries [16t, 16t + 16)
  int64_t loc[16];
  uint64_t sum = 0;
  bool neg = false;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint64_t e = 16u * (uint64_t)tid + k;
    const int64_t x = e < D ? lengths[e] : 0;
    neg |= x < 0;
    loc[k] = (int64_t)sum;
    sum += (uint64_t)x;
  }
  const uint64_t inc = wave_inclusive_scan(sum, lane);
  if (lane == kWave - 1) s_wsum[wv] = inc;
  if (__any(neg) && lane == 0) atomicOr(&s_neg, 1u);
  __syncthreads();
  uint64_t before = inc - sum, total = 0;
#pragma unroll
  for (int w = 0; w < kThreads / kWave; ++w) {
    before += w < wv ? s_wsum[w] : 0ull;
    total += s_wsum[w];
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint64_t e = 16u * (uint64_t)tid + k;
    if (e < D) s_off[e] = (int64_t)(before + (uint64_t)loc[k]);
  }
  if (tid == 0) s_off[D] = (int64_t)total;
  __syncthreads();
  if (tile == 0) {
    int64_t* off = (int64_t*)uni64((uint64_t)(uintptr_t)J.offsets);
    for (uint64_t e = (uint64_t)tid; e <= D; e += kThreads) off[e] = s_off[e];
    if (tid == 0) {
      uint64_t* sm = (uint64_t*)uni64((uint64_t)(uintptr_t)J.summary);
      sm[0] = total;
      sm[1] = s_neg;
    }
  }
  if (r0 >= n) return;
  int64_t* out_start = (int64_t*)uni64((uint64_t)(uintptr_t)J.start);
  int64_t* out_len = (int64_t*)uni64((uint64_t)(uintptr_t)J.len);
  unsigned long long* err = (unsigned long long*)uni64((uint64_t)(uintptr_t)J.err);
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const uint64_t i = r0 + (uint64_t)k * kThreads + (uint64_t)tid;
    if (i >= n) break;
    if (!((present >> k) & 1u)) {  // a null row
      out_start[i] = 0;
      out_len[i] = 0;
      continue;
    }
    const uint64_t e = (uint64_t)e_[k];
    if (e >= D) {
      report(err, i, kErrDictIndex);
      continue;
    }
    const int64_t st = s_off[e];
    out_start[i] = st;
    out_len[i] = s_off[e + 1] - st;
  }
  (void)njobs;
}

// Exclusive scans of int64 values (lengths -> offsets): direct string
// lengths (DATA offsets, StringDirectColumnReader::next, c++/src/
// ColumnReader.cc:725-793) and list/map lengths (ListColumnReader::
// nextInternal, :960-993), one workgroup (wg_scan_kernel) up to 8,192 values,
// else the single-pass look-back kernel over 4,096-value tiles.
constexpr int kScanTile = 4096;  // 256 threads x 16 values

// Single-pass exclusive scan (decoupled look-back): workgroup tickets in
// dispatch order (an atomic on status[ntiles]); a tile's 4,096 values are
// loaded coalesced into LDS (row k*256 + tid), scanned 16 consecutive per
// thread, and stored back coalesced. Each tile publishes its aggregate
// (kLbA) as soon as it has it and its inclusive prefix (kLbP) once known; one
// wave looks back over 64 predecessors at a time, waiting on any still
// unpublished, summing back to the nearest inclusive prefix. status[] (ntiles
// + 1 words, epoch-tagged) need no reset. The three-launch scan above read
// 16 consecutive values per lane (one 128-byte stride per load instruction):
// 18-28 us per kernel for configs[4]'s 2.6 M list lengths.
__global__ __launch_bounds__(kThreads) void scan_lookback_kernel(const int64_t* __restrict__ in, uint64_t n,
                                                                 int64_t* __restrict__ out,
                                                                 unsigned long long* __restrict__ status,
                                                                 uint32_t ntiles, uint32_t epoch,
                                                                 unsigned long long* __restrict__ flags,
                                                                 uint64_t* __restrict__ total) {
  __shared__ uint64_t s_v[kScanTile + kScanTile / 16];  // one pad word per thread's 16 (bank spread)
  __shared__ uint64_t s_wsum[kThreads / kWave];
  __shared__ uint32_t s_tile;
  __shared__ uint64_t s_excl;
  const int tid = (int)threadIdx.x, lane = tid % kWave, wv = tid / kWave;
  if (tid == 0) s_tile = lb_ticket(status, ntiles);
  __syncthreads();
  const uint32_t t = s_tile;
  const uint64_t base = (uint64_t)t * kScanTile;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint64_t i = base + (uint64_t)k * kThreads + tid;
    const uint32_t e = (uint32_t)(k * kThreads + tid);
    s_v[e + (e >> 4)] = i < n ? (uint64_t)in[i] : 0ull;
  }
  __syncthreads();
  uint64_t v[16], sum = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    v[k] = s_v[tid * 17 + k];
    sum += v[k];
  }
  const uint64_t inc = wave_inclusive_scan(sum);
  if (lane == kWave - 1) s_wsum[wv] = inc;
  __syncthreads();
  uint64_t before = inc - sum, agg = 0;
#pragma unroll
  for (int w = 0; w < kThreads / kWave; ++w) {
    const uint64_t c = s_wsum[w];
    before += w < wv ? c : 0ull;
    agg += c;
  }
  if (wv == 0) {
    uint64_t excl = 0;
    if (t == 0) {
      if (lane == 0) lb_publish(status, 0, 2, agg, epoch);
    } else {
      if (lane == 0) lb_publish(status, t, 1, agg, epoch);
      excl = lb_lookback(status, t, epoch, lane);
      if (lane == 0) lb_publish(status, t, 2, excl + agg, epoch);
    }
    if (lane == 0) s_excl = excl;
  }
  __syncthreads();
  uint64_t run = s_excl + before;
  bool neg = false, wrap = false;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    s_v[tid * 17 + k] = run;
    neg |= (int64_t)v[k] < 0;
    wrap |= run + v[k] < run;
    run += v[k];
  }
  if (flags) strlen_flags(flags, neg, wrap);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint64_t i = base + (uint64_t)k * kThreads + tid;
    const uint32_t e = (uint32_t)(k * kThreads + tid);
    if (i < n) out[i] = (int64_t)s_v[e + (e >> 4)];
  }
  if (t == ntiles - 1 && tid == kThreads - 1) {
    out[n] = (int64_t)(s_excl + agg);
    if (total) *total = s_excl + agg;
  }
}

// Element conversions into the reference's batch types (LongVectorBatch /
// DoubleVectorBatch): tinyint sign-extension (ByteColumnReader, c++/src/
// ColumnReader.cc:188-223), boolean 0/1 (BooleanColumnReader :131-186),
// float -> double (DoubleColumnReader<FLOAT> :359-450).
template <typename Tin, typename Tout>
__global__ void widen_kernel(const Tin* __restrict__ in, uint64_t n, Tout* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (Tout)in[i];
}

// Flags any negative dictionary entry length (loadStringDictionary's check,
// c++/src/DictionaryLoader.cc:71-77).
__global__ void flag_negative_kernel(const int64_t* __restrict__ v, uint64_t n, unsigned long long* flag) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool neg = false;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) neg |= v[i] < 0;
  if (__any(neg) && (threadIdx.x % kWave) == 0) atomicOr(flag, 1ull);
}

// ---- row-index segmentation (ColumnReader::seekToRowGroup positions) ----
// A column's streams are cut at its row groups: the row index gives, per row
// group g and stream, the run-aligned byte offset of the run holding the row
// group's first value and the values to skip in it (RleDecoder::seek + skip,
// c++/src/RleDecoderV2.cc:109-130, ByteRLE.cc:527-560). The value index of
// that first value is the number of present rows before the row group's
// first row (in the column's row space), so the segment of g starts at value
// prefix[g] - skip[g].

// counts[g] = non-zero mask bytes in rows [rows[g], rows[g + 1]) (row n ends the last)
__global__ __launch_bounds__(kThreads) void rg_count_kernel(const uint8_t* __restrict__ mask, uint64_t n,
                                                             const int64_t* __restrict__ rows, uint64_t G,
                                                             int64_t* __restrict__ counts) {
  __shared__ uint32_t red[kThreads / kWave];
  const uint64_t g = blockIdx.x;
  uint64_t a = (uint64_t)rows[g], b = g + 1 < G ? (uint64_t)rows[g + 1] : n;
  if (a > n) a = n;
  if (b > n) b = n;
  uint32_t c = 0;
  if (b > a) {
    // 16-byte loads over the aligned middle, bytes at the two ends
    const uintptr_t pa = (uintptr_t)(mask + a), pb = (uintptr_t)(mask + b);
    const uintptr_t ma = (pa + 15) & ~(uintptr_t)15, mb = pb & ~(uintptr_t)15;
    if (ma < mb) {
      const u4* v = (const u4*)ma;
      const uint64_t nv = (uint64_t)(mb - ma) / 16;
      for (uint64_t k = threadIdx.x; k < nv; k += kThreads) c += nn_bytes_count(v[k]);
      for (uintptr_t q = pa + threadIdx.x; q < ma; q += kThreads) c += *(const uint8_t*)q != 0;
      for (uintptr_t q = mb + threadIdx.x; q < pb; q += kThreads) c += *(const uint8_t*)q != 0;
    } else {
      for (uint64_t r = a + threadIdx.x; r < b; r += kThreads) c += mask[r] != 0;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor((int)c, m);
  if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kThreads / kWave; ++w) t += red[w];
    counts[g] = (int64_t)(b > a ? t : 0);
  }
}

// seg[g] = {byte offset, first value index of the run at it}. trip[g] =
// {byte offset, values (bytes for boolean streams) to skip, bits to skip};
// prefix[g] = values (rows for boolean streams) before the row group.
__global__ void rg_segtab_kernel(const int64_t* __restrict__ trip, const int64_t* __restrict__ prefix, uint64_t G,
                                 int boolean, uint64_t* __restrict__ seg) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int64_t off = trip[3 * g], skip = trip[3 * g + 1], bits = trip[3 * g + 2];
  int64_t v = boolean ? (prefix[g] - bits) / 8 - skip : prefix[g] - skip;
  if (v < 0) v = 0;  // a corrupt index: the decode reports the segment mismatch
  seg[2 * g] = (uint64_t)off;
  seg[2 * g + 1] = (uint64_t)v;
}

// rg_count + scan + rg_segtab in one launch: tile t (a ticket) counts row
// group t's set mask bytes, looks back for the set rows before it (decoupled
// look-back over the row groups) and writes prefix[t] and segment t; the
// last row group also writes prefix[G]. (Three dependent launches per
// masked row-index stream before: ~16 us of a nullable column's chain.)
__global__ __launch_bounds__(kThreads) void rg_prefix_segtab_kernel(const uint8_t* __restrict__ mask, uint64_t n,
                                                                    const int64_t* __restrict__ rows, uint64_t G,
                                                                    const int64_t* __restrict__ trip, int boolean,
                                                                    int64_t* __restrict__ prefix,
                                                                    uint64_t* __restrict__ seg,
                                                                    unsigned long long* __restrict__ status,
                                                                    uint32_t epoch) {
  __shared__ uint32_t red[kThreads / kWave];
  __shared__ uint32_t s_t;
  const int tid = (int)threadIdx.x, lane = tid % kWave, wv = tid / kWave;
  if (tid == 0) s_t = lb_ticket(status, (uint32_t)G);
  __syncthreads();
  const uint32_t g = s_t;
  uint64_t a = (uint64_t)rows[g], b = g + 1 < G ? (uint64_t)rows[g + 1] : n;
  if (a > n) a = n;
  if (b > n) b = n;
  uint32_t c = 0;
  if (b > a) {
    const uintptr_t pa = (uintptr_t)(mask + a), pb = (uintptr_t)(mask + b);
    const uintptr_t ma = (pa + 15) & ~(uintptr_t)15, mb = pb & ~(uintptr_t)15;
    if (ma < mb) {
      const u4* v = (const u4*)ma;
      const uint64_t nv = (uint64_t)(mb - ma) / 16;
      for (uint64_t k = (uint64_t)tid; k < nv; k += kThreads) c += nn_bytes_count(v[k]);
      for (uintptr_t q = pa + tid; q < ma; q += kThreads) c += *(const uint8_t*)q != 0;
      for (uintptr_t q = mb + tid; q < pb; q += kThreads) c += *(const uint8_t*)q != 0;
    } else {
      for (uint64_t r = a + tid; r < b; r += kThreads) c += mask[r] != 0;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor((int)c, m);
  if (lane == 0) red[wv] = c;
  __syncthreads();
  if (wv == 0) {
    uint64_t agg = 0;
#pragma unroll
    for (int w = 0; w < kThreads / kWave; ++w) agg += red[w];
    uint64_t excl = 0;
    if (g == 0) {
      if (lane == 0) lb_publish(status, 0, 2, agg, epoch);
    } else {
      if (lane == 0) lb_publish(status, g, 1, agg, epoch);
      excl = lb_lookback(status, g, epoch, lane);
      if (lane == 0) lb_publish(status, g, 2, excl + agg, epoch);
    }
    if (lane == 0) {
      prefix[g] = (int64_t)excl;
      if (g + 1 == G) prefix[G] = (int64_t)(excl + agg);
      const int64_t off = trip[3 * g], skip = trip[3 * g + 1], bits = trip[3 * g + 2];
      int64_t v = boolean ? ((int64_t)excl - bits) / 8 - skip : (int64_t)excl - skip;
      if (v < 0) v = 0;  // a corrupt index: the decode reports the segment mismatch
      seg[2 * g] = (uint64_t)off;
      seg[2 * g + 1] = (uint64_t)v;
    }
  }
}

// child row group starts of a list / map column: offsets[parent rows[g]]
__global__ void rg_child_rows_kernel(const int64_t* __restrict__ offsets, const int64_t* __restrict__ rows,
                                     uint64_t G, int64_t* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) out[g] = offsets[rows[g]];
}

// ---- UNION (UnionColumnReader, c++/src/ColumnReader.cc:1158-1274) ----
// tags[j] (byte RLE DATA, one per non-null row) select the child; a row's
// offset is its rank among the rows with the same tag. flags[j] = tags[j] ==
// k feeds an exclusive scan per child; the first tag >= nchildren (lowest
// index) is kept as (index << 8 | tag) for getCheckedUnionTag's message.
__global__ void union_flags_kernel(const uint8_t* __restrict__ tags, uint64_t n, uint32_t k,
                                   int64_t* __restrict__ flags) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    flags[i] = tags[i] == k ? 1 : 0;
}

__global__ void union_check_kernel(const uint8_t* __restrict__ tags, uint64_t n, uint32_t nchildren,
                                   unsigned long long* first_bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long best = ~0ull;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    if (tags[i] >= nchildren) {
      best = (unsigned long long)i << 8 | tags[i];
      break;  // later rows of this thread cannot be earlier
    }
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(best, m);
    best = o < best ? o : best;
  }
  if ((threadIdx.x % kWave) == 0 && best != ~0ull) atomicMin(first_bad, best);
}

// offsets[j] = scan_k[j] for the rows with tag k
__global__ void union_offsets_kernel(const uint8_t* __restrict__ tags, uint64_t n, uint32_t k,
                                     const int64_t* __restrict__ scan_k, int64_t* __restrict__ offsets) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    if (tags[i] == k) offsets[i] = scan_k[i];
}

}  // namespace

// The context's look-back status words for `words` entries and a fresh
// epoch (a new buffer is zeroed; epochs wrap at 16 bits with one clear).
static int lb_status(Ctx* ctx, uint64_t words, unsigned long long** out, uint32_t* epoch) {
  words += 1;  // the ticket counter
  if (ctx->lb_cap < words) {
    if (ctx->d_lb) {
      int rc = hip_check(ctx, hipStreamSynchronize(ctx->stream), "look-back status sync");
      if (rc) return rc;
      (void)hipFree(ctx->d_lb);
      ctx->d_lb = nullptr;
      ctx->lb_cap = 0;
    }
    const uint64_t cap = std::max<uint64_t>(words + words / 4, 1u << 14);
    int rc = hip_check(ctx, hipMalloc(&ctx->d_lb, cap * 8), "hipMalloc look-back status");
    if (!rc) rc = hip_check(ctx, hipMemsetAsync(ctx->d_lb, 0, cap * 8, ctx->stream), "look-back status clear");
    if (rc) return rc;
    ctx->lb_cap = cap;
    ctx->lb_epoch = 0;
  }
  if (++ctx->lb_epoch > 0xffffu) {
    const int rc = hip_check(ctx, hipMemsetAsync(ctx->d_lb, 0, ctx->lb_cap * 8, ctx->stream), "look-back status clear");
    if (rc) return rc;
    ctx->lb_epoch = 1;
  }
  *out = (unsigned long long*)ctx->d_lb + 1;  // word 0: the ticket counter
  *epoch = ctx->lb_epoch;
  return ORCG_OK;
}

// 16-byte elements (Decimal128 values, orc::Int128 layout [hi, lo])
struct alignas(16) Pair128 {
  int64_t hi, lo;
  __host__ __device__ Pair128() : hi(0), lo(0) {}
  __host__ __device__ explicit Pair128(int64_t f) : hi(f < 0 ? -1 : 0), lo(f) {}
};

// Tile counts of the not-null bytes (kScratchTileCounts), then their exclusive
// scan (kScratchTileOffsets: tiles + 1 offsets, the last one the total).
static int launch_tile_offsets(Ctx* ctx, const uint8_t* d_nn, uint64_t n, uint64_t tiles, uint64_t** d_off) {
  if (tiles > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many rows");
  void *d_counts, *off;
  int rc = scratch(ctx, kScratchTileCounts, tiles * sizeof(uint32_t), &d_counts);
  if (!rc) rc = scratch(ctx, kScratchTileOffsets, (tiles + 1) * sizeof(uint64_t), &off);
  if (rc) return rc;
  hipLaunchKernelGGL(tile_count_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, ctx->stream, d_nn, n,
                     (uint32_t*)d_counts);
  hipLaunchKernelGGL((wg_scan_kernel<uint32_t, uint64_t, kScanCounts>), dim3(1), dim3(1024), 0, ctx->stream,
                     (const uint32_t*)d_counts, tiles, (uint64_t*)off, (unsigned long long*)nullptr,
                     (uint64_t*)nullptr);
  *d_off = (uint64_t*)off;
  return ORCG_OK;
}

int launch_scatter(Ctx* ctx, const void* d_dense, const uint8_t* d_nn, uint64_t n, void* d_out, int width,
                   int fill_mode, int64_t fill) {
  if (n == 0) return ORCG_OK;
  const uint64_t tiles = (n + kTile - 1) / kTile;
  uint64_t* d_off;
  const int rc = launch_tile_offsets(ctx, d_nn, n, tiles, &d_off);
  if (rc) return rc;
#define ORCG_SC(T)                                                                                     \
  do {                                                                                                 \
    if (fill_mode)                                                                                     \
      hipLaunchKernelGGL((scatter_kernel<T, true>), dim3((unsigned)tiles), dim3(kThreads), 0, ctx->stream, \
                         (const T*)d_dense, d_nn, n, d_off, (T*)d_out, (T)fill);      \
    else                                                                                               \
      hipLaunchKernelGGL((scatter_kernel<T, false>), dim3((unsigned)tiles), dim3(kThreads), 0, ctx->stream, \
                         (const T*)d_dense, d_nn, n, d_off, (T*)d_out, (T)fill);      \
  } while (0)
  switch (width) {
    case 16: ORCG_SC(Pair128); break;
    case 8: ORCG_SC(int64_t); break;
    case 4: ORCG_SC(int32_t); break;
    case 2: ORCG_SC(int16_t); break;
    case 1: ORCG_SC(int8_t); break;
    default: return set_error(ctx, ORCG_INVALID_ARGUMENT, "width must be 16, 8, 4, 2 or 1");
  }
#undef ORCG_SC
  return hip_check(ctx, hipGetLastError(), "scatter launch");
}

int launch_dict_offsets(Ctx* ctx, const int64_t* d_lengths, uint64_t dict_size, int64_t* d_offsets,
                        uint64_t* d_summary) {
  hipLaunchKernelGGL((wg_scan_kernel<int64_t, int64_t, kScanDict>), dim3(1), dim3(1024), 0, ctx->stream, d_lengths,
                     dict_size, d_offsets, (unsigned long long*)d_summary, (uint64_t*)nullptr);
  return hip_check(ctx, hipGetLastError(), "dictionary offsets launch");
}

int launch_dict_gather(Ctx* ctx, const void* d_idx, int idx_width, const uint8_t* d_nn, uint64_t n,
                       const int64_t* d_offsets, uint64_t dict_size, int64_t* d_start, int64_t* d_len) {
  if (n == 0) return ORCG_OK;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 256 * 16);
  if (idx_width == 8)
    hipLaunchKernelGGL(dict_gather_kernel<int64_t>, dim3(grid), dim3(256), 0, ctx->stream, (const int64_t*)d_idx,
                       d_nn, n, d_offsets, dict_size, d_start, d_len, ctx->d_err);
  else if (idx_width == 4)
    hipLaunchKernelGGL(dict_gather_kernel<int32_t>, dim3(grid), dim3(256), 0, ctx->stream, (const int32_t*)d_idx,
                       d_nn, n, d_offsets, dict_size, d_start, d_len, ctx->d_err);
  else
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "index width must be 8 or 4");
  return hip_check(ctx, hipGetLastError(), "dictionary gather launch");
}

int plan_dict_multi(Ctx* ctx, const DictJob* jobs, uint32_t njobs, std::vector<MultiLaunch>& out) {
  // one copy of the column's job per tile of kDictTile rows (tile_base = the
  // tile's index): a workgroup needs no search through the table
  std::vector<DictJob> g;
  for (uint32_t j = 0; j < njobs; ++j) {
    if (jobs[j].dict_size > kDictLds) return set_error(ctx, ORCG_INVALID_ARGUMENT, "dictionary too large for a batch");
    const uint64_t tiles = std::max<uint64_t>(1, (jobs[j].n + kDictTile - 1) / kDictTile);
    for (uint64_t t = 0; t < tiles; ++t) {
      g.push_back(jobs[j]);
      g.back().tile_base = t;
    }
  }
  if (g.empty()) return ORCG_OK;
  if (g.size() > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many rows");
  const void* d = nullptr;
  const int rc = stage_table(ctx, g.data(), g.size() * sizeof(DictJob), &d);
  if (rc) return rc;
  out.push_back(MultiLaunch{MultiLaunch::kDict, 0, d, (uint32_t)g.size(), g.size(), 0});
  return ORCG_OK;
}

int launch_dict_jobs(Ctx* ctx, const DictJob* d_jobs, uint32_t njobs, uint64_t tiles) {
  hipLaunchKernelGGL(dict_multi_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, ctx->stream, d_jobs, njobs);
  return hip_check(ctx, hipGetLastError(), "dict_multi_kernel launch");
}

int launch_dict_multi(Ctx* ctx, const DictJob* jobs, uint32_t njobs) {
  std::vector<MultiLaunch> ls;
  const int rc = plan_dict_multi(ctx, jobs, njobs, ls);
  return rc ? rc : run_multi(ctx, ls);
}

}  // namespace orcg

namespace orcg {

int launch_exclusive_scan(Ctx* ctx, const int64_t* d_in, uint64_t n, int64_t* d_out, uint64_t* d_flags,
                          uint64_t* d_total) {
  if (n == 0) {
    int rc = hip_check(ctx, hipMemsetAsync(d_out, 0, sizeof(int64_t), ctx->stream), "scan memset");
    if (!rc && d_total) rc = hip_check(ctx, hipMemsetAsync(d_total, 0, sizeof(uint64_t), ctx->stream), "scan memset");
    return rc;
  }
  unsigned long long* const fl = (unsigned long long*)d_flags;
  if (n <= 8192) {
    // short inputs (varint tile counts, dictionary lengths): one workgroup
    hipLaunchKernelGGL((wg_scan_kernel<uint64_t, uint64_t, kScanFlags>), dim3(1), dim3(1024), 0, ctx->stream,
                       (const uint64_t*)d_in, n, (uint64_t*)d_out, fl, d_total);
    return hip_check(ctx, hipGetLastError(), "scan launch");
  }
  const uint64_t tiles = (n + kScanTile - 1) / kScanTile;
  if (tiles > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many values");
  unsigned long long* d_status;
  uint32_t epoch;
  const int rc = lb_status(ctx, kLbWords * (tiles + 1), &d_status, &epoch);
  if (rc) return rc;
  hipLaunchKernelGGL(scan_lookback_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, ctx->stream, d_in, n, d_out,
                     d_status, (uint32_t)tiles, epoch, fl, d_total);
  return hip_check(ctx, hipGetLastError(), "scan launch");
}

int launch_count_nonzero(Ctx* ctx, const uint8_t* d_nn, uint64_t n, uint64_t* d_total) {
  if (n == 0) return hip_check(ctx, hipMemsetAsync(d_total, 0, sizeof(uint64_t), ctx->stream), "count memset");
  const uint64_t tiles = (n + kTile - 1) / kTile;
  uint64_t* d_off;
  int rc = launch_tile_offsets(ctx, d_nn, n, tiles, &d_off);
  if (rc) return rc;
  rc = hip_check(ctx, hipMemcpyAsync(d_total, d_off + tiles, sizeof(uint64_t), hipMemcpyDeviceToDevice,
                                     ctx->stream), "count copy");
  return rc ? rc : hip_check(ctx, hipGetLastError(), "count launch");
}

int launch_flag_negative(Ctx* ctx, const int64_t* d_v, uint64_t n, uint64_t* d_flag) {
  int rc = hip_check(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint64_t), ctx->stream), "flag memset");
  if (rc || n == 0) return rc;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(flag_negative_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_v, n,
                     (unsigned long long*)d_flag);
  return hip_check(ctx, hipGetLastError(), "flag launch");
}

// A small host -> device copy by the shader: the workgroups read the pinned,
// device-mapped source over PCIe and store to HBM. For the tens of KB of a
// small stripe's staging this starts sooner than a DMA-engine copy, whose
// hand-off to the compute queue cost ~15-20 us per stripe on configs[0].
__global__ __launch_bounds__(256) void pull_kernel(const u4* __restrict__ src, u4* __restrict__ dst, uint64_t n16) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * 256)
    dst[i] = __builtin_nontemporal_load(src + i);
}

int launch_pull(Ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes) {
  if (bytes == 0) return ORCG_OK;
  if (((uintptr_t)d_dst | (uintptr_t)h_src) & 15u)
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "pull copy needs 16-byte aligned buffers");
  const uint64_t n16 = (bytes + 15) / 16;  // (the staging is allocated past whole 16-byte words)
  const unsigned grid = (unsigned)std::min<uint64_t>((n16 + 1023) / 1024, 128);
  hipLaunchKernelGGL(pull_kernel, dim3(grid), dim3(256), 0, ctx->stream, (const u4*)h_src, (u4*)d_dst, n16);
  return hip_check(ctx, hipGetLastError(), "pull launch");
}

// Mid-stripe counts the host waits for (list / map totals): one thread
// copies them into coherent pinned memory, then stores the generation into
// the flag word with a system-scope release; the host spins on the flag
// instead of an 8-byte DMA per count and a stream synchronisation (whose
// interrupt-driven wake-up and the DMA hand-offs cost ~60 us between
// configs[4]'s decode levels).
__global__ void publish_kernel(PublishArgs a, uint64_t* __restrict__ dst, uint64_t* flag, uint64_t gen) {
  if (threadIdx.x != 0) return;
  for (uint32_t i = 0; i < a.n; ++i)
    __hip_atomic_store(dst + i, (uint64_t)*a.src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(flag, gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int launch_publish(Ctx* ctx, const PublishArgs& a, uint64_t* d_dst, uint64_t* d_flag, uint64_t gen) {
  if (a.n > kPublishMax) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many counts to publish");
  hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, ctx->stream, a, d_dst, d_flag, gen);
  return hip_check(ctx, hipGetLastError(), "publish launch");
}

int launch_widen(Ctx* ctx, const void* d_in, int kind, uint64_t n, void* d_out) {
  if (n == 0) return ORCG_OK;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 256 * 32);
  switch (kind) {
    case kWidenI8:
      hipLaunchKernelGGL((widen_kernel<int8_t, int64_t>), dim3(grid), dim3(256), 0, ctx->stream,
                         (const int8_t*)d_in, n, (int64_t*)d_out);
      break;
    case kWidenU8:
      hipLaunchKernelGGL((widen_kernel<uint8_t, int64_t>), dim3(grid), dim3(256), 0, ctx->stream,
                         (const uint8_t*)d_in, n, (int64_t*)d_out);
      break;
    case kWidenF32:
      hipLaunchKernelGGL((widen_kernel<float, double>), dim3(grid), dim3(256), 0, ctx->stream, (const float*)d_in,
                         n, (double*)d_out);
      break;
    default:
      return set_error(ctx, ORCG_INVALID_ARGUMENT, "bad widen kind");
  }
  return hip_check(ctx, hipGetLastError(), "widen launch");
}

}  // namespace orcg

namespace orcg {

int launch_rg_prefix(Ctx* ctx, const uint8_t* d_mask, uint64_t n, const int64_t* d_rows, uint64_t G,
                     int64_t* d_counts, int64_t* d_prefix) {
  if (G == 0) return ORCG_OK;
  if (G > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many row groups");
  hipLaunchKernelGGL(rg_count_kernel, dim3((unsigned)G), dim3(kThreads), 0, ctx->stream, d_mask, n, d_rows, G,
                     d_counts);
  const int rc = hip_check(ctx, hipGetLastError(), "rg_count_kernel launch");
  return rc ? rc : launch_exclusive_scan(ctx, d_counts, G, d_prefix);
}

int launch_rg_segtab(Ctx* ctx, const int64_t* d_trip, const int64_t* d_prefix, uint64_t G, bool boolean,
                     uint64_t* d_seg) {
  if (G == 0) return ORCG_OK;
  hipLaunchKernelGGL(rg_segtab_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, ctx->stream, d_trip,
                     d_prefix, G, boolean ? 1 : 0, d_seg);
  return hip_check(ctx, hipGetLastError(), "rg_segtab_kernel launch");
}

int launch_rg_prefix_segtab(Ctx* ctx, const uint8_t* d_mask, uint64_t n, const int64_t* d_rows, uint64_t G,
                            const int64_t* d_trip, bool boolean, int64_t* d_prefix, uint64_t* d_seg) {
  if (G == 0) return ORCG_OK;
  if (G > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many row groups");
  unsigned long long* d_status;
  uint32_t epoch;
  const int rc = lb_status(ctx, kLbWords * (G + 1), &d_status, &epoch);
  if (rc) return rc;
  hipLaunchKernelGGL(rg_prefix_segtab_kernel, dim3((unsigned)G), dim3(kThreads), 0, ctx->stream, d_mask, n, d_rows, G,
                     d_trip, boolean ? 1 : 0, d_prefix, d_seg, d_status, epoch);
  return hip_check(ctx, hipGetLastError(), "rg_prefix_segtab_kernel launch");
}

int launch_rg_child_rows(Ctx* ctx, const int64_t* d_offsets, const int64_t* d_rows, uint64_t G, int64_t* d_out) {
  if (G == 0) return ORCG_OK;
  hipLaunchKernelGGL(rg_child_rows_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, ctx->stream, d_offsets,
                     d_rows, G, d_out);
  return hip_check(ctx, hipGetLastError(), "rg_child_rows_kernel launch");
}

int launch_union_flags(Ctx* ctx, const uint8_t* d_tags, uint64_t n, uint32_t k, int64_t* d_flags) {
  if (n == 0) return ORCG_OK;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(union_flags_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_tags, n, k, d_flags);
  return hip_check(ctx, hipGetLastError(), "union_flags_kernel launch");
}

int launch_union_check(Ctx* ctx, const uint8_t* d_tags, uint64_t n, uint32_t nchildren, uint64_t* d_first_bad) {
  int rc = hip_check(ctx, hipMemsetAsync(d_first_bad, 0xff, sizeof(uint64_t), ctx->stream), "union memset");
  if (rc || n == 0) return rc;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(union_check_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_tags, n, nchildren,
                     (unsigned long long*)d_first_bad);
  return hip_check(ctx, hipGetLastError(), "union_check_kernel launch");
}

int launch_union_offsets(Ctx* ctx, const uint8_t* d_tags, uint64_t n, uint32_t k, const int64_t* d_scan_k,
                         int64_t* d_offsets) {
  if (n == 0) return ORCG_OK;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(union_offsets_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_tags, n, k, d_scan_k,
                     d_offsets);
  return hip_check(ctx, hipGetLastError(), "union_offsets_kernel launch");
}

}  // namespace orcg

// A no-op launch that makes HIP load this file's code object (warm_modules).
namespace orcg {
namespace {
__global__ void warm_columns_kernel() {}
}  // namespace
void warm_columns(hipStream_t s) { hipLaunchKernelGGL(warm_columns_kernel, dim3(1), dim3(64), 0, s); }
}  // namespace orcg
