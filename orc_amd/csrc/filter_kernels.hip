// Row-level filter kernels (gfx950): a SearchArgument's leaves and expression
// over a decoded stripe's columns in HBM, the selection vector
// (VectorizedRowBatch.selected: ascending row indices) and the gather of the
// selected rows. Truth rules: java/core/src/java/org/apache/orc/impl/filter/
// LeafFilter.java:41-84 and leaf/*.java, restated in tests/filter_model.py.
//
//   string_leaf_kernel   one truth byte per row of a direct string column, or
//                        per entry of a dictionary (then looked up per row)
//   combine_kernel       the whole program per row in registers: numeric,
//                        date, boolean and decimal leaves read their column,
//                        string leaves their truth byte; selected byte per
//                        row, selected count per tile (ballot + popcount)
//   select_kernel        tile bases (launch_exclusive_scan) -> selected[]
//   gather_kernel        selected rows of a column's arrays and mask
#include "device_util.hh"
#include "filter_internal.hh"

namespace orcg {
namespace filter {

namespace {

using dev::kWave;
constexpr int kThreads = 256;
constexpr int kRows = kTile / kThreads;
static_assert(kRows == 4, "select_kernel reads a lane's rows as one 32-bit word");

struct alignas(16) I128 {
  int64_t hi;
  uint64_t lo;
};
struct alignas(16) Quad {
  uint64_t a, b;
};

__device__ __forceinline__ int cmp128(int64_t ah, uint64_t al, int64_t bh, uint64_t bl) {
  if (ah != bh) return ah < bh ? -1 : 1;
  return al < bl ? -1 : (al > bl ? 1 : 0);
}

// Double.compare's order (filter_plan.hh double_key)
__device__ __forceinline__ int64_t dkey(double v) {
  uint64_t b = (uint64_t)__double_as_longlong(v);
  if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
  return (int64_t)(b ^ (((uint64_t)((int64_t)b >> 63)) >> 1));
}

__device__ __forceinline__ bool in_i64(const int64_t* __restrict__ w, uint32_t n, int64_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (w[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && w[lo] == v;
}

__device__ __forceinline__ bool in_i128(const int64_t* __restrict__ w, uint32_t n, int64_t vh, uint64_t vl) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cmp128(w[2 * mid], (uint64_t)w[2 * mid + 1], vh, vl) < 0) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && w[2 * lo] == vh && (uint64_t)w[2 * lo + 1] == vl;
}

// YES / NO / NULL of leaf L on `row` (L and w are wave-uniform)
__device__ __forceinline__ uint32_t eval_leaf(const DevLeaf& L, const int64_t* __restrict__ w, uint64_t row) {
  if (L.nn && !L.nn[row]) return L.op == kIsNull ? kTruthYes : kTruthNull;
  if (L.op == kIsNull) return kTruthNo;
  bool yes = false;
  switch (L.cls) {
    case kDevI64: {
      const int64_t v = ((const int64_t*)L.data)[row];
      switch (L.op) {
        case kEquals: yes = v == w[0]; break;
        case kLessThan: yes = v < w[0]; break;
        case kLessThanEquals: yes = v <= w[0]; break;
        case kBetween: yes = w[0] <= v && v <= w[1]; break;
        default: yes = in_i64(w, L.nlit, v); break;
      }
      break;
    }
    case kDevF64: {
      const double v = ((const double*)L.data)[row];
      const double a = __longlong_as_double(w[0]);
      switch (L.op) {
        case kEquals: yes = v == a; break;
        case kLessThan: yes = v < a; break;
        case kLessThanEquals: yes = v <= a; break;
        case kBetween: yes = a <= v && v <= __longlong_as_double(w[1]); break;
        default: yes = in_i64(w, L.nlit, dkey(v)); break;
      }
      break;
    }
    case kDevDec128: {
      const I128 v = ((const I128*)L.data)[row];
      if (L.op == kIn) {
        yes = in_i128(w, L.nlit, v.hi, v.lo);
      } else {
        const int c = cmp128(v.hi, v.lo, w[0], (uint64_t)w[1]);
        switch (L.op) {
          case kEquals: yes = c == 0; break;
          case kLessThan: yes = c < 0; break;
          case kLessThanEquals: yes = c <= 0; break;
          default: yes = c >= 0 && cmp128(v.hi, v.lo, w[2], (uint64_t)w[3]) <= 0; break;
        }
      }
      break;
    }
    case kDevTruth: return ((const uint8_t*)L.data)[row];
    case kDevTruthDict: {
      // (a null row never gets here: its index is not read)
      const uint64_t e = (uint64_t)L.index[row];
      return e < L.dict_size ? ((const uint8_t*)L.data)[e] : kTruthNo;
    }
    default: break;
  }
  return yes ? kTruthYes : kTruthNo;
}

// Lane t of tile b evaluates rows b * kTile + j * kThreads + t, j < kRows: a
// wave reads 512 contiguous bytes of an 8-byte column per j. The evaluation
// stack of a row is one 32-bit register, 2 bits an entry (kMaxDepth = 16);
// the program and the leaf table are read through scalar loads.
__global__ __launch_bounds__(kThreads) void combine_kernel(const DevLeaf* __restrict__ leaves,
                                                            const uint32_t* __restrict__ ops, uint32_t nops,
                                                            const int64_t* __restrict__ words, uint64_t n,
                                                            uint8_t* __restrict__ sel, int64_t* __restrict__ tile_counts) {
  __shared__ uint32_t wave_count[kThreads / kWave];
  const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint32_t stk[kRows];
#pragma unroll
  for (int j = 0; j < kRows; ++j) stk[j] = 0;
  for (uint32_t p = 0; p < nops; ++p) {
    const uint32_t op = ops[p];
    const uint32_t kind = op & 3, arg = op >> 8;
    if (kind == kLeaf) {
      const DevLeaf L = leaves[arg];
      const int64_t* w = words + L.lit0;
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        const uint64_t row = base + (uint64_t)j * kThreads;
        uint32_t t = row < n ? eval_leaf(L, w, row) : kTruthNo;
        if (op & kOpNeg) t = 2 - t;
        stk[j] = (stk[j] << 2) | t;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        uint32_t s = stk[j] >> 2, acc = stk[j] & 3;
        for (uint32_t k = 1; k < arg; ++k) {
          const uint32_t t = s & 3;
          s >>= 2;
          acc = kind == kAnd ? min(acc, t) : max(acc, t);
        }
        stk[j] = (s << 2) | acc;
      }
    }
  }
  uint32_t count = 0;
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const uint64_t row = base + (uint64_t)j * kThreads;
    const bool yes = row < n && (stk[j] & 3) == kTruthYes;
    sel[row] = yes ? 1 : 0;  // (sel covers whole tiles)
    count += (uint32_t)__popcll(__ballot(yes));
  }
  if ((threadIdx.x & (kWave - 1)) == 0) wave_count[threadIdx.x / kWave] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (int k = 0; k < kThreads / kWave; ++k) total += wave_count[k];
    tile_counts[blockIdx.x] = total;
  }
}

// Lane t of tile b owns rows b * kTile + 4 t .. + 3: its selected bytes are one
// aligned 32-bit word, and lane order is row order.
__global__ __launch_bounds__(kThreads) void select_kernel(const uint8_t* __restrict__ sel,
                                                           const int64_t* __restrict__ tile_base,
                                                           int64_t* __restrict__ selected) {
  __shared__ uint32_t wave_total[kThreads / kWave];
  const uint64_t row0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kRows;
  const uint32_t word = *(const uint32_t*)(sel + row0) & 0x01010101u;
  const uint32_t c = (uint32_t)__popc(word);
  const uint32_t incl = dev::wave_scan_u32(c);
  const uint32_t wave = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == kWave - 1) wave_total[wave] = incl;
  __syncthreads();
  uint64_t pos = (uint64_t)tile_base[blockIdx.x] + incl - c;
  for (uint32_t k = 0; k < wave; ++k) pos += wave_total[k];
#pragma unroll
  for (int k = 0; k < kRows; ++k)
    if (word >> (8 * k) & 1) selected[pos++] = (int64_t)(row0 + k);
}

__device__ __forceinline__ int cmp_bytes(const uint8_t* __restrict__ a, uint64_t alen, const uint8_t* __restrict__ b,
                                         uint64_t blen) {
  // unsigned bytes over the common prefix, then the shorter first (StringExpr.compare)
  const uint64_t m = alen < blen ? alen : blen;
  for (uint64_t i = 0; i < m; ++i) {
    const uint32_t x = a[i], y = b[i];
    if (x != y) return x < y ? -1 : 1;
  }
  return alen < blen ? -1 : (alen > blen ? 1 : 0);
}

// A lane per element. A row compares at most min(its length, the literal's)
// bytes, so a 100 KB row costs what its literal is long.
__global__ __launch_bounds__(kThreads) void string_leaf_kernel(StringLeafArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= a.n) return;
  int64_t s, len;
  if (a.dict_offsets) {
    s = a.dict_offsets[e];
    len = a.dict_offsets[e + 1] - s;
  } else {
    if (a.nn && !a.nn[e]) {
      a.truth[e] = kTruthNo;
      return;
    }
    s = a.start[e];
    len = a.length[e];
  }
  bool yes = false;
  if (s >= 0 && len >= 0 && (uint64_t)s <= a.blob_len && (uint64_t)len <= a.blob_len - (uint64_t)s) {
    const uint8_t* row = a.blob + s;
    auto lit = [&](uint32_t k, uint64_t* ll) {
      *ll = a.lit_off[k + 1] - a.lit_off[k];
      return a.lit_bytes + a.lit_off[k];
    };
    uint64_t ll;
    const uint8_t* l0 = lit(0, &ll);
    switch (a.op) {
      case kEquals: yes = (uint64_t)len == ll && cmp_bytes(row, len, l0, ll) == 0; break;
      case kLessThan: yes = cmp_bytes(row, len, l0, ll) < 0; break;
      case kLessThanEquals: yes = cmp_bytes(row, len, l0, ll) <= 0; break;
      case kBetween:
        if (cmp_bytes(row, len, l0, ll) >= 0) {
          const uint8_t* l1 = lit(1, &ll);
          yes = cmp_bytes(row, len, l1, ll) <= 0;
        }
        break;
      default: {  // IN: the list is sorted in cmp_bytes' order
        uint32_t lo = 0, hi = a.nlit;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          const uint8_t* lm = lit(mid, &ll);
          const int c = cmp_bytes(lm, ll, row, len);
          if (c == 0) {
            yes = true;
            break;
          }
          if (c < 0) lo = mid + 1;
          else hi = mid;
        }
        break;
      }
    }
  }
  a.truth[e] = yes ? kTruthYes : kTruthNo;
}

__global__ __launch_bounds__(kThreads) void gather_kernel(GatherArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  bool null_row = false;
  if (i < a.count) {
    const uint64_t r = (uint64_t)a.sel[i];
    const bool ok = r < a.n_src;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (a.src8[k]) a.dst8[k][i] = ok ? a.src8[k][r] : 0;
    if (a.src16) ((Quad*)a.dst16)[i] = ok ? ((const Quad*)a.src16)[r] : Quad{0, 0};
    if (a.nn) {
      const uint8_t m = ok ? a.nn[r] : 0;
      a.out_nn[i] = m;
      null_row = m == 0;
    }
  }
  const uint64_t b = __ballot(null_row);
  if (a.nulls && b && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(a.nulls, (unsigned long long)__popcll(b));
}

}  // namespace

int launch_string_leaf(Ctx* ctx, const StringLeafArgs& a) {
  if (a.n == 0) return ORCG_OK;
  const uint64_t grid = (a.n + kThreads - 1) / kThreads;
  if (grid > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many values");
  hipLaunchKernelGGL(string_leaf_kernel, dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, a);
  return hip_check(ctx, hipGetLastError(), "string leaf launch");
}

int launch_combine(Ctx* ctx, const DevLeaf* d_leaves, const uint32_t* d_ops, uint32_t nops, const int64_t* d_words,
                   uint64_t n, uint8_t* d_sel, int64_t* d_tile_counts) {
  const uint64_t tiles = (n + kTile - 1) / kTile;
  if (tiles == 0) return ORCG_OK;
  if (tiles > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many values");
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, ctx->stream, d_leaves, d_ops, nops,
                     d_words, n, d_sel, d_tile_counts);
  return hip_check(ctx, hipGetLastError(), "filter combine launch");
}

int launch_select(Ctx* ctx, const uint8_t* d_sel, uint64_t tiles, const int64_t* d_tile_base, int64_t* d_selected) {
  if (tiles == 0) return ORCG_OK;
  if (tiles > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many values");
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, ctx->stream, d_sel, d_tile_base, d_selected);
  return hip_check(ctx, hipGetLastError(), "filter select launch");
}

int launch_gather(Ctx* ctx, const GatherArgs& a) {
  if (a.count == 0) return ORCG_OK;
  const uint64_t grid = (a.count + kThreads - 1) / kThreads;
  if (grid > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many values");
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, a);
  return hip_check(ctx, hipGetLastError(), "filter gather launch");
}

}  // namespace filter
}  // namespace orcg
