// Arrow export (gfx950): a decoded column's batch layout re-laid in HBM into
// Arrow's (include/orcg_arrow.h), so that what leaves the
// device is the narrow form.
//
//   validity_kernel       not_null bytes -> LSB-first bitmap + null count
//   fixed_kernel<form>    int64 -> int8 / int16 / int32, double -> float32,
//                         Decimal64 -> 16 bytes, Decimal128 [hi, lo] -> [lo, hi],
//                         (seconds, nanos) -> nanoseconds
//   bool_kernel           int64 (value != 0) -> bitmap
//   row_lengths_kernel    masked string lengths (direct or through a dictionary)
//   narrow_offsets_kernel int64 offsets -> int32 with the range check
//   dict_gather_kernel    a dictionary column's row bytes, gathered contiguously
//
// Shape: 256 threads; the elementwise kernels take one item a lane per trip of
// a grid-stride loop (the grid is capped), an item being what makes the lane's
// global accesses 8 or 16 bytes wide: 16 mask bytes -> 2 bitmap bytes, 8 / 4 / 2
// int64 -> 8 bytes of int8 / int16 / int32, 2 doubles -> 8 bytes of float, 2
// Decimal64 -> 32 bytes, 1 Decimal128 -> 16 bytes, 2 + 2 int64 -> 16 bytes of
// nanoseconds. The last items of a column (past n, or when a pointer is not
// 16-byte aligned) go element by element and write the buffer's zero padding.
// Null counts: summed per wave after the wave's last item (as convert_kernel),
// then per workgroup, one atomic a workgroup. No per-row atomics, no scratch.
#include "arrow_internal.hh"
#include "device_util.hh"

namespace orcg {
namespace arrow {
namespace {

using dev::report;
using dev::wave_sum;

constexpr int kThreads = 256;
constexpr uint64_t kMaxBlocks = 2048;  // eight workgroups a compute unit; larger columns loop
constexpr unsigned kValidityBlocks = 512;

__device__ __forceinline__ uint64_t first_item() { return (uint64_t)blockIdx.x * kThreads + threadIdx.x; }
__device__ __forceinline__ uint64_t item_stride() { return (uint64_t)gridDim.x * kThreads; }

// bit k = byte k of w is not 0
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w) {
  // the byte's high bit = the byte is not 0 (no carry leaves a byte: 0x7f + 0x7f < 0x100)
  const uint32_t t = (w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
  // bits 0, 8, 16, 24 gathered into bits 24..27: bit 8k lands on 24 + k by the
  // term 2^(24 - 7k); no two products share a position, so nothing carries
  return ((t >> 7) * 0x01020408u) >> 24;
}

__global__ __launch_bounds__(kThreads) void validity_kernel(const uint8_t* __restrict__ nn, uint64_t n,
                                                            uint16_t* __restrict__ bitmap, uint64_t items, int vec,
                                                            unsigned long long* nulls_out) {
  uint32_t nulls = 0;
  for (uint64_t i = first_item(); i < items; i += item_stride()) {
    const uint64_t row = i * 16;
    uint32_t bits = 0, rows = 0;
    if (vec && row + 16 <= n) {
      const uint4 v = *(const uint4*)(nn + row);
      bits = nonzero_bytes(v.x) | nonzero_bytes(v.y) << 4 | nonzero_bytes(v.z) << 8 | nonzero_bytes(v.w) << 12;
      rows = 16;
    } else if (row < n) {
      rows = (uint32_t)(n - row < 16 ? n - row : 16);
      for (uint32_t k = 0; k < rows; ++k) bits |= (uint32_t)(nn[row + k] != 0) << k;
    }
    bitmap[i] = (uint16_t)bits;  // (past n: the padding's zeros)
    nulls += rows - __popc(bits);
  }
  // every lane is back here: the wave's null rows summed, the workgroup's
  // four sums added in LDS, one atomic a workgroup. (One atomic a wave, as
  // convert_kernel has it, cost 94 us at 10^7 rows: 8,192 adds to one word at
  // about 11 ns each, against 2 us of traffic)
  __shared__ uint32_t s_nulls[kThreads / dev::kWave];
  nulls = wave_sum(nulls);
  if ((threadIdx.x & (dev::kWave - 1)) == 0) s_nulls[threadIdx.x / dev::kWave] = nulls;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
    for (int w = 0; w < kThreads / dev::kWave; ++w) sum += s_nulls[w];
    if (sum) atomicAdd(nulls_out, (unsigned long long)sum);
  }
}

struct FixedArgs {
  const void* src;
  const void* src2;
  void* out;
  uint64_t n;   // values
  uint64_t pn;  // values the output buffer holds with its padding
  int vec;      // every pointer is 16-byte aligned
};

// values an item (one lane, one trip) takes
template <int kForm>
constexpr int per_item() {
  return kForm == ORCG_ARROW_INT8 ? 8 : kForm == ORCG_ARROW_INT16 ? 4 : kForm == ORCG_ARROW_DEC128 ? 1 : 2;
}

// seconds * 10^9 + nanos modulo 2^64
__device__ __forceinline__ int64_t to_nanos(int64_t s, int64_t ns) {
  return (int64_t)((uint64_t)s * 1000000000ull + (uint64_t)ns);
}

// element e alone (live: e < n, else the padding's zero)
template <int kForm>
__device__ __forceinline__ void fixed_one(const FixedArgs& a, uint64_t e, bool live) {
  const int64_t* s = (const int64_t*)a.src;
  if constexpr (kForm == ORCG_ARROW_INT8) ((int8_t*)a.out)[e] = live ? (int8_t)s[e] : 0;
  if constexpr (kForm == ORCG_ARROW_INT16) ((int16_t*)a.out)[e] = live ? (int16_t)s[e] : 0;
  if constexpr (kForm == ORCG_ARROW_INT32) ((int32_t*)a.out)[e] = live ? (int32_t)s[e] : 0;
  if constexpr (kForm == ORCG_ARROW_FLOAT32) ((float*)a.out)[e] = live ? (float)((const double*)a.src)[e] : 0.0f;
  if constexpr (kForm == ORCG_ARROW_DEC64) {
    const int64_t v = live ? s[e] : 0;
    ((longlong2*)a.out)[e] = make_longlong2(v, v >> 63);
  }
  if constexpr (kForm == ORCG_ARROW_DEC128)
    ((longlong2*)a.out)[e] = live ? make_longlong2(s[2 * e + 1], s[2 * e]) : make_longlong2(0, 0);
  if constexpr (kForm == ORCG_ARROW_TIMESTAMP_NS)
    ((int64_t*)a.out)[e] = live ? to_nanos(s[e], ((const int64_t*)a.src2)[e]) : 0;
}

template <int kForm>
__global__ __launch_bounds__(kThreads) void fixed_kernel(const FixedArgs a) {
  constexpr int kPer = per_item<kForm>();
  const uint64_t items = (a.pn + kPer - 1) / kPer;
  for (uint64_t i = first_item(); i < items; i += item_stride()) {
    const uint64_t e = i * kPer;
    if (a.vec && e + kPer <= a.n) {
      const longlong2* s = (const longlong2*)a.src + (kForm == ORCG_ARROW_DEC128 ? e : e / 2);
      if constexpr (kForm == ORCG_ARROW_INT8) {
        const longlong2 v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3];
        const uint32_t lo = ((uint32_t)v0.x & 0xff) | ((uint32_t)v0.y & 0xff) << 8 | ((uint32_t)v1.x & 0xff) << 16 |
                            ((uint32_t)v1.y & 0xff) << 24;
        const uint32_t hi = ((uint32_t)v2.x & 0xff) | ((uint32_t)v2.y & 0xff) << 8 | ((uint32_t)v3.x & 0xff) << 16 |
                            ((uint32_t)v3.y & 0xff) << 24;
        ((uint2*)a.out)[i] = make_uint2(lo, hi);
      }
      if constexpr (kForm == ORCG_ARROW_INT16) {
        const longlong2 v0 = s[0], v1 = s[1];
        ((uint2*)a.out)[i] = make_uint2(((uint32_t)v0.x & 0xffff) | ((uint32_t)v0.y & 0xffff) << 16,
                                        ((uint32_t)v1.x & 0xffff) | ((uint32_t)v1.y & 0xffff) << 16);
      }
      if constexpr (kForm == ORCG_ARROW_INT32) {
        const longlong2 v = s[0];
        ((uint2*)a.out)[i] = make_uint2((uint32_t)v.x, (uint32_t)v.y);
      }
      if constexpr (kForm == ORCG_ARROW_FLOAT32) {
        const double2 v = ((const double2*)a.src)[i];
        ((float2*)a.out)[i] = make_float2((float)v.x, (float)v.y);
      }
      if constexpr (kForm == ORCG_ARROW_DEC64) {
        const longlong2 v = s[0];
        ((longlong2*)a.out)[e] = make_longlong2(v.x, v.x >> 63);
        ((longlong2*)a.out)[e + 1] = make_longlong2(v.y, v.y >> 63);
      }
      if constexpr (kForm == ORCG_ARROW_DEC128) {
        const longlong2 v = s[0];  // [hi, lo]
        ((longlong2*)a.out)[e] = make_longlong2(v.y, v.x);
      }
      if constexpr (kForm == ORCG_ARROW_TIMESTAMP_NS) {
        const longlong2 v = s[0], ns = ((const longlong2*)a.src2)[i];
        ((longlong2*)a.out)[i] = make_longlong2(to_nanos(v.x, ns.x), to_nanos(v.y, ns.y));
      }
    } else {
      for (int k = 0; k < kPer; ++k)
        if (e + k < a.pn) fixed_one<kForm>(a, e + k, e + k < a.n);
    }
  }
}

// int64 values -> bitmap, a byte (eight values) a lane
__global__ __launch_bounds__(kThreads) void bool_kernel(const int64_t* __restrict__ src, uint64_t n,
                                                        uint8_t* __restrict__ out, uint64_t out_bytes, int vec) {
  for (uint64_t i = first_item(); i < out_bytes; i += item_stride()) {
    const uint64_t row = i * 8;
    uint32_t bits = 0;
    if (vec && row + 8 <= n) {
      const longlong2* s = (const longlong2*)(src + row);
      const longlong2 v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3];
      bits = (uint32_t)(v0.x != 0) | (uint32_t)(v0.y != 0) << 1 | (uint32_t)(v1.x != 0) << 2 |
             (uint32_t)(v1.y != 0) << 3 | (uint32_t)(v2.x != 0) << 4 | (uint32_t)(v2.y != 0) << 5 |
             (uint32_t)(v3.x != 0) << 6 | (uint32_t)(v3.y != 0) << 7;
    } else {
      for (uint32_t k = 0; k < 8; ++k)
        if (row + k < n) bits |= (uint32_t)(src[row + k] != 0) << k;
    }
    out[i] = (uint8_t)bits;
  }
}

__global__ __launch_bounds__(kThreads) void row_lengths_kernel(const int64_t* __restrict__ lengths,
                                                               const int64_t* __restrict__ index,
                                                               const int64_t* __restrict__ dict_offsets,
                                                               uint64_t dict_size, const uint8_t* __restrict__ nn,
                                                               uint64_t n, int64_t* __restrict__ out,
                                                               unsigned long long* err) {
  for (uint64_t i = first_item(); i < n; i += item_stride()) {
    int64_t len = 0;
    if (!nn || nn[i]) {
      if (index) {
        const uint64_t e = (uint64_t)index[i];
        if (e < dict_size) len = dict_offsets[e + 1] - dict_offsets[e];
        else report(err, i, kArrowDictIndex);
      } else {
        len = lengths[i];
      }
    }
    out[i] = len < 0 ? 0 : len;
  }
}

__global__ __launch_bounds__(kThreads) void narrow_offsets_kernel(const int64_t* __restrict__ in, uint64_t count,
                                                                  int32_t* __restrict__ out, uint64_t pn, int vec,
                                                                  unsigned long long* err) {
  const uint64_t items = (pn + 1) / 2;
  for (uint64_t i = first_item(); i < items; i += item_stride()) {
    const uint64_t e = 2 * i;
    if (vec && e + 2 <= count) {
      const longlong2 v = ((const longlong2*)in)[i];
      ((int2*)out)[i] = make_int2((int32_t)v.x, (int32_t)v.y);
    } else {
      for (int k = 0; k < 2; ++k)
        if (e + k < pn) out[e + k] = e + k < count ? (int32_t)in[e + k] : 0;
    }
    // offsets never decrease: the last one bounds them all
    if (e + 2 >= count && e < count) {
      const int64_t last = in[count - 1];
      if (last < 0 || last > 0x7fffffffll) report(err, count - 1, kArrowOffsetRange);
    }
  }
}

// Gather by output bytes: a workgroup takes tiles of 4,096 output bytes, a
// lane one aligned 16-byte chunk of the tile, stored with one 16-byte store
// (a wave's store is 1 KiB contiguous). The rows under a tile are found once a
// tile (two binary searches over the offsets, by two lanes) and their offsets
// staged in LDS; each lane then finds its chunk's first row by a binary search
// in LDS and walks the rows its 16 bytes cross (empty and null rows have no
// bytes and are stepped over). A tile with more rows than the stage holds
// (runs of empty rows, or one-byte rows) searches the offsets in global memory
// instead. Dictionary bytes are read with unaligned 8-byte loads: they are read
// many times over and stay in L2; the new traffic is the output.
constexpr uint32_t kGatherTile = kThreads * 16;
constexpr uint32_t kGatherRows = 2048;

struct GatherArgs {
  const int32_t* offsets;  // n + 1 output offsets
  const int64_t* index;
  const int64_t* dict_offsets;
  const uint8_t* blob;
  uint8_t* out;
  uint64_t n, dict_size, blob_len;
  uint64_t total, out_bytes;  // offsets[n] and its padded size
};

__global__ __launch_bounds__(kThreads) void dict_gather_kernel(const GatherArgs a) {
  __shared__ int32_t s_off[kGatherRows + 1];
  __shared__ uint64_t s_range[2];
  const uint64_t tiles = (a.out_bytes + kGatherTile - 1) / kGatherTile;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t tb = tile * kGatherTile;
    const uint64_t te = tb + kGatherTile < a.total ? tb + kGatherTile : a.total;
    __syncthreads();  // the last tile's reads of the stage are over
    if (threadIdx.x == 0) {
      // the row holding byte tb: the last r with offsets[r] <= tb (r < n, as
      // offsets[n] = total > tb); a tile of padding alone has no rows
      uint64_t l = 0, h = a.n;  // offsets[l] <= tb < offsets[h]
      while (tb < a.total && h - l > 1) {
        const uint64_t m = l + (h - l) / 2;
        if ((uint64_t)(uint32_t)a.offsets[m] <= tb) l = m;
        else h = m;
      }
      s_range[0] = tb < a.total ? l : a.n;
    }
    if (threadIdx.x == dev::kWave) {
      // the first r with offsets[r] >= te (offsets[n] = total >= te)
      uint64_t l = 0, h = a.n;  // offsets[h] >= te throughout; rows before l are below te
      while (l < h) {
        const uint64_t m = l + (h - l) / 2;
        if ((uint64_t)(uint32_t)a.offsets[m] >= te) h = m;
        else l = m + 1;
      }
      s_range[1] = h;
    }
    __syncthreads();
    const uint64_t lo = s_range[0], hi = s_range[1] > lo ? s_range[1] : lo;
    const bool staged = hi - lo <= kGatherRows;
    if (staged)
      for (uint64_t k = threadIdx.x; k <= hi - lo && lo + k <= a.n; k += kThreads) s_off[k] = a.offsets[lo + k];
    __syncthreads();
    auto off = [&](uint64_t r) -> uint64_t { return (uint64_t)(uint32_t)(staged ? s_off[r - lo] : a.offsets[r]); };

    const uint64_t cb = tb + (uint64_t)threadIdx.x * 16;
    if (cb >= a.out_bytes) continue;
    uint64_t w0 = 0, w1 = 0;
    if (cb < te) {
      // the last row of [lo, hi) whose offset is <= cb (off(lo) <= tb <= cb, off(hi) >= te > cb)
      uint64_t l = lo, h = hi;
      while (h - l > 1) {
        const uint64_t m = l + (h - l) / 2;
        if (off(m) <= cb) l = m;
        else h = m;
      }
      uint64_t r = l, p = cb;
      const uint64_t end = cb + 16 < te ? cb + 16 : te;
      while (p < end && r < hi) {
        const uint64_t rend = off(r + 1);
        if (rend <= p) {
          ++r;
          continue;
        }
        const uint64_t e = (uint64_t)a.index[r];
        const uint64_t src = e < a.dict_size ? (uint64_t)a.dict_offsets[e] + (p - off(r)) : a.blob_len;
        const uint64_t stop = rend < end ? rend : end;
        // the row's bytes under this chunk, eight at a time where the
        // dictionary has eight left (an unaligned 8-byte load), else one
        const uint64_t left = stop - p;
        for (uint64_t k = 0; k < left;) {
          uint64_t part = 0;
          uint32_t got = 1;
          if (src + k + 8 <= a.blob_len) {
            __builtin_memcpy(&part, a.blob + src + k, 8);
            got = (uint32_t)(left - k < 8 ? left - k : 8);
            if (got < 8) part &= (1ull << (8 * got)) - 1;
          } else if (src + k < a.blob_len) {
            part = a.blob[src + k];
          }
          const uint32_t sh = (uint32_t)(p + k - cb) * 8;
          if (sh < 64) {
            w0 |= part << sh;
            if (sh) w1 |= part >> (64 - sh);
          } else {
            w1 |= part << (sh - 64);
          }
          k += got;
        }
        p = stop;
      }
    }
    *(ulonglong2*)(a.out + cb) = make_ulonglong2(w0, w1);
  }
}

template <int kForm>
void launch_form(dim3 grid, hipStream_t s, const FixedArgs& a) {
  hipLaunchKernelGGL((fixed_kernel<kForm>), grid, dim3(kThreads), 0, s, a);
}

unsigned grid_for(uint64_t items) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + kThreads - 1) / kThreads, kMaxBlocks));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

uint64_t fixed_bytes(int form, uint64_t n) {
  switch (form) {
    case ORCG_ARROW_INT8: return n;
    case ORCG_ARROW_INT16: return 2 * n;
    case ORCG_ARROW_INT32: return 4 * n;
    case ORCG_ARROW_BOOL: return (n + 7) / 8;
    case ORCG_ARROW_FLOAT32: return 4 * n;
    case ORCG_ARROW_DEC64: return 16 * n;
    case ORCG_ARROW_DEC128: return 16 * n;
    default: return 8 * n;
  }
}

int launch_validity(Ctx* ctx, const uint8_t* d_nn, uint64_t n, uint8_t* d_bitmap, uint64_t bitmap_bytes,
                    unsigned long long* d_nulls) {
  if (bitmap_bytes != padded((n + 7) / 8) || (bitmap_bytes && (!d_nn || !d_bitmap || !d_nulls)) ||
      ((uintptr_t)d_bitmap & 1u))
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "bad Arrow validity launch");
  if (bitmap_bytes == 0) return ORCG_OK;
  const uint64_t items = bitmap_bytes / 2;
  // (two workgroups a compute unit: the null count costs an atomic each)
  hipLaunchKernelGGL(validity_kernel, dim3(std::min(grid_for(items), kValidityBlocks)), dim3(kThreads), 0, ctx->stream, d_nn, n,
                     (uint16_t*)d_bitmap, items, aligned16(d_nn) ? 1 : 0, d_nulls);
  return hip_check(ctx, hipGetLastError(), "validity_kernel launch");
}

int launch_fixed(Ctx* ctx, int form, const void* d_src, const void* d_src2, uint64_t n, void* d_out,
                 uint64_t out_bytes) {
  if (form < ORCG_ARROW_INT8 || form > ORCG_ARROW_TIMESTAMP_NS || out_bytes != padded(fixed_bytes(form, n)) ||
      (out_bytes && (!d_src || !d_out)) || (n && form == ORCG_ARROW_TIMESTAMP_NS && !d_src2) ||
      ((uintptr_t)d_out & 15u) || ((uintptr_t)d_src & 7u) || ((uintptr_t)d_src2 & 7u))
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "bad Arrow fixed-width launch");
  if (out_bytes == 0) return ORCG_OK;
  const int vec = aligned16(d_src) && aligned16(d_src2) ? 1 : 0;
  if (form == ORCG_ARROW_BOOL) {
    hipLaunchKernelGGL(bool_kernel, dim3(grid_for(out_bytes)), dim3(kThreads), 0, ctx->stream, (const int64_t*)d_src,
                       n, (uint8_t*)d_out, out_bytes, vec);
    return hip_check(ctx, hipGetLastError(), "bool_kernel launch");
  }
  FixedArgs a{d_src, d_src2, d_out, n, 0, vec};
  const hipStream_t s = ctx->stream;
  switch (form) {
    case ORCG_ARROW_INT8: a.pn = out_bytes; launch_form<ORCG_ARROW_INT8>(dim3(grid_for(a.pn / 8)), s, a); break;
    case ORCG_ARROW_INT16: a.pn = out_bytes / 2; launch_form<ORCG_ARROW_INT16>(dim3(grid_for(a.pn / 4)), s, a); break;
    case ORCG_ARROW_INT32: a.pn = out_bytes / 4; launch_form<ORCG_ARROW_INT32>(dim3(grid_for(a.pn / 2)), s, a); break;
    case ORCG_ARROW_FLOAT32:
      a.pn = out_bytes / 4;
      launch_form<ORCG_ARROW_FLOAT32>(dim3(grid_for(a.pn / 2)), s, a);
      break;
    case ORCG_ARROW_DEC64: a.pn = out_bytes / 16; launch_form<ORCG_ARROW_DEC64>(dim3(grid_for(a.pn / 2)), s, a); break;
    case ORCG_ARROW_DEC128: a.pn = out_bytes / 16; launch_form<ORCG_ARROW_DEC128>(dim3(grid_for(a.pn)), s, a); break;
    default: a.pn = out_bytes / 8; launch_form<ORCG_ARROW_TIMESTAMP_NS>(dim3(grid_for(a.pn / 2)), s, a); break;
  }
  return hip_check(ctx, hipGetLastError(), "fixed_kernel launch");
}

int launch_row_lengths(Ctx* ctx, const int64_t* d_lengths, const int64_t* d_index, const int64_t* d_dict_offsets,
                       uint64_t dict_size, const uint8_t* d_nn, uint64_t n, int64_t* d_out,
                       unsigned long long* d_err) {
  if (n == 0) return ORCG_OK;
  if (!d_out || !d_err || (d_index ? !d_dict_offsets : !d_lengths))
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "bad Arrow row-length launch");
  hipLaunchKernelGGL(row_lengths_kernel, dim3(grid_for(n)), dim3(kThreads), 0, ctx->stream, d_lengths, d_index,
                     d_dict_offsets, dict_size, d_nn, n, d_out, d_err);
  return hip_check(ctx, hipGetLastError(), "row_lengths_kernel launch");
}

int launch_narrow_offsets(Ctx* ctx, const int64_t* d_in, uint64_t count, int32_t* d_out, uint64_t out_bytes,
                          unsigned long long* d_err) {
  if (count == 0 || out_bytes != padded(4 * count) || !d_in || !d_out || !d_err || ((uintptr_t)d_out & 15u) ||
      ((uintptr_t)d_in & 7u))
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "bad Arrow offsets launch");
  const uint64_t pn = out_bytes / 4;
  hipLaunchKernelGGL(narrow_offsets_kernel, dim3(grid_for(pn / 2)), dim3(kThreads), 0, ctx->stream, d_in, count,
                     d_out, pn, aligned16(d_in) ? 1 : 0, d_err);
  return hip_check(ctx, hipGetLastError(), "narrow_offsets_kernel launch");
}

int launch_dict_gather_bytes(Ctx* ctx, const int32_t* d_offsets, const int64_t* d_index, uint64_t n,
                             const int64_t* d_dict_offsets, uint64_t dict_size, const uint8_t* d_blob,
                             uint64_t blob_len, uint8_t* d_out, uint64_t total, uint64_t out_bytes) {
  if (out_bytes != padded(total) || total > 0x7fffffffull ||
      (total && (!d_offsets || !d_index || !d_dict_offsets || !d_out || !n)) || ((uintptr_t)d_out & 15u))
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "bad Arrow dictionary gather launch");
  if (out_bytes == 0) return ORCG_OK;
  const GatherArgs a{d_offsets, d_index, d_dict_offsets, d_blob, d_out, n, dict_size, blob_len, total, out_bytes};
  const uint64_t tiles = (out_bytes + kGatherTile - 1) / kGatherTile;
  hipLaunchKernelGGL(dict_gather_kernel, dim3((unsigned)std::min<uint64_t>(tiles, kMaxBlocks)), dim3(kThreads), 0,
                     ctx->stream, a);
  return hip_check(ctx, hipGetLastError(), "dict_gather_kernel launch");
}

}  // namespace arrow
}  // namespace orcg
