// Schema evolution: a decoded column converted to the read type's kind
// (gfx950). One elementwise kernel, templated on the class of the values that
// arrive and the class that leaves; precision, scales and the constants the
// host computes are runtime arguments.
//
// The rules are the reference's, value for value (c++/src/
// ConvertColumnReader.cc, c++/src/Int128.cc; DESIGN.md 3.9 lists them with
// their quirks):
//   number  -> number   convertNumericElement            ConvertColumnReader.cc:96-207
//   number  -> decimal  NumericToDecimalColumnReader     :342-415, Int128.cc:534-624
//   decimal -> number   DecimalToNumericColumnReader     :491-563, Int128.cc:473-478, :524-532
//   decimal -> decimal  DecimalConvertColumnReader       :566-617, Int128.cc:534-579
// A value the read type cannot hold becomes NULL (handleOverflow, :66-76): its
// mask byte is 0 and, unlike the reference, its slot holds 0. With
// throwOnSchemaEvolutionOverflow the first such row in value order is also
// reported through the column's error record.
//
// Representation (include/orcg_reader.h): integers of every width are int64,
// FLOAT is a double holding a float value, Decimal64 is int64, Decimal128 is
// an [hi, lo] int64 pair. A converted tinyint / smallint / int column holds the
// narrowed value in int64, a converted float column the float-rounded value in
// double.
//
// Shape: 256 threads, four values a thread, 256 apart (as timestamp_tz_kernel):
// 8 or 16 bytes of data and one mask byte in, the same out. The rows a launch
// nulled are summed per wave and added with one atomic a wave, after the
// wave's last tile. No LDS, no scratch.
//
// No product here feeds a following add as one fused operation: the reference
// rounds after each step, and so must this file.
#pragma clang fp contract(off)

#include "device_util.hh"
#include "orcg_internal.hh"

namespace orcg {
namespace {

using dev::report;
using dev::wave_sum;

constexpr int kCvThreads = 256;
constexpr int kCvPer = 4;  // values per thread, 256 apart (coalesced)
constexpr uint64_t kCvMaxBlocks = 1024;

// The 128-bit helpers of decimal_kernels.hip (U128, mul128_u64, div128_u32),
// copied: moving them to a shared header would have to leave that unit's
// kernels instruction-identical.
struct U128 {
  uint64_t lo, hi;
};

// 10^k, k = 0..38 (scaleUpInt128ByPowerOfTen(1, k), Int128.cc:502-522)
__device__ const U128 kP10[39] = {
    {0x0000000000000001ull, 0x0000000000000000ull}, {0x000000000000000aull, 0x0000000000000000ull},
    {0x0000000000000064ull, 0x0000000000000000ull}, {0x00000000000003e8ull, 0x0000000000000000ull},
    {0x0000000000002710ull, 0x0000000000000000ull}, {0x00000000000186a0ull, 0x0000000000000000ull},
    {0x00000000000f4240ull, 0x0000000000000000ull}, {0x0000000000989680ull, 0x0000000000000000ull},
    {0x0000000005f5e100ull, 0x0000000000000000ull}, {0x000000003b9aca00ull, 0x0000000000000000ull},
    {0x00000002540be400ull, 0x0000000000000000ull}, {0x000000174876e800ull, 0x0000000000000000ull},
    {0x000000e8d4a51000ull, 0x0000000000000000ull}, {0x000009184e72a000ull, 0x0000000000000000ull},
    {0x00005af3107a4000ull, 0x0000000000000000ull}, {0x00038d7ea4c68000ull, 0x0000000000000000ull},
    {0x002386f26fc10000ull, 0x0000000000000000ull}, {0x016345785d8a0000ull, 0x0000000000000000ull},
    {0x0de0b6b3a7640000ull, 0x0000000000000000ull}, {0x8ac7230489e80000ull, 0x0000000000000000ull},
    {0x6bc75e2d63100000ull, 0x0000000000000005ull}, {0x35c9adc5dea00000ull, 0x0000000000000036ull},
    {0x19e0c9bab2400000ull, 0x000000000000021eull}, {0x02c7e14af6800000ull, 0x000000000000152dull},
    {0x1bcecceda1000000ull, 0x000000000000d3c2ull}, {0x161401484a000000ull, 0x0000000000084595ull},
    {0xdcc80cd2e4000000ull, 0x000000000052b7d2ull}, {0x9fd0803ce8000000ull, 0x00000000033b2e3cull},
    {0x3e25026110000000ull, 0x00000000204fce5eull}, {0x6d7217caa0000000ull, 0x00000001431e0faeull},
    {0x4674edea40000000ull, 0x0000000c9f2c9cd0ull}, {0xc0914b2680000000ull, 0x0000007e37be2022ull},
    {0x85acef8100000000ull, 0x000004ee2d6d415bull}, {0x38c15b0a00000000ull, 0x0000314dc6448d93ull},
    {0x378d8e6400000000ull, 0x0001ed09bead87c0ull}, {0x2b878fe800000000ull, 0x0013426172c74d82ull},
    {0xb34b9f1000000000ull, 0x00c097ce7bc90715ull}, {0x00f436a000000000ull, 0x0785ee10d5da46d9ull},
    {0x098a224000000000ull, 0x4b3b4ca85a86c47aull}};

__device__ const uint32_t kP10u32[10] = {1u,      10u,      100u,      1000u,      10000u,
                                         100000u, 1000000u, 10000000u, 100000000u, 1000000000u};

__device__ __forceinline__ bool gt128(U128 a, U128 b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }
__device__ __forceinline__ bool ge128(U128 a, U128 b) { return !gt128(b, a); }
__device__ __forceinline__ bool zero128(U128 a) { return (a.lo | a.hi) == 0; }

__device__ __forceinline__ U128 add128(U128 a, U128 b) {
  const uint64_t lo = a.lo + b.lo;
  return U128{lo, a.hi + b.hi + (lo < a.lo ? 1 : 0)};
}

__device__ __forceinline__ U128 sub128(U128 a, U128 b) {
  return U128{a.lo - b.lo, a.hi - b.hi - (a.lo < b.lo ? 1 : 0)};
}

__device__ __forceinline__ U128 neg128(U128 a) {
  const uint64_t lo = ~a.lo + 1;
  return U128{lo, ~a.hi + (lo == 0 ? 1 : 0)};
}

// (a * b) mod 2^128
__device__ __forceinline__ U128 mul128(U128 a, U128 b) {
  return U128{a.lo * b.lo, __umul64hi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo};
}

// a / d for d < 2^32, in 32-bit limbs (Int128 singleDivide, Int128.cc:271-286)
__device__ __forceinline__ U128 div128_u32(U128 a, uint32_t d) {
  uint64_t r = 0;
  uint32_t q[4];
  const uint32_t limb[4] = {(uint32_t)(a.hi >> 32), (uint32_t)a.hi, (uint32_t)(a.lo >> 32), (uint32_t)a.lo};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r = (r << 32) | limb[j];
    q[j] = (uint32_t)(r / d);
    r %= d;
  }
  return U128{((uint64_t)q[2] << 32) | q[3], ((uint64_t)q[0] << 32) | q[1]};
}

// floor(m / 10^k) of a magnitude, k <= 38, as divisions by factors below 2^32
// (the floor of a floor is the floor of the whole quotient)
__device__ __forceinline__ U128 div_pow10(U128 m, uint32_t k) {
  while (k > 0 && !zero128(m)) {
    const uint32_t step = k > 9 ? 9 : k;
    m = div128_u32(m, kP10u32[step]);
    k -= step;
  }
  return m;
}

__device__ __forceinline__ U128 from_i64(int64_t v) { return U128{(uint64_t)v, v < 0 ? ~0ull : 0ull}; }

// Int128::fitsInLong (Int128.hh): the high word is the low word's sign
__device__ __forceinline__ bool fits_long(U128 v) { return v.hi == ((int64_t)v.lo < 0 ? ~0ull : 0ull); }

// downCastToInteger (ConvertColumnReader.cc:96-106): cast to `width` bytes and
// compare back
__device__ __forceinline__ bool down_cast(int64_t v, int width, int64_t* out) {
  const int sh = 64 - 8 * width;
  const int64_t t = (int64_t)((uint64_t)v << sh) >> sh;
  *out = t;
  return t == v;
}

// canFitInLong (:59-63); NaN fails both comparisons
__device__ __forceinline__ bool can_fit_in_long(double v) { return (-0x1p63 - v < 1.0) && (v < 0x1p63); }

// convertDecimal(Int128 value, fromScale, toPrecision, toScale, round = true)
// (Int128.cc:534-579) on the value's two's complement; false = overflow.
// Scaling up, the reference tests the magnitude against 10^p, multiplies in
// steps with an overflow flag and tests again: all three fail exactly when
// magnitude * 10^k > 10^p as integers (a product past 127 bits is past 10^38
// too), which is magnitude > 10^(p - k), or any non-zero magnitude for k > p.
__device__ __forceinline__ bool dec_to_dec(U128 v, int32_t from_scale, int32_t p, int32_t s, U128* out) {
  const bool neg = (int64_t)v.hi < 0;
  U128 m = neg ? neg128(v) : v;
  U128 ub = kP10[p];
  uint64_t round_off = 0;
  const int32_t d = from_scale - s;
  if (d > 0) {
    const U128 q = div_pow10(m, (uint32_t)d);
    const U128 r = sub128(m, mul128(q, kP10[d]));
    // remainder *= 2 is a signed Int128 product: past 2^127 it turns negative
    // and the comparison fails (only d = 38 gets there)
    const U128 r2 = add128(r, r);
    if ((int64_t)r2.hi >= 0 && ge128(r2, kP10[d])) {
      ub = sub128(ub, U128{1, 0});
      round_off = 1;
    }
    m = q;
  } else if (d < 0) {
    const int32_t k = -d;
    if (k > p ? !zero128(m) : gt128(m, kP10[p - k])) return false;
    m = mul128(m, kP10[k]);
  }
  if (gt128(m, ub)) return false;  // strictly greater: a magnitude of exactly 10^p passes
  m = add128(m, U128{round_off, 0});
  *out = neg ? neg128(m) : m;
  return true;
}

// convertDecimal<T>(T value, precision, scale) (Int128.cc:581-624), worked in
// T; pw = (T)pow(10, scale) from the host's libm. false = overflow.
template <typename T>
__device__ __forceinline__ bool fp_to_dec(T v, int32_t p, int32_t s, T pw, U128* out) {
  const T bound = (T)0x1p127;
  if (v != v || v <= -bound || v >= bound) return false;
  const bool neg = v < 0;
  v = neg ? -v : v;
  U128 ip;
  if (v >= (T)0x1p64) {
    const int64_t hi = (int64_t)(v * (T)0x1p-64);
    ip = U128{(uint64_t)(v - (T)hi * (T)0x1p64), (uint64_t)hi};
  } else {
    ip = U128{(uint64_t)v, 0};
  }
  const T frac = v - (sizeof(T) == 4 ? (T)floorf((float)v) : (T)floor((double)v));
  // the scaled integer part overflows, or is >= 10^p, exactly when the
  // integer part is >= 10^(p - s)
  if (ge128(ip, kP10[p - s])) return false;
  ip = mul128(ip, kP10[s]);
  const T scaled = frac * pw;
  const T r = sizeof(T) == 4 ? (T)roundf((float)scaled) : (T)round((double)scaled);
  // static_cast<int64_t> of a value past int64 (scales above 18): the x86
  // conversion's result, INT64_MIN; added with no second bound check
  const int64_t ri = (r >= (T)-0x1p63 && r < (T)0x1p63) ? (int64_t)r : INT64_MIN;
  ip = add128(ip, from_i64(ri));
  *out = neg ? neg128(ip) : ip;
  return true;
}

// Int128::toDouble (Int128.cc:473-478): (double)int64 when the value fits,
// else the two words converted apart and added (two roundings)
__device__ __forceinline__ double dec_to_double(U128 v) {
  if (fits_long(v)) return (double)(int64_t)v.lo;
  return (double)v.lo + (double)(int64_t)v.hi * 0x1p64;
}

// scaleDownInt128ByPowerOfTen (Int128.cc:524-532): truncated toward zero
__device__ __forceinline__ U128 dec_scale_down(U128 v, int32_t scale) {
  const bool neg = (int64_t)v.hi < 0;
  const U128 m = div_pow10(neg ? neg128(v) : v, (uint32_t)scale);
  return neg ? neg128(m) : m;
}

__device__ __forceinline__ uint64_t bits_of(double d) { return (uint64_t)__double_as_longlong(d); }

// One value. The result's 64-bit payload (int64, or a double's bits) is in
// out->lo; a Decimal128 result uses both words.
template <int kSrc, int kDst>
__device__ __forceinline__ bool convert_one(const ConvertArgs& a, uint64_t i, U128* out) {
  constexpr bool kSrcDec = kSrc == kConvDec64 || kSrc == kConvDec128;
  constexpr bool kSrcFp = kSrc == kConvFloat || kSrc == kConvDouble;
  int64_t iv = 0;
  double dv = 0;
  U128 xv{0, 0};
  if constexpr (kSrc == kConvInt64) iv = ((const int64_t*)a.src)[i];
  if constexpr (kSrcFp) dv = ((const double*)a.src)[i];
  if constexpr (kSrc == kConvDec64) xv = from_i64(((const int64_t*)a.src)[i]);
  if constexpr (kSrc == kConvDec128) {
    const int64_t* s = (const int64_t*)a.src + 2 * i;
    xv = U128{(uint64_t)s[1], (uint64_t)s[0]};
  }
  *out = U128{0, 0};

  if constexpr (kDst == kToBool) {
    // (int64)v == 0 ? 0 : 1 (:198, :203); a NaN or a value outside int64
    // gives 1, as the x86 conversion's INT64_MIN does. Decimals: the unscaled
    // value != 0 (:559)
    if constexpr (kSrc == kConvInt64) out->lo = iv != 0;
    if constexpr (kSrcFp) out->lo = !(fabs(dv) < 1.0);
    if constexpr (kSrcDec) out->lo = !zero128(xv);
    return true;
  } else if constexpr (kDst == kToInt) {
    int64_t t = iv;
    if constexpr (kSrcFp) {
      if (!can_fit_in_long(dv)) return false;
      t = (int64_t)dv;  // truncates toward zero
    }
    if constexpr (kSrcDec) {
      const U128 q = dec_scale_down(xv, a.src_scale);
      if (!fits_long(q)) return false;
      t = (int64_t)q.lo;
    }
    int64_t r;
    if (!down_cast(t, a.width, &r)) return false;
    out->lo = (uint64_t)r;
    return true;
  } else if constexpr (kDst == kToFloat || kDst == kToDouble) {
    double r;
    if constexpr (kSrc == kConvInt64) r = kDst == kToFloat ? (double)(float)iv : (double)iv;
    if constexpr (kSrcFp) r = kDst == kToFloat ? (double)(float)dv : dv;
    if constexpr (kSrcDec) {
      // (:533-537) the double, cast to the read type, over the cast factor
      const double d = dec_to_double(xv);
      r = kDst == kToFloat ? (double)((float)d / a.factor_f) : d / a.factor_d;
    }
    out->lo = bits_of(r);
    return true;
  } else {
    U128 r;
    bool ok;
    if constexpr (kSrc == kConvInt64) ok = dec_to_dec(from_i64(iv), 0, a.precision, a.scale, &r);
    if constexpr (kSrc == kConvFloat) ok = fp_to_dec<float>((float)dv, a.precision, a.scale, (float)a.pow_t, &r);
    if constexpr (kSrc == kConvDouble) ok = fp_to_dec<double>(dv, a.precision, a.scale, a.pow_t, &r);
    if constexpr (kSrcDec) ok = dec_to_dec(xv, a.src_scale, a.precision, a.scale, &r);
    if (!ok) return false;
    if constexpr (kDst == kToDec64)
      if (!fits_long(r)) return false;
    *out = r;
    return true;
  }
}

template <int kSrc, int kDst>
__global__ __launch_bounds__(kCvThreads) void convert_kernel(const ConvertArgs a) {
  // a workgroup takes tiles of 1,024 values, gridDim.x apart (the grid is
  // capped, launch_convert): a wave's nulled rows of all its tiles go into one
  // atomic. Uncapped, 10^7 values with overflows spent 0.45 ms on 39,000
  // atomics to the one count word.
  const uint64_t ntiles = (a.n + kCvThreads * kCvPer - 1) / (kCvThreads * kCvPer);
  uint32_t nulled = 0;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
  const uint64_t base = tile * (kCvThreads * kCvPer) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kCvPer; ++k) {
    const uint64_t i = base + (uint64_t)k * kCvThreads;
    if (i < a.n) {
      const bool live = a.nn ? a.nn[i] != 0 : true;
      U128 v{0, 0};
      bool keep = false;
      if (live) {
        keep = convert_one<kSrc, kDst>(a, i, &v);
        if (!keep) {
          ++nulled;
          v = U128{0, 0};
          if (a.throw_mode) report(a.err, i, kErrConvertOverflow);
        }
      }
      if constexpr (kDst == kToDec128) {
        int64_t* o = (int64_t*)a.out + 2 * i;
        o[0] = (int64_t)v.hi;
        o[1] = (int64_t)v.lo;
      } else {
        ((uint64_t*)a.out)[i] = v.lo;
      }
      a.out_nn[i] = keep ? 1 : 0;
    }
  }
  }
  // every lane is back here: the wave's nulled rows, one atomic a wave
  nulled = wave_sum(nulled);
  if ((threadIdx.x & (dev::kWave - 1)) == 0 && nulled) atomicAdd(a.nulled, (unsigned long long)nulled);
}

template <int kSrc>
void launch_src(int dst, dim3 grid, hipStream_t s, const ConvertArgs& a) {
  const dim3 block(kCvThreads);
  switch (dst) {
    case kToBool: hipLaunchKernelGGL((convert_kernel<kSrc, kToBool>), grid, block, 0, s, a); break;
    case kToInt: hipLaunchKernelGGL((convert_kernel<kSrc, kToInt>), grid, block, 0, s, a); break;
    case kToFloat: hipLaunchKernelGGL((convert_kernel<kSrc, kToFloat>), grid, block, 0, s, a); break;
    case kToDouble: hipLaunchKernelGGL((convert_kernel<kSrc, kToDouble>), grid, block, 0, s, a); break;
    case kToDec64: hipLaunchKernelGGL((convert_kernel<kSrc, kToDec64>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((convert_kernel<kSrc, kToDec128>), grid, block, 0, s, a); break;
  }
}

}  // namespace

int launch_convert(Ctx* ctx, int src, int dst, const ConvertArgs& a) {
  if (a.n == 0) return ORCG_OK;
  if (src < kConvInt64 || src > kConvDec128 || dst < kToBool || dst > kToDec128 || !a.src || !a.out || !a.out_nn ||
      !a.nulled || (a.throw_mode && !a.err))
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "bad conversion launch");
  if (dst == kToInt && a.width != 1 && a.width != 2 && a.width != 4 && a.width != 8)
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "bad integer width for a conversion");
  if ((dst == kToDec64 || dst == kToDec128) &&
      (a.precision < 1 || a.precision > 38 || a.scale < 0 || a.scale > a.precision))
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "bad decimal precision or scale for a conversion");
  if ((src == kConvDec64 || src == kConvDec128) && (a.src_scale < 0 || a.src_scale > 38))
    return set_error(ctx, ORCG_INVALID_ARGUMENT, "bad source scale for a conversion");
  const uint64_t per = (uint64_t)kCvThreads * kCvPer;
  const uint64_t blocks = (a.n + per - 1) / per;
  // at most kCvMaxBlocks workgroups (four a compute unit): larger columns loop
  const dim3 grid((unsigned)std::min<uint64_t>(blocks, kCvMaxBlocks));
  switch (src) {
    case kConvInt64: launch_src<kConvInt64>(dst, grid, ctx->stream, a); break;
    case kConvFloat: launch_src<kConvFloat>(dst, grid, ctx->stream, a); break;
    case kConvDouble: launch_src<kConvDouble>(dst, grid, ctx->stream, a); break;
    case kConvDec64: launch_src<kConvDec64>(dst, grid, ctx->stream, a); break;
    default: launch_src<kConvDec128>(dst, grid, ctx->stream, a); break;
  }
  return hip_check(ctx, hipGetLastError(), "convert_kernel launch");
}

}  // namespace orcg
