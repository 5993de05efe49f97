// C ABI of the schema-evolution value conversions (include/orcg.h): a decoded
// column in device memory converted to another kind by the kernel of
// convert_kernels.hip, and the constants the host computes for it.
#include <math.h>
#include <stdlib.h>

#include "orcg_internal.hh"
#include "read_type.hh"

using namespace orcg;

namespace orcg {

// The constants of one conversion. The reference's factor for a decimal
// source is an int64 product (ConvertColumnReader.cc:498-501) that overflows
// for scales above 18; there the correctly rounded 10^scale is used, in each
// width. (T)pow(10, scale) (Int128.cc:617) comes from the host's libm: a
// device pow need not agree with it.
void convert_constants(int src, ConvertArgs* a) {
  a->factor_d = 1;
  a->factor_f = 1;
  a->pow_t = 1;
  if (src == kConvDec64 || src == kConvDec128) {
    if (a->src_scale <= 18) {
      int64_t f = 1;
      for (int i = 0; i < a->src_scale; ++i) f *= 10;
      a->factor_d = (double)f;
      a->factor_f = (float)f;
    } else {
      const std::string lit = "1e" + std::to_string(a->src_scale);
      a->factor_d = strtod(lit.c_str(), nullptr);
      a->factor_f = strtof(lit.c_str(), nullptr);
    }
  } else if (src == kConvFloat) {
    a->pow_t = (double)(float)pow(10, a->scale);
  } else if (src == kConvDouble) {
    a->pow_t = pow(10, a->scale);
  }
}

}  // namespace orcg

// the arguments of one column conversion from the C ABI's (the target's class
// in *dst); the pointers are filled in by the caller
static int convert_setup(orcg_ctx* c, int src_class, int32_t src_scale, uint32_t target_kind, uint32_t precision,
                         uint32_t scale, int throw_on_overflow, ConvertArgs* a, int* dst) {
  if (src_class < kConvInt64 || src_class > kConvDec128)
    return set_error(c, ORCG_INVALID_ARGUMENT, "unknown source class for a conversion");
  const bool src_dec = src_class == kConvDec64 || src_class == kConvDec128;
  switch (target_kind) {
    case rt::kBoolean: *dst = kToBool; break;
    case rt::kByte: *dst = kToInt, a->width = 1; break;
    case rt::kShort: *dst = kToInt, a->width = 2; break;
    case rt::kInt: *dst = kToInt, a->width = 4; break;
    case rt::kLong: *dst = kToInt, a->width = 8; break;
    case rt::kFloat: *dst = kToFloat; break;
    case rt::kDouble: *dst = kToDouble; break;
    case rt::kDecimal: *dst = precision <= 18 ? kToDec64 : kToDec128; break;
    default: return set_error(c, ORCG_INVALID_ARGUMENT, "a conversion's target is a numeric or a decimal kind");
  }
  if (target_kind == rt::kDecimal && (precision < 1 || precision > 38 || scale > precision))
    return set_error(c, ORCG_INVALID_ARGUMENT, "bad decimal precision or scale for a conversion");
  if (src_dec && (src_scale < 0 || src_scale > 38))
    return set_error(c, ORCG_INVALID_ARGUMENT, "bad source scale for a conversion");
  a->src_scale = src_dec ? src_scale : 0;
  a->precision = (int32_t)precision;
  a->scale = (int32_t)scale;
  a->throw_mode = throw_on_overflow ? 1 : 0;
  convert_constants(src_class, a);
  return ORCG_OK;
}

extern "C" {

int orcg_convert_column_device(orcg_ctx* c, const void* d_src, int src_class, int32_t src_scale, uint64_t n,
                               const uint8_t* d_not_null, uint32_t target_kind, uint32_t precision, uint32_t scale,
                               int throw_on_overflow, void* d_out, uint8_t* d_out_not_null, uint64_t* nulled) {
  if (!c || !nulled || (n && (!d_src || !d_out || !d_out_not_null))) return ORCG_INVALID_ARGUMENT;
  *nulled = 0;
  int dst;
  ConvertArgs a{};
  int rc = convert_setup(c, src_class, src_scale, target_kind, precision, scale, throw_on_overflow, &a, &dst);
  if (rc || n == 0) return rc;
  (void)hipSetDevice(c->device);
  void* d_count;
  if ((rc = scratch(c, kScratchMisc, sizeof(unsigned long long), &d_count))) return rc;
  if ((rc = hip_check(c, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), c->stream), "memset"))) return rc;
  a.src = d_src;
  a.nn = d_not_null;
  a.out = d_out;
  a.out_nn = d_out_not_null;
  a.n = n;
  a.err = c->d_err;
  a.nulled = (unsigned long long*)d_count;
  if ((rc = launch_convert(c, src_class, dst, a))) return rc;
  unsigned long long count = 0;
  if ((rc = hip_check(c, hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, c->stream),
                      "D2H nulled count")))
    return rc;
  rc = sync_ctx(c);
  *nulled = count;
  if (rc && c->last_error == dev_error_message(kErrConvertOverflow)) {
    // the reference prints typeid names here; these are the ORC type names
    static const char* const src_names[] = {"bigint", "float", "double", "decimal", "decimal"};
    rt::Tree t(1);
    t[0].kind = target_kind;
    t[0].precision = precision;
    t[0].scale = scale;
    std::string from = src_names[src_class];
    if (src_class == kConvDec64 || src_class == kConvDec128)
      from += "(" + std::to_string(src_class == kConvDec64 ? 18 : 38) + "," + std::to_string(src_scale) + ")";
    return set_error(c, rc, std::string(dev_error_message(kErrConvertOverflow)) + " from " + from + " to " +
                                rt::to_string(t));
  }
  return rc;
}

// Measurement helper (no reference counterpart; scripts/ab_convert.py):
// `iters` timed launches of one conversion over n values, HIP events around
// the launch alone (the kernel reads its inputs only, so every launch sees the
// same arrays); overflows become NULLs.
int orcg_convert_bench(orcg_ctx* c, const void* d_src, int src_class, int32_t src_scale, uint64_t n,
                       const uint8_t* d_not_null, uint32_t target_kind, uint32_t precision, uint32_t scale, void* d_out,
                       uint8_t* d_out_not_null, uint32_t iters, double* ms_out) {
  if (!c || !n || !d_src || !d_out || !d_out_not_null || !ms_out) return ORCG_INVALID_ARGUMENT;
  int dst;
  ConvertArgs a{};
  int rc = convert_setup(c, src_class, src_scale, target_kind, precision, scale, 0, &a, &dst);
  if (rc) return rc;
  (void)hipSetDevice(c->device);
  void* d_count;
  if ((rc = scratch(c, kScratchMisc, sizeof(unsigned long long), &d_count))) return rc;
  if ((rc = hip_check(c, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), c->stream), "memset"))) return rc;
  a.src = d_src;
  a.nn = d_not_null;
  a.out = d_out;
  a.out_nn = d_out_not_null;
  a.n = n;
  a.err = c->d_err;
  a.nulled = (unsigned long long*)d_count;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  rc = hip_check(c, hipEventCreate(&e0), "hipEventCreate");
  if (!rc) rc = hip_check(c, hipEventCreate(&e1), "hipEventCreate");
  for (uint32_t i = 0; i < iters && !rc; ++i) {
    rc = hip_check(c, hipEventRecord(e0, c->stream), "hipEventRecord");
    if (!rc) rc = launch_convert(c, src_class, dst, a);
    if (!rc) rc = hip_check(c, hipEventRecord(e1, c->stream), "hipEventRecord");
    if (!rc) rc = sync_ctx(c);
    float ms = 0;
    if (!rc) rc = hip_check(c, hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    ms_out[i] = ms;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

}  // extern "C"
