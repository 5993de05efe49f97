// Arrow export (include/orcg_arrow.h): the launchers of arrow_kernels.hip,
// shared by the column-level entries (arrow_api.cpp) and the reader's export
// (arrow_export.cpp). Every launch is asynchronous on ctx->stream.
#pragma once

#include "../../include/orcg_arrow.h"
#include "orcg_internal.hh"

namespace orcg {
namespace arrow {

inline uint64_t padded(uint64_t bytes) { return ORCG_ARROW_PADDED(bytes); }

// The export's own device error word (atomicMin of index << 8 | code, ~0 =
// none), read back by the export itself: the codes are not DevErr's.
enum ArrowErr : uint32_t {
  kArrowOffsetRange = 1,  // an offset does not fit int32 (index = the offset's position)
  kArrowDictIndex = 2,    // a set row's dictionary entry is out of range
};

// Payload bytes of `n` values of a fixed-width form (ORCG_ARROW_*).
uint64_t fixed_bytes(int form, uint64_t n);

// nn[n] -> bitmap (bitmap_bytes = padded((n + 7) / 8), all written);
// *d_nulls (zero on entry) += the rows whose byte is 0.
int launch_validity(Ctx* ctx, const uint8_t* d_nn, uint64_t n, uint8_t* d_bitmap, uint64_t bitmap_bytes,
                    unsigned long long* d_nulls);
// out_bytes = padded(fixed_bytes(form, n)), all written.
int launch_fixed(Ctx* ctx, int form, const void* d_src, const void* d_src2, uint64_t n, void* d_out,
                 uint64_t out_bytes);
// Row lengths as int64 [n], 0 for the rows whose nn byte is 0: from lengths[]
// (d_index null) or from dict_offsets[index + 1] - dict_offsets[index]; a set
// row whose entry is >= dict_size counts 0 and reports kArrowDictIndex.
int launch_row_lengths(Ctx* ctx, const int64_t* d_lengths, const int64_t* d_index, const int64_t* d_dict_offsets,
                       uint64_t dict_size, const uint8_t* d_nn, uint64_t n, int64_t* d_out, unsigned long long* d_err);
// int64 [count] -> int32 [count] (out_bytes = padded(4 * count), all
// written); the last entry outside [0, 2^31 - 1] reports kArrowOffsetRange.
int launch_narrow_offsets(Ctx* ctx, const int64_t* d_in, uint64_t count, int32_t* d_out, uint64_t out_bytes,
                          unsigned long long* d_err);
// The bytes of a dictionary column's rows gathered into d_out
// (out_bytes = padded(total), all written; total = d_offsets[n]).
int launch_dict_gather_bytes(Ctx* ctx, const int32_t* d_offsets, const int64_t* d_index, uint64_t n,
                             const int64_t* d_dict_offsets, uint64_t dict_size, const uint8_t* d_blob,
                             uint64_t blob_len, uint8_t* d_out, uint64_t total, uint64_t out_bytes);

}  // namespace arrow
}  // namespace orcg
