// Launchers of filter_kernels.hip and the run they make up (filter_api.cpp).
#pragma once

#include "filter_plan.hh"
#include "orcg_internal.hh"

namespace orcg {
namespace filter {

// rows of one combine / select workgroup: 256 lanes x 4 rows
constexpr uint32_t kTile = 1024;

// A string leaf over n elements: rows of a direct column (start / length, nn)
// or the entries of a dictionary (dict_offsets; start = length = nn = null).
// truth[e] = kTruthYes or kTruthNo; a null row writes kTruthNo and reads
// neither its start nor its length.
struct StringLeafArgs {
  const int64_t* start;
  const int64_t* length;
  const int64_t* dict_offsets;
  const uint8_t* nn;
  const uint8_t* blob;
  uint64_t blob_len;
  uint64_t n;
  uint32_t op, nlit;
  const uint32_t* lit_off;  // nlit + 1 offsets into lit_bytes (the leaf's own first)
  const uint8_t* lit_bytes;
  uint8_t* truth;
};
int launch_string_leaf(Ctx* ctx, const StringLeafArgs& a);

// The whole program per row: sel[0 .. tiles * kTile) (rows past n: 0) and
// tile_counts[tile] = its selected rows.
int launch_combine(Ctx* ctx, const DevLeaf* d_leaves, const uint32_t* d_ops, uint32_t nops, const int64_t* d_words,
                   uint64_t n, uint8_t* d_sel, int64_t* d_tile_counts);
// selected[tile_base[t] ..) = the tile's selected rows, ascending
int launch_select(Ctx* ctx, const uint8_t* d_sel, uint64_t tiles, const int64_t* d_tile_base, int64_t* d_selected);

// Row sel[i] of up to three 8-byte arrays, one 16-byte array and the mask to
// row i; *nulls += the gathered rows whose mask byte is 0 (one atomic a wave).
// A selected index >= n_src gathers zeros.
struct GatherArgs {
  const int64_t* sel;
  uint64_t count, n_src;
  const uint64_t* src8[3];
  uint64_t* dst8[3];
  const void* src16;
  void* dst16;
  const uint8_t* nn;
  uint8_t* out_nn;
  unsigned long long* nulls;
};
int launch_gather(Ctx* ctx, const GatherArgs& a);

}  // namespace filter
}  // namespace orcg
