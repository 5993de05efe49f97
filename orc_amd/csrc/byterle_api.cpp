// liborcgpu C ABI for byte / boolean RLE streams (PRESENT, BOOLEAN, BYTE),
// the null scatter of nullable columns and the string-dictionary gather.
// Reference: ByteRleDecoder (c++/src/ByteRLE.hh:71-126, ByteRLE.cc:359-643),
// StringDictionaryColumnReader (ColumnReader.cc:509-613),
// loadStringDictionary (c++/src/DictionaryLoader.cc:43-97).
#include "host_decode.hh"

using namespace orcg;

struct orcg_byte_rle_decoder : HostCursor {
  bool boolean = false;
  std::vector<uint8_t> values;  // decoded bytes from `origin`; the cursor is in bytes, or bits in boolean mode

  orcg_byte_rle_decoder() : HostCursor(host_parse_byte_group) {}
  orcg_rlev2_plan* plan_suffix(const uint8_t* s, uint64_t len) const override {
    return make_byte_plan(s, len, 16u << 10, 16384);
  }
  int decode_suffix(const uint8_t* s, uint64_t len) override {
    values.assign(plan->values, 0);
    Ctx* c = ctx;
    return decode_host_stream(c, s, len, *plan, plan->values, 1, values.data(),
                              [c](const uint8_t* d_src, uint64_t n, const uint64_t* d_seg, uint64_t nsegs,
                                  uint64_t count, void* d_out) {
                                return launch_byterle(c, d_src, n, d_seg, nsegs, false, 0, count, (uint8_t*)d_out);
                              });
  }
  uint64_t avail_units() const { return boolean ? values.size() * 8 : values.size(); }
  int eof() { return fail(ORCG_PARSE_ERROR, dev_error_message(kErrByteBadRead)); }
  // the decoded bytes, or their bits (most significant first), from the cursor
  uint8_t operator[](uint64_t j) const {
    const uint64_t i = cursor + j;
    return boolean ? (values[i >> 3] >> (7 - (i & 7))) & 1 : values[i];
  }

  // ByteRleDecoderImpl::next (ByteRLE.cc:449-505; null slots untouched) and
  // BooleanRleDecoderImpl::next (:578-643; null slots get 0).
  int next(char* data, uint64_t n, const char* nn) {
    // the boolean decoder reads whole bytes (ByteRLE.cc:618-624)
    uint64_t need = cursor + count_set(nn, n);
    if (boolean) need = (need + 7) / 8 * 8;
    if (need <= avail_units()) {
      cursor += place_dense(data, *this, nn, n, ~0ull, boolean);
      return ORCG_OK;
    }
    // bytes up to the failure are delivered, then the read fails
    const uint64_t have = avail_units() > cursor ? avail_units() - cursor : 0;
    cursor += place_dense(data, *this, nn, n, have, boolean);
    return eof();
  }
  int skip(uint64_t n) {
    uint64_t need = cursor + n;
    if (boolean && need % 8) need = (need + 7) / 8 * 8;
    if (need > avail_units()) return eof();
    cursor += n;
    return ORCG_OK;
  }
  // byte RLE position: (byte offset, bytes to skip); boolean adds the bits
  // consumed of the next byte (BooleanRleDecoderImpl::seek, ByteRLE.cc:549-560)
  int seek(const uint64_t* pos, uint64_t npos) {
    if (npos < (boolean ? 3u : 2u)) return fail(ORCG_INVALID_ARGUMENT, "bad position");
    const uint64_t byte = pos[0], skipb = pos[1], bits = boolean ? pos[2] : 0;
    if (byte > src.size()) return fail(ORCG_INVALID_ARGUMENT, "Seek past end of stream");
    if (bits > 8) return fail(ORCG_PARSE_ERROR, "bad position");
    uint64_t vi;
    const int rc = seek_group(byte, &vi);
    if (rc) return rc;
    cursor = boolean ? 8 * (vi + skipb) : vi + skipb;
    if (cursor > avail_units()) return eof();
    if (boolean && bits) {
      if (cursor + 8 > avail_units()) return eof();
      cursor += bits;
    }
    return ORCG_OK;
  }
};

extern "C" {

int orcg_byterle_plan_create(const uint8_t* src, uint64_t len, uint64_t max_bytes, uint64_t max_values,
                             orcg_rlev2_plan** out) {
  if (!out || (len && !src)) return ORCG_INVALID_ARGUMENT;
  *out = make_byte_plan(src, len, max_bytes ? max_bytes : (16u << 10), max_values ? max_values : 16384);
  return ORCG_OK;
}

int orcg_byterle_decode_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len, const orcg_segment* d_segs,
                               uint64_t nsegs, uint64_t value_begin, uint64_t nvalues, uint8_t* d_dst) {
  if (!c || (nsegs && (!d_src || !d_segs)) || (nvalues && !d_dst)) return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  return launch_byterle(c, d_src, src_len, (const uint64_t*)d_segs, nsegs, false, value_begin, nvalues, d_dst, nullptr);
}

int orcg_boolrle_decode_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len, const orcg_segment* d_segs,
                               uint64_t nsegs, uint64_t row_begin, uint64_t nrows, uint8_t* d_dst) {
  if (!c || (nsegs && (!d_src || !d_segs)) || (nrows && !d_dst)) return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  return launch_byterle(c, d_src, src_len, (const uint64_t*)d_segs, nsegs, true, row_begin, nrows, d_dst, nullptr);
}

int orcg_boolrle_decode_counted_device(orcg_ctx* c, const uint8_t* d_src, uint64_t src_len,
                                       const orcg_segment* d_segs, uint64_t nsegs, uint64_t row_begin, uint64_t nrows,
                                       const uint64_t* d_nrows, uint8_t* d_dst, uint64_t* d_ones) {
  if (!c || (nsegs && (!d_src || !d_segs)) || (nrows && !d_dst)) return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  return launch_byterle(c, d_src, src_len, (const uint64_t*)d_segs, nsegs, true, row_begin, nrows, d_dst, d_ones,
                        d_nrows);
}

int orcg_byte_rle_decoder_create(orcg_ctx* c, const uint8_t* src, uint64_t len, int boolean,
                                 orcg_byte_rle_decoder** out) {
  return create_decoder(c, src, len, out, [&](orcg_byte_rle_decoder& d) {
    d.boolean = boolean != 0;
    return ORCG_OK;
  });
}

void orcg_byte_rle_decoder_destroy(orcg_byte_rle_decoder* d) { delete d; }

int orcg_byte_rle_decoder_next(orcg_byte_rle_decoder* d, char* data, uint64_t n, const char* not_null) {
  if (!d || (n && !data)) return ORCG_INVALID_ARGUMENT;
  return d->next(data, n, not_null);
}

int orcg_byte_rle_decoder_skip(orcg_byte_rle_decoder* d, uint64_t n) {
  return d ? d->skip(n) : ORCG_INVALID_ARGUMENT;
}

int orcg_byte_rle_decoder_seek(orcg_byte_rle_decoder* d, const uint64_t* positions, uint64_t npos) {
  if (!d || !positions) return ORCG_INVALID_ARGUMENT;
  return d->seek(positions, npos);
}

const char* orcg_byte_rle_decoder_last_error(const orcg_byte_rle_decoder* d) {
  return d ? d->last_error.c_str() : "";
}

int orcg_scatter_not_null_device(orcg_ctx* c, const void* d_dense, const uint8_t* d_not_null, uint64_t n,
                                 void* d_out, int width, int fill_nulls, int64_t fill_value) {
  if (!c || (n && (!d_dense || !d_not_null || !d_out))) return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  return launch_scatter(c, d_dense, d_not_null, n, d_out, width, fill_nulls, fill_value);
}

int orcg_dict_offsets_device(orcg_ctx* c, const int64_t* d_lengths, uint64_t dict_size, int64_t* d_offsets) {
  if (!c || !d_offsets || (dict_size && !d_lengths)) return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  return launch_dict_offsets(c, d_lengths, dict_size, d_offsets);
}

int orcg_dict_gather_device(orcg_ctx* c, const void* d_indices, int index_width, const uint8_t* d_not_null,
                            uint64_t n, const int64_t* d_offsets, uint64_t dict_size, int64_t* d_start,
                            int64_t* d_length) {
  if (!c || (n && (!d_indices || !d_offsets || !d_start || !d_length))) return ORCG_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  return launch_dict_gather(c, d_indices, index_width, d_not_null, n, d_offsets, dict_size, d_start, d_length);
}

}  // extern "C"
