// Which streams a column of a given kind and encoding reads: the one
// description the reader's host half (row-index positions, host plans), its
// multi-stream batch and its per-column decode all follow. Host-only, no HIP.
//
// The order is the order the reference's column readers take their streams:
// PRESENT (ColumnReader::seekToRowGroup, c++/src/ColumnReader.cc:106-110),
// a dictionary's LENGTH (read whole when the stripe starts,
// DictionaryLoader.cc:43-97: no row-index positions), then the value
// streams in each reader's seekToRowGroup order -- the order the writers
// record positions in (ColumnWriter.cc recordPosition). DICTIONARY_DATA is a
// blob with no positions and no plan: it is not listed.
#pragma once

#include "../../include/orcg_reader.h"
#include "orc_file.hh"

namespace orcg {
namespace reader {

enum { kSlotPresent = 0, kSlotData = 1, kSlotLength = 2, kSlotDict = 3, kSlotSecondary = 4, kNumSlots = 5 };

inline int slot_of(uint32_t stream_kind) {
  switch (stream_kind) {
    case file::kPresent: return kSlotPresent;
    case file::kData: return kSlotData;
    case file::kLength: return kSlotLength;
    case file::kDictionaryData: return kSlotDict;
    case file::kSecondary: return kSlotSecondary;
  }
  return -1;
}

inline bool is_string_kind(uint32_t k) {
  return k == ORCG_TYPE_STRING || k == ORCG_TYPE_VARCHAR || k == ORCG_TYPE_CHAR || k == ORCG_TYPE_BINARY;
}
inline bool is_int_kind(uint32_t k) {
  return k == ORCG_TYPE_SHORT || k == ORCG_TYPE_INT || k == ORCG_TYPE_LONG || k == ORCG_TYPE_DATE;
}
inline bool is_timestamp_kind(uint32_t k) { return k == ORCG_TYPE_TIMESTAMP || k == ORCG_TYPE_TIMESTAMP_INSTANT; }
inline bool is_dict(uint32_t encoding) { return encoding == file::kDictionary || encoding == file::kDictionaryV2; }
// RLE v1 for DIRECT / DICTIONARY encodings (convertRleVersion,
// DictionaryLoader.hh:42) unless the reader always takes v2
inline bool rle_v1(uint32_t encoding, bool force_v2) {
  return !force_v2 && (encoding == file::kDirect || encoding == file::kDictionary);
}
// Decimal64ColumnReaderV2 (PostScript 1.9999 files): precision 1..18; 0 is a
// Hive 0.11 decimal
inline bool decimal64_v2(const file::TypeInfo& t, bool decimal_as_long) {
  return decimal_as_long && t.precision - 1u < 18u;
}

enum Coding : uint8_t { kRaw, kVarint, kIntRle, kByteRle, kBoolRle };
// what a stream holds one value for: each incoming row (PRESENT), each
// non-null row, or each dictionary entry
enum CountOf : uint8_t { kRows, kNonNull, kDictSize };

struct StreamDesc {
  int slot;
  Coding coding;
  bool is_signed;
  bool force_v2;  // integer RLE v2 whatever the encoding
  CountOf count;
  // a stream read whole with the dictionary has no row-index positions
  bool positioned() const { return count != kDictSize; }
  // position words a row-index entry holds for it after the byte position(s):
  // the values to skip in the run, for a boolean stream also the bits
  int position_extras() const { return coding == kBoolRle ? 2 : (coding == kRaw || coding == kVarint) ? 0 : 1; }
};

struct StreamLayout {
  StreamDesc s[4];
  int n = 0;
  void add(int slot, Coding c, bool sg = false, CountOf cnt = kNonNull, bool v2 = false) {
    s[n++] = StreamDesc{slot, c, sg, v2, cnt};
  }
  const StreamDesc* begin() const { return s; }
  const StreamDesc* end() const { return s + n; }
  const StreamDesc* find(int slot) const {
    for (const StreamDesc& d : *this)
      if (d.slot == slot) return &d;
    return nullptr;
  }
};

inline StreamLayout stream_layout(const file::TypeInfo& t, uint32_t encoding, bool decimal_as_long,
                                  bool has_present) {
  StreamLayout l;
  const uint32_t k = t.kind;
  if (has_present) l.add(kSlotPresent, kBoolRle, false, kRows);
  if (k == ORCG_TYPE_BOOLEAN) l.add(kSlotData, kBoolRle);
  else if (k == ORCG_TYPE_BYTE || k == ORCG_TYPE_UNION) l.add(kSlotData, kByteRle);  // union: the tags
  else if (is_int_kind(k)) l.add(kSlotData, kIntRle, true);
  else if (k == ORCG_TYPE_FLOAT || k == ORCG_TYPE_DOUBLE) l.add(kSlotData, kRaw);
  else if (is_string_kind(k)) {
    if (is_dict(encoding)) {
      l.add(kSlotLength, kIntRle, false, kDictSize);
      l.add(kSlotData, kIntRle);
    } else {
      l.add(kSlotData, kRaw);
      l.add(kSlotLength, kIntRle);
    }
  } else if (k == ORCG_TYPE_DECIMAL) {
    if (decimal64_v2(t, decimal_as_long)) l.add(kSlotData, kIntRle, true, kNonNull, true);
    else {
      l.add(kSlotData, kVarint, true);
      l.add(kSlotSecondary, kIntRle, true);  // the scales
    }
  } else if (is_timestamp_kind(k)) {
    l.add(kSlotData, kIntRle, true);  // seconds
    l.add(kSlotSecondary, kIntRle);   // nanoseconds
  } else if (k == ORCG_TYPE_LIST || k == ORCG_TYPE_MAP) {
    l.add(kSlotLength, kIntRle);
  }
  return l;
}

}  // namespace reader
}  // namespace orcg
