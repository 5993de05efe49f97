// orc_amd/csrc/reader_layout.hh: the ordered stream list of every column
// kind x encoding the reader supports, written out here by hand. The order of
// the positioned streams is the order the reference's column readers seek
// them (c++/src/ColumnReader.cc seekToRowGroup, cited per case); a
// dictionary's LENGTH stream is read whole by the dictionary loader and comes
// before them with no row-index positions.
#include <cstdio>
#include <string>
#include <vector>

#include "../../orc_amd/csrc/reader_layout.hh"

using namespace orcg::reader;
using orcg::file::kDictionary;
using orcg::file::kDictionaryV2;
using orcg::file::kDirect;
using orcg::file::kDirectV2;

namespace {

struct Want {
  int slot;
  Coding coding;
  bool is_signed;
  bool force_v2;
  CountOf count;
};

int failures = 0;

void fail(const std::string& what, const char* why) {
  std::fprintf(stderr, "FAIL %s: %s\n", what.c_str(), why);
  ++failures;
}

// the column's list with and without a PRESENT stream: PRESENT (boolean RLE,
// one bit per incoming row) leads when the column has one
// (ColumnReader::seekToRowGroup, ColumnReader.cc:106-110, runs first in every
// reader's seekToRowGroup)
void check(const char* name, uint32_t kind, uint32_t encoding, uint32_t precision, bool decimal_as_long,
           const std::vector<Want>& want) {
  orcg::file::TypeInfo t;
  t.kind = kind;
  t.precision = precision;
  for (int present = 0; present < 2; ++present) {
    const std::string what = std::string(name) + " encoding " + std::to_string(encoding) + " precision " +
                             std::to_string(precision) + (decimal_as_long ? " as long" : "") +
                             (present ? " with PRESENT" : "");
    std::vector<Want> all;
    if (present) all.push_back({kSlotPresent, kBoolRle, false, false, kRows});
    all.insert(all.end(), want.begin(), want.end());
    const StreamLayout l = stream_layout(t, encoding, decimal_as_long, present != 0);
    if ((size_t)l.n != all.size()) {
      fail(what, "stream count");
      continue;
    }
    for (size_t i = 0; i < all.size(); ++i) {
      const StreamDesc& d = l.s[i];
      if (d.slot != all[i].slot) fail(what, "slot");
      if (d.coding != all[i].coding) fail(what, "coding");
      if (d.is_signed != all[i].is_signed) fail(what, "signedness");
      if (d.force_v2 != all[i].force_v2) fail(what, "force_v2");
      if (d.count != all[i].count) fail(what, "count source");
      if (l.find(all[i].slot) != &d) fail(what, "find");
    }
    if (l.find(kSlotDict)) fail(what, "DICTIONARY_DATA is a blob, not a listed stream");
    if (!present && l.find(kSlotPresent)) fail(what, "PRESENT listed without one");
  }
}

const uint32_t kAll[] = {kDirect, kDictionary, kDirectV2, kDictionaryV2};

}  // namespace

int main() {
  const bool S = true, U = false, V2 = true, ANY = false;
  for (uint32_t e : kAll) {
    // BooleanColumnReader::seekToRowGroup :181-186; ByteColumnReader :218-222
    check("BOOLEAN", ORCG_TYPE_BOOLEAN, e, 0, false, {{kSlotData, kBoolRle, U, ANY, kNonNull}});
    check("BYTE", ORCG_TYPE_BYTE, e, 0, false, {{kSlotData, kByteRle, U, ANY, kNonNull}});
    // IntegerColumnReader :254-257: signed RLE
    for (uint32_t k : {ORCG_TYPE_SHORT, ORCG_TYPE_INT, ORCG_TYPE_LONG, ORCG_TYPE_DATE})
      check("integer", k, e, 0, false, {{kSlotData, kIntRle, S, ANY, kNonNull}});
    // DoubleColumnReader :484-489: raw IEEE bytes
    check("FLOAT", ORCG_TYPE_FLOAT, e, 0, false, {{kSlotData, kRaw, U, ANY, kNonNull}});
    check("DOUBLE", ORCG_TYPE_DOUBLE, e, 0, false, {{kSlotData, kRaw, U, ANY, kNonNull}});
    // TimestampColumnReader :351-356: seconds (signed), then nanoseconds (unsigned)
    for (uint32_t k : {ORCG_TYPE_TIMESTAMP, ORCG_TYPE_TIMESTAMP_INSTANT})
      check("timestamp", k, e, 0, false,
            {{kSlotData, kIntRle, S, ANY, kNonNull}, {kSlotSecondary, kIntRle, U, ANY, kNonNull}});
    // ListColumnReader :996-1001, MapColumnReader :1137-1146: unsigned lengths
    check("LIST", ORCG_TYPE_LIST, e, 0, false, {{kSlotLength, kIntRle, U, ANY, kNonNull}});
    check("MAP", ORCG_TYPE_MAP, e, 0, false, {{kSlotLength, kIntRle, U, ANY, kNonNull}});
    // StructColumnReader :873-880: PRESENT only; UnionColumnReader :1276-1284: byte-RLE tags
    check("STRUCT", ORCG_TYPE_STRUCT, e, 0, false, {});
    check("UNION", ORCG_TYPE_UNION, e, 0, false, {{kSlotData, kByteRle, U, ANY, kNonNull}});
    // Decimal64 / Decimal128 / DecimalHive11 (precision 0) readers,
    // Decimal64ColumnReader::seekToRowGroup :1458-1464: varint values, then
    // signed scales; a PostScript-1.9999 file's precision 1..18 columns are
    // Decimal64ColumnReaderV2 (:1544-1556: one signed RLEv2 DATA stream)
    const std::vector<Want> varint = {{kSlotData, kVarint, S, ANY, kNonNull}, {kSlotSecondary, kIntRle, S, ANY, kNonNull}};
    for (uint32_t p : {0u, 10u, 20u}) check("DECIMAL", ORCG_TYPE_DECIMAL, e, p, false, varint);
    check("DECIMAL", ORCG_TYPE_DECIMAL, e, 0, true, varint);
    check("DECIMAL", ORCG_TYPE_DECIMAL, e, 20, true, varint);
    check("DECIMAL", ORCG_TYPE_DECIMAL, e, 10, true, {{kSlotData, kIntRle, S, V2, kNonNull}});
  }
  for (uint32_t k : {ORCG_TYPE_STRING, ORCG_TYPE_VARCHAR, ORCG_TYPE_CHAR, ORCG_TYPE_BINARY}) {
    // StringDirectColumnReader::seekToRowGroup :785-790: the blob, then its lengths
    for (uint32_t e : {kDirect, kDirectV2})
      check("direct string", k, e, 0, false,
            {{kSlotData, kRaw, U, ANY, kNonNull}, {kSlotLength, kIntRle, U, ANY, kNonNull}});
    // StringDictionaryColumnReader: the dictionary's LENGTH (one value per
    // entry, loaded whole: DictionaryLoader.cc:43-97), then the row's entry
    // indices, the only positioned stream (seekToRowGroup :609-613)
    for (uint32_t e : {kDictionary, kDictionaryV2})
      check("dictionary string", k, e, 0, false,
            {{kSlotLength, kIntRle, U, ANY, kDictSize}, {kSlotData, kIntRle, U, ANY, kNonNull}});
  }

  // the predicates the list is built from
  if (is_dict(kDirect) || is_dict(kDirectV2) || !is_dict(kDictionary) || !is_dict(kDictionaryV2))
    fail("is_dict", "encoding");
  if (!rle_v1(kDirect, false) || !rle_v1(kDictionary, false) || rle_v1(kDirectV2, false) ||
      rle_v1(kDictionaryV2, false) || rle_v1(kDirect, true) || rle_v1(kDictionary, true))
    fail("rle_v1", "version");
  // row-index entries: byte position(s), then per coding the run's values to
  // skip (RLE) and the bits to skip (boolean); a dictionary's LENGTH has none
  const StreamDesc bits{kSlotPresent, kBoolRle, false, false, kRows}, ints{kSlotData, kIntRle, true, false, kNonNull},
      raw{kSlotData, kRaw, false, false, kNonNull}, var{kSlotData, kVarint, true, false, kNonNull},
      bytes{kSlotData, kByteRle, false, false, kNonNull}, dlen{kSlotLength, kIntRle, false, false, kDictSize};
  if (bits.position_extras() != 2 || ints.position_extras() != 1 || bytes.position_extras() != 1 ||
      raw.position_extras() != 0 || var.position_extras() != 0)
    fail("position_extras", "count");
  if (!bits.positioned() || !ints.positioned() || !raw.positioned() || dlen.positioned()) fail("positioned", "flag");
  const uint32_t kinds[] = {orcg::file::kPresent, orcg::file::kData, orcg::file::kLength, orcg::file::kDictionaryData,
                            orcg::file::kSecondary};
  const int slots[] = {kSlotPresent, kSlotData, kSlotLength, kSlotDict, kSlotSecondary};
  for (int i = 0; i < 5; ++i)
    if (slot_of(kinds[i]) != slots[i]) fail("slot_of", "slot");
  if (slot_of(orcg::file::kRowIndex) != -1 || slot_of(orcg::file::kDictionaryCount) != -1) fail("slot_of", "no slot");

  if (failures) return 1;
  std::printf("stream layouts ok\n");
  return 0;
}
