// Schema evolution through the C++ RowReader adapter
// (orc_amd/csrc/GpuRowReader.hh): RowReaderOptions::setReadType /
// throwOnSchemaEvolutionOverflow with tight numeric vectors, as the
// reference's TestConvertColumnReader.cc reads its files.
//
//   read_type_reader_test <file.orc> <read type> [--batch N] [--throw] [--loose]
//
// Prints one line per row: the top-level columns separated by blanks, each
// "N" for a NULL, an integer, a decimal's unscaled value with "@scale", or a
// float / double as the hex of its bits ("f" / "d" prefix), and before the
// rows one line "#classes" naming each column's batch class. --loose leaves
// setUseTightNumericVector off (the reference refuses that). Errors go to
// stdout as "#error <text>" with exit status 2.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../orc_amd/csrc/GpuRowReader.hh"

using namespace orcg::cxx;

static std::string int128_str(__int128 v) {
  const bool neg = v < 0;
  unsigned __int128 m = neg ? (unsigned __int128)(-(v + 1)) + 1 : (unsigned __int128)v;
  std::string digits;
  do {
    digits.insert(digits.begin(), (char)('0' + (int)(m % 10)));
    m /= 10;
  } while (m);
  return (neg ? "-" : "") + digits;
}

static const char* class_name(BatchClass c) {
  switch (c) {
    case BatchClass::kLong: return "long";
    case BatchClass::kInt: return "int";
    case BatchClass::kShort: return "short";
    case BatchClass::kByte: return "byte";
    case BatchClass::kDouble: return "double";
    case BatchClass::kFloat: return "float";
    case BatchClass::kDecimal64: return "decimal64";
    case BatchClass::kDecimal128: return "decimal128";
    default: return "other";
  }
}

static std::string cell(const ColumnVectorBatch& b, uint64_t i) {
  if (b.hasNulls && !b.notNull[i]) return "N";
  char buf[64];
  switch (b.cls) {
    case BatchClass::kLong: return std::to_string(static_cast<const LongVectorBatch&>(b).data[i]);
    case BatchClass::kInt: return std::to_string(static_cast<const IntVectorBatch&>(b).data[i]);
    case BatchClass::kShort: return std::to_string(static_cast<const ShortVectorBatch&>(b).data[i]);
    case BatchClass::kByte: return std::to_string((int)static_cast<const ByteVectorBatch&>(b).data[i]);
    case BatchClass::kDouble: {
      uint64_t u;
      memcpy(&u, &static_cast<const DoubleVectorBatch&>(b).data[i], 8);
      snprintf(buf, sizeof buf, "d%016llx", (unsigned long long)u);
      return buf;
    }
    case BatchClass::kFloat: {
      uint32_t u;
      memcpy(&u, &static_cast<const FloatVectorBatch&>(b).data[i], 4);
      snprintf(buf, sizeof buf, "f%08x", u);
      return buf;
    }
    case BatchClass::kDecimal64: {
      const auto& d = static_cast<const Decimal64VectorBatch&>(b);
      return std::to_string(d.values[i]) + "@" + std::to_string(d.scale);
    }
    case BatchClass::kDecimal128: {
      const auto& d = static_cast<const Decimal128VectorBatch&>(b);
      const __int128 v = (__int128)(((unsigned __int128)(uint64_t)d.values[i].highbits << 64) | d.values[i].lowbits);
      return int128_str(v) + "@" + std::to_string(d.scale);
    }
    default: return "?";
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  uint64_t batch = 1000;
  bool thrown = false, tight = true;
  for (int i = 3; i < argc; ++i) {
    if (!strcmp(argv[i], "--batch") && i + 1 < argc) batch = strtoull(argv[++i], nullptr, 10);
    else if (!strcmp(argv[i], "--throw")) thrown = true;
    else if (!strcmp(argv[i], "--loose")) tight = false;
  }
  try {
    Context ctx(0);
    Reader reader(ctx, argv[1]);
    RowReaderOptions opts;
    opts.setReadType(argv[2]).throwOnSchemaEvolutionOverflow(thrown).setUseTightNumericVector(tight);
    auto rr = reader.createRowReader(opts);
    // the option does not stay on the reader: a second row reader reads the file's types
    auto plain = reader.createRowReader(RowReaderOptions().setUseTightNumericVector(true));
    auto b = rr->createRowBatch(batch);
    auto& root = static_cast<StructVectorBatch&>(*b);
    printf("#classes");
    for (auto& f : root.fields) printf(" %s", class_name(f->cls));
    printf("\n#plain");
    auto pb = plain->createRowBatch(batch);
    for (auto& f : static_cast<StructVectorBatch&>(*pb).fields) printf(" %s", class_name(f->cls));
    printf("\n");
    uint64_t rows = 0;
    while (rr->next(*b)) {
      if (b->numElements > batch) return 3;
      for (uint64_t i = 0; i < b->numElements; ++i) {
        for (size_t c = 0; c < root.fields.size(); ++c) printf(c ? " %s" : "%s", cell(*root.fields[c], i).c_str());
        printf("\n");
      }
      rows += b->numElements;
    }
    if (rows != reader.getNumberOfRows()) return 4;
  } catch (const std::exception& e) {
    printf("#error %s\n", e.what());
    return 2;
  }
  return 0;
}
