// RowReaderOptions::setTimezoneName through the C++ adapter
// (orc_amd/csrc/GpuRowReader.hh): reads <file.orc> in <zone> and prints the
// first rows of its first TIMESTAMP column, one "seconds nanoseconds" (or
// "null") per line. Zone rules are looked up under $TZDIR.
// Usage: timezone_test <file.orc> <zone> [rows]
#include <cstdio>
#include <cstdlib>

#include "../../orc_amd/csrc/GpuRowReader.hh"

using namespace orcg::cxx;

static const TimestampVectorBatch* find_timestamps(const ColumnVectorBatch& b) {
  if (auto* t = dynamic_cast<const TimestampVectorBatch*>(&b)) return t;
  if (auto* s = dynamic_cast<const StructVectorBatch*>(&b))
    for (const auto& f : s->fields)
      if (auto* t = find_timestamps(*f)) return t;
  return nullptr;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const uint64_t limit = argc > 3 ? strtoull(argv[3], nullptr, 10) : 3;
  try {
    Context ctx(0);
    Reader reader(ctx, argv[1], ReaderOptions());
    RowReaderOptions opts;
    if (opts.getTimezoneName() != "GMT") return 3;  // the reference's default
    opts.setTimezoneName(argv[2]);
    auto rows = reader.createRowReader(opts);
    auto batch = rows->createRowBatch(limit);
    if (!rows->next(*batch)) return 4;
    const TimestampVectorBatch* t = find_timestamps(*batch);
    if (!t) return 5;
    for (uint64_t i = 0; i < t->numElements && i < limit; ++i) {
      if (t->hasNulls && !t->notNull[i]) puts("null");
      else printf("%lld %lld\n", (long long)t->data[i], (long long)t->nanoseconds[i]);
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
