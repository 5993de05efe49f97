// Hostile-input driver of the TZif parser (orc_amd/csrc/timezone.cpp), built
// with -fsanitize=address,undefined by tests/test_timezone_host.py: every
// prefix of a zone file, and every single-byte overwrite of the six header
// counts of both blocks with 0x00 / 0x7f / 0xff, must either parse or raise
// TimezoneError; a parsed zone must answer variant() and build its device
// table. Usage: tz_parse_test <zone file>. Exit 0, or 1 with a message.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orc_amd/csrc/timezone.hh"

using orcg::tz::Zone;

static unsigned long g_parsed = 0, g_rejected = 0;

static void feed(const std::vector<uint8_t>& b, size_t len) {
  // an exact-size copy: a read past `len` is a heap overflow the sanitizer sees
  std::vector<uint8_t> copy(b.begin(), b.begin() + (long)len);
  try {
    std::unique_ptr<Zone> z = Zone::parse("fuzz", copy.data(), copy.size());
    const int64_t probes[] = {INT64_MIN, -12622780801LL, -1, 0, 1420070400, 4108701600LL, 12622780800LL, INT64_MAX};
    int64_t sink = 0;
    for (int64_t p : probes) sink += z->variant(p).gmt_offset + z->convert_from_utc(p) + z->convert_to_utc(p);
    const std::vector<int64_t> t = z->device_table();
    if (t.size() < orcg::tz::kTableHeaderWords + z->transitions().size() + z->cycle().size()) {
      fprintf(stderr, "device table too small\n");
      exit(1);
    }
    (void)sink;
    ++g_parsed;
  } catch (const orcg::tz::TimezoneError&) {
    ++g_rejected;
  }
}

static uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | p[1] << 16 | p[2] << 8 | p[3]; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> b;
  int c;
  while ((c = fgetc(f)) != EOF) b.push_back((uint8_t)c);
  fclose(f);
  if (b.size() < 44) return 2;
  for (size_t len = 0; len <= b.size(); ++len) feed(b, len);
  // the second block starts where the first one ends
  const uint8_t* h = b.data() + 20;
  const size_t nt = be32(h + 12), nv = be32(h + 16), nn = be32(h + 20);
  const size_t second = 44 + nt * 5 + nv * 6 + nn + be32(h + 8) * 8 + be32(h) + be32(h + 4);
  const size_t headers[2] = {20, second + 20};
  const uint8_t values[3] = {0x00, 0x7f, 0xff};
  for (size_t hdr : headers) {
    if (hdr + 24 > b.size()) continue;
    for (size_t i = 0; i < 24; ++i)
      for (uint8_t v : values) {
        std::vector<uint8_t> m = b;
        m[hdr + i] = v;
        feed(m, m.size());
      }
  }
  // NULL / empty input
  try {
    Zone::parse("empty", nullptr, 0);
    return 1;
  } catch (const orcg::tz::TimezoneError&) {
  }
  printf("parsed %lu rejected %lu\n", g_parsed, g_rejected);
  return g_parsed > 0 && g_rejected > 0 ? 0 : 1;
}
