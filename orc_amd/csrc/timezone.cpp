// Time zone rules on the host (timezone.hh) and their C ABI (orcg_timezone_*,
// include/orcg.h). No HIP: the file compiles alone with a host compiler.
#include "timezone.hh"

#include <stdlib.h>
#include <string.h>

#include <cstdio>

#include "../../include/orcg.h"

namespace orcg {
namespace tz {

int64_t search_le(const int64_t* a, uint64_t n, int64_t target) {
  if (n == 0) return -1;
  uint64_t lo = 0, hi = n - 1, mid = (lo + hi) / 2;
  while (a[mid] != target && lo < hi) {
    if (a[mid] < target) lo = mid + 1;
    else hi = mid == 0 ? 0 : mid - 1;
    mid = (lo + hi) / 2;
  }
  return target < a[mid] ? (int64_t)mid - 1 : (int64_t)mid;
}

namespace {

bool is_leap(int64_t y) { return y % 4 == 0 && (y % 100 != 0 || y % 400 == 0); }

const int64_t kMonthDays[2][12] = {{31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31},
                                   {31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31}};

// one "day[/time]" of the rule (Timezone.cc Transition, :115-193)
struct RuleDay {
  enum Kind { kJulian, kDay, kMonth } kind = kDay;
  int64_t day = 0, week = 0, month = 0, time = 0;
  // seconds past local 1 January 00:00:00 of `year` (Transition::getTime);
  // unsigned sums: the fields come from the file
  int64_t at(int64_t year) const {
    uint64_t r = (uint64_t)time;
    const bool leap = is_leap(year);
    if (kind == kJulian) {
      r += (uint64_t)kSecondsPerDay * (uint64_t)day;
      if (day > 60 && leap) r += kSecondsPerDay;
    } else if (kind == kDay) {
      r += (uint64_t)kSecondsPerDay * (uint64_t)day;
    } else {
      // Zeller: week day of the month's first day
      const int64_t m = (month + 9) % 12 + 1;
      const int64_t y = month <= 2 ? year - 1 : year;
      const int64_t c = y / 100, yr = y % 100;
      int64_t dow = ((26 * m - 2) / 10 + 1 + yr + yr / 4 + c / 4 - 2 * c) % 7;
      if (dow < 0) dow += 7;
      int64_t d = day - dow;
      if (d < 0) d += 7;
      const int64_t* md = kMonthDays[leap];
      const int64_t mi = month - 1;  // checked 1..12 by the parser
      for (int64_t w = 1; w < week; ++w) {
        if (d + 7 >= md[mi]) break;
        d += 7;
      }
      r += (uint64_t)d * kSecondsPerDay;
      for (int64_t k = 0; k < mi; ++k) r += (uint64_t)md[k] * kSecondsPerDay;
    }
    return (int64_t)r;
  }
};

}  // namespace

// rule = name offset [name [offset] , day[/time] , day[/time]]
// (FutureRuleParser, Timezone.cc:307-466)
struct RuleParser {
  const std::string& s;
  size_t pos = 0;
  explicit RuleParser(const std::string& str) : s(str) {}

  [[noreturn]] void fail(const char* msg) const {
    throw TimezoneError(std::string(msg) + " at " + std::to_string(pos) + " in '" + s + "'");
  }
  char peek() const { return pos < s.size() ? s[pos] : '\0'; }
  static bool digit(char c) { return c >= '0' && c <= '9'; }

  std::string name() {
    if (pos == s.size()) fail("name required");
    const size_t start = pos;
    if (s[pos] == '<') {
      while (pos < s.size() && s[pos] != '>') ++pos;
      if (pos == s.size()) fail("missing close '>'");
      ++pos;
    } else {
      while (pos < s.size() && !digit(s[pos]) && s[pos] != '-' && s[pos] != '+' && s[pos] != ',') ++pos;
    }
    if (pos == start) fail("empty string not allowed");
    return s.substr(start, pos - start);
  }
  int64_t number() {
    if (pos >= s.size()) fail("missing number");
    uint64_t v = 0;  // wraps on absurd input, as any 64-bit accumulation does
    while (pos < s.size() && digit(s[pos])) v = v * 10 + (uint64_t)(s[pos++] - '0');
    return (int64_t)v;
  }
  int64_t offset() {
    int64_t scale = 3600;
    bool neg = false;
    if (pos < s.size() && (s[pos] == '-' || s[pos] == '+')) neg = s[pos++] == '-';
    uint64_t v = (uint64_t)number() * (uint64_t)scale;
    while (pos < s.size() && scale > 1 && s[pos] == ':') {
      scale /= 60;
      ++pos;
      v += (uint64_t)number() * (uint64_t)scale;
    }
    return (int64_t)(neg ? 0 - v : v);
  }
  void day(RuleDay& d) {
    if (s.size() - pos < 2 || s[pos] != ',') fail("missing transition");
    ++pos;
    if (s[pos] == 'J') {
      d.kind = RuleDay::kJulian;
      ++pos;
      d.day = number();
    } else if (s[pos] == 'M') {
      d.kind = RuleDay::kMonth;
      ++pos;
      d.month = number();
      if (peek() != '.') fail("missing first .");
      ++pos;
      d.week = number();
      if (peek() != '.') fail("missing second .");
      ++pos;
      d.day = number();
      // the month indexes the days-per-month table
      if (d.month < 1 || d.month > 12) fail("month out of range");
    } else {
      d.kind = RuleDay::kDay;
      d.day = number();
    }
    if (peek() == '/') {
      ++pos;
      d.time = offset();
    } else {
      d.time = 2 * 60 * 60;
    }
  }
};

void Zone::parse_rule(const std::string& rule) {
  rule_defined_ = !rule.empty();
  has_dst_ = false;
  start_in_std_ = true;
  cycle_.assign(1, 0);
  if (!rule_defined_) return;
  RuleParser p(rule);
  RuleDay start, end;
  std_.name = p.name();
  std_.gmt_offset = (int64_t)(0 - (uint64_t)p.offset());
  std_.is_dst = false;
  has_dst_ = p.pos < rule.size();
  if (has_dst_) {
    dst_.name = p.name();
    dst_.is_dst = true;
    if (p.peek() != ',') dst_.gmt_offset = (int64_t)(0 - (uint64_t)p.offset());
    else dst_.gmt_offset = std_.gmt_offset + 60 * 60;
    p.day(start);
    p.day(end);
  }
  if (p.pos != rule.size()) p.fail("Extra text");
  if (!has_dst_) return;
  // computeOffsets (:225-252): the epoch, then two transitions a year
  cycle_.assign(kCycleEntries, 0);
  start_in_std_ = start.at(1970) < end.at(1970);
  uint64_t base = 0;
  for (int64_t y = 1970; y < 1970 + 400; ++y) {
    const uint64_t to_dst = base + (uint64_t)start.at(y) - (uint64_t)std_.gmt_offset;
    const uint64_t to_std = base + (uint64_t)end.at(y) - (uint64_t)dst_.gmt_offset;
    const size_t k = (size_t)(y - 1970) * 2;
    cycle_[k + 1] = (int64_t)(start_in_std_ ? to_dst : to_std);
    cycle_[k + 2] = (int64_t)(start_in_std_ ? to_std : to_dst);
    base += (uint64_t)(is_leap(y) ? 366 : 365) * kSecondsPerDay;
  }
}

const Variant& Zone::rule_variant(int64_t clk) const {
  if (!has_dst_) return std_;
  int64_t adj = clk % kSecondsPer400Years;
  if (adj < 0) adj += kSecondsPer400Years;
  const int64_t idx = search_le(cycle_.data(), cycle_.size(), adj);
  return start_in_std_ == (idx % 2 == 0) ? std_ : dst_;
}

const Variant& Zone::variant(int64_t clk) const {
  if (clk > last_) return rule_variant(clk);
  const int64_t i = search_le(trans_.data(), trans_.size(), clk);
  return variants_[i < 0 ? ancient_ : cur_[(size_t)i]];
}

int64_t Zone::convert_to_utc(int64_t clk) const { return (int64_t)((uint64_t)clk + (uint64_t)variant(clk).gmt_offset); }

int64_t Zone::convert_from_utc(int64_t clk) const {
  const int64_t adj = (int64_t)((uint64_t)clk - (uint64_t)variant(clk).gmt_offset);
  return (int64_t)((uint64_t)clk - (uint64_t)variant(adj).gmt_offset);
}

static uint32_t be32(const uint8_t* p) {
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}

// One TZif block at `section` (parseZoneFile, :869-946). Every count is a
// 32-bit value from the file: the block's end is computed in 64 bits (six
// counts times at most 12 cannot wrap) and checked against `len` before any
// byte past the header is read.
void Zone::parse_section(const uint8_t* p, uint64_t section, uint64_t len, bool v2) {
  const uint64_t header = section + 20;
  if (len < header + 24 || memcmp(p + section, "TZif", 4) != 0) throw TimezoneError("non-tzfile " + name_);
  const uint64_t n_gmt = be32(p + header), n_std = be32(p + header + 4), n_leap = be32(p + header + 8);
  const uint64_t n_time = be32(p + header + 12), n_var = be32(p + header + 16), n_name = be32(p + header + 20);
  const uint64_t tsize = v2 ? 8 : 4;
  const uint64_t time_off = header + 24;
  const uint64_t idx_off = time_off + tsize * n_time;
  const uint64_t var_off = idx_off + n_time;
  const uint64_t name_off = var_off + n_var * 6;
  const uint64_t end = name_off + n_name + (tsize + 4) * n_leap + n_gmt + n_std;
  if (end > len)
    throw TimezoneError("tzfile too short " + name_ + " needs " + std::to_string(end) + " and has " +
                        std::to_string(len));
  // a v2+ file: the 64-bit block after the v1 block replaces it
  if (section == 0 && p[4] != 0) {
    parse_section(p, end, len, true);
    return;
  }
  version_ = v2 ? 2 : 1;
  variants_.assign(n_var, Variant());
  for (uint64_t v = 0; v < n_var; ++v) {
    const uint8_t* q = p + var_off + 6 * v;
    variants_[v].gmt_offset = (int32_t)be32(q);
    variants_[v].is_dst = q[4] != 0;
    const uint64_t at = q[5];
    if (at >= n_name)
      throw TimezoneError("name out of range in variant " + std::to_string(v) + " - " + std::to_string(at) +
                          " >= " + std::to_string(n_name));
    // the name ends at its NUL or at the end of the name block
    const char* s = (const char*)p + name_off + at;
    variants_[v].name.assign(s, strnlen(s, n_name - at));
  }
  trans_.assign(n_time, 0);
  cur_.assign(n_time, 0);
  bool found = false;
  ancient_ = 0;
  for (uint64_t t = 0; t < n_time; ++t) {
    const uint8_t* q = p + time_off + t * tsize;
    trans_[t] = v2 ? (int64_t)((uint64_t)be32(q) << 32 | be32(q + 4)) : (int64_t)(int32_t)be32(q);
    cur_[t] = p[idx_off + t];
    if (cur_[t] >= n_var)
      throw TimezoneError("tzfile rule out of range " + name_ + " references rule " + std::to_string(cur_[t]) +
                          " of " + std::to_string(n_var));
    // the oldest standard time is the variant before the first transition
    if (!found && !variants_[cur_[t]].is_dst) {
      found = true;
      ancient_ = cur_[t];
    }
  }
  if (variants_.empty()) throw TimezoneError("tzfile too short " + name_ + " has no time variants");
  // the footer "\n<rule>\n" of a v2+ file
  std::string rule;
  if (v2 && len - end >= 2) rule.assign((const char*)p + end + 1, len - end - 2);
  parse_rule(rule);
  last_ = rule_defined_ ? (n_time ? trans_[n_time - 1] : INT64_MIN) : INT64_MAX;
}

std::unique_ptr<Zone> Zone::parse(const std::string& name, const uint8_t* buf, uint64_t len) {
  std::unique_ptr<Zone> z(new Zone());
  z->name_ = name;
  static const uint8_t kNone = 0;
  z->parse_section(buf ? buf : &kNone, 0, buf ? len : 0, false);
  z->epoch_ = kOrcEpochUtc - z->variant(kOrcEpochUtc).gmt_offset;
  return z;
}

std::unique_ptr<Zone> Zone::utc(const std::string& name) {
  std::unique_ptr<Zone> z(new Zone());
  z->name_ = name;
  z->variants_.assign(1, Variant());
  z->variants_[0].name = "UTC";
  z->parse_rule("");
  return z;
}

std::vector<int64_t> Zone::device_table() const {
  auto pack = [](const Variant& v) { return (uint32_t)(((uint64_t)v.gmt_offset << 1) | (v.is_dst ? 1u : 0u)); };
  const uint64_t n = trans_.size(), nc = cycle_.size();
  std::vector<int64_t> t(kTableHeaderWords + n + (n + 1) / 2 + nc, 0);
  const Variant& s = rule_defined_ ? std_ : variants_[ancient_];
  const Variant& d = has_dst_ ? dst_ : s;
  t[0] = (int64_t)(n | nc << 32);
  t[1] = (int64_t)((uint64_t)pack(variants_[ancient_]) | (uint64_t)pack(s) << 32);
  t[2] = (int64_t)((uint64_t)pack(d) | (uint64_t)(start_in_std_ ? 1 : 0) << 32);
  t[3] = last_;
  t[4] = epoch_;
  int64_t* tr = t.data() + kTableHeaderWords;
  int32_t* var = (int32_t*)(tr + n);
  int64_t* cy = tr + n + (n + 1) / 2;
  for (uint64_t i = 0; i < n; ++i) {
    tr[i] = trans_[i];
    var[i] = (int32_t)pack(variants_[cur_[i]]);
  }
  for (uint64_t i = 0; i < nc; ++i) cy[i] = cycle_[i];
  return t;
}

std::string canonical_name(const std::string& name) {
  static const char* kAlias[][2] = {{"US/Alaska", "America/Anchorage"},
                                    {"US/Aleutian", "America/Adak"},
                                    {"US/Arizona", "America/Phoenix"},
                                    {"US/Central", "America/Chicago"},
                                    {"US/East-Indiana", "America/Indiana/Indianapolis"},
                                    {"US/Eastern", "America/New_York"},
                                    {"US/Hawaii", "Pacific/Honolulu"},
                                    {"US/Indiana-Starke", "America/Indiana/Knox"},
                                    {"US/Michigan", "America/Detroit"},
                                    {"US/Mountain", "America/Denver"},
                                    {"US/Pacific", "America/Los_Angeles"},
                                    {"US/Samoa", "Pacific/Pago_Pago"}};
  for (auto& a : kAlias)
    if (name == a[0]) return a[1];
  return name;
}

bool is_utc_name(const std::string& z) {
  static const char* kUtc[] = {"GMT", "UTC", "UCT", "Zulu", "Universal", "Greenwich", "GMT0", "GMT+0", "GMT-0",
                               "Etc/GMT", "Etc/UTC", "Etc/UCT", "Etc/Zulu", "Etc/Universal", "Etc/Greenwich",
                               "Etc/GMT0", "Etc/GMT+0", "Etc/GMT-0"};
  for (const char* u : kUtc)
    if (z == u) return true;
  return false;
}

std::string zone_directory() {
  if (const char* d = getenv("TZDIR")) return d;
  if (const char* c = getenv("CONDA_PREFIX")) return std::string(c) + "/share/zoneinfo";
  return "/usr/share/zoneinfo";
}

bool safe_zone_name(const std::string& n) {
  if (n.empty() || n.size() > 255 || n[0] == '/' || n.find('\0') != std::string::npos) return false;
  size_t at = 0;
  while (at <= n.size()) {
    size_t e = n.find('/', at);
    if (e == std::string::npos) e = n.size();
    if (e - at == 2 && n[at] == '.' && n[at + 1] == '.') return false;
    at = e + 1;
  }
  return true;
}

bool load_zone_file(const std::string& name, std::unique_ptr<Zone>* out) {
  const std::string canon = canonical_name(name);
  if (!safe_zone_name(canon)) return false;
  const std::string path = zone_directory() + "/" + canon;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  std::vector<uint8_t> buf;
  uint8_t chunk[4096];
  size_t got;
  // zone files are a few KB; 1 MiB is no zone file
  while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0 && buf.size() <= (1u << 20)) buf.insert(buf.end(), chunk, chunk + got);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) return false;  // a directory, an unreadable file
  *out = Zone::parse(path, buf.data(), buf.size());
  return true;
}

}  // namespace tz
}  // namespace orcg

// ---- C ABI (include/orcg.h) -------------------------------------------------

struct orcg_timezone {
  std::unique_ptr<orcg::tz::Zone> z;
};

namespace {
thread_local std::string t_tz_error;
}

extern "C" {

const char* orcg_timezone_last_error(void) { return t_tz_error.c_str(); }

int orcg_timezone_parse(const char* name, const uint8_t* tzif, uint64_t len, orcg_timezone** out) {
  if (!name || (len && !tzif) || !out) return ORCG_INVALID_ARGUMENT;
  *out = nullptr;
  try {
    std::unique_ptr<orcg_timezone> t(new orcg_timezone());
    t->z = orcg::tz::Zone::parse(name, tzif, len);
    *out = t.release();
    return ORCG_OK;
  } catch (const orcg::tz::TimezoneError& e) {
    t_tz_error = e.what();
    return ORCG_PARSE_ERROR;
  } catch (const std::bad_alloc&) {
    t_tz_error = "out of memory";
    return ORCG_OUT_OF_MEMORY;
  }
}

int orcg_timezone_load(const char* name, orcg_timezone** out) {
  if (!name || !out) return ORCG_INVALID_ARGUMENT;
  *out = nullptr;
  try {
    std::unique_ptr<orcg_timezone> t(new orcg_timezone());
    const std::string n(name);
    if (orcg::tz::is_utc_name(n)) {
      t->z = orcg::tz::Zone::utc(n);
    } else if (!orcg::tz::load_zone_file(n, &t->z)) {
      t_tz_error = "Time zone file " + orcg::tz::zone_directory() + "/" + orcg::tz::canonical_name(n) +
                   " does not exist. Please install IANA time zone database and set TZDIR env.";
      return ORCG_INVALID_ARGUMENT;
    }
    *out = t.release();
    return ORCG_OK;
  } catch (const orcg::tz::TimezoneError& e) {
    t_tz_error = e.what();
    return ORCG_PARSE_ERROR;
  } catch (const std::bad_alloc&) {
    t_tz_error = "out of memory";
    return ORCG_OUT_OF_MEMORY;
  }
}

void orcg_timezone_destroy(orcg_timezone* tz) { delete tz; }
uint64_t orcg_timezone_version(const orcg_timezone* tz) { return tz ? tz->z->version() : 0; }
int64_t orcg_timezone_epoch(const orcg_timezone* tz) { return tz ? tz->z->epoch() : orcg::tz::kOrcEpochUtc; }

int orcg_timezone_variant(const orcg_timezone* tz, int64_t clk, int64_t* gmt_offset, int* is_dst, const char** name) {
  if (!tz) return ORCG_INVALID_ARGUMENT;
  const orcg::tz::Variant& v = tz->z->variant(clk);
  if (gmt_offset) *gmt_offset = v.gmt_offset;
  if (is_dst) *is_dst = v.is_dst ? 1 : 0;
  if (name) *name = v.name.c_str();
  return ORCG_OK;
}

int64_t orcg_timezone_convert_to_utc(const orcg_timezone* tz, int64_t clk) {
  return tz ? tz->z->convert_to_utc(clk) : clk;
}
int64_t orcg_timezone_convert_from_utc(const orcg_timezone* tz, int64_t clk) {
  return tz ? tz->z->convert_from_utc(clk) : clk;
}

}  // extern "C"

namespace orcg {
namespace tz {
const Zone* zone_of(const orcg_timezone* t) { return t ? t->z.get() : nullptr; }
}  // namespace tz
}  // namespace orcg
