// IANA time zone rules on the host (no HIP dependency: this header and
// timezone.cpp compile alone with a C++17 host compiler).
//
// Mirrors the reference's Timezone (c++/src/Timezone.cc): TZif v1 / v2+
// parsing (:869-946), getVariant (:948-963), the POSIX future rule expanded
// over one 400-year cycle (:208-290, parser :307-466), getEpoch (:664-679),
// the zone directory (:681-695) and the US/* aliases (:47-59).
#ifndef ORCG_TIMEZONE_HH
#define ORCG_TIMEZONE_HH

#include <stdint.h>

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

struct orcg_timezone;  // the C ABI's handle (include/orcg.h)

namespace orcg {
namespace tz {

class Zone;
const Zone* zone_of(const orcg_timezone* t);

// the reference's TimezoneError (c++/src/Timezone.hh)
struct TimezoneError : std::runtime_error {
  explicit TimezoneError(const std::string& m) : std::runtime_error(m) {}
};

struct Variant {
  int64_t gmt_offset = 0;
  bool is_dst = false;
  std::string name;
  // TimezoneVariant::hasSameTzRule
  bool same_rule(const Variant& o) const { return gmt_offset == o.gmt_offset && is_dst == o.is_dst; }
};

constexpr int64_t kSecondsPerDay = 86400;
// leap years and week days repeat every 400 years (Timezone.cc:72-75)
constexpr int64_t kSecondsPer400Years = kSecondsPerDay * (365 * (300 + 3) + 366 * (100 - 3));
constexpr int64_t kOrcEpochUtc = 1420070400;  // 2015-01-01 00:00:00 UTC

// The last element <= target, or -1 (the reference's binarySearch,
// Timezone.cc:85-113, probe for probe: an unsorted array from a hostile file
// searches the same way everywhere)
int64_t search_le(const int64_t* a, uint64_t n, int64_t target);

// Words (int64) of the device table's header; timestamp_tz_kernel reads the
// same layout (decimal_kernels.hip).
//   word 0: ntrans (low 32) | ncycle (high 32)       ncycle is 1 or 801
//   word 1: ancient (low 32) | standard (high 32)    variants packed gmtOffset << 1 | isDst
//   word 2: dst (low 32) | startInStd (high 32)
//   word 3: lastTransition
//   word 4: epoch
//   word 5: 0 (keeps the arrays 16-byte aligned)
// then int64 trans[ntrans], int32 var[ntrans] (padded to 8 bytes), int64 cycle[ncycle]
constexpr uint32_t kTableHeaderWords = 6;
constexpr uint32_t kCycleEntries = 801;

class Zone {
 public:
  // Parses TZif bytes as if read from `name`; throws TimezoneError.
  static std::unique_ptr<Zone> parse(const std::string& name, const uint8_t* buf, uint64_t len);
  // zero offset, no transitions (the UTC names resolve to it)
  static std::unique_ptr<Zone> utc(const std::string& name);

  const Variant& variant(int64_t clk) const;
  int64_t epoch() const { return epoch_; }
  uint64_t version() const { return version_; }
  int64_t convert_to_utc(int64_t clk) const;
  int64_t convert_from_utc(int64_t clk) const;
  const std::string& name() const { return name_; }

  const std::vector<int64_t>& transitions() const { return trans_; }
  int64_t last_transition() const { return last_; }
  bool rule_defined() const { return rule_defined_; }
  bool start_in_std() const { return start_in_std_; }
  const std::vector<int64_t>& cycle() const { return cycle_; }

  // the flat table timestamp_tz_kernel searches
  std::vector<int64_t> device_table() const;

 private:
  friend struct RuleParser;
  void parse_section(const uint8_t* p, uint64_t section, uint64_t len, bool v2);
  void parse_rule(const std::string& rule);
  const Variant& rule_variant(int64_t clk) const;

  std::string name_;
  uint64_t version_ = 1;
  std::vector<Variant> variants_;
  std::vector<int64_t> trans_;
  std::vector<uint32_t> cur_;
  uint32_t ancient_ = 0;
  int64_t last_ = INT64_MAX;
  int64_t epoch_ = kOrcEpochUtc;
  // future rule
  bool rule_defined_ = false, has_dst_ = false, start_in_std_ = true;
  Variant std_, dst_;
  std::vector<int64_t> cycle_;
};

// the reference's US/* aliases applied (Timezone.cc:47-59)
std::string canonical_name(const std::string& name);
// the zones whose rules are UTC: no file is read for them
bool is_utc_name(const std::string& name);
// $TZDIR, else $CONDA_PREFIX/share/zoneinfo, else /usr/share/zoneinfo
std::string zone_directory();
// A zone name from a file becomes a path below the directory: empty, longer
// than 255 bytes, absolute, with a ".." component or a NUL is never opened.
bool safe_zone_name(const std::string& name);
// Reads <directory>/<canonical name>. false: not found (or an unsafe name);
// a file that is found but malformed throws TimezoneError.
bool load_zone_file(const std::string& name, std::unique_ptr<Zone>* out);

}  // namespace tz
}  // namespace orcg

#endif  // ORCG_TIMEZONE_HH
