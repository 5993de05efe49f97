// Schema evolution on the host: the type-string parser (the grammar of
// Type::buildTypeFromString, c++/src/TypeImpl.cc:688-960, the inverse of
// Type::toString) and the check of a file type against a read type
// (checkConversion / buildConversion, c++/src/SchemaEvolution.cc:79-159).
// Host-only C++ with no HIP dependency (tests/cxx/read_type_test.cpp).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

namespace orcg {
namespace rt {

// Type.Kind (the ORCG_TYPE_* values of include/orcg_reader.h)
enum Kind : uint32_t {
  kBoolean = 0, kByte = 1, kShort = 2, kInt = 3, kLong = 4, kFloat = 5, kDouble = 6, kString = 7, kBinary = 8,
  kTimestamp = 9, kList = 10, kMap = 11, kStruct = 12, kUnion = 13, kDecimal = 14, kDate = 15, kVarchar = 16,
  kChar = 17, kTimestampInstant = 18, kNumKinds = 19
};

// One node of a type tree; a tree is a vector in pre-order, so a node's index
// is its column id (Type::getColumnId).
struct Node {
  uint32_t kind = 0, maximum_length = 0, precision = 0, scale = 0;
  std::vector<uint32_t> subtypes;
  std::vector<std::string> field_names;
};
using Tree = std::vector<Node>;

inline const char* kind_name(uint32_t k) {
  static const char* const names[kNumKinds] = {"boolean", "tinyint", "smallint", "int", "bigint", "float", "double",
                                               "string", "binary", "timestamp", "array", "map", "struct", "uniontype",
                                               "decimal", "date", "varchar", "char", "timestamp with local time zone"};
  return k < kNumKinds ? names[k] : "unknown";
}

// Type::toString (TypeImpl.cc), as Reader.type_string prints it
inline std::string to_string(const Tree& t, uint32_t id = 0) {
  const Node& n = t[id];
  auto list = [&](bool names) {
    std::string s = std::string(kind_name(n.kind)) + "<";
    for (size_t i = 0; i < n.subtypes.size(); ++i) {
      if (i) s += ",";
      if (names) s += (i < n.field_names.size() ? n.field_names[i] : std::string()) + ":";
      s += to_string(t, n.subtypes[i]);
    }
    return s + ">";
  };
  switch (n.kind) {
    case kStruct: return list(true);
    case kList:
    case kMap:
    case kUnion: return list(false);
    case kDecimal: return "decimal(" + std::to_string(n.precision) + "," + std::to_string(n.scale) + ")";
    case kVarchar:
    case kChar: return std::string(kind_name(n.kind)) + "(" + std::to_string(n.maximum_length) + ")";
    default: return kind_name(n.kind);
  }
}

class Parser {
 public:
  Parser(const std::string& s, Tree* out) : s_(s), out_(out) {}

  bool run(std::string* err) {
    out_->clear();
    if (!type() || (pos_ != s_.size() && fail("Invalid type string."))) {
      out_->clear();
      if (err) *err = err_;
      return false;
    }
    return true;
  }

 private:
  bool fail(const std::string& m) {
    if (err_.empty()) err_ = m;
    return true;  // so that `cond && fail(...)` reads as "failed"
  }
  bool eat(char c) {
    if (pos_ < s_.size() && s_[pos_] == c) {
      ++pos_;
      return true;
    }
    return false;
  }
  bool number(uint32_t* v) {
    const size_t b = pos_;
    uint64_t x = 0;
    while (pos_ < s_.size() && s_[pos_] >= '0' && s_[pos_] <= '9' && x <= 0xffffffffull) x = x * 10 + (s_[pos_++] - '0');
    *v = (uint32_t)x;
    return pos_ > b && x <= 0xffffffffull;
  }
  // the category name: letters, and the blanks of "timestamp with local time zone"
  std::string word() {
    const size_t b = pos_;
    while (pos_ < s_.size() && ((s_[pos_] >= 'a' && s_[pos_] <= 'z') || s_[pos_] == ' ')) ++pos_;
    return s_.substr(b, pos_ - b);
  }
  // a field name: plain up to ':', or `quoted` with `` for a back quote
  bool field_name(std::string* name) {
    name->clear();
    if (eat('`')) {
      for (;;) {
        if (pos_ >= s_.size()) return !fail("Invalid field name. Unmatched quote");
        const char c = s_[pos_++];
        if (c == '`') {
          if (!eat('`')) break;
        }
        name->push_back(c);
      }
      if (name->empty()) return !fail("Empty quoted field name.");
    } else {
      while (pos_ < s_.size() && s_[pos_] != ':' && s_[pos_] != '<' && s_[pos_] != '>' && s_[pos_] != ',') name->push_back(s_[pos_++]);
      if (name->empty()) return !fail("Missing field name.");
    }
    return true;
  }
  // "<" sub types ">" of node `id`: exactly `want` of them (0 = one or more;
  // a struct may be empty)
  bool children(uint32_t id, const char* what, size_t want, bool names) {
    if (!eat('<')) return !fail(std::string("Missing < after ") + what + ".");
    if (names && eat('>')) return true;
    for (;;) {
      if (names) {
        std::string name;
        if (!field_name(&name)) return false;
        if (!eat(':')) return !fail("Invalid struct type. Missing : after the field name.");
        (*out_)[id].field_names.push_back(name);
      }
      const uint32_t child = (uint32_t)out_->size();
      if (!type()) return false;
      (*out_)[id].subtypes.push_back(child);
      if (eat(',')) continue;
      if (eat('>')) break;
      return !fail("Invalid type string. Cannot find closing >");
    }
    if (want && (*out_)[id].subtypes.size() != want)
      return !fail(std::string(what) + " type must contain exactly " + std::to_string(want) + " sub type(s).");
    return true;
  }
  bool type() {
    if (++depth_ > 256) return !fail("Invalid type string. Nested too deep");
    const std::string w = word();
    uint32_t kind = kNumKinds;
    for (uint32_t k = 0; k < kNumKinds; ++k)
      if (w == kind_name(k)) kind = k;
    if (kind == kNumKinds) return !fail("Unknown type " + w);
    const uint32_t id = (uint32_t)out_->size();
    out_->emplace_back();
    (*out_)[id].kind = kind;
    bool ok = true;
    if (kind == kList) ok = children(id, "array", 1, false);
    else if (kind == kMap) ok = children(id, "map", 2, false);
    else if (kind == kStruct) ok = children(id, "struct", 0, true);
    else if (kind == kUnion) ok = children(id, "uniontype", 0, false);
    else if (kind == kDecimal) {
      uint32_t p = 0, s = 0;
      if (!eat('(')) return !fail("Missing ( after decimal.");
      if (!number(&p) || !eat(',') || !number(&s)) return !fail("Decimal type must specify precision and scale.");
      if (!eat(')')) return !fail("Invalid type string. Cannot find closing )");
      (*out_)[id].precision = p;
      (*out_)[id].scale = s;
    } else if (kind == kVarchar || kind == kChar) {
      uint32_t n = 0;
      if (!eat('(')) return !fail(std::string("Missing ( after ") + kind_name(kind) + ".");
      if (!number(&n)) return !fail(std::string(kind_name(kind)) + " type must specify its maximum length.");
      if (!eat(')')) return !fail("Invalid type string. Cannot find closing )");
      (*out_)[id].maximum_length = n;
    }
    --depth_;
    return ok;
  }

  const std::string& s_;
  Tree* out_;
  size_t pos_ = 0;
  int depth_ = 0;
  std::string err_;
};

inline bool parse_type(const std::string& s, Tree* out, std::string* err) { return Parser(s, out).run(err); }

inline bool is_numeric(uint32_t k) { return k <= kDouble; }
inline bool is_string_variant(uint32_t k) { return k == kString || k == kChar || k == kVarchar; }
inline bool is_timestamp(uint32_t k) { return k == kTimestamp || k == kTimestampInstant; }

// checkConversion (SchemaEvolution.cc:79-135), with the reference's valid
// conversions split into those built here and those not yet:
//   kInvalid      the reference refuses it: "Cannot convert from F to R"
//   kPass         same kind, nothing to convert
//   kConvert      numeric / decimal conversions (convert_kernels.hip)
//   kUnsupported  valid in the reference, not built: anything to or from
//                 string, char or varchar (a length change included), anything
//                 to timestamp, a precision-0 (Hive 0.11) decimal as a source:
//                 "Conversion from F to R is not supported"
enum Conv { kInvalid = 0, kPass = 1, kConvert = 2, kUnsupported = 3 };

inline Conv check_conversion(const Node& file, const Node& read) {
  const uint32_t f = file.kind, r = read.kind;
  if (f == r) {
    if (f == kChar || f == kVarchar) return read.maximum_length != file.maximum_length ? kUnsupported : kPass;
    if (f == kDecimal) {
      if (read.precision == file.precision && read.scale == file.scale) return kPass;
      return file.precision == 0 ? kUnsupported : kConvert;
    }
    return kPass;
  }
  if (is_numeric(f)) {
    if (is_numeric(r) || r == kDecimal) return kConvert;
    return is_string_variant(r) || is_timestamp(r) ? kUnsupported : kInvalid;
  }
  if (f == kDecimal) {
    if (is_numeric(r)) return file.precision == 0 ? kUnsupported : kConvert;
    return is_string_variant(r) || is_timestamp(r) ? kUnsupported : kInvalid;
  }
  if (is_string_variant(f))
    return is_string_variant(r) || is_numeric(r) || is_timestamp(r) || r == kDecimal ? kUnsupported : kInvalid;
  return kInvalid;  // timestamp, date, binary sources; a kind change on a compound type
}

// buildConversion (SchemaEvolution.cc:137-159) over whole trees: the read
// type must have the file type's shape (the same column ids and child counts;
// field names are not compared). conv[id] = the node's result; false with the
// message of the first refused node in column order.
inline bool plan_conversion(const Tree& file, const Tree& read, std::vector<Conv>* conv, std::string* err) {
  auto refuse = [&](const char* lead, const char* tail, uint32_t fid, uint32_t rid) {
    if (err) *err = std::string(lead) + to_string(file, fid) + " to " + to_string(read, rid) + tail;
    return false;
  };
  if (file.empty() || read.empty()) {
    if (err) *err = "Cannot convert from an empty type";
    return false;
  }
  if (conv) conv->assign(file.size(), kPass);
  if (read.size() != file.size()) return refuse("Cannot convert from ", "", 0, 0);
  for (uint32_t id = 0; id < file.size(); ++id) {
    const Node &f = file[id], &r = read[id];
    const Conv c = check_conversion(f, r);
    if (c == kInvalid || f.subtypes != r.subtypes) return refuse("Cannot convert from ", "", id, id);
    if (c == kUnsupported) return refuse("Conversion from ", " is not supported", id, id);
    if (c == kConvert && r.kind == kDecimal && (r.precision < 1 || r.precision > 38 || r.scale > r.precision)) {
      if (err) *err = "Invalid decimal precision or scale in the read type " + to_string(read, id);
      return false;
    }
    if (conv) (*conv)[id] = c;
  }
  return true;
}

}  // namespace rt
}  // namespace orcg
