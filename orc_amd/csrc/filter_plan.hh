// Search arguments as a row-level filter, on the host: the leaves and the
// postfix expression of a SearchArgument (c++/include/orc/sargs/
// SearchArgument.hh, Literal.hh; Java's SearchArgumentImpl), verified, with NOT
// pushed down to the leaves (SearchArgumentBuilderImpl.pushDownNot), and its
// binding to a type tree (Java's LeafFilterFactory.createLeafVectorFilter,
// java/core/src/java/org/apache/orc/impl/filter/leaf/LeafFilterFactory.java:
// 226-279: which leaves the row-level filter builds, and on which column
// kinds). Host-only C++ with no HIP dependency (tests/cxx/filter_plan_test.cpp);
// the device tables at the end are plain structs the kernels of
// filter_kernels.hip read.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "read_type.hh"

namespace orcg {
namespace filter {

// Limits (checked by create(); beyond them: an error with a text)
constexpr uint32_t kMaxLeaves = 64;         // leaves of one filter
constexpr uint32_t kMaxOps = 256;           // ops of the postfix program given to create()
constexpr uint32_t kMaxDepth = 16;          // stack depth of the emitted program (2 bits an entry in one register):
                                            // nesting, not width: an n-ary AND / OR is folded and needs 2
constexpr uint32_t kMaxInList = 1024;       // literals of one IN list
constexpr uint32_t kMaxStringBytes = 65536; // string literal bytes of the whole filter

// PredicateLeaf::Operator (sargs/SearchArgument.hh order)
enum LeafOp : uint32_t {
  kEquals = 0, kNullSafeEquals = 1, kLessThan = 2, kLessThanEquals = 3, kIn = 4, kBetween = 5, kIsNull = 6,
  kNumLeafOps = 7
};
// PredicateDataType (sargs/Literal.hh order)
enum LitType : uint32_t {
  kLong = 0, kFloat = 1, kString = 2, kDate = 3, kDecimal = 4, kTimestamp = 5, kBoolean = 6, kNumLitTypes = 7
};
// Ops of the postfix program: a leaf (arg = its index), n-ary AND / OR (arg =
// operand count), NOT, a constant truth value (ExpressionTree::CONSTANT; refused)
enum ExprOp : uint32_t { kLeaf = 0, kAnd = 1, kOr = 2, kNot = 3, kConstant = 4 };

struct Literal {
  int64_t lo = 0;   // LONG, DATE (days), BOOLEAN (0 / 1); DECIMAL: low word of the unscaled value
  int64_t hi = 0;   // DECIMAL: high word (orc::Int128 [hi, lo])
  double d = 0;     // FLOAT
  std::string s;    // STRING bytes
  int32_t scale = 0;  // DECIMAL
};

struct Leaf {
  uint32_t op = 0, column = 0, type = 0;
  std::vector<Literal> lits;
};

struct ExprItem {
  uint32_t op, arg;
};

// The device program's op: bits 0-1 kLeaf / kAnd / kOr, bit 2 the leaf is
// negated, bits 8.. the leaf index or the operand count
constexpr uint32_t kOpNeg = 4;
inline uint32_t dev_op(uint32_t kind, bool neg, uint32_t arg) { return kind | (neg ? kOpNeg : 0) | (arg << 8); }

// A verified filter: its leaves (IN lists sorted and de-duplicated, but for
// decimals, which sort at their column's scale) and the pushed-down program
struct Plan {
  std::vector<Leaf> leaves;
  std::vector<uint32_t> ops;  // dev_op words: binary AND / OR over possibly negated leaves (n-ary ones folded)
  uint32_t depth = 0;         // stack depth the program reaches
};

// Verifies and builds; false with *err on a refusal.
bool create(const std::vector<Leaf>& leaves, const std::vector<ExprItem>& program, Plan* out, std::string* err);

// Double.compare's total order as an int64 key (IN lists of FLOAT leaves,
// FloatFilters.java:72-77: Arrays.binarySearch): -0.0 < 0.0, every NaN equal
// and above +inf
inline int64_t double_key(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, 8);
  if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
  return (int64_t)(b ^ (((uint64_t)((int64_t)b >> 63)) >> 1));
}

// What the combine kernel does for a leaf
enum LeafClass : uint32_t {
  kClsI64 = 0,     // int64 compare: integers, boolean, date, decimal of precision <= 18
  kClsF64 = 1,     // IEEE compare; IN on double_key
  kClsDec128 = 2,  // signed 128-bit compare of [hi, lo]
  kClsString = 3,  // materialised by the string kernel (per row, or per dictionary entry)
  kClsNull = 4,    // IS_NULL: the mask alone
};

struct BoundLeaf {
  uint32_t cls, op, column;
  uint32_t lit0, nlit;  // kClsString: first literal in str_off; else first word in `words`
};

// A plan bound to a type tree: literal tables in device form
struct Bound {
  std::vector<BoundLeaf> leaves;
  std::vector<int64_t> words;     // int64 / double bits / IN keys / [hi, lo] pairs
  std::vector<uint32_t> str_off;  // string literal k = str_bytes[str_off[k], str_off[k + 1])
  std::string str_bytes;
  std::vector<uint32_t> order;    // leaf indices in column order (errors are reported in it)
};

// Binds every leaf to `tree` (the read type's tree when one is set); false
// with *err: the first refusal in column order.
bool bind(const Plan& p, const rt::Tree& tree, Bound* out, std::string* err);

// id or an ancestor of it is a list, map or union (tree in pre-order)
bool under_repeated(const rt::Tree& tree, uint32_t id, bool include_self);

// ---- device tables (filter_kernels.hip)
constexpr uint32_t kTruthNo = 0, kTruthNull = 1, kTruthYes = 2;  // AND = min, OR = max, NOT = 2 - t
enum DevLeafClass : uint32_t { kDevI64 = 0, kDevF64 = 1, kDevDec128 = 2, kDevTruth = 3, kDevTruthDict = 4, kDevNull = 5 };
struct DevLeaf {
  const void* data;      // the column's values; kDevTruth / kDevTruthDict: truth bytes (per row / per entry)
  const uint8_t* nn;     // the column's mask, or null
  const int64_t* index;  // kDevTruthDict: the row's dictionary entry
  uint64_t dict_size;
  uint32_t cls, op, lit0, nlit;
};

}  // namespace filter
}  // namespace orcg
