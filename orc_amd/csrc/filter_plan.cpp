// filter_plan.hh: verification, NOT push-down and binding of a row-level
// filter. No HIP.
#include "filter_plan.hh"

#include <string.h>

#include <algorithm>

namespace orcg {
namespace filter {

namespace {

const char* const kOpNames[kNumLeafOps] = {"EQUALS", "NULL_SAFE_EQUALS", "LESS_THAN", "LESS_THAN_EQUALS",
                                           "IN",     "BETWEEN",          "IS_NULL"};
const char* const kLitNames[kNumLitTypes] = {"LONG", "FLOAT", "STRING", "DATE", "DECIMAL", "TIMESTAMP", "BOOLEAN"};

bool refuse(std::string* err, const std::string& m) {
  if (err) *err = m;
  return false;
}

typedef __int128 i128;
i128 dec_value(const Literal& l) { return (i128)(((unsigned __int128)(uint64_t)l.hi << 64) | (uint64_t)l.lo); }

// the tree of the postfix program, for the push-down
struct Node {
  uint32_t op, arg;
  std::vector<uint32_t> kids;
};

// AND and OR are associative: an n-ary node is emitted folded, operand, operand,
// op 2, operand, op 2 ..., so a flat AND / OR of any width needs two stack
// entries on the device and the depth limit bounds nesting alone.
void emit(const std::vector<Node>& nodes, uint32_t at, bool neg, std::vector<uint32_t>& out) {
  const Node& n = nodes[at];
  if (n.op == kLeaf) {
    out.push_back(dev_op(kLeaf, neg, n.arg));
  } else if (n.op == kNot) {
    emit(nodes, n.kids[0], !neg, out);
  } else {
    // De Morgan: NOT (a AND b) = (NOT a) OR (NOT b)
    const uint32_t kind = (n.op == kAnd) != neg ? kAnd : kOr;
    for (size_t k = 0; k < n.kids.size(); ++k) {
      emit(nodes, n.kids[k], neg, out);
      if (k) out.push_back(dev_op(kind, false, 2));
    }
  }
}

// stack entries the emitted program needs
uint32_t emitted_depth(const std::vector<uint32_t>& ops) {
  uint32_t depth = 0, top = 0;
  for (uint32_t op : ops) {
    depth = (op & 3) == kLeaf ? depth + 1 : depth - ((op >> 8) - 1);
    top = std::max(top, depth);
  }
  return top;
}

template <typename Less>
void sort_unique(std::vector<Literal>& v, Less less) {
  std::sort(v.begin(), v.end(), less);
  v.erase(std::unique(v.begin(), v.end(), [&](const Literal& a, const Literal& b) { return !less(a, b) && !less(b, a); }),
          v.end());
}

}  // namespace

bool create(const std::vector<Leaf>& leaves, const std::vector<ExprItem>& program, Plan* out, std::string* err) {
  if (leaves.size() > kMaxLeaves)
    return refuse(err, "a filter has at most " + std::to_string(kMaxLeaves) + " leaves, not " +
                           std::to_string(leaves.size()));
  if (program.empty()) return refuse(err, "a filter's expression is empty");
  if (program.size() > kMaxOps)
    return refuse(err, "a filter's expression has at most " + std::to_string(kMaxOps) + " ops, not " +
                           std::to_string(program.size()));
  uint64_t str_bytes = 0;
  for (size_t i = 0; i < leaves.size(); ++i) {
    const Leaf& l = leaves[i];
    const std::string at = "leaf " + std::to_string(i) + ": ";
    if (l.op >= kNumLeafOps) return refuse(err, at + "unknown operator " + std::to_string(l.op));
    // Java's row-level filter refuses it too (LeafFilterFactory.java:276, UnSupportedSArgException)
    if (l.op == kNullSafeEquals) return refuse(err, at + "NULL_SAFE_EQUALS is not supported");
    if (l.type >= kNumLitTypes) return refuse(err, at + "unknown literal type " + std::to_string(l.type));
    if (l.type == kTimestamp) return refuse(err, at + "TIMESTAMP predicates are not supported");
    const size_t nl = l.lits.size();
    bool ok;
    switch (l.op) {
      case kIsNull: ok = nl == 0; break;
      case kBetween: ok = nl == 2; break;
      case kIn: ok = nl >= 1; break;
      default: ok = nl == 1; break;
    }
    if (!ok) return refuse(err, at + kOpNames[l.op] + " does not take " + std::to_string(nl) + " literals");
    if (nl > kMaxInList)
      return refuse(err, at + "an IN list has at most " + std::to_string(kMaxInList) + " literals, not " +
                             std::to_string(nl));
    for (const Literal& v : l.lits) {
      if (l.type == kString) str_bytes += v.s.size();
      if (l.type == kBoolean && v.lo != 0 && v.lo != 1) return refuse(err, at + "a BOOLEAN literal is 0 or 1");
      if (l.type == kDecimal && (v.scale < 0 || v.scale > 38)) return refuse(err, at + "bad DECIMAL literal scale");
    }
  }
  if (str_bytes > kMaxStringBytes)
    return refuse(err, "a filter has at most " + std::to_string(kMaxStringBytes) + " bytes of string literals, not " +
                           std::to_string(str_bytes));
  // the postfix program: no underflow, every leaf in range, one result
  std::vector<Node> nodes;
  std::vector<uint32_t> stack;
  for (size_t p = 0; p < program.size(); ++p) {
    const ExprItem& e = program[p];
    const std::string at = "op " + std::to_string(p) + ": ";
    Node n{e.op, e.arg, {}};
    uint32_t take = 0;
    switch (e.op) {
      case kLeaf:
        if (e.arg >= leaves.size()) return refuse(err, at + "leaf " + std::to_string(e.arg) + " is out of range");
        break;
      case kAnd:
      case kOr:
        if (e.arg == 0) return refuse(err, at + "AND / OR of no operands");
        take = e.arg;
        break;
      case kNot: take = 1; break;
      // Java: "Do not support CONSTANT" (FilterFactory.java, UnSupportedSArgException)
      case kConstant: return refuse(err, at + "constant truth values are not supported");
      default: return refuse(err, at + "unknown expression op " + std::to_string(e.op));
    }
    if (take > stack.size()) return refuse(err, at + "stack underflow");
    n.kids.assign(stack.end() - take, stack.end());
    stack.resize(stack.size() - take);
    stack.push_back((uint32_t)nodes.size());
    nodes.push_back(std::move(n));
  }
  if (stack.size() != 1)
    return refuse(err, "the expression leaves " + std::to_string(stack.size()) + " results, not 1");
  out->leaves = leaves;
  out->ops.clear();
  emit(nodes, stack[0], false, out->ops);
  out->depth = emitted_depth(out->ops);
  if (out->depth > kMaxDepth)
    return refuse(err, "the expression nests to a stack of " + std::to_string(out->depth) + ", deeper than " +
                           std::to_string(kMaxDepth));
  for (Leaf& l : out->leaves) {
    if (l.op != kIn) continue;
    switch (l.type) {
      case kFloat:
        sort_unique(l.lits, [](const Literal& a, const Literal& b) { return double_key(a.d) < double_key(b.d); });
        break;
      case kString:
        // unsigned bytewise, a proper prefix first (StringExpr.compare)
        sort_unique(l.lits, [](const Literal& a, const Literal& b) {
          const size_t m = std::min(a.s.size(), b.s.size());
          const int c = m ? memcmp(a.s.data(), b.s.data(), m) : 0;
          return c ? c < 0 : a.s.size() < b.s.size();
        });
        break;
      case kDecimal: break;  // at the column's scale (bind)
      default: sort_unique(l.lits, [](const Literal& a, const Literal& b) { return a.lo < b.lo; }); break;
    }
  }
  return true;
}

bool under_repeated(const rt::Tree& tree, uint32_t id, bool include_self) {
  std::vector<int64_t> parent(tree.size(), -1);
  for (size_t i = 0; i < tree.size(); ++i)
    for (uint32_t k : tree[i].subtypes)
      if (k < tree.size()) parent[k] = (int64_t)i;
  int64_t at = include_self ? (int64_t)id : parent[id];
  for (size_t hops = 0; at >= 0 && hops <= tree.size(); ++hops, at = parent[at]) {
    const uint32_t k = tree[at].kind;
    if (k == rt::kList || k == rt::kMap || k == rt::kUnion) return true;
  }
  return false;
}

bool bind(const Plan& p, const rt::Tree& tree, Bound* out, std::string* err) {
  out->leaves.assign(p.leaves.size(), BoundLeaf{});
  out->words.clear();
  out->str_off.assign(1, 0);
  out->str_bytes.clear();
  out->order.resize(p.leaves.size());
  for (uint32_t i = 0; i < p.leaves.size(); ++i) out->order[i] = i;
  std::stable_sort(out->order.begin(), out->order.end(),
                   [&](uint32_t a, uint32_t b) { return p.leaves[a].column < p.leaves[b].column; });
  for (uint32_t li : out->order) {
    const Leaf& l = p.leaves[li];
    BoundLeaf& b = out->leaves[li];
    const std::string col = "column " + std::to_string(l.column);
    if (l.column >= tree.size()) return refuse(err, col + " is not in the schema");
    const rt::Node& t = tree[l.column];
    if (t.kind == rt::kList || t.kind == rt::kMap || t.kind == rt::kStruct || t.kind == rt::kUnion)
      return refuse(err, col + " is not a primitive column: " + rt::kind_name(t.kind));
    if (under_repeated(tree, l.column, false)) return refuse(err, col + " is under a list, map or union");
    b.op = l.op;
    b.column = l.column;
    b.lit0 = (uint32_t)out->words.size();
    b.nlit = (uint32_t)l.lits.size();
    if (l.op == kIsNull) {  // the mask alone: any primitive
      b.cls = kClsNull;
      continue;
    }
    uint32_t want;
    switch (t.kind) {
      case rt::kByte: case rt::kShort: case rt::kInt: case rt::kLong: want = kLong; break;
      case rt::kBoolean: want = kBoolean; break;
      case rt::kFloat: case rt::kDouble: want = kFloat; break;
      case rt::kDate: want = kDate; break;
      case rt::kString: case rt::kVarchar: case rt::kChar: want = kString; break;
      case rt::kDecimal: want = kDecimal; break;
      default:
        return refuse(err, col + " is " + rt::kind_name(t.kind) + ": only IS_NULL applies to it");
    }
    if (l.type != want)
      return refuse(err, col + " is " + rt::kind_name(t.kind) + ": it takes a " + kLitNames[want] + " literal, not " +
                             kLitNames[l.type]);
    switch (want) {
      case kFloat:
        b.cls = kClsF64;
        for (const Literal& v : l.lits) {
          int64_t w;
          if (l.op == kIn) w = double_key(v.d);
          else memcpy(&w, &v.d, 8);
          out->words.push_back(w);
        }
        break;
      case kString:
        b.cls = kClsString;
        b.lit0 = (uint32_t)out->str_off.size() - 1;
        for (const Literal& v : l.lits) {
          out->str_bytes += v.s;
          out->str_off.push_back((uint32_t)out->str_bytes.size());
        }
        break;
      case kDecimal: {
        if (t.precision == 0) return refuse(err, col + " is a Hive 0.11 decimal without a precision");
        const bool wide = t.precision > 18;
        b.cls = wide ? kClsDec128 : kClsI64;
        std::vector<i128> vals;
        for (const Literal& v : l.lits) {
          // Java asserts the same (LeafFilterFactory.java:59)
          if ((uint32_t)v.scale > t.scale)
            return refuse(err, "decimal literal scale " + std::to_string(v.scale) + " exceeds " + col + "'s scale " +
                                   std::to_string(t.scale));
          i128 x = dec_value(v);
          for (uint32_t k = (uint32_t)v.scale; k < t.scale; ++k)
            if (__builtin_mul_overflow(x, (i128)10, &x))
              return refuse(err, "decimal literal does not fit 128 bits at " + col + "'s scale " +
                                     std::to_string(t.scale));
          vals.push_back(x);
        }
        if (l.op == kIn) {
          std::sort(vals.begin(), vals.end());
          vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
        }
        if (!wide) {
          // a column of <= 18 digits holds |v| < 10^18 < 2^63 - 1: a literal past
          // int64 compares the same once saturated
          std::vector<int64_t> sat;
          for (i128 x : vals) sat.push_back(x > (i128)INT64_MAX ? INT64_MAX : x < (i128)INT64_MIN ? INT64_MIN : (int64_t)x);
          if (l.op == kIn) sat.erase(std::unique(sat.begin(), sat.end()), sat.end());
          out->words.insert(out->words.end(), sat.begin(), sat.end());
          b.nlit = (uint32_t)sat.size();
        } else {
          for (i128 x : vals) {
            out->words.push_back((int64_t)(x >> 64));
            out->words.push_back((int64_t)(uint64_t)x);
          }
          b.nlit = (uint32_t)vals.size();
        }
        break;
      }
      default:
        b.cls = kClsI64;
        for (const Literal& v : l.lits) out->words.push_back(v.lo);
        break;
    }
  }
  return true;
}

}  // namespace filter
}  // namespace orcg
