// orc_amd/csrc/filter_plan.hh on its own (no HIP): malformed programs, every
// limit at its edge and one past, every refusal with its text, the NOT
// push-down, the binding's classes and literal tables, IN sorting and
// de-duplication. Built plain and with -fsanitize=address,undefined
// (tests/test_cxx_filter_plan.py).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../orc_amd/csrc/filter_plan.hh"

using namespace orcg;
using namespace orcg::filter;

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static Literal lng(int64_t v) {
  Literal l;
  l.lo = v;
  return l;
}
static Literal dbl(double v) {
  Literal l;
  l.d = v;
  return l;
}
static Literal str(const std::string& s) {
  Literal l;
  l.s = s;
  return l;
}
static Literal dec(__int128 u, int32_t scale) {
  Literal l;
  l.hi = (int64_t)(u >> 64);
  l.lo = (int64_t)(uint64_t)u;
  l.scale = scale;
  return l;
}
static Leaf leaf(uint32_t op, uint32_t col, uint32_t type, std::vector<Literal> lits) {
  Leaf l;
  l.op = op;
  l.column = col;
  l.type = type;
  l.lits = std::move(lits);
  return l;
}

// create()'s refusal text ("" when it builds)
static std::string refusal(const std::vector<Leaf>& leaves, const std::vector<ExprItem>& prog, Plan* out = nullptr) {
  Plan p;
  std::string err;
  const bool ok = create(leaves, prog, out ? out : &p, &err);
  CHECK(ok == err.empty());
  return err;
}

// struct<a:bigint, b:double, c:string, d:decimal(10,2), e:decimal(30,4), f:array<int>, g:struct<h:date, i:boolean>,
//        j:map<string,int>, k:uniontype<int>, l:timestamp, m:binary, n:char(4), o:float>, and as its last child
//        a Hive 0.11 decimal (precision 0), which no type string spells: added by hand
static rt::Tree schema() {
  rt::Tree t;
  std::string err;
  const bool ok = rt::Parser("struct<a:bigint,b:double,c:string,d:decimal(10,2),e:decimal(30,4),f:array<int>,"
                             "g:struct<h:date,i:boolean>,j:map<string,int>,k:uniontype<int>,l:timestamp,m:binary,"
                             "n:char(4),o:float>",
                             &t)
                      .run(&err);
  if (!ok) printf("FAILED schema: %s\n", err.c_str()), ++failures;
  rt::Node hive11;
  hive11.kind = rt::kDecimal;
  t[0].subtypes.push_back((uint32_t)t.size());
  t[0].field_names.push_back("p");
  t.push_back(hive11);
  return t;
}
enum { A = 1, B, C, D, E, F, F_ELEM, G, G_H, G_I, J, J_KEY, J_VAL, K, K_0, L, M, N, O, P };

static std::string bind_refusal(const std::vector<Leaf>& leaves, Bound* out = nullptr) {
  std::vector<ExprItem> prog;
  for (uint32_t i = 0; i < leaves.size(); ++i) prog.push_back(ExprItem{kLeaf, i});
  if (leaves.size() > 1) prog.push_back(ExprItem{kAnd, (uint32_t)leaves.size()});
  Plan p;
  std::string err;
  if (!create(leaves, prog, &p, &err)) return "create: " + err;
  Bound b;
  const bool ok = bind(p, schema(), out ? out : &b, &err);
  CHECK(ok == err.empty());
  return err;
}

static void programs() {
  const std::vector<Leaf> two = {leaf(kEquals, A, kLong, {lng(1)}), leaf(kIsNull, B, kFloat, {})};
  CHECK(refusal(two, {}) == "a filter's expression is empty");
  CHECK(refusal(two, {{kLeaf, 0}, {kAnd, 2}}) == "op 1: stack underflow");
  CHECK(refusal(two, {{kNot, 0}}) == "op 0: stack underflow");
  CHECK(refusal(two, {{kLeaf, 0}, {kLeaf, 1}}) == "the expression leaves 2 results, not 1");
  CHECK(refusal(two, {{kLeaf, 2}}) == "op 0: leaf 2 is out of range");
  CHECK(refusal(two, {{kLeaf, 0}, {kAnd, 0}}) == "op 1: AND / OR of no operands");
  CHECK(refusal(two, {{kConstant, 0}}) == "op 0: constant truth values are not supported");
  CHECK(refusal(two, {{9, 0}}) == "op 0: unknown expression op 9");
  CHECK(refusal(two, {{kLeaf, 0}, {kLeaf, 1}, {kOr, 2}}).empty());
  // leaves
  CHECK(refusal({leaf(kNullSafeEquals, A, kLong, {lng(1)})}, {{kLeaf, 0}}) ==
        "leaf 0: NULL_SAFE_EQUALS is not supported");
  CHECK(refusal({leaf(kEquals, A, kTimestamp, {lng(1)})}, {{kLeaf, 0}}) ==
        "leaf 0: TIMESTAMP predicates are not supported");
  CHECK(refusal({leaf(7, A, kLong, {lng(1)})}, {{kLeaf, 0}}) == "leaf 0: unknown operator 7");
  CHECK(refusal({leaf(kEquals, A, 7, {lng(1)})}, {{kLeaf, 0}}) == "leaf 0: unknown literal type 7");
  CHECK(refusal({leaf(kEquals, A, kLong, {})}, {{kLeaf, 0}}) == "leaf 0: EQUALS does not take 0 literals");
  CHECK(refusal({leaf(kBetween, A, kLong, {lng(1)})}, {{kLeaf, 0}}) == "leaf 0: BETWEEN does not take 1 literals");
  CHECK(refusal({leaf(kIsNull, A, kLong, {lng(1)})}, {{kLeaf, 0}}) == "leaf 0: IS_NULL does not take 1 literals");
  CHECK(refusal({leaf(kIn, A, kLong, {})}, {{kLeaf, 0}}) == "leaf 0: IN does not take 0 literals");
  CHECK(refusal({leaf(kEquals, A, kBoolean, {lng(2)})}, {{kLeaf, 0}}) == "leaf 0: a BOOLEAN literal is 0 or 1");
}

static void limits() {
  // leaves: 64 / 65
  for (uint32_t n : {kMaxLeaves, kMaxLeaves + 1}) {
    std::vector<Leaf> ls(n, leaf(kIsNull, A, kLong, {}));
    const std::string e = refusal(ls, {{kLeaf, n - 1}});
    CHECK(n == kMaxLeaves ? e.empty() : e == "a filter has at most 64 leaves, not 65");
  }
  // ops: 256 / 257
  const std::vector<Leaf> one = {leaf(kIsNull, A, kLong, {})};
  for (uint32_t n : {kMaxOps, kMaxOps + 1}) {
    std::vector<ExprItem> prog = {{kLeaf, 0}};
    while (prog.size() + 2 <= 255) prog.push_back({kLeaf, 0}), prog.push_back({kAnd, 2});
    while (prog.size() < n) prog.push_back({kNot, 0});
    Plan p;
    const std::string e = refusal(one, prog, &p);
    CHECK(n == kMaxOps ? e.empty() : e == "a filter's expression has at most 256 ops, not 257");
    if (n == kMaxOps) CHECK(p.ops.size() == 255 && p.depth == 2);  // the NOT went to the leaves
  }
  // width is free: a flat n-ary AND / OR is folded as it is emitted and needs 2 entries
  for (uint32_t n : {kMaxDepth + 1, kMaxLeaves, kMaxOps - 2}) {
    std::vector<ExprItem> prog(n, ExprItem{kLeaf, 0});
    prog.push_back({kOr, n});
    Plan p;
    CHECK(refusal(one, prog, &p).empty());
    CHECK(p.depth == 2 && p.ops.size() == 2 * n - 1 && p.ops[2] == dev_op(kOr, false, 2) &&
          p.ops.back() == dev_op(kOr, false, 2));
    prog.push_back({kNot, 0});  // NOT over it: negated leaves under a folded AND
    CHECK(refusal(one, prog, &p).empty());
    CHECK(p.depth == 2 && p.ops[0] == dev_op(kLeaf, true, 0) && p.ops.back() == dev_op(kAnd, false, 2));
  }
  // depth bounds nesting: a AND (a OR (a AND ...)), 16 / 17 levels
  for (uint32_t n : {kMaxDepth, kMaxDepth + 1}) {
    std::vector<ExprItem> prog(n, ExprItem{kLeaf, 0});
    for (uint32_t k = 0; k + 1 < n; ++k) prog.push_back({k % 2 ? kAnd : kOr, 2});
    Plan p;
    const std::string e = refusal(one, prog, &p);
    CHECK(n == kMaxDepth ? e.empty() : e == "the expression nests to a stack of 17, deeper than 16");
    if (n == kMaxDepth) CHECK(p.depth == 16);
  }
  // IN list: 1024 / 1025
  for (uint32_t n : {kMaxInList, kMaxInList + 1}) {
    std::vector<Literal> lits;
    for (uint32_t i = 0; i < n; ++i) lits.push_back(lng(i));
    const std::string e = refusal({leaf(kIn, A, kLong, lits)}, {{kLeaf, 0}});
    CHECK(n == kMaxInList ? e.empty() : e == "leaf 0: an IN list has at most 1024 literals, not 1025");
  }
  // string bytes over the whole filter: 65536 / 65537
  for (uint32_t n : {kMaxStringBytes, kMaxStringBytes + 1}) {
    const std::vector<Leaf> ls = {leaf(kEquals, C, kString, {str(std::string(40000, 'x'))}),
                                  leaf(kLessThan, C, kString, {str(std::string(n - 40000, 'y'))})};
    const std::string e = refusal(ls, {{kLeaf, 0}, {kLeaf, 1}, {kAnd, 2}});
    CHECK(n == kMaxStringBytes ? e.empty()
                               : e == "a filter has at most 65536 bytes of string literals, not 65537");
  }
}

static void push_down() {
  const std::vector<Leaf> ls = {leaf(kIsNull, A, kLong, {}), leaf(kIsNull, B, kLong, {}), leaf(kIsNull, C, kLong, {})};
  Plan p;
  // NOT (a AND (NOT b) AND (b OR c)) = (NOT a) OR b OR ((NOT b) AND (NOT c))
  CHECK(refusal(ls, {{kLeaf, 0}, {kLeaf, 1}, {kNot, 0}, {kLeaf, 1}, {kLeaf, 2}, {kOr, 2}, {kAnd, 3}, {kNot, 0}}, &p)
            .empty());
  const std::vector<uint32_t> want = {dev_op(kLeaf, true, 0), dev_op(kLeaf, false, 1), dev_op(kOr, false, 2),
                                      dev_op(kLeaf, true, 1), dev_op(kLeaf, true, 2),  dev_op(kAnd, false, 2),
                                      dev_op(kOr, false, 2)};
  CHECK(p.ops == want);
  // a double NOT cancels; an AND of one operand disappears
  CHECK(refusal(ls, {{kLeaf, 2}, {kNot, 0}, {kNot, 0}, {kAnd, 1}}, &p).empty());
  CHECK(p.ops == std::vector<uint32_t>{dev_op(kLeaf, false, 2)});
}

static void binding() {
  CHECK(bind_refusal({leaf(kEquals, 40, kLong, {lng(1)})}) == "column 40 is not in the schema");
  CHECK(bind_refusal({leaf(kIsNull, 0, kLong, {})}) == "column 0 is not a primitive column: struct");
  CHECK(bind_refusal({leaf(kIsNull, F, kLong, {})}) == "column 6 is not a primitive column: array");
  CHECK(bind_refusal({leaf(kEquals, F_ELEM, kLong, {lng(1)})}) == "column 7 is under a list, map or union");
  CHECK(bind_refusal({leaf(kEquals, J_VAL, kLong, {lng(1)})}) == "column 13 is under a list, map or union");
  CHECK(bind_refusal({leaf(kEquals, K_0, kLong, {lng(1)})}) == "column 15 is under a list, map or union");
  CHECK(bind_refusal({leaf(kEquals, A, kFloat, {dbl(1)})}) == "column 1 is bigint: it takes a LONG literal, not FLOAT");
  CHECK(bind_refusal({leaf(kEquals, B, kLong, {lng(1)})}) == "column 2 is double: it takes a FLOAT literal, not LONG");
  CHECK(bind_refusal({leaf(kEquals, O, kDecimal, {dec(1, 0)})}) ==
        "column 19 is float: it takes a FLOAT literal, not DECIMAL");
  CHECK(bind_refusal({leaf(kEquals, C, kLong, {lng(1)})}) == "column 3 is string: it takes a STRING literal, not LONG");
  CHECK(bind_refusal({leaf(kEquals, N, kDate, {lng(1)})}) == "column 18 is char: it takes a STRING literal, not DATE");
  CHECK(bind_refusal({leaf(kEquals, D, kLong, {lng(1)})}) ==
        "column 4 is decimal: it takes a DECIMAL literal, not LONG");
  CHECK(bind_refusal({leaf(kEquals, G_H, kLong, {lng(1)})}) == "column 9 is date: it takes a DATE literal, not LONG");
  CHECK(bind_refusal({leaf(kEquals, G_I, kLong, {lng(1)})}) ==
        "column 10 is boolean: it takes a BOOLEAN literal, not LONG");
  CHECK(bind_refusal({leaf(kEquals, L, kLong, {lng(1)})}) == "column 16 is timestamp: only IS_NULL applies to it");
  CHECK(bind_refusal({leaf(kEquals, M, kString, {str("x")})}) == "column 17 is binary: only IS_NULL applies to it");
  CHECK(bind_refusal({leaf(kEquals, D, kDecimal, {dec(1, 3)})}) == "decimal literal scale 3 exceeds column 4's scale 2");
  CHECK(bind_refusal({leaf(kEquals, P, kDecimal, {dec(1, 0)})}) ==
        "column 20 is a Hive 0.11 decimal without a precision");
  CHECK(bind_refusal({leaf(kIsNull, P, kDecimal, {})}).empty());
  const __int128 big = (__int128)1 << 120;
  CHECK(bind_refusal({leaf(kEquals, E, kDecimal, {dec(big, 0)})}) ==
        "decimal literal does not fit 128 bits at column 5's scale 4");
  // the first refusal in column order, whatever the leaf order
  CHECK(bind_refusal({leaf(kEquals, B, kLong, {lng(1)}), leaf(kEquals, A, kFloat, {dbl(1)})}) ==
        "column 1 is bigint: it takes a LONG literal, not FLOAT");

  // classes and tables; a struct ancestor is fine, IS_NULL takes any primitive
  Bound b;
  CHECK(bind_refusal({leaf(kLessThan, A, kLong, {lng(-3)}), leaf(kBetween, B, kFloat, {dbl(-0.0), dbl(2.5)}),
                      leaf(kEquals, D, kDecimal, {dec(15, 1)}), leaf(kEquals, E, kDecimal, {dec(-15, 1)}),
                      leaf(kEquals, G_H, kDate, {lng(19000)}), leaf(kEquals, G_I, kBoolean, {lng(1)}),
                      leaf(kIsNull, L, kLong, {}), leaf(kEquals, C, kString, {str("ab")}),
                      leaf(kEquals, N, kString, {str("cd  ")})},
                     &b)
            .empty());
  CHECK(b.leaves[0].cls == kClsI64 && b.words[b.leaves[0].lit0] == -3);
  double lo;
  memcpy(&lo, &b.words[b.leaves[1].lit0], 8);
  CHECK(b.leaves[1].cls == kClsF64 && lo == 0 && signbit(lo));
  CHECK(b.leaves[2].cls == kClsI64 && b.words[b.leaves[2].lit0] == 150);  // 1.5 at scale 2
  CHECK(b.leaves[3].cls == kClsDec128 && b.words[b.leaves[3].lit0] == -1 && b.words[b.leaves[3].lit0 + 1] == -15000);
  CHECK(b.leaves[4].cls == kClsI64 && b.leaves[5].cls == kClsI64 && b.leaves[6].cls == kClsNull);
  CHECK(b.leaves[7].cls == kClsString && b.leaves[8].cls == kClsString);
  CHECK(b.str_bytes == "abcd  " && b.str_off == (std::vector<uint32_t>{0, 2, 6}));
  CHECK(b.leaves[7].lit0 == 0 && b.leaves[8].lit0 == 1);
  CHECK(b.order == (std::vector<uint32_t>{0, 1, 7, 2, 3, 4, 5, 6, 8}));
  // a decimal64 literal past int64 saturates (the column holds 18 digits)
  const __int128 wide = (__int128)INT64_MAX * 4;
  CHECK(bind_refusal({leaf(kLessThan, D, kDecimal, {dec(wide, 2)}), leaf(kLessThan, D, kDecimal, {dec(-wide, 2)})}, &b)
            .empty());
  CHECK(b.words[0] == INT64_MAX && b.words[1] == INT64_MIN);
}

static void in_lists() {
  Bound b;
  CHECK(bind_refusal({leaf(kIn, A, kLong, {lng(5), lng(-1), lng(5), lng(INT64_MIN), lng(3), lng(-1)})}, &b).empty());
  CHECK(b.leaves[0].nlit == 4 && b.words == (std::vector<int64_t>{INT64_MIN, -1, 3, 5}));
  // Double.compare's order: -inf < -0.0 < 0.0 < inf < NaN, every NaN one value
  CHECK(bind_refusal({leaf(kIn, B, kFloat, {dbl(NAN), dbl(0.0), dbl(INFINITY), dbl(-0.0), dbl(-NAN), dbl(-INFINITY),
                                            dbl(0.0)})},
                     &b)
            .empty());
  CHECK(b.leaves[0].nlit == 5);
  CHECK(b.words == (std::vector<int64_t>{double_key(-INFINITY), double_key(-0.0), double_key(0.0),
                                         double_key(INFINITY), double_key(NAN)}));
  CHECK(double_key(-0.0) == -1 && double_key(0.0) == 0 && double_key(-NAN) == double_key(NAN));
  CHECK(double_key(-1.0) < double_key(-0.5) && double_key(1e300) < double_key(INFINITY));
  // unsigned bytes, a proper prefix first
  CHECK(bind_refusal({leaf(kIn, C, kString, {str("b"), str("\x80"), str("ab"), str(""), str("a"), str("ab"),
                                             str("\x7f")})},
                     &b)
            .empty());
  CHECK(b.leaves[0].nlit == 6 && b.str_bytes == std::string("aabb\x7f\x80"));
  CHECK(b.str_off == (std::vector<uint32_t>{0, 0, 1, 3, 4, 5, 6}));
  // decimals sort and de-duplicate at the column's scale: 1.5 = 1.50
  CHECK(bind_refusal({leaf(kIn, D, kDecimal, {dec(150, 2), dec(15, 1), dec(-2, 0), dec(1, 2)})}, &b).empty());
  CHECK(b.leaves[0].nlit == 3 && b.words == (std::vector<int64_t>{-200, 1, 150}));
  CHECK(bind_refusal({leaf(kIn, E, kDecimal, {dec(15, 1), dec(-2, 0), dec(150, 2)})}, &b).empty());
  CHECK(b.leaves[0].nlit == 2 && b.words == (std::vector<int64_t>{-1, -20000, 0, 15000}));
}

int main() {
  programs();
  limits();
  push_down();
  binding();
  in_lists();
  if (failures) return 1;
  printf("filter plans ok\n");
  return 0;
}
