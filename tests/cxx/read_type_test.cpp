// orc_amd/csrc/read_type.hh on its own: the type-string parser against the
// strings Reader.type_string prints, malformed input, and the conversion
// check for every pair of the 19 kinds against a table written out by hand
// from the reference's checkConversion (c++/src/SchemaEvolution.cc:79-135).
// Built with -fsanitize=address,undefined by tests/test_cxx_read_type.py.
#include <stdio.h>

#include "../../orc_amd/csrc/read_type.hh"

using namespace orcg::rt;

static int failures = 0;

#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                            \
    }                                                        \
  } while (0)

// Rows: the file kind; columns: the read kind; both in Type.Kind order
// (boolean tinyint smallint int bigint float double string binary timestamp
// array map struct uniontype decimal date varchar char timestamp-instant).
// P = valid, nothing to convert; C = valid, converted here; U = valid in the
// reference, not built here; I = the reference refuses it. Same-kind decimal,
// char and varchar entries are for equal precision / scale / length.
static const char* const kTable[kNumKinds] = {
    "PCCCCCCUIUIIIICIUUU",  // boolean
    "CPCCCCCUIUIIIICIUUU",  // tinyint
    "CCPCCCCUIUIIIICIUUU",  // smallint
    "CCCPCCCUIUIIIICIUUU",  // int
    "CCCCPCCUIUIIIICIUUU",  // bigint
    "CCCCCPCUIUIIIICIUUU",  // float
    "CCCCCCPUIUIIIICIUUU",  // double
    "UUUUUUUPIUIIIIUIUUU",  // string
    "IIIIIIIIPIIIIIIIIII",  // binary
    "IIIIIIIIIPIIIIIIIII",  // timestamp
    "IIIIIIIIIIPIIIIIIII",  // array
    "IIIIIIIIIIIPIIIIIII",  // map
    "IIIIIIIIIIIIPIIIIII",  // struct
    "IIIIIIIIIIIIIPIIIII",  // uniontype
    "CCCCCCCUIUIIIIPIUUU",  // decimal
    "IIIIIIIIIIIIIIIPIII",  // date
    "UUUUUUUUIUIIIIUIPUU",  // varchar
    "UUUUUUUUIUIIIIUIUPU",  // char
    "IIIIIIIIIIIIIIIIIIP",  // timestamp with local time zone
};

static Conv from_char(char c) { return c == 'P' ? kPass : c == 'C' ? kConvert : c == 'U' ? kUnsupported : kInvalid; }

static void round_trip(const char* s) {
  Tree t;
  std::string err;
  if (!parse_type(s, &t, &err)) {
    printf("FAILED to parse %s: %s\n", s, err.c_str());
    ++failures;
    return;
  }
  if (to_string(t) != s) {
    printf("FAILED round trip %s -> %s\n", s, to_string(t).c_str());
    ++failures;
  }
}

static void refused(const char* s) {
  Tree t;
  std::string err;
  if (parse_type(s, &t, &err) || err.empty() || !t.empty()) {
    printf("FAILED: accepted malformed '%s'\n", s);
    ++failures;
  }
}

static std::string plan_error(const char* file, const char* read, std::vector<Conv>* conv = nullptr) {
  Tree f, r;
  std::string err;
  if (!parse_type(file, &f, &err) || !parse_type(read, &r, &err)) return "parse: " + err;
  return plan_conversion(f, r, conv, &err) ? "" : err;
}

int main() {
  // the strings tests/test_reader_cpu.py expects of Reader.type_string
  round_trip(
      "struct<boolean1:boolean,byte1:tinyint,short1:smallint,int1:int,long1:bigint,float1:float,"
      "double1:double,bytes1:binary,string1:string,middle:struct<list:array<struct<int1:int,string1:string>>>,"
      "list:array<struct<int1:int,string1:string>>,map:map<string,struct<int1:int,string1:string>>>");
  round_trip("struct<_col0:int,_col1:varchar(4)>");
  round_trip("struct<s:struct<a:array<int>,m:map<string,int>>>");
  // the rest of the grammar
  round_trip("struct<d:decimal(38,10),c:char(7),u:uniontype<int,string>,t:timestamp,i:timestamp with local time zone>");
  round_trip("struct<a:date,b:decimal(10,0),c:map<varchar(10),array<uniontype<float,double>>>>");
  round_trip("struct<>");
  round_trip("int");
  round_trip("timestamp with local time zone");
  {
    // column ids are pre-order positions
    Tree t;
    std::string err;
    CHECK(parse_type("struct<a:array<int>,m:map<string,bigint>,x:double>", &t, &err));
    CHECK(t.size() == 7 && t[0].kind == kStruct && t[0].subtypes == std::vector<uint32_t>({1, 3, 6}));
    CHECK(t[1].kind == kList && t[1].subtypes == std::vector<uint32_t>({2}) && t[2].kind == kInt);
    CHECK(t[3].kind == kMap && t[3].subtypes == std::vector<uint32_t>({4, 5}) && t[6].kind == kDouble);
    CHECK(t[0].field_names == std::vector<std::string>({"a", "m", "x"}));
    CHECK(parse_type("struct<`a``b:c`:int>", &t, &err) && t[0].field_names[0] == "a`b:c");
  }

  // malformed input
  refused("");
  refused("struct<a:int");                // unbalanced <
  refused("array<int");                   //
  refused("struct<a:array<int>");         //
  refused("decimal(10)");                 // missing scale
  refused("decimal(10,");                 //
  refused("decimal");                     //
  refused("decimal(10,2");                // unbalanced (
  refused("int>");                        // trailing text
  refused("int,int");                     //
  refused("struct<a:int>x");              //
  refused("integer");                     // unknown names
  refused("struct<a:long>");              //
  refused("INT");                         //
  refused("array<int,int>");              // child counts
  refused("map<int>");                    //
  refused("map<int,int,int>");            //
  refused("uniontype<>");                 //
  refused("varchar");                     //
  refused("char()");                      //
  refused("struct<:int>");                // field names
  refused("struct<a int>");               //
  refused("struct<`a:int>");              //

  // checkConversion, every pair of kinds
  for (uint32_t f = 0; f < kNumKinds; ++f)
    for (uint32_t r = 0; r < kNumKinds; ++r) {
      Node fn, rn;
      fn.kind = f;
      rn.kind = r;
      fn.precision = rn.precision = 10;
      fn.scale = rn.scale = 2;
      fn.maximum_length = rn.maximum_length = 5;
      const Conv got = check_conversion(fn, rn);
      if (got != from_char(kTable[f][r])) {
        printf("FAILED %s -> %s: got %d, want %c\n", kind_name(f), kind_name(r), (int)got, kTable[f][r]);
        ++failures;
      }
    }
  {
    // what the same-kind entries depend on
    Node a, b;
    a.kind = b.kind = kDecimal;
    a.precision = 10, a.scale = 2, b.precision = 18, b.scale = 4;
    CHECK(check_conversion(a, b) == kConvert);
    b.precision = 10, b.scale = 3;
    CHECK(check_conversion(a, b) == kConvert);
    a.precision = 0, a.scale = 0;  // Hive 0.11 decimals as a source
    CHECK(check_conversion(a, b) == kUnsupported);
    b.kind = kLong;
    CHECK(check_conversion(a, b) == kUnsupported);
    a.kind = b.kind = kVarchar;
    a.maximum_length = 4, b.maximum_length = 8;
    CHECK(check_conversion(a, b) == kUnsupported);
    a.kind = b.kind = kChar;
    CHECK(check_conversion(a, b) == kUnsupported);
  }

  // whole trees: shape, messages, per-node results
  {
    std::vector<Conv> conv;
    CHECK(plan_error("struct<a:int,b:array<decimal(10,2)>,c:string>", "struct<x:bigint,y:array<decimal(18,4)>,z:string>",
                     &conv) == "");
    CHECK(conv == std::vector<Conv>({kPass, kConvert, kPass, kConvert, kPass}));
    CHECK(plan_error("struct<a:int>", "struct<a:int>", &conv) == "" && conv == std::vector<Conv>({kPass, kPass}));
  }
  CHECK(plan_error("struct<a:int>", "struct<a:string>") == "Conversion from int to string is not supported");
  CHECK(plan_error("struct<a:varchar(4)>", "struct<a:varchar(8)>") ==
        "Conversion from varchar(4) to varchar(8) is not supported");
  CHECK(plan_error("struct<a:double>", "struct<a:timestamp>") == "Conversion from double to timestamp is not supported");
  CHECK(plan_error("struct<a:date>", "struct<a:int>") == "Cannot convert from date to int");
  CHECK(plan_error("struct<a:binary>", "struct<a:string>") == "Cannot convert from binary to string");
  CHECK(plan_error("struct<a:timestamp>", "struct<a:bigint>") == "Cannot convert from timestamp to bigint");
  CHECK(plan_error("struct<a:array<int>>", "struct<a:map<int,int>>") ==
        "Cannot convert from struct<a:array<int>> to struct<a:map<int,int>>");
  CHECK(plan_error("struct<a:array<int>>", "struct<a:int,b:int>") ==
        "Cannot convert from struct<a:array<int>> to struct<a:int,b:int>");
  CHECK(plan_error("struct<a:int,b:int>", "struct<a:int>") == "Cannot convert from struct<a:int,b:int> to struct<a:int>");
  CHECK(plan_error("struct<a:int>", "struct<a:decimal(39,2)>").find("Invalid decimal") == 0);
  CHECK(plan_error("struct<a:int>", "struct<a:decimal(10,11)>").find("Invalid decimal") == 0);

  if (failures) return 1;
  printf("read types ok\n");
  return 0;
}
