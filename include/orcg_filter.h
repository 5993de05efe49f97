/*
 * orcg_filter.h — search arguments as a row-level filter over decoded columns
 * in HBM.
 *
 * Stands for the half of the reference's predicate support that selects rows:
 *   SearchArgument / SearchArgumentBuilder   c++/include/orc/sargs/SearchArgument.hh
 *   Literal, PredicateDataType               c++/include/orc/sargs/Literal.hh
 *   TruthValue                               c++/include/orc/sargs/TruthValue.hh
 *   Reader.Options.allowSARGToFilter         java/core/src/java/org/apache/orc/Reader.java
 *   FilterFactory.createSArgFilter           java/core/src/java/org/apache/orc/impl/filter/FilterFactory.java:106-163
 *   LeafFilter.filter                        .../impl/filter/LeafFilter.java:41-84
 *   LeafFilterFactory                        .../impl/filter/leaf/LeafFilterFactory.java:226-279
 * Row-group pruning on index statistics (SargsApplier) is not built.
 *
 * Truth rules. Per row a leaf is YES, NO or NULL: a null row is NULL for every
 * operator but IS_NULL (YES on a null row, NO otherwise); NOT swaps YES and
 * NO and keeps NULL; AND / OR are Kleene's; a row is selected iff the whole
 * expression is YES. That is what Java's filter selects: a leaf, negated or
 * not, never selects a null row (LeafFilter.java:67-77), AND intersects and
 * OR unites selections. Integers, boolean and date compare as int64;
 * float / double by IEEE rules (NaN is NO, -0.0 = 0.0) except IN, which
 * follows Double.compare (a NaN literal matches NaN, -0.0 and 0.0 differ;
 * FloatFilters.java:72-77); strings by unsigned bytes, a proper prefix first
 * (a char column keeps its padding); decimals as signed 128-bit unscaled
 * values at the column's scale; BETWEEN is low <= v && v <= high.
 */
#ifndef ORCG_FILTER_H
#define ORCG_FILTER_H

#include "orcg_reader.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PredicateLeaf::Operator (SearchArgument.hh) */
enum { ORCG_SARG_EQUALS = 0, ORCG_SARG_NULL_SAFE_EQUALS = 1, ORCG_SARG_LESS_THAN = 2,
       ORCG_SARG_LESS_THAN_EQUALS = 3, ORCG_SARG_IN = 4, ORCG_SARG_BETWEEN = 5, ORCG_SARG_IS_NULL = 6 };
/* PredicateDataType (Literal.hh) */
enum { ORCG_LIT_LONG = 0, ORCG_LIT_FLOAT = 1, ORCG_LIT_STRING = 2, ORCG_LIT_DATE = 3, ORCG_LIT_DECIMAL = 4,
       ORCG_LIT_TIMESTAMP = 5, ORCG_LIT_BOOLEAN = 6 };
/* ExpressionTree::Operator, as postfix ops: LEAF (arg = leaf index), AND / OR
 * (arg = operand count), NOT, CONSTANT (a TruthValue; refused) */
enum { ORCG_EXPR_LEAF = 0, ORCG_EXPR_AND = 1, ORCG_EXPR_OR = 2, ORCG_EXPR_NOT = 3, ORCG_EXPR_CONSTANT = 4 };

/* Limits; beyond them orcg_filter_create fails with a text. */
#define ORCG_FILTER_MAX_LEAVES 64
#define ORCG_FILTER_MAX_OPS 256
#define ORCG_FILTER_MAX_DEPTH 16          /* nesting: an AND / OR of any width counts 2 */
#define ORCG_FILTER_MAX_IN_LIST 1024
#define ORCG_FILTER_MAX_STRING_BYTES 65536 /* all string literals together */

/* Literal (Literal.hh): LONG / DATE (days since 1970) / BOOLEAN (0, 1) in
 * `lo`; FLOAT in `d`; STRING in bytes[len]; DECIMAL unscaled [hi, lo]
 * (orc::Int128) at `scale`. */
typedef struct {
  int64_t lo, hi;
  double d;
  const uint8_t* bytes;
  uint64_t len;
  int32_t scale;
} orcg_literal;

/* PredicateLeaf: operator, column (type id), literal type, literals (none for
 * IS_NULL, two for BETWEEN, the list for IN, else one). */
typedef struct {
  uint32_t op, column, literal_type, nliterals;
  const orcg_literal* literals;
} orcg_filter_leaf;

typedef struct {
  uint32_t op, arg;
} orcg_filter_op;

typedef struct orcg_filter orcg_filter;

/* SearchArgumentBuilder::build: verifies the postfix program (no stack
 * underflow, one result, leaf indices in range, the limits above), pushes NOT
 * down to the leaves (SearchArgumentBuilderImpl.pushDownNot), sorts and
 * de-duplicates IN lists. Refused with ORCG_INVALID_ARGUMENT and a text
 * (orcg_filter_last_error(NULL)): NULL_SAFE_EQUALS and CONSTANT, as Java's
 * row-level filter refuses them (UnSupportedSArgException), and TIMESTAMP
 * leaves ("TIMESTAMP predicates are not supported"). */
int orcg_filter_create(const orcg_filter_leaf* leaves, uint32_t nleaves, const orcg_filter_op* program,
                       uint32_t nprog, orcg_filter** out);
void orcg_filter_destroy(orcg_filter* f);
/* The filter's last failure; f = NULL: this thread's last failed create.
 * A filter may be shared by readers on several threads: its runs take turns
 * (a run binds the filter to its reader's types); its last error is then the
 * last run's, whichever thread made it. */
const char* orcg_filter_last_error(const orcg_filter* f);

/* LeafFilter.filter over device buffers (the kernels' own entry): column
 * views[i] (device pointers; type_id, num_elements = n, has_nulls / not_null,
 * data, length, blob, index, dict_offsets as orcg_reader_column gives them) is
 * read as types[i]. The filter is bound to these types (the checks of
 * orcg_reader_filter_stripe). *d_selected: count ascending int64 row indices
 * (VectorizedRowBatch.selected / size) in the context's scratch, valid until
 * its next call. Synchronous on the context's stream. */
int orcg_filter_columns_device(orcg_ctx* ctx, orcg_filter* f, const orcg_column_view* views,
                               const orcg_type_info* types, uint32_t ncols, uint64_t n, const int64_t** d_selected,
                               uint64_t* count);
/* Rows d_sel[0 .. count) of a column's arrays (the gather of
 * orcg_reader_filtered_column): src8[k] / dst8[k] 8-byte arrays (NULL: none),
 * src16 / dst16 a 16-byte array, not_null / out_not_null the mask; *nulls =
 * gathered rows whose mask byte is 0. n_src = rows of the source. */
int orcg_filter_gather_device(orcg_ctx* ctx, const int64_t* d_sel, uint64_t count, uint64_t n_src,
                              const void* const src8[3], void* const dst8[3], const void* src16, void* dst16,
                              const uint8_t* not_null, uint8_t* out_not_null, uint64_t* nulls);

/* The filter over stripe k of the reader's last read_stripe / read_stripes
 * (Reader.Options.allowSARGToFilter; runs after the decode, not inside it).
 * Binds on first use against this reader's types (the read type's where one is
 * set: a leaf on a converted column compares the converted values) and fails
 * with the binding's text, in column order: "column <id> is not in the
 * schema", "... is not a primitive column: <kind>", "... is under a list, map
 * or union", "... is <kind>: it takes a <T> literal, not <U>", "decimal
 * literal scale <s> exceeds column <id>'s scale <c>", "decimal literal does
 * not fit 128 bits at ...". Every leaf column must be selected and decoded:
 * "column <id> was not decoded". *d_selected and what
 * orcg_reader_filtered_column returns come from the stripe's device arena and
 * live until the reader's next read. */
int orcg_reader_filter_stripe(orcg_reader* r, uint64_t k, orcg_filter* f, const int64_t** d_selected,
                              uint64_t* count);
/* Column type_id of stripe k gathered by its last orcg_reader_filter_stripe:
 * num_elements = count, has_nulls counted among the selected rows; values,
 * masks, string (start, length) pairs and dictionary indices are gathered,
 * blobs and dictionaries shared. Primitive columns and structs of them; a
 * list, map or union column, or anything under one: ORCG_INVALID_ARGUMENT
 * "column <id> is not filtered: nested". */
int orcg_reader_filtered_column(orcg_reader* r, uint64_t k, uint32_t type_id, orcg_column_view* out);

/* ---- Measurement only (no reference counterpart; scripts/bench_filter.py),
 * not for a product path: with timing on, every kernel of a run is bracketed
 * by HIP events and the host waits for each, so a run is slower. Off by
 * default. Milliseconds of the last run's launches: [0] string leaves,
 * [1] combine, [2] scan, [3] select. */
int orcg_filter_set_timing(orcg_filter* f, int on);
int orcg_filter_last_timing(const orcg_filter* f, double out_ms[4]);

#ifdef __cplusplus
}
#endif
#endif /* ORCG_FILTER_H */
