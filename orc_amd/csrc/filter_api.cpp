// C ABI of the row-level filter (include/orcg_filter.h): the filter object
// (filter_plan.hh), one run of its kernels (filter_kernels.hip) over column
// views in device memory, and the reader's entries over a decoded stripe.
#include "../../include/orcg_filter.h"

#include <functional>

#include "filter_internal.hh"
#include "reader_internal.hh"

using namespace orcg::filter;

struct orcg_filter {
  // a run rebinds `bound` and rebuilds `table`: one run of a filter at a time
  // (two readers on two threads may share one filter)
  std::mutex mu;
  Plan plan;
  Bound bound;
  std::string err;
  std::vector<uint8_t> table;  // the device tables' host copy (the upload's source)
  bool timing = false;
  double ms[4] = {0, 0, 0, 0};
};

namespace {

thread_local std::string g_create_error;

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Timer {
  Ctx* c;
  bool on;
  hipEvent_t a = nullptr, b = nullptr;
  Timer(Ctx* ctx, bool enabled) : c(ctx), on(enabled) {
    if (on && (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)) on = false;
  }
  ~Timer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  // times f's launches (a synchronisation each: measurement only)
  template <class Fn>
  int run(double* ms, Fn&& f) {
    if (!on) return f();
    (void)hipEventRecord(a, c->stream);
    const int rc = f();
    (void)hipEventRecord(b, c->stream);
    (void)hipEventSynchronize(b);
    float t = 0;
    if (hipEventElapsedTime(&t, a, b) == hipSuccess) *ms += t;
    return rc;
  }
};

// One run: views[l] is leaf l's column (device pointers), n its rows.
// alloc(bytes): 256-byte aligned device memory that outlives the run's result.
int run_filter(Ctx* c, orcg_filter* f, const std::vector<orcg_column_view>& views, uint64_t n,
               const std::function<void*(size_t)>& alloc, const int64_t** d_selected, uint64_t* count,
               std::string* err) {
  const Bound& b = f->bound;
  const size_t nl = b.leaves.size(), nops = f->plan.ops.size();
  const uint64_t tiles = (n + kTile - 1) / kTile;
  for (double& m : f->ms) m = 0;
  // the device tables: leaves, ops, literal words, string literal offsets and bytes
  const size_t o_leaves = 0, o_ops = up256(nl * sizeof(DevLeaf)), o_words = o_ops + up256(nops * 4),
               o_soff = o_words + up256(b.words.size() * 8), o_sbytes = o_soff + up256(b.str_off.size() * 4),
               table_bytes = o_sbytes + up256(b.str_bytes.size());
  // then the run's buffers
  size_t at = table_bytes;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += up256(std::max<size_t>(bytes, 1));
    return o;
  };
  std::vector<size_t> o_truth(nl, 0);
  for (size_t l = 0; l < nl; ++l) {
    if (b.leaves[l].cls != kClsString) continue;
    const orcg_column_view& v = views[l];
    const bool dict = v.index && v.dict_offsets;
    if (!dict && !(v.data && v.length) && n) {
      *err = "column " + std::to_string(b.leaves[l].column) + " has no string layout";
      return ORCG_INVALID_ARGUMENT;
    }
    o_truth[l] = take(dict ? v.dict_size : n);
  }
  const size_t o_sel = take(tiles * kTile), o_counts = take(tiles * 8), o_base = take((tiles + 1) * 8),
               o_total = take(8), o_selected = take(n * 8);
  (void)hipSetDevice(c->device);
  uint8_t* d = (uint8_t*)alloc(at);
  if (!d) {
    *err = "device allocation failed";
    return ORCG_OUT_OF_MEMORY;
  }
  *d_selected = (const int64_t*)(d + o_selected);
  *count = 0;
  if (n == 0) return ORCG_OK;
  f->table.assign(table_bytes, 0);
  DevLeaf* hl = (DevLeaf*)(f->table.data() + o_leaves);
  for (size_t l = 0; l < nl; ++l) {
    const BoundLeaf& bl = b.leaves[l];
    const orcg_column_view& v = views[l];
    DevLeaf& dl = hl[l];
    dl.nn = v.has_nulls ? v.not_null : nullptr;
    dl.op = bl.op;
    dl.lit0 = bl.lit0;
    dl.nlit = bl.nlit;
    dl.data = v.data;
    dl.index = nullptr;
    dl.dict_size = 0;
    if (v.has_nulls && !v.not_null) {
      *err = "column " + std::to_string(bl.column) + " has nulls and no mask";
      return ORCG_INVALID_ARGUMENT;
    }
    switch (bl.cls) {
      case kClsI64: dl.cls = kDevI64; break;
      case kClsF64: dl.cls = kDevF64; break;
      case kClsDec128: dl.cls = kDevDec128; break;
      case kClsNull: dl.cls = kDevNull; break;
      default:
        dl.data = d + o_truth[l];
        dl.lit0 = 0;
        if (v.index && v.dict_offsets) {
          dl.cls = kDevTruthDict;
          dl.index = v.index;
          dl.dict_size = v.dict_size;
        } else {
          dl.cls = kDevTruth;
        }
        break;
    }
    if (dl.cls <= kDevDec128 && !dl.data) {
      *err = "column " + std::to_string(bl.column) + " has no values";
      return ORCG_INVALID_ARGUMENT;
    }
  }
  memcpy(f->table.data() + o_ops, f->plan.ops.data(), nops * 4);
  if (!b.words.empty()) memcpy(f->table.data() + o_words, b.words.data(), b.words.size() * 8);
  memcpy(f->table.data() + o_soff, b.str_off.data(), b.str_off.size() * 4);
  if (!b.str_bytes.empty()) memcpy(f->table.data() + o_sbytes, b.str_bytes.data(), b.str_bytes.size());
  int rc = hip_check(c, hipMemcpyAsync(d, f->table.data(), table_bytes, hipMemcpyHostToDevice, c->stream),
                     "filter tables H2D");
  if (rc) return rc;
  Timer tm(c, f->timing);
  rc = tm.run(&f->ms[0], [&] {
    for (size_t l = 0; l < nl; ++l) {
      const BoundLeaf& bl = b.leaves[l];
      if (bl.cls != kClsString) continue;
      const orcg_column_view& v = views[l];
      StringLeafArgs a{};
      const bool dict = v.index && v.dict_offsets;
      if (dict) {
        a.dict_offsets = v.dict_offsets;
        a.n = v.dict_size;
      } else {
        a.start = (const int64_t*)v.data;
        a.length = v.length;
        a.nn = v.has_nulls ? v.not_null : nullptr;
        a.n = n;
      }
      a.blob = v.blob;
      a.blob_len = v.blob ? v.blob_len : 0;
      a.op = bl.op;
      a.nlit = bl.nlit;
      a.lit_off = (const uint32_t*)(d + o_soff) + bl.lit0;
      a.lit_bytes = d + o_sbytes;
      a.truth = d + o_truth[l];
      if (const int e = launch_string_leaf(c, a)) return e;
    }
    return (int)ORCG_OK;
  });
  if (rc) return rc;
  int64_t* d_counts = (int64_t*)(d + o_counts);
  int64_t* d_base = (int64_t*)(d + o_base);
  uint64_t* d_total = (uint64_t*)(d + o_total);
  rc = tm.run(&f->ms[1], [&] {
    return launch_combine(c, (const DevLeaf*)(d + o_leaves), (const uint32_t*)(d + o_ops), (uint32_t)nops,
                          (const int64_t*)(d + o_words), n, d + o_sel, d_counts);
  });
  if (rc) return rc;
  rc = tm.run(&f->ms[2], [&] { return launch_exclusive_scan(c, d_counts, tiles, d_base, nullptr, d_total); });
  if (rc) return rc;
  rc = tm.run(&f->ms[3], [&] { return launch_select(c, d + o_sel, tiles, d_base, (int64_t*)(d + o_selected)); });
  if (rc) return rc;
  uint64_t total = 0;
  if ((rc = hip_check(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, c->stream), "D2H selected count")))
    return rc;
  if ((rc = sync_ctx(c))) return rc;
  *count = total;
  return ORCG_OK;
}

int gather(Ctx* c, const GatherArgs& a, unsigned long long* d_nulls, uint64_t* nulls) {
  *nulls = 0;
  if (a.count == 0) return ORCG_OK;
  int rc = hip_check(c, hipMemsetAsync(d_nulls, 0, 8, c->stream), "memset");
  if (rc) return rc;
  if ((rc = launch_gather(c, a))) return rc;
  unsigned long long h = 0;
  if ((rc = hip_check(c, hipMemcpyAsync(&h, d_nulls, 8, hipMemcpyDeviceToHost, c->stream), "D2H null count")))
    return rc;
  if ((rc = sync_ctx(c))) return rc;
  *nulls = h;
  return ORCG_OK;
}

}  // namespace

extern "C" {

int orcg_filter_create(const orcg_filter_leaf* leaves, uint32_t nleaves, const orcg_filter_op* program,
                       uint32_t nprog, orcg_filter** out) {
  if (!out || (nleaves && !leaves) || (nprog && !program)) {
    g_create_error = "null argument";
    return ORCG_INVALID_ARGUMENT;
  }
  *out = nullptr;
  if (nleaves > kMaxLeaves) {
    g_create_error = "a filter has at most " + std::to_string(kMaxLeaves) + " leaves, not " + std::to_string(nleaves);
    return ORCG_INVALID_ARGUMENT;
  }
  std::vector<Leaf> ls(nleaves);
  uint64_t str_total = 0;
  for (uint32_t i = 0; i < nleaves; ++i) {
    ls[i].op = leaves[i].op;
    ls[i].column = leaves[i].column;
    ls[i].type = leaves[i].literal_type;
    if (leaves[i].nliterals && !leaves[i].literals) {
      g_create_error = "leaf " + std::to_string(i) + ": null literals";
      return ORCG_INVALID_ARGUMENT;
    }
    // the limits are checked before anything is copied, with the caller's counts
    if (leaves[i].nliterals > kMaxInList) {
      g_create_error = "leaf " + std::to_string(i) + ": an IN list has at most " + std::to_string(kMaxInList) +
                       " literals, not " + std::to_string(leaves[i].nliterals);
      return ORCG_INVALID_ARGUMENT;
    }
    const uint32_t take = leaves[i].nliterals;
    ls[i].lits.resize(take);
    for (uint32_t k = 0; k < take; ++k) {
      const orcg_literal& s = leaves[i].literals[k];
      Literal& l = ls[i].lits[k];
      l.lo = s.lo;
      l.hi = s.hi;
      l.d = s.d;
      l.scale = s.scale;
      if (leaves[i].literal_type == ORCG_LIT_STRING && s.bytes && s.len) {
        if (s.len > kMaxStringBytes || (str_total += s.len) > kMaxStringBytes) {
          // the whole filter's total, without copying past the limit
          uint64_t all = 0;
          for (uint32_t a = 0; a < nleaves; ++a)
            // (a later leaf's literals pointer has not been checked yet)
            for (uint32_t b = 0; leaves[a].literal_type == ORCG_LIT_STRING && leaves[a].literals &&
                                 b < leaves[a].nliterals && b <= kMaxInList; ++b)
              all += leaves[a].literals[b].bytes ? leaves[a].literals[b].len : 0;
          g_create_error = "a filter has at most " + std::to_string(kMaxStringBytes) +
                           " bytes of string literals, not " + std::to_string(all);
          return ORCG_INVALID_ARGUMENT;
        }
        l.s.assign((const char*)s.bytes, (size_t)s.len);
      }
    }
  }
  std::vector<ExprItem> prog(nprog);
  for (uint32_t i = 0; i < nprog; ++i) prog[i] = ExprItem{program[i].op, program[i].arg};
  std::unique_ptr<orcg_filter> f(new orcg_filter());
  if (!create(ls, prog, &f->plan, &g_create_error)) return ORCG_INVALID_ARGUMENT;
  *out = f.release();
  return ORCG_OK;
}

void orcg_filter_destroy(orcg_filter* f) { delete f; }

const char* orcg_filter_last_error(const orcg_filter* f) { return f ? f->err.c_str() : g_create_error.c_str(); }

int orcg_filter_set_timing(orcg_filter* f, int on) {
  if (!f) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> fl(f->mu);
  f->timing = on != 0;
  return ORCG_OK;
}

int orcg_filter_last_timing(const orcg_filter* f, double out_ms[4]) {
  if (!f || !out_ms) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> fl(const_cast<orcg_filter*>(f)->mu);
  for (int i = 0; i < 4; ++i) out_ms[i] = f->ms[i];
  return ORCG_OK;
}

int orcg_filter_columns_device(orcg_ctx* c, orcg_filter* f, const orcg_column_view* views, const orcg_type_info* types,
                               uint32_t ncols, uint64_t n, const int64_t** d_selected, uint64_t* count) {
  if (!c || !f || !d_selected || !count || (ncols && (!views || !types))) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> fl(f->mu);
  auto fail = [&](int rc, const std::string& m) {
    f->err = m;
    return set_error(c, rc, m);
  };
  // the columns as children of a root struct, each at its type id
  uint32_t top = 0;
  for (uint32_t i = 0; i < ncols; ++i) top = std::max(top, views[i].type_id);
  if (top > 65535)
    return fail(ORCG_INVALID_ARGUMENT, "bad type ids for the filter's columns");
  rt::Tree tree(top + 1);
  tree[0].kind = rt::kStruct;
  std::vector<int64_t> at(top + 1, -1);
  for (uint32_t i = 0; i < ncols; ++i) {
    const uint32_t id = views[i].type_id;
    if (id == 0 || at[id] >= 0) return fail(ORCG_INVALID_ARGUMENT, "bad type ids for the filter's columns");
    at[id] = i;
    tree[id].kind = types[i].kind;
    tree[id].precision = types[i].precision;
    tree[id].scale = types[i].scale;
    tree[id].maximum_length = types[i].maximum_length;
    tree[0].subtypes.push_back(id);
  }
  for (uint32_t id = 1; id <= top; ++id)
    if (at[id] < 0) tree[id].kind = rt::kStruct;  // a gap: no leaf may name it
  // a leaf on a column the caller did not give (the lowest such column)
  uint32_t missing = ~0u;
  for (const Leaf& l : f->plan.leaves)
    if (l.column <= top && l.column > 0 && at[l.column] < 0) missing = std::min(missing, l.column);
  if (missing != ~0u) return fail(ORCG_INVALID_ARGUMENT, "column " + std::to_string(missing) + " was not decoded");
  std::string err;
  if (!filter::bind(f->plan, tree, &f->bound, &err)) return fail(ORCG_INVALID_ARGUMENT, err);
  std::vector<orcg_column_view> lv(f->bound.leaves.size());
  for (uint32_t li : f->bound.order) {
    const uint32_t col = f->bound.leaves[li].column;
    if (at[col] < 0 || views[at[col]].num_elements != n)
      return fail(ORCG_INVALID_ARGUMENT, "column " + std::to_string(col) + " was not decoded");
    lv[li] = views[at[col]];
  }
  const int rc = run_filter(c, f, lv, n, [&](size_t bytes) {
    void* p = nullptr;
    return scratch(c, kScratchColumn, bytes, &p) ? nullptr : p;
  }, d_selected, count, &err);
  if (rc && !err.empty()) return fail(rc, err);
  if (rc) f->err = c->last_error;
  return rc;
}

int orcg_filter_gather_device(orcg_ctx* c, const int64_t* d_sel, uint64_t count, uint64_t n_src,
                              const void* const src8[3], void* const dst8[3], const void* src16, void* dst16,
                              const uint8_t* not_null, uint8_t* out_not_null, uint64_t* nulls) {
  if (!c || !nulls || (count && !d_sel) || (src16 && !dst16) || (not_null && !out_not_null))
    return ORCG_INVALID_ARGUMENT;
  GatherArgs a{};
  a.sel = d_sel;
  a.count = count;
  a.n_src = n_src;
  for (int k = 0; k < 3; ++k) {
    a.src8[k] = src8 ? (const uint64_t*)src8[k] : nullptr;
    a.dst8[k] = dst8 ? (uint64_t*)dst8[k] : nullptr;
    if (a.src8[k] && !a.dst8[k]) return ORCG_INVALID_ARGUMENT;
  }
  a.src16 = src16;
  a.dst16 = dst16;
  a.nn = not_null;
  a.out_nn = out_not_null;
  (void)hipSetDevice(c->device);
  void* d_nulls;
  if (const int rc = scratch(c, kScratchMisc, 8, &d_nulls)) return rc;
  a.nulls = (unsigned long long*)d_nulls;
  return gather(c, a, a.nulls, nulls);
}

int orcg_reader_filter_stripe(orcg_reader* r, uint64_t k, orcg_filter* f, const int64_t** d_selected,
                              uint64_t* count) {
  if (!r || !f || !d_selected || !count) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  std::lock_guard<std::mutex> fl(f->mu);  // (always after a reader's)
  Ctx* c = r->own.ctx;
  auto fail = [&](int rc, const std::string& m) {
    f->err = m;
    r->last_error = m;
    if (c) c->last_error = m;
    return rc;
  };
  if (!c) return fail(ORCG_INVALID_ARGUMENT, "reader has no device context");
  if (k >= r->nslots) return fail(ORCG_INVALID_ARGUMENT, "stripe index out of range of the last read");
  DevSlot& ds = *r->slots[k];
  ds.f_valid = false;
  const std::shared_ptr<const ReadPlan> plan = r->own.read;
  std::string err;
  if (!filter::bind(f->plan, plan ? plan->tree : r->file_tree(), &f->bound, &err)) return fail(ORCG_INVALID_ARGUMENT, err);
  const uint64_t n = ds.out.empty() ? 0 : ds.out[0].n;
  std::vector<orcg_column_view> lv(f->bound.leaves.size());
  for (uint32_t li : f->bound.order) {
    const uint32_t col = f->bound.leaves[li].column;
    if (col >= ds.out.size() || !ds.out[col].decoded)
      return fail(ORCG_INVALID_ARGUMENT, "column " + std::to_string(col) + " was not decoded");
    const ColOut& co = ds.out[col];
    // defensive: a primitive with no list, map or union ancestor has the root's
    // rows, so no read reaches this; the kernels index every leaf column by n
    if (co.n != n)
      return fail(ORCG_INVALID_ARGUMENT, "column " + std::to_string(col) + " does not have the root's row count");
    memset(&lv[li], 0, sizeof(lv[li]));
    lv[li].type_id = col;
    fill_view(co, &lv[li]);
  }
  const int rc = run_filter(c, f, lv, n, [&](size_t bytes) { return ds.pool.get(bytes); }, d_selected, count, &err);
  if (rc) return fail(rc, err.empty() ? c->last_error : err);
  ds.f_selected = *d_selected;
  ds.f_count = *count;
  ds.f_valid = true;
  return ORCG_OK;
}

int orcg_reader_filtered_column(orcg_reader* r, uint64_t k, uint32_t id, orcg_column_view* out) {
  if (!r || !out) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  Ctx* c = r->own.ctx;
  auto fail = [&](int rc, const std::string& m) {
    r->last_error = m;
    if (c) c->last_error = m;
    return rc;
  };
  if (!c) return fail(ORCG_INVALID_ARGUMENT, "reader has no device context");
  if (k >= r->nslots || id >= r->footer.types.size())
    return fail(ORCG_INVALID_ARGUMENT, "stripe or column index out of range of the last read");
  DevSlot& ds = *r->slots[k];
  if (!ds.f_valid) return fail(ORCG_INVALID_ARGUMENT, "the stripe has not been filtered");
  const std::string col = "column " + std::to_string(id);
  if (under_repeated(r->file_tree(), id, true)) return fail(ORCG_INVALID_ARGUMENT, col + " is not filtered: nested");
  if (id >= ds.out.size() || !ds.out[id].decoded) return fail(ORCG_INVALID_ARGUMENT, col + " was not decoded");
  const ColOut& co = ds.out[id];
  const uint32_t kind = co.out_kind();
  const uint64_t cnt = ds.f_count;
  memset(out, 0, sizeof(*out));
  out->type_id = id;
  out->kind = kind;
  fill_view(co, out);
  out->num_elements = cnt;
  GatherArgs a{};
  a.sel = ds.f_selected;
  a.count = cnt;
  a.n_src = co.n;
  auto get = [&](size_t bytes) { return ds.pool.get(std::max<size_t>(bytes, 1)); };
  bool oom = false;
  int slot = 0;
  auto add8 = [&](const void* src) -> const void* {
    if (!src) return nullptr;
    void* dst = get(cnt * 8);
    oom |= !dst;
    a.src8[slot] = (const uint64_t*)src;
    a.dst8[slot] = (uint64_t*)dst;
    ++slot;
    return dst;
  };
  const bool wide = kind == ORCG_TYPE_DECIMAL &&
                    (co.out_precision(r->footer.types[id].precision) > 18 ||
                     co.out_precision(r->footer.types[id].precision) == 0);
  if (kind == ORCG_TYPE_STRUCT) {
    // the mask alone
  } else if (wide) {
    a.src16 = co.data;
    a.dst16 = get(cnt * 16);
    oom |= !a.dst16;
    out->data = a.dst16;
  } else {
    out->data = add8(co.data);
    out->length = (const int64_t*)add8(co.length);
    if (co.secondary) out->secondary = (const int64_t*)add8(co.secondary);
    else out->index = (const int64_t*)add8(co.index);
  }
  if (co.has_nulls && co.nn) {
    a.nn = co.nn;
    a.out_nn = (uint8_t*)get(cnt);
    oom |= !a.out_nn;
  }
  a.nulls = (unsigned long long*)get(8);
  oom |= !a.nulls;
  if (oom) return fail(ORCG_OUT_OF_MEMORY, "device allocation failed");
  (void)hipSetDevice(c->device);
  uint64_t nulls = 0;
  if (const int rc = gather(c, a, a.nulls, &nulls)) return fail(rc, c->last_error);
  out->has_nulls = nulls ? 1 : 0;
  out->not_null = a.out_nn;
  return ORCG_OK;
}

}  // extern "C"
