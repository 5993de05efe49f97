// The reader's Arrow entries (include/orcg_arrow.h): the Arrow schema of the
// selected columns (host only), and the stripe last decoded exported as Arrow
// arrays, re-laid in HBM by the kernels of arrow_kernels.hip.
//
// An export runs in two steps on the reader's context stream. First every
// string column's row lengths are scanned (the materialised dictionary
// columns' byte totals are the one thing the host has to read before it can
// lay the buffers out). Then one contiguous region of the stripe's device
// arena is carved into the 64-byte aligned buffers, every kernel is launched
// into it, and the export's block (per column: error word, null count, byte
// total) comes back with the stripe's one synchronisation.
#include <stdlib.h>

#include "arrow_internal.hh"
#include "reader_internal.hh"

using namespace orcg::arrow;

namespace {

// What a column is exported as: its kind, and a decimal's precision and scale
struct Kind {
  uint32_t kind, precision, scale;
};

Kind schema_kind(const orcg_reader* r, const ReadPlan* plan, uint32_t id) {
  if (plan && plan->conv[id] == rt::kConvert) {
    const rt::Node& n = plan->tree[id];
    return Kind{n.kind, n.precision, n.scale};
  }
  const TypeInfo& t = r->footer.types[id];
  return Kind{t.kind, t.precision, t.scale};
}

bool is_string_kind(uint32_t k) {
  return k == ORCG_TYPE_STRING || k == ORCG_TYPE_VARCHAR || k == ORCG_TYPE_CHAR || k == ORCG_TYPE_BINARY;
}

// the Arrow format string of a leaf kind ("" for the compound kinds)
std::string leaf_format(const orcg_reader* r, const Kind& k) {
  switch (k.kind) {
    case ORCG_TYPE_BOOLEAN: return "b";
    case ORCG_TYPE_BYTE: return "c";
    case ORCG_TYPE_SHORT: return "s";
    case ORCG_TYPE_INT: return "i";
    case ORCG_TYPE_LONG: return "l";
    case ORCG_TYPE_FLOAT: return "f";
    case ORCG_TYPE_DOUBLE: return "g";
    case ORCG_TYPE_DATE: return "tdD";
    case ORCG_TYPE_TIMESTAMP: return "tsn:";
    case ORCG_TYPE_TIMESTAMP_INSTANT: return "tsn:UTC";
    case ORCG_TYPE_BINARY: return "z";
    case ORCG_TYPE_STRING:
    case ORCG_TYPE_VARCHAR:
    case ORCG_TYPE_CHAR: return "u";
    case ORCG_TYPE_DECIMAL:
      // Hive 0.11 decimals (precision 0) are decoded at the forced scale
      if (k.precision == 0) return "d:38," + std::to_string(r->hive11_scale);
      return "d:" + std::to_string(k.precision) + "," + std::to_string(k.scale);
    default: return "";
  }
}

std::string union_error(uint32_t id) { return "union column " + std::to_string(id) + " is not exported to Arrow"; }

// ---- schema ----

struct SchemaPriv {
  std::string format, name;
  std::vector<std::unique_ptr<ArrowSchema>> kids;
  std::vector<ArrowSchema*> kid_ptrs;
  std::unique_ptr<ArrowSchema> dict;
};

void release_schema(ArrowSchema* s) {
  if (!s || !s->release) return;
  SchemaPriv* p = (SchemaPriv*)s->private_data;
  for (ArrowSchema* k : p->kid_ptrs)
    if (k->release) k->release(k);
  if (s->dictionary && s->dictionary->release) s->dictionary->release(s->dictionary);
  delete p;
  s->release = nullptr;
}

void schema_node(ArrowSchema* s, SchemaPriv* p, const std::string& format, const std::string& name, int64_t flags) {
  p->format = format;
  p->name = name;
  memset(s, 0, sizeof *s);
  s->format = p->format.c_str();
  s->name = p->name.c_str();
  s->flags = flags;
  s->release = release_schema;
  s->private_data = p;
}

void schema_finish(ArrowSchema* s, SchemaPriv* p) {
  for (auto& k : p->kids) p->kid_ptrs.push_back(k.get());
  s->n_children = (int64_t)p->kid_ptrs.size();
  s->children = p->kid_ptrs.empty() ? nullptr : p->kid_ptrs.data();
  s->dictionary = p->dict.get();
}

struct SchemaBuild {
  const orcg_reader* r;
  const ReadPlan* plan;
  const std::vector<uint8_t>* sel;
  const DevSlot* slot;  // the stripe at hand (dictionary form), or null
  bool selected(uint32_t id) const { return id < sel->size() && (*sel)[id]; }

  // false: a selected union below (err set)
  bool build(uint32_t id, const std::string& name, int64_t flags, ArrowSchema* s, std::string* err) const {
    const Kind k = schema_kind(r, plan, id);
    const TypeInfo& t = r->footer.types[id];
    std::unique_ptr<SchemaPriv> p(new SchemaPriv());
    bool ok = true;
    if (k.kind == ORCG_TYPE_UNION) {
      *err = union_error(id);
      return false;
    } else if (k.kind == ORCG_TYPE_STRUCT) {
      schema_node(s, p.get(), "+s", name, flags);
      for (size_t j = 0; j < t.subtypes.size() && ok; ++j) {
        if (!selected(t.subtypes[j])) continue;
        p->kids.emplace_back(new ArrowSchema());
        ok = build(t.subtypes[j], j < t.field_names.size() ? t.field_names[j] : "", ARROW_FLAG_NULLABLE,
                   p->kids.back().get(), err);
        if (!ok) p->kids.pop_back();
      }
    } else if (k.kind == ORCG_TYPE_LIST && t.subtypes.size() == 1) {
      schema_node(s, p.get(), "+l", name, flags);
      p->kids.emplace_back(new ArrowSchema());
      ok = build(t.subtypes[0], "item", ARROW_FLAG_NULLABLE, p->kids.back().get(), err);
      if (!ok) p->kids.pop_back();
    } else if (k.kind == ORCG_TYPE_MAP && t.subtypes.size() == 2) {
      schema_node(s, p.get(), "+m", name, flags);
      p->kids.emplace_back(new ArrowSchema());
      ArrowSchema* e = p->kids.back().get();
      std::unique_ptr<SchemaPriv> ep(new SchemaPriv());
      schema_node(e, ep.get(), "+s", "entries", 0);
      ep->kids.emplace_back(new ArrowSchema());
      ok = build(t.subtypes[0], "key", 0, ep->kids.back().get(), err);
      if (!ok) ep->kids.pop_back();
      if (ok) {
        ep->kids.emplace_back(new ArrowSchema());
        ok = build(t.subtypes[1], "value", ARROW_FLAG_NULLABLE, ep->kids.back().get(), err);
        if (!ok) ep->kids.pop_back();
      }
      schema_finish(e, ep.release());
    } else {
      const std::string f = leaf_format(r, k);
      if (f.empty()) {
        *err = "column " + std::to_string(id) + " has a malformed type";
        return false;
      }
      const ColOut* c = slot && id < slot->out.size() ? &slot->out[id] : nullptr;
      if (c && c->decoded && is_string_kind(k.kind) && c->index && c->dict_offsets) {
        schema_node(s, p.get(), "i", name, flags);
        p->dict.reset(new ArrowSchema());
        SchemaPriv* dp = new SchemaPriv();
        schema_node(p->dict.get(), dp, f, "", ARROW_FLAG_NULLABLE);
        schema_finish(p->dict.get(), dp);
      } else {
        schema_node(s, p.get(), f, name, flags);
      }
    }
    schema_finish(s, p.release());
    if (!ok) release_schema(s);
    return ok;
  }
};

// ---- arrays ----

// Everything an exported tree shares: the host allocation of a host export
struct Shared {
  void* host = nullptr;
  ~Shared() { free(host); }
};

struct ArrayPriv {
  std::shared_ptr<Shared> shared;
  std::vector<const void*> bufs;
  std::vector<std::unique_ptr<ArrowArray>> kids;
  std::vector<ArrowArray*> kid_ptrs;
  std::unique_ptr<ArrowArray> dict;
};

void release_array(ArrowArray* a) {
  if (!a || !a->release) return;
  ArrayPriv* p = (ArrayPriv*)a->private_data;
  for (ArrowArray* k : p->kid_ptrs)
    if (k->release) k->release(k);
  if (a->dictionary && a->dictionary->release) a->dictionary->release(a->dictionary);
  delete p;
  a->release = nullptr;
}

// One buffer of a node: re-laid into the region (region_off), or the decode's
// own device buffer (alias); none: a NULL buffer (no validity)
struct Buf {
  bool none = true;
  bool is_alias = false;
  const void* alias = nullptr;
  uint64_t bytes = 0;       // re-laid: padded; alias: the payload
  uint64_t region_off = 0;  // re-laid
  uint64_t host_off = 0;    // a host export's offset in its allocation
};

struct Node {
  uint32_t id = 0;
  int64_t length = 0;
  int word = -1;  // its words in the export's block (3 each: error, nulls, byte total)
  bool has_validity = false;
  std::vector<Buf> bufs;
  std::vector<Node> kids;
  std::unique_ptr<Node> dict;
  // string columns: the int64 scan of the row lengths (step one)
  int64_t* scan = nullptr;
  bool gathered = false;  // a materialised dictionary column
};

struct Export {
  orcg_reader* r;
  Ctx* ctx;
  DevSlot* slot;
  bool dictionary;
  std::vector<uint8_t> sel;
  uint64_t region = 0;  // bytes laid out so far
  int words = 0;
  std::vector<std::pair<uint32_t, int>> word_of;  // (column, block word) in column order
  std::vector<std::function<int(uint8_t*)>> ops;  // launches into the region
  unsigned long long* d_block = nullptr;
  std::vector<unsigned long long> h_block;
  bool need_totals = false;

  bool selected(uint32_t id) const { return id < sel.size() && sel[id]; }
  int fail(int rc, const std::string& m) {
    r->last_error = m;
    if (ctx) ctx->last_error = m;
    return rc;
  }
  Kind kind_of(uint32_t id) const {
    const ColOut& c = slot->out[id];
    const TypeInfo& t = r->footer.types[id];
    if (c.converted) return Kind{c.rkind, c.rprecision, c.rscale};
    return Kind{t.kind, t.precision, t.scale};
  }
  template <typename T>
  T* temp(uint64_t count) {
    return (T*)slot->pool.get(std::max<uint64_t>(count, 1) * sizeof(T));
  }

  // the first selected column, in column order, that cannot be exported
  int validate() {
    const size_t nt = r->footer.types.size();
    if (nt == 0 || r->footer.types[0].kind != ORCG_TYPE_STRUCT)
      return fail(ORCG_INVALID_ARGUMENT, "the file's top level is not a struct: not exported to Arrow");
    if (slot->out.size() < nt) return fail(ORCG_INVALID_ARGUMENT, "no decoded stripe to export");
    for (uint32_t id = 0; id < nt; ++id) {
      if (!selected(id)) continue;
      if (kind_of(id).kind == ORCG_TYPE_UNION) return fail(ORCG_INVALID_ARGUMENT, union_error(id));
      if (!slot->out[id].decoded)
        return fail(ORCG_INVALID_ARGUMENT,
                    "column " + std::to_string(id) + " was not decoded (" +
                        rt::kind_name(r->footer.types[id].kind) +
                        "; not selected at the stripe's read, or its writer time zone did not resolve)");
    }
    return ORCG_OK;
  }

  Buf relaid(uint64_t payload) {
    Buf b;
    b.none = false;
    b.bytes = padded(payload);
    b.region_off = region;
    region += b.bytes;
    return b;
  }
  static Buf aliased(const void* p, uint64_t bytes) {
    Buf b;
    b.none = false;
    b.is_alias = true;
    b.alias = p;
    b.bytes = bytes;
    return b;
  }
  int new_word(uint32_t id) {
    word_of.push_back({id, words});
    words += 3;
    return words - 3;
  }

  // Step one of a string column: its masked row lengths scanned into int64
  int scan_lengths(Node& nd, const ColOut& c, bool dict) {
    const uint64_t n = c.n;
    int64_t* lens = temp<int64_t>(n);
    nd.scan = temp<int64_t>(n + 1);
    if (!lens || !nd.scan) return fail(ORCG_OUT_OF_MEMORY, "device allocation failed");
    int rc = launch_row_lengths(ctx, dict ? nullptr : c.length, dict ? c.index : nullptr, c.dict_offsets, c.dict_size,
                                c.has_nulls ? c.nn : nullptr, n, lens, d_block + nd.word);
    if (!rc) rc = launch_exclusive_scan(ctx, lens, n, nd.scan, nullptr, (uint64_t*)(d_block + nd.word + 2));
    return rc;
  }

  // The node of column id: its words, step-one launches and children. The
  // buffers are laid out by layout(), once the byte totals are known.
  int plan(uint32_t id, Node& nd) {
    const ColOut& c = slot->out[id];
    const TypeInfo& t = r->footer.types[id];
    const Kind k = kind_of(id);
    nd.id = id;
    nd.length = (int64_t)c.n;
    nd.word = new_word(id);
    nd.has_validity = c.has_nulls && c.nn && c.n;
    int rc = ORCG_OK;
    if (k.kind == ORCG_TYPE_STRUCT) {
      for (uint32_t st : t.subtypes) {
        if (!selected(st)) continue;
        nd.kids.emplace_back();
        if ((rc = plan(st, nd.kids.back()))) return rc;
      }
    } else if (k.kind == ORCG_TYPE_LIST || k.kind == ORCG_TYPE_MAP) {
      for (uint32_t st : t.subtypes) {
        nd.kids.emplace_back();
        if ((rc = plan(st, nd.kids.back()))) return rc;
      }
    } else if (is_string_kind(k.kind)) {
      const bool dict = c.index && c.dict_offsets;
      if (dict && dictionary) {
        nd.dict.reset(new Node());
        nd.dict->id = id;
        nd.dict->length = (int64_t)c.dict_size;
        nd.dict->word = new_word(id);
      } else {
        nd.gathered = dict;
        need_totals |= dict;
        rc = scan_lengths(nd, c, dict);
      }
    }
    return rc;
  }

  // Buffers and launches of a node (column order, so the region is too)
  int layout(Node& nd) {
    const uint32_t id = nd.id;
    const ColOut& c = slot->out[id];
    const Kind k = kind_of(id);
    const uint64_t n = c.n;
    unsigned long long* const d_words = d_block + nd.word;
    Buf validity;
    if (nd.has_validity) {
      validity = relaid((n + 7) / 8);
      const uint8_t* nn = c.nn;
      ops.push_back([=](uint8_t* base) {
        return launch_validity(ctx, nn, n, base + validity.region_off, validity.bytes, d_words + 1);
      });
    }
    nd.bufs.push_back(validity);
    auto fixed = [&](int form, const void* src, const void* src2) {
      const Buf b = relaid(fixed_bytes(form, n));
      ops.push_back(
          [=](uint8_t* base) { return launch_fixed(ctx, form, src, src2, n, base + b.region_off, b.bytes); });
      nd.bufs.push_back(b);
    };
    auto offsets = [&](const int64_t* src, uint64_t count) {
      const Buf b = relaid(4 * count);
      ops.push_back([=](uint8_t* base) {
        return launch_narrow_offsets(ctx, src, count, (int32_t*)(base + b.region_off), b.bytes, d_words);
      });
      nd.bufs.push_back(b);
      return b;
    };
    int rc = ORCG_OK;
    switch (k.kind) {
      case ORCG_TYPE_BOOLEAN: fixed(ORCG_ARROW_BOOL, c.data, nullptr); break;
      case ORCG_TYPE_BYTE: fixed(ORCG_ARROW_INT8, c.data, nullptr); break;
      case ORCG_TYPE_SHORT: fixed(ORCG_ARROW_INT16, c.data, nullptr); break;
      case ORCG_TYPE_INT:
      case ORCG_TYPE_DATE: fixed(ORCG_ARROW_INT32, c.data, nullptr); break;
      case ORCG_TYPE_FLOAT: fixed(ORCG_ARROW_FLOAT32, c.data, nullptr); break;
      case ORCG_TYPE_LONG:
      case ORCG_TYPE_DOUBLE: nd.bufs.push_back(aliased(c.data, 8 * n)); break;  // already Arrow's layout
      case ORCG_TYPE_DECIMAL:
        fixed(k.precision > 18 || k.precision == 0 ? ORCG_ARROW_DEC128 : ORCG_ARROW_DEC64, c.data, nullptr);
        break;
      case ORCG_TYPE_TIMESTAMP:
      case ORCG_TYPE_TIMESTAMP_INSTANT: fixed(ORCG_ARROW_TIMESTAMP_NS, c.data, c.secondary); break;
      case ORCG_TYPE_STRUCT: break;
      case ORCG_TYPE_LIST:
      case ORCG_TYPE_MAP:
        if (!c.offsets) return fail(ORCG_INVALID_ARGUMENT, "column " + std::to_string(id) + " has no offsets");
        offsets(c.offsets, n + 1);
        break;
      default: {  // string kinds
        if (nd.dict) {
          fixed(ORCG_ARROW_INT32, c.index, nullptr);
          Node& d = *nd.dict;
          unsigned long long* const dict_words = d_block + d.word;
          d.bufs.push_back(Buf());
          const Buf ob = relaid(4 * (c.dict_size + 1));
          const int64_t* src = c.dict_offsets;
          const uint64_t count = c.dict_size + 1;
          ops.push_back([=](uint8_t* base) {
            return launch_narrow_offsets(ctx, src, count, (int32_t*)(base + ob.region_off), ob.bytes, dict_words);
          });
          d.bufs.push_back(ob);
          d.bufs.push_back(aliased(c.blob, c.blob_len));
        } else if (nd.gathered) {
          const Buf ob = offsets(nd.scan, n + 1);
          const uint64_t total = h_block[nd.word + 2];
          if (total > 0x7fffffffull) break;  // (the offsets' range check reports it)
          const Buf db = relaid(total);
          const ColOut* cc = &c;
          ops.push_back([=](uint8_t* base) {
            return launch_dict_gather_bytes(ctx, (const int32_t*)(base + ob.region_off), cc->index, n,
                                            cc->dict_offsets, cc->dict_size, cc->blob, cc->blob_len,
                                            base + db.region_off, total, db.bytes);
          });
          nd.bufs.push_back(db);
        } else {
          offsets(nd.scan, n + 1);
          nd.bufs.push_back(aliased(c.blob, c.blob_len));  // the DATA stream's bytes: no copy
        }
      }
    }
    for (Node& kid : nd.kids)
      if ((rc = layout(kid))) return rc;
    return rc;
  }

  // The block's errors, the first column in column order
  int check_block() {
    for (const auto& w : word_of) {
      const unsigned long long e = h_block[w.second];
      if (e == kNoError) continue;
      if ((e & 0xff) == kArrowDictIndex)
        return fail(ORCG_PARSE_ERROR, "column " + std::to_string(w.first) +
                                          ": Entry index out of range in StringDictionaryColumn");
      return fail(ORCG_INVALID_ARGUMENT, "column " + std::to_string(w.first) +
                                             ": offsets do not fit int32 (the last offset is above 2^31 - 1)");
    }
    return ORCG_OK;
  }

  int read_block() {
    int rc = hip_check(ctx, hipMemcpyAsync(h_block.data(), d_block, 8 * h_block.size(), hipMemcpyDeviceToHost,
                                           ctx->stream), "D2H export block");
    if (!rc) rc = sync_ctx(ctx);
    if (rc) return fail(rc, ctx->last_error);
    return check_block();
  }

  // host export: room for the buffers that were not re-laid, after the region
  void place_host(Node& nd, uint64_t* at) {
    for (Buf& b : nd.bufs) {
      if (b.none) continue;
      b.host_off = b.is_alias ? *at : b.region_off;
      if (b.is_alias) *at += padded(b.bytes);
    }
    if (nd.dict) place_host(*nd.dict, at);
    for (Node& k : nd.kids) place_host(k, at);
  }

  int copy_aliases(const Node& nd, uint8_t* host) {
    for (const Buf& b : nd.bufs) {
      if (b.none || !b.is_alias || !b.alias || !b.bytes) continue;
      const int rc = hip_check(ctx, hipMemcpyAsync(host + b.host_off, b.alias, b.bytes, hipMemcpyDeviceToHost,
                                                   ctx->stream), "D2H column buffer");
      if (rc) return rc;
      memset(host + b.host_off + b.bytes, 0, padded(b.bytes) - b.bytes);  // its padding
    }
    if (nd.dict) {
      const int rc = copy_aliases(*nd.dict, host);
      if (rc) return rc;
    }
    for (const Node& k : nd.kids) {
      const int rc = copy_aliases(k, host);
      if (rc) return rc;
    }
    return ORCG_OK;
  }

  // The ArrowArray of a node; base: the region on the device, or the host
  // allocation. A buffer of no bytes still gets an address (base).
  void emit(const Node& nd, ArrowArray* a, const uint8_t* base, bool host, const std::shared_ptr<Shared>& sh) {
    ArrayPriv* p = new ArrayPriv();
    p->shared = sh;
    memset(a, 0, sizeof *a);
    a->length = nd.length;
    a->null_count = nd.has_validity ? (int64_t)h_block[nd.word + 1] : 0;
    for (const Buf& b : nd.bufs) {
      if (b.none) p->bufs.push_back(nullptr);
      else if (host) p->bufs.push_back(base + b.host_off);
      else if (b.is_alias) p->bufs.push_back(b.alias ? b.alias : base);
      else p->bufs.push_back(base + b.region_off);
    }
    const Kind k = kind_of(nd.id);
    if (k.kind == ORCG_TYPE_MAP && nd.kids.size() == 2) {
      // map: one child, the entries struct (no validity) of key and value
      p->kids.emplace_back(new ArrowArray());
      ArrowArray* e = p->kids.back().get();
      ArrayPriv* ep = new ArrayPriv();
      ep->shared = sh;
      memset(e, 0, sizeof *e);
      e->length = nd.kids[0].length;
      ep->bufs.push_back(nullptr);
      for (const Node& kid : nd.kids) {
        ep->kids.emplace_back(new ArrowArray());
        emit(kid, ep->kids.back().get(), base, host, sh);
      }
      finish(e, ep);
    } else {
      for (const Node& kid : nd.kids) {
        p->kids.emplace_back(new ArrowArray());
        emit(kid, p->kids.back().get(), base, host, sh);
      }
    }
    if (nd.dict) {
      p->dict.reset(new ArrowArray());
      emit(*nd.dict, p->dict.get(), base, host, sh);
    }
    finish(a, p);
  }

  static void finish(ArrowArray* a, ArrayPriv* p) {
    for (auto& k : p->kids) p->kid_ptrs.push_back(k.get());
    a->n_buffers = (int64_t)p->bufs.size();
    a->buffers = p->bufs.data();
    a->n_children = (int64_t)p->kid_ptrs.size();
    a->children = p->kid_ptrs.empty() ? nullptr : p->kid_ptrs.data();
    a->dictionary = p->dict.get();
    a->release = release_array;
    a->private_data = p;
  }

  int run(bool host, ArrowArray* out) {
    int rc = validate();
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    Node root;
    // the block is sized before the plan: three words a column and dictionary
    const size_t cap = 3 * 2 * r->footer.types.size();
    h_block.assign(cap, 0);
    for (size_t i = 0; i < cap; i += 3) h_block[i] = kNoError;
    d_block = temp<unsigned long long>(cap);
    if (!d_block) return fail(ORCG_OUT_OF_MEMORY, "device allocation failed");
    rc = hip_check(ctx, hipMemcpyAsync(d_block, h_block.data(), 8 * cap, hipMemcpyHostToDevice, ctx->stream),
                   "H2D export block");
    if (!rc) rc = plan(0, root);
    if (rc) {
      (void)hipStreamSynchronize(ctx->stream);  // h_block may still be read by the copy
      return fail(rc, ctx->last_error);
    }
    if (need_totals) {
      if ((rc = read_block())) return rc;
    }
    if ((rc = layout(root))) return rc;
    uint8_t* d_region = (uint8_t*)slot->pool.get(std::max<uint64_t>(region, 64));
    if (!d_region) return fail(ORCG_OUT_OF_MEMORY, "device allocation failed");
    for (auto& op : ops)
      if ((rc = op(d_region))) break;
    std::shared_ptr<Shared> sh(new Shared());
    if (!rc && host) {
      uint64_t total = std::max<uint64_t>(region, 64);
      place_host(root, &total);
      if (posix_memalign(&sh->host, 64, total)) {
        sh->host = nullptr;
        rc = set_error(ctx, ORCG_OUT_OF_MEMORY, "host allocation failed");
      } else {
        if (region < 64) memset((uint8_t*)sh->host + region, 0, 64 - region);
        if (region)
          rc = hip_check(ctx, hipMemcpyAsync(sh->host, d_region, region, hipMemcpyDeviceToHost, ctx->stream),
                         "D2H Arrow region");
        if (!rc) rc = copy_aliases(root, (uint8_t*)sh->host);
      }
    }
    if (rc) {
      (void)hipStreamSynchronize(ctx->stream);
      return fail(rc, ctx->last_error);
    }
    if ((rc = read_block())) return rc;
    emit(root, out, host ? (const uint8_t*)sh->host : d_region, host, sh);
    device_region = d_region;
    return ORCG_OK;
  }
  const uint8_t* device_region = nullptr;
};

int export_stripe(orcg_reader* r, int dictionary, bool host, ArrowArray* out) {
  if (!r || !out) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  memset(out, 0, sizeof *out);
  Export e{r, r->own.ctx, nullptr, dictionary != 0, r->own.selected};
  if (!r->own.ctx) return e.fail(ORCG_INVALID_ARGUMENT, "reader has no device context");
  if (r->nslots == 0 || r->slots.empty()) return e.fail(ORCG_INVALID_ARGUMENT, "no decoded stripe to export");
  e.slot = r->slots[0].get();
  return e.run(host, out);
}

}  // namespace

extern "C" {

int orcg_reader_arrow_schema(const orcg_reader* r, int dictionary, struct ArrowSchema* out) {
  if (!r || !out) return ORCG_INVALID_ARGUMENT;
  orcg_reader* rw = const_cast<orcg_reader*>(r);
  memset(out, 0, sizeof *out);
  std::vector<uint8_t> sel;
  std::shared_ptr<const ReadPlan> plan;
  const DevSlot* slot = nullptr;
  {
    std::lock_guard<std::mutex> lk(rw->mu);
    sel = r->own.selected;
    plan = r->own.read;
    if (dictionary && r->nslots > 0 && !r->slots.empty()) slot = r->slots[0].get();
  }
  if (r->footer.types.empty() || r->footer.types[0].kind != ORCG_TYPE_STRUCT)
    return rw->fail_user(ORCG_INVALID_ARGUMENT, "the file's top level is not a struct: not exported to Arrow");
  const SchemaBuild b{r, plan.get(), &sel, slot};
  std::string err;
  if (!b.build(0, "", 0, out, &err)) {
    memset(out, 0, sizeof *out);
    return rw->fail_user(ORCG_INVALID_ARGUMENT, err);
  }
  return ORCG_OK;
}

int orcg_reader_export_arrow_device(orcg_reader* r, int dictionary, struct ArrowDeviceArray* out) {
  if (!r || !out) return ORCG_INVALID_ARGUMENT;
  memset(out, 0, sizeof *out);
  const int rc = export_stripe(r, dictionary, false, &out->array);
  if (rc) return rc;
  out->device_id = r->own.ctx->device;
  out->device_type = ARROW_DEVICE_ROCM;
  out->sync_event = nullptr;  // the stream was synchronised
  return ORCG_OK;
}

int orcg_reader_export_arrow_host(orcg_reader* r, int dictionary, struct ArrowArray* out) {
  return export_stripe(r, dictionary, true, out);
}

}  // extern "C"
