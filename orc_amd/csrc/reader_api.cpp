// The reader's C entry points (include/orcg_reader.h); the row reader's are
// in row_reader.cpp.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "reader_internal.hh"

static thread_local std::string t_open_error;

orcg_reader::~orcg_reader() {
  if (B.ev_pre) (void)hipEventDestroy(B.ev_pre);
  if (h_pub) (void)hipHostFree(h_pub);
  slots.clear();
  if (mapped) munmap(mapped, file_len);
  if (h_sync) (void)hipHostFree(h_sync);
  for (Flight& f : flights) {
    if (f.h_defer) (void)hipHostFree(f.h_defer);
    if (f.h_rb) (void)hipHostFree(f.h_rb);
    for (const EvPair& p : f.ev_used) ev_pool.push_back(p.a), ev_pool.push_back(p.b);
    if (f.done) (void)hipEventDestroy(f.done);
    for (hipEvent_t e : {f.ev_up0, f.ev_up1, f.ev_dec})
      if (e) (void)hipEventDestroy(e);
  }
  for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
}

int orcg::reader::compute_selection(orcg_reader* r, const uint8_t* include, uint32_t ntypes,
                                    std::vector<uint8_t>& sel) {
  const size_t nt = r->footer.types.size();
  sel.assign(nt, 1);
  if (!include) return ORCG_OK;
  if (ntypes > nt) return r->fail_user(ORCG_INVALID_ARGUMENT, "include list longer than the type list");
  std::vector<uint32_t> parent(nt, 0);
  for (size_t i = 0; i < nt; ++i)
    for (uint32_t st : r->footer.types[i].subtypes) parent[st] = (uint32_t)i;
  for (auto& c : sel) c = 0;
  sel[0] = 1;
  for (uint32_t i = 0; i < ntypes; ++i) {
    if (!include[i]) continue;
    for (uint32_t a = i; a != 0; a = parent[a]) sel[a] = 1;
    std::vector<uint32_t> st{i};
    while (!st.empty()) {
      const uint32_t x = st.back();
      st.pop_back();
      sel[x] = 1;
      for (uint32_t y : r->footer.types[x].subtypes) st.push_back(y);
    }
  }
  return ORCG_OK;
}

void orcg::reader::fill_view(const ColView& c, orcg_column_view* out) {
  out->encoding = c.encoding;
  out->decoded = c.decoded ? 1u : 0u;
  if (!c.decoded) return;  // not selected, or not decodable (view.decoded == 0)
  out->num_elements = c.n;
  out->has_nulls = c.has_nulls ? 1 : 0;
  out->not_null = c.nn;
  out->data = c.data;
  out->length = c.length;
  out->offsets = c.offsets;
  out->blob = c.blob;
  out->blob_len = c.blob_len;
  out->secondary = c.secondary;
  out->tags = c.tags;
  out->index = c.index;
  out->dict_offsets = c.dict_offsets;
  out->dict_size = c.dict_size;
}

extern "C" {

const char* orcg_reader_open_error(void) { return t_open_error.c_str(); }

int orcg_reader_open(orcg_ctx* ctx, const uint8_t* file, uint64_t file_len, orcg_reader** out) {
  if (!out || (file_len && !file)) return ORCG_INVALID_ARGUMENT;
  *out = nullptr;
  std::unique_ptr<orcg_reader> r(new orcg_reader());
  r->own.ctx = ctx;
  r->file = file;
  r->file_len = file_len;
  const int rc = r->open_tail();
  if (rc) {
    t_open_error = r->last_error;
    if (ctx) ctx->last_error = r->last_error;
    return rc;
  }
  *out = r.release();
  return ORCG_OK;
}

int orcg_reader_open_file(orcg_ctx* ctx, const char* path, orcg_reader** out) {
  if (!out || !path) return ORCG_INVALID_ARGUMENT;
  *out = nullptr;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) {
    t_open_error = std::string("Can't open ") + path;
    if (ctx) ctx->last_error = t_open_error;
    return ORCG_INVALID_ARGUMENT;
  }
  struct stat st;
  fstat(fd, &st);
  const uint64_t len = (uint64_t)st.st_size;
  void* m = len ? mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
  close(fd);
  if (len && m == MAP_FAILED) {
    t_open_error = std::string("Can't map ") + path;
    if (ctx) ctx->last_error = t_open_error;
    return ORCG_INVALID_ARGUMENT;
  }
  std::unique_ptr<orcg_reader> r(new orcg_reader());
  r->own.ctx = ctx;
  r->file = (const uint8_t*)m;
  r->file_len = len;
  r->mapped = m;
  const int rc = r->open_tail();
  if (rc) {
    t_open_error = r->last_error;
    if (ctx) ctx->last_error = r->last_error;
    return rc;
  }
  *out = r.release();
  return ORCG_OK;
}

void orcg_reader_destroy(orcg_reader* r) { delete r; }
const char* orcg_reader_last_error(const orcg_reader* r) { return r ? r->last_error.c_str() : "null reader"; }
uint64_t orcg_reader_num_rows(const orcg_reader* r) { return r ? r->footer.num_rows : 0; }
uint64_t orcg_reader_num_stripes(const orcg_reader* r) { return r ? r->footer.stripes.size() : 0; }
uint32_t orcg_reader_row_index_stride(const orcg_reader* r) { return r ? r->footer.row_index_stride : 0; }
uint32_t orcg_reader_compression(const orcg_reader* r) { return r ? r->ps.compression : 0; }
uint64_t orcg_reader_compression_block_size(const orcg_reader* r) { return r ? r->ps.block_size : 0; }
uint32_t orcg_reader_writer_version(const orcg_reader* r) { return r ? r->ps.writer_version : 0; }
uint64_t orcg_reader_content_length(const orcg_reader* r) { return r ? r->footer.content_length : 0; }
const char* orcg_reader_software_version(const orcg_reader* r) {
  if (!r) return "";
  static const char* kNames[] = {"ORC Java", "ORC C++", "Presto", "Scritchley Go", "Trino", "CUDF"};
  auto* rr = const_cast<orcg_reader*>(r);
  const uint32_t id = r->footer.writer;
  rr->software_version = id < 6 ? kNames[id] : "Unknown(" + std::to_string(id) + ")";
  if (r->footer.has_software_version) rr->software_version += " " + r->footer.software_version;
  return rr->software_version.c_str();
}
uint32_t orcg_reader_num_metadata(const orcg_reader* r) { return r ? (uint32_t)r->footer.metadata.size() : 0; }
const char* orcg_reader_metadata_key(const orcg_reader* r, uint32_t i) {
  return r && i < r->footer.metadata.size() ? r->footer.metadata[i].first.c_str() : nullptr;
}
const uint8_t* orcg_reader_metadata_value(const orcg_reader* r, uint32_t i, uint64_t* len) {
  if (!r || i >= r->footer.metadata.size()) return nullptr;
  if (len) *len = r->footer.metadata[i].second.size();
  return (const uint8_t*)r->footer.metadata[i].second.data();
}
int orcg_reader_set_lazy_dictionary(orcg_reader* r, int on) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  r->own.lazy_dict = on != 0;
  return ORCG_OK;
}
int orcg_reader_set_device_decompression(orcg_reader* r, int on) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  r->own.dev_inflate = on != 0;
  return ORCG_OK;
}
int orcg_reader_last_device_inflate(const orcg_reader* r, uint64_t out2[2]) {
  if (!r || !out2) return ORCG_INVALID_ARGUMENT;
  out2[0] = r->last_dev_inflate[0];
  out2[1] = r->last_dev_inflate[1];
  return ORCG_OK;
}
int orcg_reader_set_hive11_decimal(orcg_reader* r, int32_t forced_scale, int throw_on_overflow) {
  if (!r || forced_scale < 0 || forced_scale > 38) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  r->hive11_scale = forced_scale;
  r->hive11_throw = throw_on_overflow != 0;
  return ORCG_OK;
}
int32_t orcg_reader_hive11_scale(const orcg_reader* r) { return r ? r->hive11_scale : 6; }

int orcg_reader_set_read_type(orcg_reader* r, const char* type_string) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  std::shared_ptr<ReadPlan> plan;
  if (type_string && *type_string) {
    plan.reset(new ReadPlan());
    plan->text = type_string;
    std::string err;
    if (!rt::parse_type(plan->text, &plan->tree, &err)) return r->fail_user(ORCG_INVALID_ARGUMENT, err);
    if (!rt::plan_conversion(r->file_tree(), plan->tree, &plan->conv, &err))
      return r->fail_user(ORCG_INVALID_ARGUMENT, err);
  }
  std::lock_guard<std::mutex> lk(r->mu);
  r->own.read = plan;
  return ORCG_OK;
}

int orcg_reader_set_throw_on_schema_evolution_overflow(orcg_reader* r, int on) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  r->own.evo_throw = on != 0;
  return ORCG_OK;
}

int orcg_reader_read_type(const orcg_reader* r, uint32_t id, orcg_type_info* out) {
  if (!r || !out || id >= r->footer.types.size()) return ORCG_INVALID_ARGUMENT;
  const std::shared_ptr<const ReadPlan> plan = r->own.read;
  if (!plan || plan->conv[id] != rt::kConvert) return orcg_reader_type(r, id, out);
  const rt::Node& n = plan->tree[id];
  out->kind = n.kind;
  out->num_subtypes = (uint32_t)n.subtypes.size();
  out->maximum_length = n.maximum_length;
  out->precision = n.precision;
  out->scale = n.scale;
  return ORCG_OK;
}

}  // extern "C"

rt::Tree orcg_reader::file_tree() const {
  rt::Tree t(footer.types.size());
  for (size_t i = 0; i < t.size(); ++i) {
    const TypeInfo& f = footer.types[i];
    t[i].kind = f.kind;
    t[i].maximum_length = f.maximum_length;
    t[i].precision = f.precision;
    t[i].scale = f.scale;
    t[i].subtypes = f.subtypes;
    t[i].field_names = f.field_names;
  }
  return t;
}

extern "C" {

int orcg_reader_set_zone_rules(orcg_reader* r, const char* name, const uint8_t* tzif, uint64_t len) {
  if (!r || !name || !*name || (len && !tzif)) return ORCG_INVALID_ARGUMENT;
  std::unique_ptr<ZoneEntry> e(new ZoneEntry());
  const std::string canon = tz::canonical_name(name);
  try {
    e->zone = tz::Zone::parse(canon, tzif, len);
  } catch (const tz::TimezoneError& x) {
    e->err = x.what();  // raised by the read that needs the zone
  }
  std::lock_guard<std::mutex> lk(r->mu);  // no decode holds the old entry
  std::lock_guard<std::mutex> lz(r->tz_mu);
  std::unique_ptr<ZoneEntry>& slot = r->zones[canon];
  if (slot) r->zones_replaced.push_back(std::move(slot));  // a row reader may still name it
  slot = std::move(e);
  return ORCG_OK;
}

int orcg_reader_set_timezone_name(orcg_reader* r, const char* name) {
  if (!r || !name) return ORCG_INVALID_ARGUMENT;
  const ZoneEntry* z = r->resolve_zone(name);
  if (!z) return r->fail_user(ORCG_INVALID_ARGUMENT, std::string("Time zone ") + name + " not found");
  if (!z->zone) return r->fail_user(ORCG_PARSE_ERROR, z->err);
  std::lock_guard<std::mutex> lk(r->mu);
  r->own.reader_tz = z;
  return ORCG_OK;
}

int orcg_reader_set_local_timezone(orcg_reader* r, const char* name) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  r->own.local_tz = name ? name : "";
  return ORCG_OK;
}
int orcg_reader_format_version(const orcg_reader* r, uint32_t* major, uint32_t* minor) {
  if (!r || !major || !minor) return ORCG_INVALID_ARGUMENT;
  // the reference reports 0.11 when the version is absent (FileVersion::v_0_11)
  *major = r->ps.version.size() > 0 ? r->ps.version[0] : 0;
  *minor = r->ps.version.size() > 1 ? r->ps.version[1] : 11;
  return ORCG_OK;
}
uint32_t orcg_reader_num_types(const orcg_reader* r) { return r ? (uint32_t)r->footer.types.size() : 0; }
int orcg_reader_type(const orcg_reader* r, uint32_t id, orcg_type_info* out) {
  if (!r || !out || id >= r->footer.types.size()) return ORCG_INVALID_ARGUMENT;
  const TypeInfo& t = r->footer.types[id];
  out->kind = t.kind;
  out->num_subtypes = (uint32_t)t.subtypes.size();
  out->maximum_length = t.maximum_length;
  out->precision = t.precision;
  out->scale = t.scale;
  return ORCG_OK;
}
int orcg_reader_subtypes(const orcg_reader* r, uint32_t id, uint32_t* out, uint32_t cap) {
  if (!r || id >= r->footer.types.size() || (cap && !out)) return ORCG_INVALID_ARGUMENT;
  const auto& st = r->footer.types[id].subtypes;
  for (uint32_t i = 0; i < cap && i < st.size(); ++i) out[i] = st[i];
  return ORCG_OK;
}
const char* orcg_reader_field_name(const orcg_reader* r, uint32_t id, uint32_t i) {
  if (!r || id >= r->footer.types.size() || i >= r->footer.types[id].field_names.size()) return nullptr;
  return r->footer.types[id].field_names[i].c_str();
}
int orcg_reader_stripe(const orcg_reader* r, uint64_t s, orcg_stripe_info* out) {
  if (!r || !out || s >= r->footer.stripes.size()) return ORCG_INVALID_ARGUMENT;
  const StripeInfo& si = r->footer.stripes[s];
  out->offset = si.offset;
  out->index_length = si.index_length;
  out->data_length = si.data_length;
  out->footer_length = si.footer_length;
  out->num_rows = si.num_rows;
  return ORCG_OK;
}

int orcg_reader_select(orcg_reader* r, const uint8_t* include, uint32_t ntypes) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  std::vector<uint8_t> sel;
  const int rc = compute_selection(r, include, ntypes, sel);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  r->own.selected.swap(sel);
  return ORCG_OK;
}

int orcg_reader_is_selected(const orcg_reader* r, uint32_t type_id) {
  return r && type_id < r->own.selected.size() && r->own.selected[type_id] ? 1 : 0;
}

int orcg_reader_read_stripe(orcg_reader* r, uint64_t stripe) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  ReaderCallScope call(r);
  std::lock_guard<std::mutex> lk(r->mu);
  orcg_reader::Active scope(r, r->own);
  return r->read_stripes(stripe, 1);
}

int orcg_reader_bench_stripe_decode(orcg_reader* r, uint64_t stripe, uint32_t iters, double* decode_s, double* h2d_s) {
  if (!r || !decode_s || !h2d_s || iters == 0) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  orcg_reader::Active scope(r, r->own);
  if (!r->act.ctx) return r->fail(ORCG_INVALID_ARGUMENT, "reader has no device context");
  if (stripe >= r->footer.stripes.size()) return r->fail(ORCG_INVALID_ARGUMENT, "stripe index out of range");
  hipSetDevice(r->act.ctx->device);
  int rc = r->prepare(stripe, r->stages[0], r->act);
  if (rc) return rc;
  if (r->slots.empty()) r->slots.emplace_back(new DevSlot());
  // one untimed decode (allocations), then `iters` back-to-back decodes of
  // the prepared stripe: the GPU never waits for host decompression
  rc = r->upload_and_decode(r->stages[0], *r->slots[0]);
  for (auto& t : r->timings) t = 0;
  for (uint32_t i = 0; i < iters && !rc; ++i) rc = r->upload_and_decode(r->stages[0], *r->slots[0]);
  r->nslots = rc ? 0 : 1;
  *decode_s = r->timings[4] / iters;
  *h2d_s = r->timings[3] / iters;
  return rc;
}

int orcg_reader_read_stripes(orcg_reader* r, uint64_t first, uint64_t count) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  ReaderCallScope call(r);
  std::lock_guard<std::mutex> lk(r->mu);
  orcg_reader::Active scope(r, r->own);
  return r->read_stripes(first, count);
}

int orcg_reader_stripe_column(const orcg_reader* r, uint64_t k, uint32_t id, orcg_column_view* out) {
  if (!r || !out || id >= r->footer.types.size() || k >= r->nslots) return ORCG_INVALID_ARGUMENT;
  const ColOut& c = r->slots[k]->out[id];
  memset(out, 0, sizeof(*out));
  out->type_id = id;
  out->kind = c.converted ? c.rkind : r->footer.types[id].kind;
  fill_view(c, out);
  return ORCG_OK;
}

int orcg_reader_column(const orcg_reader* r, uint32_t id, orcg_column_view* out) {
  return orcg_reader_stripe_column(r, 0, id, out);
}

int orcg_reader_copy_to_host(orcg_reader* r, void* dst, const void* src, uint64_t bytes) {
  if (!r || !r->own.ctx || (bytes && (!dst || !src))) return ORCG_INVALID_ARGUMENT;
  if (!bytes) return ORCG_OK;
  Ctx* c = r->own.ctx;  // never a row reader worker's context
  int rc = hip_check(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream), "D2H");
  if (!rc) rc = sync_ctx(c);
  return rc;
}

int orcg_reader_last_timings(const orcg_reader* r, double* out5) {
  if (!r || !out5) return ORCG_INVALID_ARGUMENT;
  for (int i = 0; i < 5; ++i) out5[i] = r->timings[i];
  return ORCG_OK;
}

int orcg_reader_last_stream_stats(const orcg_reader* r, uint64_t* out2) {
  if (!r || !out2) return ORCG_INVALID_ARGUMENT;
  out2[0] = r->stream_stats[0];
  out2[1] = r->stream_stats[1];
  return ORCG_OK;
}

uint64_t orcg_reader_last_batched_streams(const orcg_reader* r) { return r ? r->batched_streams : 0; }

int orcg_reader_get_metrics(orcg_reader* r, orcg_reader_metrics* out) {
  if (!r || !out) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  static_assert(sizeof(orcg_reader_metrics) == 14 * sizeof(uint64_t), "orcg_reader_metrics layout");
  uint64_t* o = (uint64_t*)out;
  for (int i = 0; i < 14; ++i) o[i] = r->metrics[i].load(std::memory_order_relaxed);
  return ORCG_OK;
}

int orcg_reader_reset_metrics(orcg_reader* r) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  for (auto& m : r->metrics) m.store(0, std::memory_order_relaxed);
  return ORCG_OK;
}

int orcg_reader_set_metrics_timing(orcg_reader* r, int on) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(r->mu);
  r->metrics_timing = on != 0;
  return ORCG_OK;
}
uint64_t orcg_reader_last_stage_bytes(const orcg_reader* r) { return r ? r->stage_bytes : 0; }

int orcg_reader_set_stream_batching(orcg_reader* r, int on) {
  if (!r) return ORCG_INVALID_ARGUMENT;
  r->batch_on = on != 0;
  return ORCG_OK;
}

}  // extern "C"
