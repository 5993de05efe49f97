// liborcgpu contexts: life cycle and warm-up, error plumbing, device scratch,
// side lanes and the stream sync that folds the device error record into a
// status.
#include <stdio.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "orcg_internal.hh"

namespace orcg {

int set_error(Ctx* ctx, int status, const std::string& msg) {
  if (ctx) ctx->last_error = msg;
  return status;
}

int hip_check(Ctx* ctx, hipError_t e, const char* what) {
  if (e == hipSuccess) return ORCG_OK;
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  return set_error(ctx, e == hipErrorOutOfMemory ? ORCG_OUT_OF_MEMORY : ORCG_DEVICE_ERROR, m);
}

int scratch(Ctx* ctx, ScratchSlot slot, size_t bytes, void** out) {
  if (bytes == 0) bytes = 16;
  if (ctx->scratch_cap[slot] < bytes) {
    if (ctx->d_scratch[slot]) {
      hipStreamSynchronize(ctx->stream);
      hipFree(ctx->d_scratch[slot]);
      ctx->d_scratch[slot] = nullptr;
      ctx->scratch_cap[slot] = 0;
    }
    size_t cap = std::max(bytes, (size_t)1 << 20);
    int rc = hip_check(ctx, hipMalloc(&ctx->d_scratch[slot], cap), "hipMalloc scratch");
    if (rc) return rc;
    ctx->scratch_cap[slot] = cap;
  }
  *out = ctx->d_scratch[slot];
  return ORCG_OK;
}

// ORCG_DEBUG: comma-separated topics (alloc, stale, rowreader, defer, jobs)
// whose diagnostics go to stderr
bool debug_on(const char* topic) {
  static const std::string topics = [] {
    const char* e = getenv("ORCG_DEBUG");
    return std::string(",") + (e ? e : "") + ",";
  }();
  return topics.find(std::string(",") + topic + ",") != std::string::npos;
}

void debug_stale(const char* where) {
  if (!debug_on("stale")) return;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) fprintf(stderr, "orcg: pending HIP error at %s: %s\n", where, hipGetErrorString(e));
}

unsigned side_lanes() {
  static const unsigned n = [] {
    const char* e = getenv("ORCG_LANES");
    const int v = e ? atoi(e) : 4;
    return (unsigned)std::max(1, std::min(v, 16));
  }();
  return n;
}

Ctx* ctx_lane(Ctx* base, size_t k) {
  if (!base->ev_fork && hipEventCreateWithFlags(&base->ev_fork, hipEventDisableTiming) != hipSuccess) {
    base->ev_fork = nullptr;
    return nullptr;
  }
  while (base->lanes.size() <= k) {
    orcg_ctx* l = nullptr;
    hipEvent_t e = nullptr;
    if (orcg_ctx_create(base->device, &l) != ORCG_OK) return nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      orcg_ctx_destroy(l);
      return nullptr;
    }
    base->lanes.push_back(l);
    base->ev_join.push_back(e);
  }
  Ctx* l = base->lanes[k];
  l->rlev2_variant = base->rlev2_variant;
  if (!l->num_cus) l->num_cus = base->num_cus;
  return l;
}

int LaneFork::begin() {
  if (!base->ev_fork && !ctx_lane(base, 0)) return set_error(base, ORCG_DEVICE_ERROR, "side stream creation failed");
  return hip_check(base, hipEventRecord(base->ev_fork, base->stream), "fork event");
}

int LaneFork::lane(size_t k, Ctx** out) {
  Ctx* const l = ctx_lane(base, k);
  if (!l) return set_error(base, ORCG_DEVICE_ERROR, "side stream creation failed");
  *out = l;
  if (used.size() < base->lanes.size()) used.resize(base->lanes.size(), 0);
  if (used[k]) return ORCG_OK;
  used[k] = 1;
  return hip_check(base, hipStreamWaitEvent(l->stream, base->ev_fork, 0), "fork wait");
}

int LaneFork::chain(size_t from, size_t to) {
  int rc = hip_check(base, hipEventRecord(base->ev_join[from], base->lanes[from]->stream), "fork event");
  if (!rc) rc = hip_check(base, hipStreamWaitEvent(base->lanes[to]->stream, base->ev_join[from], 0), "fork wait");
  if (used.size() < base->lanes.size()) used.resize(base->lanes.size(), 0);
  if (!rc) used[to] = 1;
  return rc;
}

int LaneFork::join() {
  int rc = ORCG_OK;
  for (size_t k = 0; k < used.size(); ++k) {
    if (!used[k]) continue;
    int jr = hip_check(base, hipEventRecord(base->ev_join[k], base->lanes[k]->stream), "join event");
    if (!jr) jr = hip_check(base, hipStreamWaitEvent(base->stream, base->ev_join[k], 0), "join wait");
    if (jr && !rc) rc = jr;
  }
  used.clear();
  return rc;
}
}  // namespace orcg

using namespace orcg;

extern "C" {

const char* orcg_version(void) { return "orcg 0.1.0 (gfx950)"; }

int orcg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int orcg_ctx_create(int device, orcg_ctx** out) {
  if (!out) return ORCG_INVALID_ARGUMENT;
  *out = nullptr;
  int n = orcg_device_count();
  if (device < 0 || device >= n) return ORCG_DEVICE_ERROR;
  auto* c = new orcg_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&c->d_err, sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(c->d_err, 0xff, sizeof(unsigned long long)) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    delete c;
    return ORCG_DEVICE_ERROR;
  }
  c->stream = c->own_stream;
  // the process's first context on a device loads every kernel file's code
  // object now (orcg_internal.hh warm_*)
  static std::mutex warm_mu;
  static std::vector<int> warmed;
  static const bool warm = [] {
    const char* e = getenv("ORCG_WARMUP");
    return !e || atoi(e) != 0;
  }();
  if (warm) {
    std::lock_guard<std::mutex> lk(warm_mu);
    if (std::find(warmed.begin(), warmed.end(), device) == warmed.end()) {
      orcg::warm_rlev2_walk(c->stream);
      orcg::warm_rlev2_tiled(c->stream);
      orcg::warm_rlev2_expand(c->stream);
      orcg::warm_byterle(c->stream);
      orcg::warm_columns(c->stream);
      orcg::warm_rlev1(c->stream);
      orcg::warm_decimal(c->stream);
      // and the copy paths: the process's first host <-> device copies cost
      // ~10-100 ms of runtime setup (scripts/probes/pin_first_dma.py: a
      // fresh pinned buffer copies at full rate afterwards)
      void* h = nullptr;
      void* dv = nullptr;
      if (hipHostMalloc(&h, 4096, hipHostMallocDefault) == hipSuccess && hipMalloc(&dv, 4096) == hipSuccess) {
        (void)hipMemcpyAsync(dv, h, 4096, hipMemcpyHostToDevice, c->stream);
        (void)hipMemcpyAsync(h, dv, 4096, hipMemcpyDeviceToHost, c->stream);
        (void)hipStreamSynchronize(c->stream);
      }
      (void)hipGetLastError();
      if (dv) (void)hipFree(dv);
      if (h) (void)hipHostFree(h);
      // large copies take the DMA engines (small ones a blit kernel): one
      // each way from registered pinned memory (ORCG_WARMUP_MB, default 16)
      static const size_t big = [] {
        const char* e = getenv("ORCG_WARMUP_MB");
        return (size_t)(e ? std::max(0, atoi(e)) : 16) << 20;
      }();
      void* hb = big ? pinned_alloc(big) : nullptr;
      void* db = nullptr;
      if (hb && hipMalloc(&db, big) == hipSuccess) {
        (void)hipMemcpyAsync(db, hb, big, hipMemcpyHostToDevice, c->stream);
        (void)hipMemcpyAsync(hb, db, big, hipMemcpyDeviceToHost, c->stream);
        (void)hipStreamSynchronize(c->stream);
      }
      (void)hipGetLastError();
      if (db) (void)hipFree(db);
      if (hb) pinned_free(hb);
      if (hipStreamSynchronize(c->stream) != hipSuccess) {
        (void)hipGetLastError();
        orcg_ctx_destroy(c);
        return ORCG_DEVICE_ERROR;
      }
      // only a warm-up that completed marks the device (a failed one is
      // retried by the next context)
      warmed.push_back(device);
    }
  }
  *out = c;
  return ORCG_OK;
}

void orcg_ctx_destroy(orcg_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  for (Ctx* l : c->lanes) orcg_ctx_destroy(static_cast<orcg_ctx*>(l));
  if (c->ev_fork) hipEventDestroy(c->ev_fork);
  for (hipEvent_t e : c->ev_join)
    if (e) hipEventDestroy(e);
  if (c->stream) hipStreamSynchronize(c->stream);
  for (int i = 0; i < kScratchSlots; ++i)
    if (c->d_scratch[i]) hipFree(c->d_scratch[i]);
  if (c->d_err) hipFree(c->d_err);
  if (c->d_defer) hipFree(c->d_defer);
  if (c->d_lb) hipFree(c->d_lb);
  if (c->d_rtab) hipFree(c->d_rtab);
  if (c->d_rhdr) hipFree(c->d_rhdr);
  if (c->d_jobs) hipFree(c->d_jobs);
  if (c->h_jobs) hipHostFree(c->h_jobs);
  if (c->own_stream) hipStreamDestroy(c->own_stream);
  delete c;
}

int orcg_ctx_set_stream(orcg_ctx* c, void* s) {
  if (!c) return ORCG_INVALID_ARGUMENT;
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return ORCG_OK;
}

int orcg_rlev2_variants(int* out, int cap) {
  int n = 0;
  for (int v = 0; v <= kMaxRlev2Variant; ++v)
    if (rlev2_variant_valid(v)) {
      if (out && n < cap) out[n] = v;
      ++n;
    }
  return n;
}

int orcg_ctx_set_rlev2_variant(orcg_ctx* c, int v) {
  // 0 tiled (default), 1 wave-walk; the others pin one tiled instance
  // (rlev2_route.hh: the ids and rlev2_variant_valid)
  if (!c || !rlev2_variant_valid(v)) return ORCG_INVALID_ARGUMENT;
  c->rlev2_variant = v;
  return ORCG_OK;
}

void* orcg_ctx_stream(orcg_ctx* c) { return c ? (void*)c->stream : nullptr; }

const char* orcg_ctx_last_error(const orcg_ctx* c) { return c ? c->last_error.c_str() : ""; }

uint64_t orcg_ctx_last_error_value(const orcg_ctx* c) { return c ? c->last_error_value : 0; }

int orcg_ctx_synchronize(orcg_ctx* c) { return c ? sync_ctx(c) : ORCG_INVALID_ARGUMENT; }

}  // extern "C"

namespace orcg {
int sync_ctx(Ctx* c) {
  (void)hipSetDevice(c->device);
  int rc = hip_check(c, hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  if (rc) return rc;
  unsigned long long rec = kNoError;
  rc = hip_check(c, hipMemcpy(&rec, c->d_err, sizeof rec, hipMemcpyDeviceToHost), "read error record");
  if (rc) return rc;
  if (rec == kNoError) return ORCG_OK;
  const uint32_t code = (uint32_t)(rec & 0xff);
  c->last_error_value = rec >> 8;
  hipMemset(c->d_err, 0xff, sizeof rec);
  return set_error(c, dev_error_status(code), dev_error_message(code));
}
}  // namespace orcg
