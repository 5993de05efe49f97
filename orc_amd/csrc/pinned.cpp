// Page-locked host memory (pinned_alloc / pinned_free) and its C ABI.
#include <linux/mempolicy.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "orcg_internal.hh"

namespace orcg {

// Page-locked host memory. Large buffers (the reader's staging, the row
// reader's slabs) are anonymous mappings advised to transparent huge pages,
// faulted in by several threads and then registered with HIP: measured on the
// MI355X hosts (scripts/probes/pin_probe.cpp), 256 MB costs ~15 ms to fault +
// 0.5 ms to register this way against ~48 ms for hipHostMalloc (4 KB pages
// pinned one by one), at the same D2H rate (57 GB/s). Small buffers, or a
// failed registration, use hipHostMalloc.
namespace {
std::mutex g_pin_mu;
std::unordered_map<void*, size_t> g_pin_maps;  // registered mappings -> length
constexpr size_t kHuge = size_t(2) << 20;
}  // namespace

int current_numa_node() {
  unsigned cpu = 0, node = 0;
  return getcpu(&cpu, &node) == 0 ? (int)node : -1;
}

void* pinned_alloc(size_t bytes, int node) {
  if (bytes == 0) bytes = 1;
  if (bytes >= (size_t(8) << 20)) {
    const size_t len = (bytes + kHuge - 1) & ~(kHuge - 1);
    void* m = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m != MAP_FAILED) {
      (void)madvise(m, len, MADV_HUGEPAGE);
      if (node >= 0 && node < 64) {  // before the faults below place the pages
        const unsigned long mask = 1ul << node;
        (void)syscall(SYS_mbind, m, len, MPOL_PREFERRED, &mask, 64ul, 0u);
      }
      // fault the pages in on a few threads (one write per 4 KB page: a huge
      // page faults whole on its first write, a small one each)
      const size_t pages = len >> 12;
      const unsigned nt = (unsigned)std::min<size_t>(8, std::max<size_t>(1, len / (size_t(32) << 20)));
      std::vector<std::thread> ts;
      for (unsigned t = 0; t < nt; ++t)
        ts.emplace_back([=] {
          volatile char* b = (volatile char*)m;
          for (size_t pg = pages * t / nt; pg < pages * (t + 1) / nt; ++pg) b[pg << 12] = 0;
        });
      for (auto& th : ts) th.join();
      if (hipHostRegister(m, len, hipHostRegisterDefault) == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        g_pin_maps[m] = len;
        return m;
      }
      (void)hipGetLastError();
      munmap(m, len);
    }
  }
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

void pinned_free(void* p) {
  if (!p) return;
  size_t len = 0;
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    auto it = g_pin_maps.find(p);
    if (it != g_pin_maps.end()) {
      len = it->second;
      g_pin_maps.erase(it);
    }
  }
  if (len) {
    (void)hipHostUnregister(p);
    munmap(p, len);
  } else {
    (void)hipHostFree(p);
  }
}

}  // namespace orcg

extern "C" {

int orcg_host_register(void* p, uint64_t bytes) {
  if (!p || !bytes) return ORCG_INVALID_ARGUMENT;
  return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? ORCG_OK : ORCG_DEVICE_ERROR;
}

int orcg_host_unregister(void* p) {
  if (!p) return ORCG_INVALID_ARGUMENT;
  return hipHostUnregister(p) == hipSuccess ? ORCG_OK : ORCG_DEVICE_ERROR;
}

void* orcg_host_alloc(uint64_t bytes) { return orcg::pinned_alloc(bytes); }

void orcg_host_free(void* p) { orcg::pinned_free(p); }

}  // extern "C"
