// dr_common.h -- shared host-side helpers of libdr_mi355x.so: dr_host.h (error plumbing, no HIP) + the HIP checks + the one
// device allocator (dalloc / dfree; device_alloc / device_free are their non-throwing forms).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dr_host.h"
#include "guard_host.h"

#ifdef DR_PARITY_HOOKS
#include <map>
#include <mutex>
#endif

namespace dr {

#define DR_HIP(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      ::dr::fail(DR_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

#ifdef DR_PARITY_HOOKS
// The parity build's allocator can put a guard band on either side of every allocation and poison all of it (guard_host.h has the
// layout and the pattern).  Off (the default, guard_bytes == 0) it is the single hipMalloc / hipFree of the product library.  One
// registry per library: the three engines' translation units share it.
namespace guard {

struct Entry {
  size_t bytes = 0, G = 0;
  std::string label;
};
struct Registry {
  std::mutex mu;
  std::map<void *, Entry> live;    // keyed by the pointer handed out
  std::vector<Violation> sticky;   // found when a buffer was freed; kept until clear()
  size_t guard_bytes = 0;          // of later allocations; 0: guards off
  uint64_t since_clear = 0;        // buffers guarded since the last clear()
};
inline Registry &registry() {
  static Registry *r = new Registry;  // never destroyed: engines may be released after the library's statics
  return *r;
}

// both guards of one buffer copied back and compared; the caller holds the lock and has synchronised the device
inline void scan_entry(void *p, const Entry &e, std::vector<Violation> &into) {
  unsigned char *user = (unsigned char *)p;
  const size_t nb = back_guard_bytes(e.bytes, e.G);
  std::vector<unsigned char> h(std::max(e.G, nb));
  if (hipMemcpy(h.data(), user - e.G, e.G, hipMemcpyDeviceToHost) == hipSuccess) {
    const Scan s = scan(h.data(), e.G, (uintptr_t)(user - e.G));
    if (s.count) into.push_back(front_violation(e.label, e.bytes, e.G, s));
  }
  if (hipMemcpy(h.data(), user + e.bytes, nb, hipMemcpyDeviceToHost) == hipSuccess) {
    const Scan s = scan(h.data(), nb, (uintptr_t)(user + e.bytes));
    if (s.count) into.push_back(back_violation(e.label, e.bytes, s));
  }
}

}  // namespace guard

inline hipError_t device_alloc(void **p, size_t bytes, const char *label = nullptr, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
  guard::Registry &r = guard::registry();
  std::lock_guard<std::mutex> lk(r.mu);
  const size_t G = r.guard_bytes;
  if (!G) return hipMalloc(p, bytes);
  void *base = nullptr;
  const size_t total = guard::total_bytes(bytes, G);
  hipError_t e = hipMalloc(&base, total);
  if (e != hipSuccess) return e;
  // hipMalloc returns word-aligned memory, so the address-defined pattern is the same word throughout
  e = hipMemsetD32((hipDeviceptr_t)base, (int)guard::kWord, total / 4);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // the engines' streams do not wait for the null stream
  if (e != hipSuccess) { (void)hipFree(base); return e; }
  guard::Entry en;
  en.bytes = bytes; en.G = G;
  if (label && *label) en.label = label;
  else {
    const char *s = strrchr(file, '/');
    en.label = std::string(s ? s + 1 : file) + ":" + std::to_string(line);
  }
  *p = (unsigned char *)base + G;
  r.live[*p] = en;
  ++r.since_clear;
  return hipSuccess;
}
// Frees what device_alloc returned.  A guarded buffer is checked first: the device is synchronised, both guards are copied back
// and what differs from the pattern goes to the sticky list (dr_guard_check reports it).
inline hipError_t device_free(void *p) {
  if (!p) return hipSuccess;
  guard::Registry &r = guard::registry();
  std::lock_guard<std::mutex> lk(r.mu);
  auto it = r.live.find(p);
  if (it == r.live.end()) return hipFree(p);
  (void)hipDeviceSynchronize();
  guard::scan_entry(p, it->second, r.sticky);
  void *base = (unsigned char *)p - it->second.G;
  r.live.erase(it);
  return hipFree(base);
}
#else
inline hipError_t device_alloc(void **p, size_t bytes, const char * = nullptr) { return hipMalloc(p, bytes); }
inline hipError_t device_free(void *p) { return hipFree(p); }
#endif

#ifdef DR_PARITY_HOOKS
template <class T>
inline T *dalloc(size_t n, const char *label = nullptr, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
  void *p = nullptr;
  DR_HIP(device_alloc(&p, n * sizeof(T) > 0 ? n * sizeof(T) : 16, label, file, line));
  return reinterpret_cast<T *>(p);
}
#else
template <class T>
inline T *dalloc(size_t n, const char * = nullptr, const char * = nullptr, int = 0) {  // (label, file and line name the buffer for the parity build's guards only)
  void *p = nullptr;
  DR_HIP(hipMalloc(&p, n * sizeof(T) > 0 ? n * sizeof(T) : 16));
  return reinterpret_cast<T *>(p);
}
#endif
// the matching release; never throws (destructors call it)
inline void dfree(void *p) { (void)device_free(p); }

}  // namespace dr
