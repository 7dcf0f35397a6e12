// dr_common.h -- shared host-side helpers of libdr_mi355x.so: dr_host.h (error plumbing, no HIP) + the HIP checks.
#pragma once
#include <hip/hip_runtime.h>

#include "dr_host.h"

namespace dr {

#define DR_HIP(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      ::dr::fail(DR_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

template <class T>
inline T *dalloc(size_t n) {
  void *p = nullptr;
  DR_HIP(hipMalloc(&p, n * sizeof(T) > 0 ? n * sizeof(T) : 16));
  return reinterpret_cast<T *>(p);
}

}  // namespace dr
