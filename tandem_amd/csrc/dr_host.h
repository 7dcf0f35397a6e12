// dr_host.h -- the part of dr_common.h that needs no HIP header: error plumbing, cdiv, hook_env.  Plain C++17: the host halves
// (mvs_host.h) include only this one, so g++ compiles them alone for the CPU tests.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dr_mi355x.h"

namespace dr {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

std::string &last_error_slot();

[[noreturn]] inline void fail(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  throw Error(code, buf);
}

// Wraps a C-ABI body: exceptions -> status code + dr_last_error().
template <class F>
inline int guarded(F &&f) {
  try {
    last_error_slot().clear();
    f();
    return DR_OK;
  } catch (const Error &e) {
    last_error_slot() = e.what();
    return e.code;
  } catch (const std::exception &e) {
    last_error_slot() = e.what();
    return DR_ERR_DEVICE;
  }
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// A DR_* switch that selects a superseded kernel generation or the losing side of a settled A/B exists only in the PARITY build
// (-DDR_PARITY_HOOKS, libdr_mi355x_hooks.so: test infrastructure).  In the product library hook_env() is a constant: the variable is not read, the
// branch behind it folds away.  What the product library does read from the environment is listed in INTEGRATION.md ("Environment switches").
#ifdef DR_PARITY_HOOKS
inline const char *hook_env(const char *name) { return getenv(name); }
#else
inline const char *hook_env(const char *) { return nullptr; }
#endif

}  // namespace dr
