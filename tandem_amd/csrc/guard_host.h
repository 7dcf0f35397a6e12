// guard_host.h -- the host half of the guarded device allocator of the parity build (dr_common.h: dalloc / dfree): the poison
// pattern, the scan of a guard that was copied back, the violation record and the report text.  Plain C++17, no HIP header, so
// g++ compiles it alone for the CPU tests (tests/cpp/guard_check.cpp).
//
// Layout of a guarded allocation of `bytes`:   base | G front guard | payload, rounded up to 4 | G back guard |
// The pointer handed out is base + G.  The back guard starts at the byte right behind the payload (base + G + bytes), so for a
// payload that is no multiple of 4 it is up to 3 bytes longer than G.  Everything -- both guards and the payload -- starts as the
// pattern, which is defined by ABSOLUTE address: the byte at address a is kPattern[a & 3].  Every aligned 32-bit word then reads
// 0x7fc5a5a5, a quiet NaN (exponent all ones, top mantissa bit set), and no byte is 0x00 or 0xff: a float read from a guard or from
// a payload element nobody wrote propagates as NaN, and a never-initialised u8 / integer buffer is not zero.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace dr {
namespace guard {

constexpr unsigned char kPattern[4] = {0xa5, 0xa5, 0xc5, 0x7f};  // little-endian bytes of kWord
constexpr uint32_t kWord = 0x7fc5a5a5u;                          // what every aligned word of poisoned memory reads
constexpr size_t kGranule = 4096;                                // a guard size is a multiple of this

inline unsigned char pattern_byte(uintptr_t addr) { return kPattern[addr & 3]; }
inline size_t round4(size_t bytes) { return (bytes + 3) & ~(size_t)3; }
// the whole allocation / the back guard (from the byte behind the payload to the end of the allocation)
inline size_t total_bytes(size_t bytes, size_t G) { return G + round4(bytes) + G; }
inline size_t back_guard_bytes(size_t bytes, size_t G) { return round4(bytes) - bytes + G; }

// n bytes of pattern into dst, which stands for the device (or host) address addr
inline void fill(unsigned char *dst, size_t n, uintptr_t addr) {
  for (size_t i = 0; i < n; ++i) dst[i] = pattern_byte(addr + i);
}

struct Scan {
  size_t count = 0, first = 0, last = 0;  // bytes that differ from the pattern; offsets of the first and last of them in the range
};
// buf: n bytes copied back from address addr
inline Scan scan(const unsigned char *buf, size_t n, uintptr_t addr) {
  Scan s;
  for (size_t i = 0; i < n; ++i) {
    if (buf[i] == pattern_byte(addr + i)) continue;
    if (!s.count) s.first = i;
    s.last = i;
    ++s.count;
  }
  return s;
}

struct Violation {
  std::string label;     // tensor name where the allocation knows one, else file:line
  size_t payload = 0;    // bytes requested
  int side = 0;          // -1: front guard (before the payload), +1: back guard (behind it)
  long long first = 0, last = 0;  // relative to the payload edge: front -G .. -1 (-1 = the byte before the payload), back +0 .. (+0 = the byte behind it)
  size_t count = 0;      // bytes that differ
};
// the record of a front-guard scan (range = the G bytes before the payload) / a back-guard scan (range starts behind the payload)
inline Violation front_violation(const std::string &label, size_t payload, size_t G, const Scan &s) {
  Violation v; v.label = label; v.payload = payload; v.side = -1; v.count = s.count;
  v.first = (long long)s.first - (long long)G; v.last = (long long)s.last - (long long)G;
  return v;
}
inline Violation back_violation(const std::string &label, size_t payload, const Scan &s) {
  Violation v; v.label = label; v.payload = payload; v.side = +1; v.count = s.count;
  v.first = (long long)s.first; v.last = (long long)s.last;
  return v;
}

inline std::string describe(const Violation &v) {
  char buf[512];
  snprintf(buf, sizeof buf, "%s (%zu bytes): %s guard, %zu byte%s changed, offsets %+lld..%+lld\n", v.label.c_str(), v.payload,
           v.side < 0 ? "front" : "back", v.count, v.count == 1 ? "" : "s", v.first, v.last);
  return buf;
}
// One line per record into out (cap bytes, always NUL-terminated when cap > 0); returns the length of the whole text, which may
// exceed what fitted.
inline size_t report(const std::vector<Violation> &vs, char *out, size_t cap) {
  std::string all;
  for (const Violation &v : vs) all += describe(v);
  if (out && cap) {
    const size_t n = all.size() < cap - 1 ? all.size() : cap - 1;
    memcpy(out, all.data(), n);
    out[n] = 0;
  }
  return all.size();
}

}  // namespace guard
}  // namespace dr
