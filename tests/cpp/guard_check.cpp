// guard_check.cpp -- the host half of the guarded allocator (tandem_amd/csrc/guard_host.h) as a stand-alone program:
// tests/test_guard_host.py builds it with g++ under AddressSanitizer + UBSan and runs it.  No device, no HIP header.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../tandem_amd/csrc/guard_host.h"

using namespace dr::guard;

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) { fprintf(stderr, "guard_check: line %d: %s\n", __LINE__, #c); exit(1); } \
  } while (0)

// a heap range that stands for device memory at `addr`: the scan takes the address apart from the copy, as the allocator does
struct Range {
  std::vector<unsigned char> b;
  uintptr_t addr;
  Range(size_t n, uintptr_t a) : b(n), addr(a) { fill(b.data(), n, a); }
  Scan scan_() const { return scan(b.data(), b.size(), addr); }
};

static void pattern() {
  CHECK(kGranule % 4 == 0);
  for (unsigned char c : kPattern) CHECK(c != 0x00 && c != 0xff);
  uint32_t w; memcpy(&w, kPattern, 4);
  CHECK(w == kWord);
  CHECK((w & 0x7f800000u) == 0x7f800000u && (w & 0x00400000u));  // exponent all ones, quiet bit set
  // aligned and unaligned starts: whichever byte the range starts at, every ALIGNED word inside it is the NaN word
  for (uintptr_t start = 0x7f0000001000u; start < 0x7f0000001000u + 8; ++start) {
    Range r(64, start);
    for (size_t i = 0; i < 64; ++i) CHECK(r.b[i] == kPattern[(start + i) & 3]);
    int words = 0;
    for (size_t i = (4 - (start & 3)) & 3; i + 4 <= 64; i += 4, ++words) {
      float f; memcpy(&f, &r.b[i], 4);
      uint32_t u; memcpy(&u, &r.b[i], 4);
      CHECK(std::isnan(f) && u == kWord);
    }
    CHECK(words >= 15);
    CHECK(r.scan_().count == 0);
  }
  fill(nullptr, 0, 3);  // an empty range touches nothing
  CHECK(scan(nullptr, 0, 3).count == 0);
}

static void scans() {
  for (uintptr_t a : {(uintptr_t)0x1000, (uintptr_t)0x1001, (uintptr_t)0x1003}) {
    const size_t n = 4096;
    Range clean(n, a);
    Scan s = clean.scan_();
    CHECK(s.count == 0);
    Range first(n, a); first.b[0] ^= 1;
    s = first.scan_();
    CHECK(s.count == 1 && s.first == 0 && s.last == 0);
    Range last(n, a); last.b[n - 1] = 0;
    s = last.scan_();
    CHECK(s.count == 1 && s.first == n - 1 && s.last == n - 1);
    Range run(n, a);
    for (size_t i = 100; i < 140; ++i) run.b[i] = 0;  // (0x00 is no pattern byte: all forty differ)
    s = run.scan_();
    CHECK(s.count == 40 && s.first == 100 && s.last == 139);
    Range two(n, a); two.b[7] = 0xff; two.b[4000] = 0xff;
    s = two.scan_();
    CHECK(s.count == 2 && s.first == 7 && s.last == 4000);
    // a store of the pattern's own word at an aligned address is invisible -- and only that
    Range same(n, a);
    const size_t al = (4 - (a & 3)) & 3;
    memcpy(&same.b[al + 8], &kWord, 4);
    CHECK(same.scan_().count == 0);
    memcpy(&same.b[al + 9], &kWord, 4);
    CHECK(same.scan_().count > 0);
  }
}

// The back guard starts at the byte behind the payload, also when the payload is no multiple of 4.
static void back_guards() {
  const size_t G = 4096;
  const uintptr_t base = 0x7f0000200000u;
  for (size_t bytes : {(size_t)1000, (size_t)1001, (size_t)1002, (size_t)1003, (size_t)1, (size_t)2, (size_t)3, (size_t)4}) {
    CHECK(total_bytes(bytes, G) == 2 * G + round4(bytes) && total_bytes(bytes, G) % 4 == 0);
    const size_t nb = back_guard_bytes(bytes, G);
    CHECK(nb == G + (4 - bytes % 4) % 4);
    CHECK(G + bytes + nb == total_bytes(bytes, G));
    // the whole allocation as the device holds it after the fill
    Range all(total_bytes(bytes, G), base);
    const uintptr_t user = base + G;
    // a write of payload + 1 bytes: the byte right behind the payload is the guard's offset +0
    std::vector<unsigned char> dev = all.b;
    for (size_t i = 0; i <= bytes; ++i) dev[G + i] = 0;
    Scan s = scan(&dev[G + bytes], nb, user + bytes);
    CHECK(s.count == 1 && s.first == 0 && s.last == 0);
    Violation v = back_violation("buf", bytes, s);
    CHECK(v.side == 1 && v.first == 0 && v.last == 0 && v.count == 1 && v.payload == bytes);
    // the last byte of the allocation
    dev = all.b; dev.back() = 0;
    s = scan(&dev[G + bytes], nb, user + bytes);
    CHECK(s.count == 1 && s.first == nb - 1);
    // a payload written in full and nothing else: both guards clean
    dev = all.b;
    for (size_t i = 0; i < bytes; ++i) dev[G + i] = 0;
    CHECK(scan(&dev[G + bytes], nb, user + bytes).count == 0);
    CHECK(scan(&dev[0], G, base).count == 0);
    // the byte before the payload is the front guard's offset -1, its first byte -G
    dev = all.b; dev[G - 1] = 0; dev[0] = 0;
    s = scan(&dev[0], G, base);
    v = front_violation("buf", bytes, G, s);
    CHECK(v.side == -1 && v.first == -(long long)G && v.last == -1 && v.count == 2);
  }
}

static void reports() {
  Scan a; a.count = 1; a.first = 0; a.last = 0;
  Scan b; b.count = 12; b.first = 4092; b.last = 4095;
  std::vector<Violation> vs = {back_violation("s1.conv11", 1000, a), front_violation("dr_tracker.hip:267", 36864, 4096, b)};
  const std::string want =
      "s1.conv11 (1000 bytes): back guard, 1 byte changed, offsets +0..+0\n"
      "dr_tracker.hip:267 (36864 bytes): front guard, 12 bytes changed, offsets -4..-1\n";
  char big[512];
  memset(big, 'x', sizeof big);
  CHECK(report(vs, big, sizeof big) == want.size());
  CHECK(want == big);
  // truncation: exactly cap - 1 characters and the terminator, nothing behind it
  for (size_t cap : {(size_t)1, (size_t)2, (size_t)40, want.size(), want.size() + 1}) {
    std::vector<char> out(cap + 8, 'x');
    CHECK(report(vs, out.data(), cap) == want.size());
    const size_t n = std::min(cap - 1, want.size());
    CHECK(memcmp(out.data(), want.data(), n) == 0 && out[n] == 0);
    for (size_t i = n + 1; i < out.size(); ++i) CHECK(out[i] == 'x');
  }
  CHECK(report(vs, nullptr, 0) == want.size());  // no buffer: the length only
  char one[4] = {'x', 'x', 'x', 'x'};
  CHECK(report({}, one, 4) == 0 && one[0] == 0 && one[1] == 'x');
}

int main() {
  pattern();
  scans();
  back_guards();
  reports();
  printf("guard_check ok\n");
  return 0;
}
