// edge_network_check.cpp -- the selection network of the edge measure (tandem_amd/csrc/edge_network.h) checked on the host, no HIP, no device.
//
// The zero-one principle: a comparator network puts the k-th smallest of its inputs on a wire for EVERY input iff it does so for every input of
// zeros and ones (a comparator commutes with any monotone map of the values, ties included).  For zero-one inputs min = AND and max = OR, so 64
// inputs go through the network at once as the 64 bits of a word: all 2^25 inputs are 2^19 words.  The 15th smallest of 25 zero-one values is 1
// exactly when at most 14 of them are 0, i.e. when at least 11 are 1.
//
//   edge_network_check              the network as the kernel expands it (the X-macro itself, unrolled) AND the same list walked from a table:
//                                   wire 14 right for all 2^25 inputs, 113 comparators, every comparator (a, b) with 0 <= a < b < 25; then
//                                   the mutated networks below, each of which MUST be found wrong.  Prints "edge_network_check ok".
//   edge_network_check MUTANT       only that mutated network: exit status 1 and the number of inputs it gets wrong -- the checker can fail.
//       drop-last   the last comparator left out
//       swap-pair   one comparator and its successor exchanged in order (they share wire 13)
//       reversed    one comparator with min and max exchanged
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tandem_amd/csrc/edge_network.h"

namespace {

struct Cmp { int a, b; };
#define DR_CE_ROW(A, B) {A, B},
const Cmp kNetwork[] = {DR_EDGE_NETWORK(DR_CE_ROW)};
#undef DR_CE_ROW
#define DR_CE_ONE(A, B) +1
constexpr int kCount = 0 DR_EDGE_NETWORK(DR_CE_ONE);
#undef DR_CE_ONE
static_assert(kCount == DR_EDGE_COMPARATORS, "edge_network.h: DR_EDGE_COMPARATORS is not the length of the list");
static_assert(sizeof kNetwork / sizeof kNetwork[0] == (size_t)kCount, "table and count disagree");

constexpr int N = DR_EDGE_INPUTS, WIRE = DR_EDGE_WIRE, LOW = 6;  // input bit i < 6 comes from the lane number, bit i >= 6 from the word number
constexpr uint64_t kLane[LOW] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull, 0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};

inline void load(uint64_t (&v)[N], uint32_t word) {
  for (int i = 0; i < LOW; ++i) v[i] = kLane[i];
  for (int i = LOW; i < N; ++i) v[i] = ((word >> (i - LOW)) & 1u) ? ~0ull : 0ull;
}

// lanes of a word whose own six bits hold at least t ones, t = 0 .. 7
void lane_tables(uint64_t (&at_least)[LOW + 2]) {
  for (int t = 0; t <= LOW + 1; ++t) {
    at_least[t] = 0;
    for (int lane = 0; lane < 64; ++lane)
      if (__builtin_popcount((unsigned)lane) >= t) at_least[t] |= 1ull << lane;
  }
}

inline uint64_t expected(const uint64_t (&at_least)[LOW + 2], uint32_t word) {
  const int need = (N - WIRE) - __builtin_popcount(word);  // ones still needed from the lane's six bits: 11 - (ones of the word number)
  return need <= 0 ? ~0ull : (need > LOW ? 0ull : at_least[need]);
}

// the macro as edge_pixel expands it, with AND / OR for fminf / fmaxf
inline uint64_t run_macro(uint32_t word) {
  uint64_t v[N];
  load(v, word);
#define CE(A, B) { const uint64_t lo_ = v[A] & v[B], hi_ = v[A] | v[B]; v[A] = lo_; v[B] = hi_; }
  DR_EDGE_NETWORK(CE)
#undef CE
  return v[WIRE];
}

struct Net { std::vector<Cmp> c; std::vector<char> reversed; };
inline uint64_t run_table(const Net &n, uint32_t word) {
  uint64_t v[N];
  load(v, word);
  for (size_t i = 0; i < n.c.size(); ++i) {
    const uint64_t lo = v[n.c[i].a] & v[n.c[i].b], hi = v[n.c[i].a] | v[n.c[i].b];
    v[n.c[i].a] = n.reversed[i] ? hi : lo;
    v[n.c[i].b] = n.reversed[i] ? lo : hi;
  }
  return v[WIRE];
}

template <class F>
uint64_t wrong_inputs(F &&wire) {
  uint64_t at_least[LOW + 2];
  lane_tables(at_least);
  uint64_t wrong = 0;
  for (uint32_t word = 0; word < (1u << (N - LOW)); ++word) wrong += (uint64_t)__builtin_popcountll(wire(word) ^ expected(at_least, word));
  return wrong;
}

Net network() {
  Net n;
  n.c.assign(kNetwork, kNetwork + kCount);
  n.reversed.assign(kCount, 0);
  return n;
}
Net mutant(const char *name) {
  Net n = network();
  if (!strcmp(name, "drop-last")) { n.c.pop_back(); n.reversed.pop_back(); }
  else if (!strcmp(name, "swap-pair")) std::swap(n.c[kCount - 2], n.c[kCount - 1]);  // CE(13,16) CE(13,14) -> CE(13,14) CE(13,16)
  else if (!strcmp(name, "reversed")) n.reversed[kCount / 2] = 1;
  else n.c.clear();
  return n;
}
const char *const kMutants[] = {"drop-last", "swap-pair", "reversed"};

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1) {
    const Net n = mutant(argv[1]);
    if (n.c.empty()) { fprintf(stderr, "unknown mutant %s\n", argv[1]); return 2; }
    const uint64_t wrong = wrong_inputs([&](uint32_t w) { return run_table(n, w); });
    printf("%s: %llu of %llu inputs wrong\n", argv[1], (unsigned long long)wrong, 1ull << N);
    return wrong ? 1 : 0;
  }
  int bad = 0;
  for (int i = 0; i < kCount; ++i)
    if (!(0 <= kNetwork[i].a && kNetwork[i].a < kNetwork[i].b && kNetwork[i].b < N)) { printf("comparator %d: (%d, %d) is not 0 <= a < b < %d\n", i, kNetwork[i].a, kNetwork[i].b, N); ++bad; }
  printf("%d comparators\n", kCount);
  if (kCount != 113) { printf("expected 113 comparators\n"); ++bad; }
  const uint64_t wm = wrong_inputs(run_macro);
  printf("macro: %llu of %llu inputs wrong\n", (unsigned long long)wm, 1ull << N);
  const Net n = network();
  const uint64_t wt = wrong_inputs([&](uint32_t w) { return run_table(n, w); });
  printf("table: %llu of %llu inputs wrong\n", (unsigned long long)wt, 1ull << N);
  bad += (wm != 0) + (wt != 0);
  for (const char *m : kMutants) {
    const Net mn = mutant(m);
    const uint64_t w = wrong_inputs([&](uint32_t x) { return run_table(mn, x); });
    printf("%s: %llu of %llu inputs wrong\n", m, (unsigned long long)w, 1ull << N);
    if (!w) { printf("the mutated network %s passes: the check cannot fail\n", m); ++bad; }
  }
  if (bad) return 1;
  printf("edge_network_check ok\n");
  return 0;
}
