// mvs_engine_host_check.cpp -- the DrMvsnet engine's decisions that need no device (tandem_amd/csrc/mvs_engine_host.h: WindowTicket,
// ResultSlots, ForwardCursor, FlagScope, span_holds) as a stand-alone program: plain g++, no HIP.  tests/test_mvs_engine_host.py builds
// it with -Wall -Werror -pthread, and once more with -fsanitize=address,undefined, and runs it.  Every check is a CHECK(): a failed one
// prints its line and the program exits 1.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../tandem_amd/csrc/mvs_engine_host.h"

using dr::FlagScope;
using dr::ForwardCursor;
using dr::ForwardRange;
using dr::ResultSlots;
using dr::WindowTicket;

namespace dr { std::string &last_error_slot() { static std::string s; return s; } }

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "mvs_engine_host_check.cpp:%d: CHECK(%s) failed\n", __LINE__, #c); } } while (0)

// ------------------------------------------------------------------ WindowTicket
static int in_flight(int dev) { return dr::windows_in_flight(dev).load(); }

static void ticket_cases() {
  const int dev = 3;
  CHECK(in_flight(dev) == 0);
  {
    WindowTicket a(dev);
    CHECK(in_flight(dev) == 1 && (bool)a);
    WindowTicket b(std::move(a));  // a move counts nothing, and the moved-from ticket holds nothing
    CHECK(in_flight(dev) == 1 && !(bool)a && (bool)b);
    WindowTicket c(dev);
    CHECK(in_flight(dev) == 2);
    c = std::move(b);  // move-assignment releases what the target held
    CHECK(in_flight(dev) == 1 && !(bool)b && (bool)c);
    WindowTicket &self = c;
    c = std::move(self);  // onto itself: nothing
    CHECK(in_flight(dev) == 1 && (bool)c);
    WindowTicket none;
    CHECK(!(bool)none);
    none = WindowTicket();
    c = std::move(none);  // an empty ticket assigned: the count is released now, not twice later
    CHECK(in_flight(dev) == 0 && !(bool)c);
  }
  CHECK(in_flight(dev) == 0);
  // destruction during stack unwinding
  try {
    WindowTicket a(dev), b(dev);
    WindowTicket c(std::move(a));
    CHECK(in_flight(dev) == 2);
    throw std::runtime_error("unwind");
  } catch (const std::exception &) {}
  CHECK(in_flight(dev) == 0);
  // devices 16 and above share the table with device & 15 (the table stays as it was)
  { WindowTicket a(19); CHECK(in_flight(3) == 1); }
  CHECK(in_flight(3) == 0);
  // the holder: a ticket parked by one thread and taken by another releases once
  {
    WindowTicket parked;
    std::thread t([&] { parked = WindowTicket(dev); });
    t.join();
    CHECK(in_flight(dev) == 1 && (bool)parked);
    std::thread u([&] {
      WindowTicket mine = WindowTicket::take(parked, dev);
      CHECK(in_flight(dev) == 1 && (bool)mine);
    });
    u.join();
    CHECK(in_flight(dev) == 0 && !(bool)parked);
  }
  CHECK(in_flight(dev) == 0);
  // taking from an empty holder acquires exactly one
  {
    WindowTicket parked;
    WindowTicket mine = WindowTicket::take(parked, dev);
    CHECK(in_flight(dev) == 1 && (bool)mine && !(bool)parked);
  }
  CHECK(in_flight(dev) == 0);
  // the worker's error path: the parked ticket is taken before anything throws, so the count does not leak and nothing stays parked
  {
    WindowTicket parked(dev);
    try {
      WindowTicket mine = WindowTicket::take(parked, dev);
      throw std::runtime_error("hipSetDevice");
    } catch (const std::exception &) {}
    CHECK(in_flight(dev) == 0 && !(bool)parked);
  }
}

// ------------------------------------------------------------------ ResultSlots
static const char *kTwice = "Output should be valid. Maybe you called GetResult more than once?";
// what take() answers: the block, -1 = the protocol error with its text, -2 = the worker's error
static int take(ResultSlots &s, const char *worker_text = "") {
  try {
    return s.take();
  } catch (const dr::Error &e) {
    if (e.code == DR_ERR_PROTOCOL) { CHECK(std::string(e.what()) == kTwice); return -1; }
    CHECK(e.code == DR_ERR_DEVICE && std::string(e.what()) == worker_text);
    return -2;
  }
}
static void slots_cases() {
  {  // the legal cycle; the blocks alternate
    ResultSlots s;
    CHECK(!s.unprocessed());
    CHECK(take(s) == -1);  // nothing was ever submitted
    int prev = -1;
    for (int k = 0; k < 5; ++k) {
      s.submit();
      CHECK(s.unprocessed());
      const int blk = s.next_block();
      CHECK(blk == 0 || blk == 1);
      CHECK(blk != prev);  // never the block the previous result lives in
      s.done(blk);
      CHECK(!s.unprocessed());
      CHECK(take(s) == blk);
      prev = blk;
    }
  }
  {  // take twice: the second fails with the existing text
    ResultSlots s;
    s.submit(); s.done(s.next_block());
    CHECK(take(s) >= 0);
    CHECK(take(s) == -1);
    CHECK(take(s) == -1);
  }
  {  // take after failed rethrows once, then reports no output
    ResultSlots s;
    s.submit(); s.failed("k_conv_m: a ring wait gave up");
    CHECK(!s.unprocessed());
    CHECK(take(s, "k_conv_m: a ring wait gave up") == -2);
    CHECK(take(s) == -1);
    // rethrow() alone (drm_wait) consumes the error too
    s.submit(); s.failed("again");
    try { s.rethrow(); CHECK(!"rethrow() must throw"); } catch (const dr::Error &e) { CHECK(e.code == DR_ERR_DEVICE && std::string(e.what()) == "again"); }
    s.rethrow();
    CHECK(take(s) == -1);
    // ... and the engine goes on: the next window is a legal cycle
    s.submit(); const int blk = s.next_block(); s.done(blk);
    CHECK(take(s) == blk);
  }
  {  // drop between done and take (configure, set_feature_cache: the blocks were the old plan's)
    ResultSlots s;
    s.submit(); s.done(s.next_block());
    s.drop();
    CHECK(take(s) == -1);
    s.submit(); const int blk = s.next_block(); s.done(blk);
    CHECK(take(s) == blk);
  }
}

// ------------------------------------------------------------------ ForwardCursor
// an op list shaped like the plan's: FeatureNet (10 ops, the fork range [5, 10), feat2 complete after op 6), three times
// cost volume, two convolutions, prob, regress, then three filter ops
struct TestOp { char kind; int stage; };  // 'c' cost volume, 'r' regress, '.' anything else
static std::vector<TestOp> ops() {
  std::vector<TestOp> o(10, TestOp{'.', 0});
  for (int s = 1; s <= 3; ++s) { o.push_back({'c', s}); o.push_back({'.', 0}); o.push_back({'.', 0}); o.push_back({'.', s}); o.push_back({'r', s}); }
  for (int k = 0; k < 3; ++k) o.push_back({'.', 0});
  return o;
}
static const size_t kForkLo = 5, kForkHi = 10, kFeat2 = 6;
static size_t cv_at(int s) { return 10 + 5 * (size_t)(s - 1); }
static size_t rg_at(int s) { return cv_at(s) + 4; }

static ForwardCursor::Setup whole_alone() {
  ForwardCursor::Setup s{};
  s.range = ForwardRange{0, ~(size_t)0, ops().size()};
  s.timed = false; s.alone = true; s.side_stream = true; s.cached = false;
  s.fork_lo = kForkLo; s.fork_hi = kForkHi; s.feat2_op = kFeat2;
  s.collective = ForwardCursor::kNone; s.rank = 0; s.phase_mode = false;
  s.has_src[0] = s.has_src[1] = s.has_src[2] = true;
  return s;
}
static std::vector<ForwardCursor::Step> run(const ForwardCursor::Setup &s) {
  const std::vector<TestOp> o = ops();
  ForwardCursor c(s);
  std::vector<ForwardCursor::Step> out;
  for (size_t i = 0; i < o.size(); ++i) out.push_back(c.at(i, o[i].kind == 'c', o[i].kind == 'r', o[i].stage));
  CHECK(!c.idle_stage());  // a forward never ends inside an idle stage
  return out;
}
static bool collective(const ForwardCursor::Step &t) { return t.reduce || t.all_reduce || t.broadcast_depth || t.broadcast_conf3; }
static bool forkish(const ForwardCursor::Step &t) { return t.side || t.open_fork || t.wait_feat2 || t.wait_feat3 || t.record_feat2 || t.record_feat3; }
static bool launched(const ForwardCursor::Step &t) { return !t.skip && t.launch; }

static void cursor_cases() {
  const size_t n = ops().size();
  {  // whole, alone, untimed
    const auto st = run(whole_alone());
    int forks = 0;
    for (size_t i = 0; i < n; ++i) {
      CHECK(launched(st[i]) && !st[i].zero_volume && !collective(st[i]));
      CHECK(st[i].side == (i >= kForkLo && i < kForkHi));
      forks += st[i].open_fork;
      CHECK(st[i].open_fork == (i == kForkLo));
      CHECK(st[i].wait_feat2 == (i == cv_at(2)));
      CHECK(st[i].wait_feat3 == (i == cv_at(3)));
      CHECK(st[i].record_feat2 == (i == kFeat2));
      CHECK(st[i].record_feat3 == (i == kForkHi - 1));
    }
    CHECK(forks == 1);
    CHECK(ForwardCursor(whole_alone()).forks() && ForwardCursor(whole_alone()).whole());
  }
  // timed, not alone, partial, cached, the switch off, an empty fork range -- each alone: no side-stream flag anywhere
  for (int why = 0; why < 6; ++why) {
    ForwardCursor::Setup s = whole_alone();
    if (why == 0) s.timed = true;
    if (why == 1) s.alone = false;
    if (why == 2) s.range.last = n - 1;
    if (why == 3) s.cached = true;
    if (why == 4) s.side_stream = false;
    if (why == 5) s.fork_lo = s.fork_hi;
    CHECK(!ForwardCursor(s).forks());
    const auto st = run(s);
    for (size_t i = 0; i < n; ++i) {
      CHECK(!forkish(st[i]));
      const bool expect_launch = why == 2 ? i < n - 1 : (why == 3 ? i >= kForkHi : true);
      CHECK(launched(st[i]) == expect_launch);
      CHECK(st[i].skip == !expect_launch);
    }
  }
  {  // rooted, rank 1: idle between a stage's cost volume and its regress; the regress does not launch but broadcasts
    ForwardCursor::Setup s = whole_alone();
    s.collective = ForwardCursor::kRooted; s.rank = 1;
    const std::vector<TestOp> o = ops();
    ForwardCursor c(s);
    for (size_t i = 0; i < n; ++i) {
      const ForwardCursor::Step t = c.at(i, o[i].kind == 'c', o[i].kind == 'r', o[i].stage);
      int stage = 0;
      for (int k = 1; k <= 3; ++k) if (i >= cv_at(k) && i <= rg_at(k)) stage = k;
      const bool between = stage && i > cv_at(stage) && i < rg_at(stage);
      CHECK(t.skip == between);
      CHECK(launched(t) == !(between || (stage && i == rg_at(stage))));
      CHECK(t.reduce == (stage && i == cv_at(stage)));
      CHECK(!t.all_reduce);
      CHECK(t.broadcast_depth == (stage && i == rg_at(stage)));
      CHECK(t.broadcast_conf3 == (i == rg_at(3)));
      CHECK(c.idle_stage() == (stage && i >= cv_at(stage) && i < rg_at(stage)));  // live again behind the regress
    }
    // the fork is kept on a sharded engine: the side stream's heads and the reduce of stage 1 overlap
    CHECK(c.forks());
  }
  {  // rooted, rank 0: everything launches, with the same collectives
    ForwardCursor::Setup s = whole_alone();
    s.collective = ForwardCursor::kRooted; s.rank = 0;
    const auto st = run(s);
    for (size_t i = 0; i < n; ++i) {
      CHECK(launched(st[i]));
      bool cv = false, rg = false;
      for (int k = 1; k <= 3; ++k) { cv |= i == cv_at(k); rg |= i == rg_at(k); }
      CHECK(st[i].reduce == cv && st[i].broadcast_depth == rg && st[i].broadcast_conf3 == (i == rg_at(3)) && !st[i].all_reduce);
    }
  }
  for (int rank = 0; rank < 3; ++rank) {  // all-reduce: every rank launches everything, with no broadcast
    ForwardCursor::Setup s = whole_alone();
    s.collective = ForwardCursor::kAllReduce; s.rank = rank;
    const auto st = run(s);
    for (size_t i = 0; i < n; ++i) {
      bool cv = false;
      for (int k = 1; k <= 3; ++k) cv |= i == cv_at(k);
      CHECK(launched(st[i]) && st[i].all_reduce == cv && !st[i].reduce && !st[i].broadcast_depth && !st[i].broadcast_conf3);
    }
  }
  for (int form = 0; form < 3; ++form)  // phase mode: no collective at all, and every rank launches what its range holds
    for (int rank = 0; rank < 2; ++rank) {
      ForwardCursor::Setup s = whole_alone();
      s.collective = (ForwardCursor::Collective)form; s.rank = rank; s.phase_mode = true;
      const auto st = run(s);
      for (size_t i = 0; i < n; ++i) CHECK(launched(st[i]) && !collective(st[i]));
    }
  {  // a rank with no source views: zero-fill before each cost volume, and only there
    ForwardCursor::Setup s = whole_alone();
    s.has_src[0] = s.has_src[1] = s.has_src[2] = false;
    s.collective = ForwardCursor::kRooted; s.rank = 1;
    const auto st = run(s);
    for (size_t i = 0; i < n; ++i) {
      bool cv = false;
      for (int k = 1; k <= 3; ++k) cv |= i == cv_at(k);
      CHECK(st[i].zero_volume == cv);
      if (cv) CHECK(launched(st[i]) && st[i].reduce);
    }
    s.has_src[1] = true;  // per stage
    const auto st2 = run(s);
    CHECK(st2[cv_at(1)].zero_volume && !st2[cv_at(2)].zero_volume && st2[cv_at(3)].zero_volume);
  }
  {  // partial ranges: the four phase ranges cut at the cost volumes visit every op exactly once between them
    const size_t cut[5] = {0, cv_at(1) + 1, cv_at(2) + 1, cv_at(3) + 1, n};
    std::vector<int> visits(n, 0);
    for (int p = 0; p < 4; ++p) {
      ForwardCursor::Setup s = whole_alone();
      s.range = ForwardRange{cut[p], cut[p + 1], n};
      s.phase_mode = true; s.collective = ForwardCursor::kRooted; s.rank = 1;
      CHECK(!ForwardCursor(s).whole() && !ForwardCursor(s).forks());
      const auto st = run(s);
      for (size_t i = 0; i < n; ++i) {
        CHECK(!forkish(st[i]) && !collective(st[i]));
        CHECK(st[i].skip == !(i >= cut[p] && i < cut[p + 1]));
        visits[i] += launched(st[i]);
      }
    }
    for (size_t i = 0; i < n; ++i) CHECK(visits[i] == 1);
  }
  // the "whole forward" predicate
  CHECK((ForwardRange{0, ~(size_t)0, n}.whole()) && (ForwardRange{0, n, n}.whole()) && !(ForwardRange{0, n - 1, n}.whole()) && !(ForwardRange{1, n, n}.whole()));
  CHECK((ForwardRange{2, 4, n}.has(2)) && (ForwardRange{2, 4, n}.has(3)) && !(ForwardRange{2, 4, n}.has(4)) && !(ForwardRange{2, 4, n}.has(1)));
}

// ------------------------------------------------------------------ FlagScope, span_holds
static void small_cases() {
  bool f = false;
  { FlagScope up(f); CHECK(f); }
  CHECK(!f);
  try { FlagScope up(f); CHECK(f); throw std::runtime_error("x"); } catch (const std::exception &) {}
  CHECK(!f);

  const uintptr_t base = 0x10000;
  const size_t span = 4096, bytes = 1024;
  CHECK(dr::span_holds(base, span, base + 512, bytes));                 // inside the range
  CHECK(!dr::span_holds(base, span, base + span - 512, bytes));         // starts inside the range and ends past it
  CHECK(!dr::span_holds(base, span, base - 16, bytes));                 // before the base
  CHECK(dr::span_holds(base, span, base, span));                        // exact fit
  CHECK(dr::span_holds(base, span, base + span - bytes, bytes));        // ends with the range
  CHECK(!dr::span_holds(base, span, base + span - bytes + 1, bytes));   // one byte past it
  CHECK(!dr::span_holds(base, span, base, span + 1));                   // larger than the range
  CHECK(!dr::span_holds(base, span, base + span, 1));                   // at its end
  CHECK(!dr::span_holds(~(uintptr_t)0 - 4095, span, ~(uintptr_t)0 - 15, bytes));  // (no wrap-around at the top of the address space)
}

int main() {
  ticket_cases();
  slots_cases();
  cursor_cases();
  small_cases();
  if (failures) { fprintf(stderr, "mvs_engine_host_check: %d failure(s)\n", failures); return 1; }
  printf("mvs_engine_host_check ok\n");
  return 0;
}
