// mvs_engine_host.h -- the decisions of the DrMvsnet engine (dr_mvsnet.hip) as values with no HIP in them: the count of windows in flight
// (WindowTicket), the reference's call protocol without its threads (ResultSlots), what forward() does for each op of the plan
// (ForwardRange, ForwardCursor), a flag that is up for a scope (FlagScope) and whether a page-locked range holds a whole image
// (span_holds).  Plain C++17 over dr_host.h (fail) and mvs_host.h: tests/cpp/mvs_engine_host_check.cpp runs all of it on the CPU.
// The engine and its parts (mvs_stage.h, mvs_cache.h, mvs_shard.h) keep everything that touches the device.
#pragma once
#include <atomic>
#include <string>

#include "dr_host.h"
#include "mvs_host.h"

namespace dr {

// windows whose kernels are enqueued or running, per device, over all engines of the process (forward() forks onto its side stream only when it is alone)
inline std::atomic<int> &windows_in_flight(int device) {
  static std::atomic<int> n[16];
  return n[device & 15];
}
// One window in flight on a device: counted when acquired, released exactly once, when the ticket that holds it goes (a moved-from
// ticket holds nothing).  CallAsync's prelaunch parks its ticket in the engine; the worker takes it from there.
class WindowTicket {
 public:
  WindowTicket() = default;  // holds nothing
  explicit WindowTicket(int device) : n_(&windows_in_flight(device)) { n_->fetch_add(1, std::memory_order_relaxed); }
  WindowTicket(WindowTicket &&o) noexcept : n_(o.n_) { o.n_ = nullptr; }
  WindowTicket &operator=(WindowTicket &&o) noexcept {
    if (this != &o) { release(); n_ = o.n_; o.n_ = nullptr; }
    return *this;
  }
  ~WindowTicket() { release(); }
  explicit operator bool() const { return n_ != nullptr; }
  // the parked ticket if there is one (the window was counted when its forward was enqueued), else a new one
  static WindowTicket take(WindowTicket &parked, int device) { return parked ? std::move(parked) : WindowTicket(device); }

 private:
  void release() {
    if (n_) n_->fetch_sub(1, std::memory_order_relaxed);
    n_ = nullptr;
  }
  std::atomic<int> *n_ = nullptr;
};

// The reference's protocol state (dr_mvsnet.cpp:54-107): an input waits for the worker; the worker leaves a result in one of two
// blocks, or its error; the result is handed out once.  Every transition is made under the engine's mutex; unprocessed() alone is
// also read without it (ready(); dr_mvsnet.cpp:54 does the same with a plain bool).
class ResultSlots {
 public:
  bool unprocessed() const { return unprocessed_; }
  void submit() { unprocessed_ = true; }
  int next_block() const { return cur_ ^ 1; }  // the block the previous result does NOT live in (drm_get_result_view: that one may still be read)
  void done(int block) { cur_ = block; has_output_ = true; unprocessed_ = false; }
  void failed(const std::string &text) { error_ = text; unprocessed_ = false; }
  void rethrow() {
    if (!error_.empty()) { std::string e = error_; error_.clear(); fail(DR_ERR_DEVICE, "%s", e.c_str()); }
  }
  // rethrows what the window's worker threw, else hands the block of the four maps out ONCE
  int take() {
    rethrow();
    if (!has_output_) fail(DR_ERR_PROTOCOL, "Output should be valid. Maybe you called GetResult more than once?");
    has_output_ = false;
    return cur_;
  }
  void drop() { has_output_ = false; }  // (the result blocks were the old plan's)

 private:
  std::atomic<bool> unprocessed_{false};
  bool has_output_ = false;
  int cur_ = 0;  // the result block the last result is in
  std::string error_;
};

// up for a scope, down on every way out of it
class FlagScope {
 public:
  explicit FlagScope(bool &f) : f_(f) { f_ = true; }
  FlagScope(const FlagScope &) = delete;
  void operator=(const FlagScope &) = delete;
  ~FlagScope() { f_ = false; }

 private:
  bool &f_;
};

// the ops [first, last) of a plan of n
struct ForwardRange {
  size_t first = 0, last = ~(size_t)0, n = 0;
  bool whole() const { return first == 0 && last >= n; }
  bool has(size_t i) const { return i >= first && i < last; }
};

// What forward() does for op i of the plan, in plan order.
//  * A whole forward (no per-op events, no range) forks: the ops [fork_lo, fork_hi) run on the side stream, opened at fork_lo;
//    stage 2 / 3's cost volume waits for feat2 / feat3, recorded after feat2_op and after the last op of the fork range -- unless the
//    switch is off, the feature cache answers FeatureNet (its ops are then skipped) or other windows are in flight on the device.
//  * View shard (a communicator and a source-view total, outside phase mode): every cost volume is summed over the ranks.  In the
//    rooted form it is reduced to rank 0, the other ranks idle through the stage up to its REGRESS op, which they do not launch, and the
//    stage's depth (at stage 3 also conf3) is broadcast from rank 0; in the all-reduce form every rank goes on with the sum.
//  * A rank that holds the reference view only zeroes its volume first: its partial sum is the empty one.
class ForwardCursor {
 public:
  enum Collective { kNone, kAllReduce, kRooted };
  struct Setup {
    ForwardRange range;
    bool timed, alone, side_stream, cached;
    size_t fork_lo, fork_hi, feat2_op;
    Collective collective;  // of a sharded engine; phase_mode: the caller reduces between phases, no collective here
    int rank;
    bool phase_mode;
    bool has_src[3];        // per stage: the window holds source views
  };
  struct Step {
    bool skip;                           // nothing at all for this op (the range, the cache, an idle rank)
    bool side;                           // on the side stream
    bool open_fork;                      // first: the side stream goes behind the main stream
    bool wait_feat2, wait_feat3;         // first: the main stream goes behind the side stream's feat2 / feat3
    bool zero_volume;                    // first: the stage's volume is cleared
    bool launch;
    bool reduce, all_reduce;             // after: the stage's volume to rank 0 / summed on every rank
    bool broadcast_depth, broadcast_conf3;  // after: from rank 0
    bool record_feat2, record_feat3;     // after: on the side stream
  };
  explicit ForwardCursor(const Setup &s)
      : s_(s), fork_(s.side_stream && s.alone && !s.timed && s.range.whole() && s.fork_lo < s.fork_hi && !s.cached),
        collective_(s.phase_mode ? kNone : s.collective) {}
  bool whole() const { return s_.range.whole(); }
  bool forks() const { return fork_; }
  bool idle_stage() const { return idle_stage_; }  // between a stage's cost volume and its regression only rank 0 works
  Step at(size_t i, bool is_costvol, bool is_regress, int stage) {
    Step t{};
    if (!s_.range.has(i) || (s_.cached && i < s_.fork_hi) || (idle_stage_ && !is_regress)) { t.skip = true; return t; }
    t.side = fork_ && i >= s_.fork_lo && i < s_.fork_hi;
    t.open_fork = fork_ && i == s_.fork_lo;
    t.wait_feat2 = fork_ && is_costvol && stage == 2;
    t.wait_feat3 = fork_ && is_costvol && stage == 3;
    t.zero_volume = is_costvol && !s_.has_src[stage - 1];
    t.launch = !idle_stage_;  // (idle here: the REGRESS op of a stage that rank 0 alone regularised)
    if (is_costvol && collective_ == kRooted) { t.reduce = true; idle_stage_ = s_.rank != 0; }
    if (is_costvol && collective_ == kAllReduce) t.all_reduce = true;
    if (is_regress && collective_ == kRooted) { t.broadcast_depth = true; t.broadcast_conf3 = stage == 3; idle_stage_ = false; }
    t.record_feat2 = t.side && i == s_.feat2_op;
    t.record_feat3 = t.side && i == s_.fork_hi - 1;
    return t;
  }

 private:
  const Setup s_;
  const bool fork_;
  const Collective collective_;
  bool idle_stage_ = false;
};

// "Page-locked" is decided for the WHOLE image, not for its first byte: the allocation (or registered range) [base, base + span) that
// byte p lies in has to contain all `bytes` from p on.
inline bool span_holds(uintptr_t base, size_t span, uintptr_t p, size_t bytes) {
  return p >= base && bytes <= span && p - base <= span - bytes;
}

}  // namespace dr
