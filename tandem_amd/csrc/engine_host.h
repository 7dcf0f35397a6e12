// engine_host.h -- two decisions of the DrFusion engine as values with no HIP in them: the order in which its calls may come
// (CallOrder) and when a map-scope localisation must select and stage stored blocks again (LocateStageCursor).  Plain C++17 over
// dr_host.h (fail) and fusion_host.h, which includes this header at its end: tests/cpp/engine_host_check.cpp runs both on the CPU.
// The engine and its components (fusion_core.h, render_ops.h, pose_ops.h) keep everything that touches the device.
#pragma once
#include <string>
#include <vector>

#include "dr_host.h"
#include "fusion_host.h"

namespace dr {

// IntegrateScanAsync -> RenderAsync -> GetRenderResult, in a loop (tsdf_volume.cu:515-737).  Every other call is legal where
// IntegrateScanAsync is.  A check refuses with DR_ERR_PROTOCOL and changes nothing; a transition is made by the caller once every
// other refusal of its call is past.
class CallOrder {
 public:
  enum Next { kIntegrate, kRender, kGetRender };
  void expect(Next want, const char *msg) const {
    static const char *names[] = {"IntegrateScanAsync", "RenderAsync", "GetRenderResult"};
    if (next_ != want) fail(DR_ERR_PROTOCOL, "%s You should have called %s", msg, names[next_]);
  }
  void expect_integrate(const char *who) const { expect(kIntegrate, (std::string(who) + ": call it where IntegrateScanAsync may be called.").c_str()); }
  // a render comes after a scan -- or where a scan may come, while the map is one that was loaded or merged and no scan followed
  void expect_render(const char *msg) const {
    if (!(loaded_ && next_ == kIntegrate)) expect(kRender, msg);
  }
  void scan_begun() { next_ = kRender; loaded_ = false; }
  void render_begun() { next_ = kGetRender; }
  void result_fetched() { next_ = kIntegrate; }
  void map_loaded() { loaded_ = true; }  // drf_load_map, drf_merge_map
  bool render_pending() const { return next_ == kGetRender; }  // between RenderAsync and GetRenderResult
  bool scan_may_come() const { return next_ == kIntegrate; }

 private:
  Next next_ = kIntegrate;
  bool loaded_ = false;
};

// Which stored blocks the evaluations of one drf_locate_* call in map scope read, pose by pose (the rules: fusion_host.h
// select_locate_blocks, locate_stage_serves).  begin() selects at the call's first pose, before anything is evaluated; at() says
// for the pose of each evaluation whether the staging stands, or what to stage in its place.  A selection above the capacity is
// answered with its count and leaves the cursor as it was: the caller refuses, in its own words.
class LocateStageCursor {
 public:
  enum Kind { kKeep, kStage, kTooMany };
  struct Step {
    Kind kind;
    size_t count;  // kStage: blocks to stage -- 0: release the staging, the resident kernel serves; kTooMany: blocks selected
  };
  LocateStageCursor(const HostBlockStore &store, const drf_options_t &o, double slack, size_t capacity) : store_(store), o_(o), slack_(slack), capacity_(capacity) {}
  // the first pose: kStage if its selection fits (nothing is staged yet: the first at() hands it out), kTooMany if not
  Step begin(const float *pose16) { return select(pose16); }
  Step at(const float *pose16) {
    if (store_.empty()) return {kKeep, 0};  // nothing to stage, ever
    if (current_ && !locate_stage_serves(o_, pose_, pose16, slack_)) {
      const Step s = select(pose16);
      if (s.kind == kTooMany) return s;
    }
    if (current_) return {kKeep, keys_.size()};
    current_ = true;
    return {kStage, keys_.size()};
  }
  const std::vector<unsigned long long> &keys() const { return keys_; }  // the selection: what the last kStage asked for
  const float *pose() const { return pose_; }                             // where it was selected

 private:
  Step select(const float *pose16) {
    std::vector<unsigned long long> k = select_locate_blocks(store_, o_, pose16);
    if (k.size() > capacity_) return {kTooMany, k.size()};
    keys_.swap(k);
    memcpy(pose_, pose16, sizeof pose_);
    current_ = false;
    return {kStage, keys_.size()};
  }
  const HostBlockStore &store_;
  const drf_options_t o_;
  const double slack_;
  const size_t capacity_;
  std::vector<unsigned long long> keys_;
  float pose_[16] = {};
  bool current_ = false;  // the selection has been handed out by at()
};

}  // namespace dr
