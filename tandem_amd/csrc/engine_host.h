// engine_host.h -- three decisions of the DrFusion engine as values with no HIP in them: the order in which its calls may come
// (CallOrder), when a map-scope localisation must select and stage stored blocks again (LocateStageCursor), and what the score of
// a map-scope search stages for which candidates (plan_search_stage).  Plain C++17 over dr_host.h (fail) and fusion_host.h, which
// includes this header at its end: tests/cpp/engine_host_check.cpp and tests/cpp/search_scope_check.cpp run them on the CPU.
// The engine and its components (fusion_core.h, render_ops.h, pose_ops.h, search_ops.h) keep everything that touches the device.
#pragma once
#include <iterator>
#include <string>
#include <utility>
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

// Which stored blocks the score stage of a search in map scope stages, and for which candidates (the rule: fusion_host.h "the
// search scope").  A pure function of the store, the options and the candidates: the passes in candidate order, each a run of
// candidates [first, first + count) and the ascending, de-duplicated keys every one of them may read.  Candidates are independent,
// so any such split scores the same bits.  A lattice (pose_host.h SearchLattice) starts from whole table entries -- candidates
// (((e) Nx + ix) Ny + iy) Nz + iz over all offsets of entry e = a n_rot + r, a contiguous range, as is every ix-range [x0, x1) of
// it.  A unit whose selection exceeds `capacity` is halved along ix, the lower half taking the floor, down to single ix-slabs; a
// single slab -- or, in a plain table, a single pose -- above the capacity fails the plan with its count.  Consecutive units are
// merged greedily into one pass while the union of their keys stays within the capacity.  An empty store: one pass without keys.
struct SearchStagePass {
  size_t first, count;
  std::vector<unsigned long long> keys;
};
struct SearchStagePlan {
  bool ok = true;
  size_t too_many = 0;  // !ok: what the candidates of one slab (one plain pose) can read
  std::vector<SearchStagePass> passes;
};
// the selection of candidates [x0, x1) x all iy x all iz of table entry e (plain: the pose e; x0, x1 are not read): ascending
inline std::vector<unsigned long long> select_search_unit(const HostBlockStore &store, const drf_options_t &o, const double *table, const SearchLattice &L, size_t e,
                                                          int x0, int x1) {
  MapMotion m;
  memcpy(m.R, table + 12 * e, 72);
  memcpy(m.tv, table + 12 * e + 9, 24);
  double extra = 0.0;
  if (!L.plain) {
    // the unit's offset box: ix - half_x in [x0 - half_x, x1 - 1 - half_x], iy - half_y in [-half_y, half_y], iz alike
    const double hx = 0.5 * (double)(x1 - 1 - x0), hy = (double)L.half[1], hz = (double)L.half[2];
    m.tv[0] += (0.5 * (double)(x0 + x1 - 1) - (double)L.half[0]) * L.dstep;
    extra = search_unit_extra(std::sqrt(hx * hx + hy * hy + hz * hz) * L.dstep * (double)o.voxel_size);
  }
  float p16[16];
  locate_pose16(m, o.voxel_size, p16);
  std::vector<unsigned long long> keys;
  select_render_blocks(store, o, p16, keys, nullptr, extra);
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  return keys;
}
inline SearchStagePlan plan_search_stage(const HostBlockStore &store, const drf_options_t &o, const double *table, const SearchLattice &L, size_t n, size_t capacity) {
  SearchStagePlan p;
  if (store.empty() || n == 0) {
    p.passes.push_back({0, n, {}});
    return p;
  }
  const size_t slab = L.plain ? 1 : (size_t)L.N[1] * (size_t)L.N[2], cells = L.plain ? 1 : slab * (size_t)L.N[0];
  std::vector<unsigned long long> merged;
  // one unit, in candidate order: into the open pass if the union fits, else it opens the next one
  auto add = [&](size_t first, size_t count, std::vector<unsigned long long> &keys) {
    if (!p.passes.empty()) {
      SearchStagePass &last = p.passes.back();
      merged.clear();
      std::set_union(last.keys.begin(), last.keys.end(), keys.begin(), keys.end(), std::back_inserter(merged));
      if (merged.size() <= capacity) {
        last.keys.swap(merged);
        last.count += count;
        return;
      }
    }
    p.passes.push_back({first, count, std::move(keys)});
  };
  for (size_t e = 0; e * cells < n && p.ok; ++e) {
    // the ix-ranges of entry e still to place, the lowest on top
    std::vector<std::pair<int, int>> todo(1, {0, L.plain ? 1 : L.N[0]});
    while (!todo.empty()) {
      const std::pair<int, int> u = todo.back();
      todo.pop_back();
      std::vector<unsigned long long> keys = select_search_unit(store, o, table, L, e, u.first, u.second);
      if (keys.size() <= capacity) {
        add(e * cells + (size_t)u.first * slab, (size_t)(u.second - u.first) * slab, keys);
        continue;
      }
      if (u.second - u.first == 1) {
        p.ok = false;
        p.too_many = keys.size();
        p.passes.clear();
        break;
      }
      const int mid = u.first + (u.second - u.first) / 2;
      todo.push_back({mid, u.second});
      todo.push_back({u.first, mid});
    }
  }
  return p;
}

}  // namespace dr
