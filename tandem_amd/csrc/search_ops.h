// search_ops.h -- drf_score_poses / drf_search_frame as two components over FusionCore (the rule: pose_host.h score_point /
// search_candidate / search_refine; the kernels: search_kernels.h; DESIGN.md §7c "Searching a pose lattice").  PoseScorer owns the
// score stage's device scratch and the statistics of the search calls.  PoseSearch holds it and is the entry points: the prologue
// and the frame's intake (pose_ops.h FramePose), the score, and the refinement composed from FrameTracker::track_levels and
// FrameLocator::with_locate + locate_loop as drf_track_frame and drf_locate_frame run them -- there is no second copy of either
// loop.  Included by dr_fusion.hip after pose_ops.h.
#pragma once
#include <vector>

#include "fusion_core.h"
#include "map_ops.h"
#include "pose_ops.h"

namespace dr {

class PoseScorer {
 public:
  explicit PoseScorer(FusionCore &core) : core_(core) {}
  uint64_t stats[8] = {};  // drf_search_stats
  void reset() { for (auto &v : stats) v = 0; }

  // candidates per launch: 32 bytes of results each, and with a plain table 96 bytes of poses
  size_t chunk_size() const {
    size_t c = 65536;
    if (const char *e = hook_env("DR_SEARCH_CHUNK")) c = (size_t)std::min(1 << 20, std::max(1, atoi(e)));  // parity hook: chunk seams on small lattices
    return c;
  }
  // The layout for a call whose table holds table_entries poses at a time.  mine: where a host-given depth image goes.
  float *prepare(int step, size_t table_entries) {
    lg_ = locate_grid(core_.o, step);
    total_ = (int)locate_positions(lg_); groups_ = (int)locate_groups(lg_);
    chunk_ = chunk_size();
    const size_t padded = (size_t)groups_ * 512;
    float *mine = nullptr;
    carve(buf_, core_.int_stream, [&](Carver &c) {
      g_ = c.take<double>(padded * 3);
      table_ = c.take<double>(std::max<size_t>(table_entries, 1) * 12);
      out_ = c.take<SearchOut>(chunk_);
      mine = c.take<float>(core_.npix);
      flag_ = c.take<unsigned char>(padded);
    });
    stats[1] = (uint64_t)total_; stats[6] = buf_.capacity();
    return mine;
  }
  // k_search_points over the depth image (device memory), once per call
  void points(const float *depth) {
    const int padded = groups_ * 512;
    if (padded == 0) return;
    hipLaunchKernelGGL(k_search_points, dim3(cdiv(padded, 256)), dim3(256), 0, core_.int_stream, depth, lg_, (double)core_.o.voxel_size, total_, padded, g_, flag_);
    DR_HIP(hipGetLastError());
  }
  // Candidates [0, n) of the lattice L in chunks; cost, counts (4 per candidate) and score may each be null.  A plain table (one pose
  // per candidate) is uploaded chunk by chunk, a search's (n_anchors x n_rot entries) once.
  void score(const SearchLattice &L, const double *table, size_t table_entries, size_t n, const ScoreOpt &so, double *cost, uint32_t *counts, double *score) {
    std::vector<SearchOut> host(std::min(n, chunk_));
    if (!L.plain) DR_HIP(hipMemcpyAsync(table_, table, table_entries * 96, hipMemcpyHostToDevice, core_.int_stream));
    for (size_t first = 0; first < n; first += chunk_) {
      const size_t m = std::min(chunk_, n - first);
      if (L.plain) DR_HIP(hipMemcpyAsync(table_, table + 12 * first, m * 96, hipMemcpyHostToDevice, core_.int_stream));
      hipLaunchKernelGGL(k_search_score, dim3(cdiv((int)m, 4)), dim3(256), 0, core_.int_stream, core_.d, g_, flag_, groups_, table_, L, first, L.plain ? first : (size_t)0,
                         (int)m, so, (double)core_.o.voxel_size, out_);
      DR_HIP(hipGetLastError());
      DR_HIP(hipMemcpyAsync(host.data(), out_, m * sizeof(SearchOut), hipMemcpyDeviceToHost, core_.int_stream));
      DR_HIP(hipStreamSynchronize(core_.int_stream));
      for (size_t i = 0; i < m; ++i) {
        if (cost) cost[first + i] = host[i].cost;
        if (counts) memcpy(counts + 4 * (first + i), host[i].counts, 16);
        if (score) score[first + i] = host[i].score;
      }
      ++stats[3];
      if (first == 0) stats[2] = host[0].counts[0];
    }
    stats[0] = n;
  }

 private:
  FusionCore &core_;
  DeviceBuf<unsigned char> buf_;  // sized by the largest call so far
  LocateGrid lg_{};
  int total_ = 0, groups_ = 0;
  size_t chunk_ = 0;
  double *g_ = nullptr, *table_ = nullptr;
  unsigned char *flag_ = nullptr;
  SearchOut *out_ = nullptr;
};

// A depth frame found in the map from many poses.  The score stage is scorer_'s (k_search_points once, k_search_score in chunks, the
// resident map through find_block); what is added here is the call order -- frame_prologue -- the frame's intake, and the
// refinement: track_levels and with_locate + locate_loop on the device image the score read.  Nothing of the map, the public
// render buffers or the streaming state is written.
class PoseSearch {
 public:
  PoseSearch(FramePose &frame, FrameTracker &tracker, FrameLocator &locator) : frame_(frame), core_(frame.core), streamer_(frame.streamer), tracker_(tracker), locator_(locator), scorer_(frame.core) {}
  void score_poses(const char *who, const float *h_depth, const void *d_depth, const float *poses16, size_t n, const drf_score_options_t *opt, double *cost,
                   uint32_t *counts, double *score) {
    scorer_.reset();
    if (!(h_depth || d_depth) || !poses16 || !(cost || counts || score)) fail(DR_ERR_ARG, "%s: null argument", who);
    ScoreOpt so{};
    const char *bad = score_options(opt, core_.o.truncation_distance, core_.o.voxel_size, so);
    if (!bad && (n == 0 || n > kSearchMaxCandidates)) fail(DR_ERR_ARG, "%s: %zu poses (at least 1, at most 2^24)", who, n);
    with_score(who, bad, so.step, std::min(n, scorer_.chunk_size()), h_depth, d_depth, [&](const float *) {
      std::vector<double> table(n * 12);
      for (size_t i = 0; i < n; ++i) {
        if (const char *why = transform_pose_fault(poses16 + 16 * i)) fail(DR_ERR_ARG, "%s: pose %zu %s", who, i, why);
        const MapMotion m = map_motion(poses16 + 16 * i, core_.o.voxel_size);
        memcpy(&table[12 * i], m.R, 72);
        memcpy(&table[12 * i + 9], m.tv, 24);
      }
      const SearchLattice plain = {{1, 1, 1}, {0, 0, 0}, 0.0, 1};
      scorer_.score(plain, table.data(), n, n, so, cost, counts, score);
    });
  }
  // returns what dr_last_error() says after a search that ran but found no pose (empty otherwise)
  std::string search_frame(const char *who, const float *h_depth, const void *d_depth, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot,
                           const drf_search_options_t *opt, const drf_track_options_t *topt, const drf_locate_options_t *lopt, float *pose16_out,
                           drf_search_result_t *res, double *all_scores) {
    scorer_.reset();
    if (!(h_depth || d_depth) || !anchors16 || !rotations9 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    SearchOpt so{};
    TrackPyramidOpt po{{}, 1, 0};
    LocateOpt lo;
    const char *bad = search_options(opt, core_.o.truncation_distance, core_.o.voxel_size, so);
    if (!bad) bad = FrameTracker::track_options_of(topt, core_.o.voxel_size, po.c);
    if (!bad) bad = locate_options(lopt, core_.o.truncation_distance, lo);
    const size_t n = bad ? 1 : search_count(n_anchors, n_rot, so.L);
    if (n == 0) fail(DR_ERR_ARG, "%s: %zu anchors x %zu rotations x %d x %d x %d offsets is no count of candidates (at least 1, at most 2^24)", who, n_anchors, n_rot,
                     so.L.N[0], so.L.N[1], so.L.N[2]);
    drf_search_result_t r;
    with_score(who, bad, so.s.step, n_anchors * n_rot, h_depth, d_depth, [&](const float *depth) {
      std::vector<double> table;
      const std::string why = search_table(anchors16, n_anchors, rotations9, n_rot, core_.o.voxel_size, table);
      if (!why.empty()) fail(DR_ERR_ARG, "%s: %s", who, why.c_str());
      std::vector<double> cost(n), score(n);
      std::vector<uint32_t> counts(4 * n);
      scorer_.score(so.L, table.data(), n_anchors * n_rot, n, so.s, cost.data(), counts.data(), score.data());
      if (all_scores) memcpy(all_scores, score.data(), n * 8);
      const FramePair frame = FramePair::device(nullptr, depth);
      FrameTracker::TrackSide &tk = tracker_.geometric();
      search_refine(so, table.data(), search_select(score.data(), n, so.top_k), cost.data(), counts.data(), score.data(), n, core_.o.voxel_size,
                    [&](const float *p16, drf_align_result_t &tr) {
                      tk.reset();
                      uint64_t last[5] = {0, 0, 0, 0, 0};
                      tracker_.track_levels(who, tk, false, po, frame, p16, tr, last);
                      scorer_.stats[4] += tk.stats[4]; scorer_.stats[5] += tk.stats[3];
                    },
                    [&](const float *p16, drf_align_result_t &lr) {
                      locator_.with_locate(who, nullptr, depth, p16, lopt, [&](const LocateOpt &l, auto &eval) { locate_loop(eval, map_motion(p16, core_.o.voxel_size), l, core_.o.voxel_size, lr); });
                      scorer_.stats[5] += locator_.locate_stats()[3];
                    },
                    pose16_out, r);
    });
    if (res) *res = r;
    if (r.status != DRF_ALIGN_LOST) return std::string();
    return std::string(who) + ": no candidate of the best " + std::to_string(r.n_entries) + " of " + std::to_string((unsigned long long)n) +
           " ended its tracking and its localisation with a pose (the best score is " + std::to_string(r.entries[0].score) + " voxels per sample with " +
           std::to_string(r.entries[0].counts[1]) + " of " + std::to_string(r.entries[0].counts[0]) + " samples valid; " + std::to_string(streamer_.store().size()) +
           " blocks are in the host store); pose16_out is the best-scoring candidate";
  }
  void search_stats(uint64_t out[8]) const {
    if (!out) fail(DR_ERR_ARG, "drf_search_stats: null argument");
    for (int i = 0; i < 8; ++i) out[i] = scorer_.stats[i];
  }

 private:
  template <class Body>
  void with_score(const char *who, const char *bad_option, int step, size_t table_entries, const float *h_depth, const void *d_depth, Body &&body) {
    static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    frame_.frame_prologue(who, bad_option, identity, nullptr);  // the call's poses are many: body refuses them, each by its index
    float *mine = scorer_.prepare(step, table_entries);
    const float *depth = (const float *)d_depth;
    if (h_depth) {
      core_.upload_frame(nullptr, h_depth, nullptr, mine);
      depth = mine;
    }
    scorer_.stats[7] = streamer_.store().size();
    try {
      scorer_.points(depth);
      body(depth);
    } catch (...) {
      scorer_.reset();
      throw;
    }
  }
  FramePose &frame_;
  FusionCore &core_;
  BlockStreamer &streamer_;
  FrameTracker &tracker_;
  FrameLocator &locator_;
  PoseScorer scorer_;  // the score stage and the statistics of both calls
};

}  // namespace dr
