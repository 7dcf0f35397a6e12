// search_ops.h -- drf_score_poses / drf_search_frame as two components over FusionCore (the rule: pose_host.h score_point /
// search_candidate / search_refine; the kernels: search_kernels.h; DESIGN.md §7c "Searching a pose lattice").  PoseScorer owns the
// score stage's device scratch and the statistics of the search calls.  PoseSearch holds it and is the entry points: the prologue
// and the frame's intake (pose_ops.h FramePose), the score, and the refinement composed from FrameTracker::track_levels and
// FrameLocator::with_locate + locate_loop as drf_track_frame and drf_locate_frame run them -- there is no second copy of either
// loop.  Both hold the colour forms as well (drf_score_colour_poses / drf_search_colour_frame; DESIGN.md §7c "Searching with
// colour"): a second layout of the same scratch, the two colour kernels, and the same intake and refinement with the frame's bgr.
// Included by dr_fusion.hip after pose_ops.h.
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

  // candidates per launch: 32 bytes of results each (40 with colour), and with a plain table 96 bytes of poses
  size_t chunk_size() const {
    size_t c = 65536;
    if (const char *e = hook_env("DR_SEARCH_CHUNK")) c = (size_t)std::min(1 << 20, std::max(1, atoi(e)));  // parity hook: chunk seams on small lattices
    return c;
  }
  // The layout for a call whose table holds table_entries poses at a time.  mine: where a host-given depth image goes.  mine_bgr
  // given: the colour layout -- yf at 4 bytes per padded position, the 40-byte record, and room for a host-given bgr image.
  float *prepare(int step, size_t table_entries, unsigned char **mine_bgr = nullptr) {
    lg_ = locate_grid(core_.o, step);
    total_ = (int)locate_positions(lg_); groups_ = (int)locate_groups(lg_);
    chunk_ = chunk_size();
    const size_t padded = (size_t)groups_ * 512;
    float *mine = nullptr;
    carve(buf_, core_.int_stream, [&](Carver &c) {
      g_ = c.take<double>(padded * 3);
      table_ = c.take<double>(std::max<size_t>(table_entries, 1) * 12);
      if (mine_bgr) outc_ = c.take<SearchColourOut>(chunk_);
      else out_ = c.take<SearchOut>(chunk_);
      mine = c.take<float>(core_.npix);
      if (mine_bgr) {
        yf_ = c.take<float>(padded);
        *mine_bgr = c.take<unsigned char>(core_.npix * 3);
      }
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
  // k_search_points_colour over the image pair (device memory), once per call
  void points_colour(const unsigned char *bgr, const float *depth) {
    const int padded = groups_ * 512;
    if (padded == 0) return;
    hipLaunchKernelGGL(k_search_points_colour, dim3(cdiv(padded, 256)), dim3(256), 0, core_.int_stream, depth, bgr, lg_, (double)core_.o.voxel_size, total_, padded, g_, flag_,
                       yf_);
    DR_HIP(hipGetLastError());
  }
  // Candidates [0, n) of the lattice L in chunks; cost, counts (4 per candidate) and score may each be null.  A plain table (one pose
  // per candidate) is uploaded chunk by chunk, a search's (n_anchors x n_rot entries) once.
  void score(const SearchLattice &L, const double *table, size_t table_entries, size_t n, const ScoreOpt &so, double *cost, uint32_t *counts, double *score) {
    chunks(L, table, table_entries, n, out_, true, [&](size_t first, size_t m) {
      hipLaunchKernelGGL(k_search_score, dim3(cdiv((int)m, 4)), dim3(256), 0, core_.int_stream, core_.d, g_, flag_, groups_, table_, L, first, L.plain ? first : (size_t)0,
                         (int)m, so, (double)core_.o.voxel_size, out_);
    }, [&](size_t c, const SearchOut &o) {
      if (cost) cost[c] = o.cost;
      if (counts) memcpy(counts + 4 * c, o.counts, 16);
      if (score) score[c] = o.score;
    });
  }
  // The same with colour (k_search_score_colour): photo beside cost.  counted false: the final re-score of a search, which leaves
  // the candidates, the samples and the chunks of the statistics what the score stage made them.
  void score_colour(const SearchLattice &L, const double *table, size_t table_entries, size_t n, const ScoreColourOpt &so, double *cost, double *photo, uint32_t *counts,
                    double *score, bool counted = true) {
    chunks(L, table, table_entries, n, outc_, counted, [&](size_t first, size_t m) {
      hipLaunchKernelGGL(k_search_score_colour, dim3(cdiv((int)m, 4)), dim3(256), 0, core_.int_stream, core_.d, g_, flag_, yf_, groups_, table_, L, first,
                         L.plain ? first : (size_t)0, (int)m, so, (double)core_.o.voxel_size, outc_);
    }, [&](size_t c, const SearchColourOut &o) {
      if (cost) cost[c] = o.cost;
      if (photo) photo[c] = o.photo;
      if (counts) memcpy(counts + 4 * c, o.counts, 16);
      if (score) score[c] = o.score;
    });
  }

 private:
  // the chunk loop of both scores: launch(first, m) enqueues the kernel over candidates [first, first + m), take(c, record) hands
  // out candidate c's record
  template <class Out, class Launch, class Take>
  void chunks(const SearchLattice &L, const double *table, size_t table_entries, size_t n, const Out *d_out, bool counted, Launch &&launch, Take &&take) {
    std::vector<Out> host(std::min(n, chunk_));
    if (!L.plain) DR_HIP(hipMemcpyAsync(table_, table, table_entries * 96, hipMemcpyHostToDevice, core_.int_stream));
    for (size_t first = 0; first < n; first += chunk_) {
      const size_t m = std::min(chunk_, n - first);
      if (L.plain) DR_HIP(hipMemcpyAsync(table_, table + 12 * first, m * 96, hipMemcpyHostToDevice, core_.int_stream));
      launch(first, m);
      DR_HIP(hipGetLastError());
      DR_HIP(hipMemcpyAsync(host.data(), d_out, m * sizeof(Out), hipMemcpyDeviceToHost, core_.int_stream));
      DR_HIP(hipStreamSynchronize(core_.int_stream));
      for (size_t i = 0; i < m; ++i) take(first + i, host[i]);
      if (!counted) continue;
      ++stats[3];
      if (first == 0) stats[2] = host[0].counts[0];
    }
    if (counted) stats[0] = n;
  }
  FusionCore &core_;
  DeviceBuf<unsigned char> buf_;  // sized by the largest call so far
  LocateGrid lg_{};
  int total_ = 0, groups_ = 0;
  size_t chunk_ = 0;
  double *g_ = nullptr, *table_ = nullptr;
  unsigned char *flag_ = nullptr;
  SearchOut *out_ = nullptr;
  float *yf_ = nullptr;              // the colour layout
  SearchColourOut *outc_ = nullptr;
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
    with_score(who, bad, so.step, std::min(n, scorer_.chunk_size()), pair_of(nullptr, h_depth, nullptr, d_depth), false, [&](const unsigned char *, const float *) {
      const std::vector<double> table = plain_table(who, poses16, n);
      scorer_.score(kPlain, table.data(), n, n, so, cost, counts, score);
    });
  }
  void score_colour_poses(const char *who, const uint8_t *h_bgr, const float *h_depth, const void *d_bgr, const void *d_depth, const float *poses16, size_t n,
                          const drf_score_colour_options_t *opt, double *cost, double *photo, uint32_t *counts, double *score) {
    scorer_.reset();
    const FramePair in = pair_of(h_bgr, h_depth, d_bgr, d_depth);
    if (!in.has(true) || !poses16 || !(cost || photo || counts || score)) fail(DR_ERR_ARG, "%s: null argument", who);
    ScoreColourOpt so{};
    const char *bad = score_colour_options(opt, core_.o.truncation_distance, core_.o.voxel_size, so);
    if (!bad && (n == 0 || n > kSearchMaxCandidates)) fail(DR_ERR_ARG, "%s: %zu poses (at least 1, at most 2^24)", who, n);
    with_score(who, bad, so.s.step, std::min(n, scorer_.chunk_size()), in, true, [&](const unsigned char *, const float *) {
      const std::vector<double> table = plain_table(who, poses16, n);
      scorer_.score_colour(kPlain, table.data(), n, n, so, cost, photo, counts, score);
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
    with_score(who, bad, so.s.step, n_anchors * n_rot, pair_of(nullptr, h_depth, nullptr, d_depth), false, [&](const unsigned char *, const float *depth) {
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
  // The search with colour (pose_host.h score_colour_point / search_colour_refine; DESIGN.md §7c "Searching with colour"): the
  // colour score selects, the tracking is the pyramid's with the frame's bgr on the pyramid's side, and the located float poses of
  // the qualifying entries are scored once more, in one plain-table launch, for the winner.
  std::string search_colour_frame(const char *who, const uint8_t *h_bgr, const float *h_depth, const void *d_bgr, const void *d_depth, const float *anchors16,
                                  size_t n_anchors, const double *rotations9, size_t n_rot, const drf_search_colour_options_t *opt,
                                  const drf_track_pyramid_options_t *topt, const drf_locate_options_t *lopt, float *pose16_out, drf_search_colour_result_t *res,
                                  double *all_scores) {
    scorer_.reset();
    const FramePair in = pair_of(h_bgr, h_depth, d_bgr, d_depth);
    if (!in.has(true) || !anchors16 || !rotations9 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    SearchColourOpt so{};
    TrackPyramidOpt po{{}, 1, 0};
    LocateOpt lo;
    const char *bad = search_colour_options(opt, core_.o.truncation_distance, core_.o.voxel_size, so);
    if (!bad) bad = track_pyramid_options(topt, core_.o.voxel_size, core_.o.width, core_.o.height, po);
    if (!bad) bad = locate_options(lopt, core_.o.truncation_distance, lo);
    const size_t n = bad ? 1 : search_count(n_anchors, n_rot, so.s.L);
    if (n == 0) fail(DR_ERR_ARG, "%s: %zu anchors x %zu rotations x %d x %d x %d offsets is no count of candidates (at least 1, at most 2^24)", who, n_anchors, n_rot,
                     so.s.L.N[0], so.s.L.N[1], so.s.L.N[2]);
    drf_search_colour_result_t r;
    // the table holds the search's entries, then the final re-score's poses
    with_score(who, bad, so.s.s.step, std::max(n_anchors * n_rot, (size_t)DRF_SEARCH_MAX_TOP), in, true, [&](const unsigned char *bgr, const float *depth) {
      std::vector<double> table;
      const std::string why = search_table(anchors16, n_anchors, rotations9, n_rot, core_.o.voxel_size, table);
      if (!why.empty()) fail(DR_ERR_ARG, "%s: %s", who, why.c_str());
      std::vector<double> cost(n), photo(n), score(n);
      std::vector<uint32_t> counts(4 * n);
      scorer_.score_colour(so.s.L, table.data(), n_anchors * n_rot, n, so.c, cost.data(), photo.data(), counts.data(), score.data());
      if (all_scores) memcpy(all_scores, score.data(), n * 8);
      const FramePair frame = FramePair::device(bgr, depth);
      FrameTracker::TrackSide &tp = tracker_.pyramid();
      search_colour_refine(so, table.data(), search_select(score.data(), n, so.s.top_k), cost.data(), photo.data(), counts.data(), score.data(), n, core_.o.voxel_size,
                           [&](const float *p16, drf_align_result_t &tr) {
                             tp.reset();
                             uint64_t last[5] = {0, 0, 0, 0, 0};
                             tracker_.track_levels(who, tp, true, po, frame, p16, tr, last);
                             scorer_.stats[4] += tp.stats[4]; scorer_.stats[5] += tp.stats[3];
                           },
                           [&](const float *p16, drf_align_result_t &lr) {
                             locator_.with_locate(who, nullptr, depth, p16, lopt, [&](const LocateOpt &l, auto &eval) { locate_loop(eval, map_motion(p16, core_.o.voxel_size), l, core_.o.voxel_size, lr); });
                             scorer_.stats[5] += locator_.locate_stats()[3];
                           },
                           [&](const float *poses16, size_t nq, double *final_score, double *final_photo) {
                             const std::vector<double> located = plain_table(who, poses16, nq);
                             scorer_.score_colour(kPlain, located.data(), nq, nq, so.c, nullptr, final_photo, nullptr, final_score, false);
                           },
                           pose16_out, r);
    });
    if (res) *res = r;
    if (r.status != DRF_ALIGN_LOST) return std::string();
    return std::string(who) + ": no candidate of the best " + std::to_string(r.n_entries) + " of " + std::to_string((unsigned long long)n) +
           " ended its tracking and its localisation with a pose (the best colour score is " + std::to_string(r.entries[0].score) + " voxels per sample with " +
           std::to_string(r.entries[0].counts[1]) + " of " + std::to_string(r.entries[0].counts[0]) + " samples valid; " + std::to_string(streamer_.store().size()) +
           " blocks are in the host store); pose16_out is the best-scoring candidate";
  }
  void search_stats(uint64_t out[8]) const {
    if (!out) fail(DR_ERR_ARG, "drf_search_stats: null argument");
    for (int i = 0; i < 8; ++i) out[i] = scorer_.stats[i];
  }

 private:
  static constexpr SearchLattice kPlain = {{1, 1, 1}, {0, 0, 0}, 0.0, 1};  // drf_score_*_poses: candidate c is entry c of the table
  // the intake of both families: bgr null is the geometric one (body's bgr is then null)
  template <class Body>
  void with_score(const char *who, const char *bad_option, int step, size_t table_entries, const FramePair &in, bool colour, Body &&body) {
    static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    frame_.frame_prologue(who, bad_option, identity, nullptr);  // the call's poses are many: body refuses them, each by its index
    unsigned char *mine_bgr = nullptr;
    float *mine = scorer_.prepare(step, table_entries, colour ? &mine_bgr : nullptr);
    const float *depth = (const float *)in.depth;
    const unsigned char *bgr = colour ? (const unsigned char *)in.bgr : nullptr;
    if (in.on_host) {
      core_.upload_frame((const uint8_t *)in.bgr, (const float *)in.depth, mine_bgr, mine);
      depth = mine;
      bgr = mine_bgr;
    }
    scorer_.stats[7] = streamer_.store().size();
    try {
      if (colour) scorer_.points_colour(bgr, depth);
      else scorer_.points(depth);
      body(bgr, depth);
    } catch (...) {
      scorer_.reset();
      throw;
    }
  }
  static FramePair pair_of(const void *h_bgr, const float *h_depth, const void *d_bgr, const void *d_depth) {
    return h_depth ? FramePair::host((const uint8_t *)h_bgr, h_depth) : FramePair::device(d_bgr, d_depth);
  }
  // n float poses as a plain table
  std::vector<double> plain_table(const char *who, const float *poses16, size_t n) const {
    std::vector<double> table(n * 12);
    for (size_t i = 0; i < n; ++i) {
      if (const char *why = transform_pose_fault(poses16 + 16 * i)) fail(DR_ERR_ARG, "%s: pose %zu %s", who, i, why);
      const MapMotion m = map_motion(poses16 + 16 * i, core_.o.voxel_size);
      memcpy(&table[12 * i], m.R, 72);
      memcpy(&table[12 * i + 9], m.tv, 24);
    }
    return table;
  }
  FramePose &frame_;
  FusionCore &core_;
  BlockStreamer &streamer_;
  FrameTracker &tracker_;
  FrameLocator &locator_;
  PoseScorer scorer_;  // the score stage and the statistics of both calls
};

}  // namespace dr
