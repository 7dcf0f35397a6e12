// search_ops.h -- drf_score_poses / drf_search_frame and their colour forms (drf_score_colour_poses / drf_search_colour_frame) as two
// components over FusionCore (the rule: pose_host.h score_sample / search_candidate / search_refine; the kernels: search_kernels.h;
// DESIGN.md §7c "Searching a pose lattice", "Searching with colour", "Searching the whole map").  PoseScorer owns the score stage's
// device scratch, the search scope and the statistics of the search calls.  PoseSearch holds it and is the entry points: the
// prologue and the frame's intake (pose_ops.h FramePose), the score, and the refinement composed from FrameTracker::track_levels and FrameLocator::with_locate + locate_loop as
// drf_track_frame and drf_locate_frame run them -- there is no second copy of either loop.  Each of the two has one score and one
// search, a template over the resolved options (pose_host.h: ScoreOpt / ScoreColourOpt, SearchOpt / SearchColourOpt), whose
// family fixes the layout of the scratch, the kernel, the track side and the winner rule.  Included by dr_fusion.hip after
// pose_ops.h.
#pragma once
#include <vector>

#include "fusion_core.h"
#include "map_ops.h"
#include "pose_ops.h"

namespace dr {

class PoseScorer {
 public:
  PoseScorer(FusionCore &core, BlockStreamer &streamer, MapStage &stage) : core_(core), streamer_(streamer), stage_(stage) {}
  uint64_t stats[8] = {};        // drf_search_stats
  uint64_t stage_stats[4] = {};  // drf_search_stage_stats: stagings, the largest in blocks, blocks staged, score launches over a staging
  void reset() {
    for (auto &v : stats) v = 0;
    for (auto &v : stage_stats) v = 0;
  }

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
      if (mine_bgr) out_ = c.take<SearchColourOut>(chunk_);
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
  // k_search_points over the depth image, or given bgr (the colour layout) k_search_points_colour over the image pair (device
  // memory), once per call
  void points(const unsigned char *bgr, const float *depth) {
    const int padded = groups_ * 512;
    if (padded == 0) return;
    const dim3 grid(cdiv(padded, 256)), block(256);
    if (bgr) hipLaunchKernelGGL(k_search_points_colour, grid, block, 0, core_.int_stream, depth, bgr, lg_, (double)core_.o.voxel_size, total_, padded, g_, flag_, yf_);
    else hipLaunchKernelGGL(k_search_points, grid, block, 0, core_.int_stream, depth, lg_, (double)core_.o.voxel_size, total_, padded, g_, flag_);
    DR_HIP(hipGetLastError());
  }
  // Candidates [0, n) of the lattice L in chunks, by k_search_score or (Opt = ScoreColourOpt, over the colour layout)
  // k_search_score_colour; cost, photo (colour only), counts (4 per candidate) and score may each be null.  A plain table (one pose
  // per candidate) is uploaded chunk by chunk, a search's (n_anchors x n_rot entries) once.  counted false: the final re-score of
  // a search, which leaves the candidates, the samples and the chunks of the statistics what the score stage made them.
  // Map scope (drf_set_search_scope; DESIGN.md §7c "Searching the whole map"): the table is planned once (engine_host.h
  // plan_search_stage) -- a plan that does not fit is refused before a candidate is evaluated -- and each pass stages its keys
  // through the map staging, scores its candidates in chunks with the staged kernel and releases the slot behind them, on the
  // throwing path too: the score holds no slot when the refinement starts.  No render reads the staging here: the call is legal only
  // where a scan is, and the device is idle.  A pass without keys, an empty store and the resident scope launch the resident kernel.
  template <class Opt>
  void score(const char *who, const SearchLattice &L, const double *table, size_t table_entries, size_t n, const Opt &so, double *cost, double *photo,
             uint32_t *counts, double *score, bool counted = true) {
    using Out = SearchOutOf<Opt>;
    Out *out = (Out *)out_;
    SearchStagePlan plan;
    if (scope_ == DRF_SEARCH_MAP) {
      plan = plan_search_stage(streamer_.store(), core_.o, table, L, n, stage_.capacity_for_search());
      if (!plan.ok)
        fail(DR_ERR_CAPACITY, "%s: %s can read %zu stored blocks, the search staging holds %zu (drf_set_search_scope with a larger capacity, or drf_stream_in_region)",
             who, L.plain ? "one pose" : "the candidates of one slab of the lattice", plan.too_many, stage_.capacity_for_search());
    } else {
      plan.passes.push_back({0, n, {}});
    }
    std::vector<Out> host(std::min(n, chunk_));
    if (!L.plain) DR_HIP(hipMemcpyAsync(table_, table, table_entries * 96, hipMemcpyHostToDevice, core_.int_stream));
    RenderStage sg{};
    bool staged = false;
    // the slot's flags go back to zero behind the launches that read it (they are on core_.int_stream)
    auto release = [&](bool may_throw) {
      if (!staged) return;
      staged = false;
      hipError_t err = hipEventRecord(stage_.used(), core_.int_stream);
      if (err == hipSuccess) err = hipStreamWaitEvent(stage_.stream(), stage_.used(), 0);
      if (err == hipSuccess) {
        stage_.launch_clear(sg);
        err = hipGetLastError();
      }
      if (may_throw) DR_HIP(err);
    };
    try {
      for (const SearchStagePass &pass : plan.passes) {
        if (!pass.keys.empty()) {
          sg = stage_.stage(pass.keys);
          staged = true;
          stage_.wait_ready(core_.int_stream);
          ++stage_stats[0]; stage_stats[1] = std::max<uint64_t>(stage_stats[1], pass.keys.size()); stage_stats[2] += pass.keys.size();
        }
        for (size_t first = pass.first; first < pass.first + pass.count; first += chunk_) {
          const size_t m = std::min(chunk_, pass.first + pass.count - first), table_first = L.plain ? first : 0;
          if (L.plain) DR_HIP(hipMemcpyAsync(table_, table + 12 * first, m * 96, hipMemcpyHostToDevice, core_.int_stream));
          const dim3 grid(cdiv((int)m, 4)), block(256);
          const double vs = (double)core_.o.voxel_size;
          if constexpr (Opt::colour) {
            if (staged) hipLaunchKernelGGL(k_search_score_colour_staged, grid, block, 0, core_.int_stream, core_.d, g_, flag_, yf_, groups_, table_, L, first, table_first, (int)m, so, vs, out, sg);
            else hipLaunchKernelGGL(k_search_score_colour, grid, block, 0, core_.int_stream, core_.d, g_, flag_, yf_, groups_, table_, L, first, table_first, (int)m, so, vs, out);
          } else {
            if (staged) hipLaunchKernelGGL(k_search_score_staged, grid, block, 0, core_.int_stream, core_.d, g_, flag_, groups_, table_, L, first, table_first, (int)m, so, vs, out, sg);
            else hipLaunchKernelGGL(k_search_score, grid, block, 0, core_.int_stream, core_.d, g_, flag_, groups_, table_, L, first, table_first, (int)m, so, vs, out);
          }
          DR_HIP(hipGetLastError());
          DR_HIP(hipMemcpyAsync(host.data(), out, m * sizeof(Out), hipMemcpyDeviceToHost, core_.int_stream));
          DR_HIP(hipStreamSynchronize(core_.int_stream));
          for (size_t i = 0; i < m; ++i) {
            const Out &o = host[i];
            const size_t c = first + i;
            if (cost) cost[c] = o.cost;
            if constexpr (Opt::colour)
              if (photo) photo[c] = o.photo;
            if (counts) memcpy(counts + 4 * c, o.counts, 16);
            if (score) score[c] = o.score;
          }
          if (staged) ++stage_stats[3];
          if (!counted) continue;
          ++stats[3];
          if (first == 0) stats[2] = host[0].counts[0];
        }
        release(true);
      }
    } catch (...) {
      release(false);
      throw;
    }
    if (counted) stats[0] = n;
  }
  // DRF_SEARCH_RESIDENT: the score reads the pool (the default); DRF_SEARCH_MAP: the pool and the host store together.
  // stage_capacity_blocks bounds what one pass may stage (0 = the render's default); the staging holds the largest need of its users.
  void set_scope(int scope, size_t stage_capacity_blocks) {
    if (scope != DRF_SEARCH_RESIDENT && scope != DRF_SEARCH_MAP) fail(DR_ERR_ARG, "drf_set_search_scope: unknown scope %d", scope);
    if (core_.order.render_pending()) fail(DR_ERR_PROTOCOL, "drf_set_search_scope: a render is pending, call GetRenderResult first");
    scope_ = scope;
    stage_.set_search_need(stage_capacity_blocks, scope == DRF_SEARCH_MAP);
  }

 private:
  FusionCore &core_;
  BlockStreamer &streamer_;
  MapStage &stage_;
  int scope_ = DRF_SEARCH_RESIDENT;  // drf_set_search_scope
  DeviceBuf<unsigned char> buf_;  // sized by the largest call so far
  LocateGrid lg_{};
  int total_ = 0, groups_ = 0;
  size_t chunk_ = 0;
  double *g_ = nullptr, *table_ = nullptr;
  unsigned char *flag_ = nullptr;
  void *out_ = nullptr;   // SearchOut, in the colour layout SearchColourOut, per candidate of a chunk
  float *yf_ = nullptr;   // the colour layout
};

// A depth frame found in the map from many poses.  The score stage is scorer_'s (k_search_points once, k_search_score in chunks, the
// resident map through find_block -- in map scope k_search_score_staged over the passes of a plan, pool and staged blocks together);
// what is added here is the call order -- frame_prologue -- the frame's intake, and the
// refinement: track_levels and with_locate + locate_loop on the device image the score read.  Nothing of the map, the public
// render buffers or the streaming state is written.
class PoseSearch {
 public:
  PoseSearch(FramePose &frame, FrameTracker &tracker, FrameLocator &locator, MapStage &stage)
      : frame_(frame), core_(frame.core), streamer_(frame.streamer), tracker_(tracker), locator_(locator), scorer_(frame.core, frame.streamer, stage) {}
  void score_poses(const char *who, const float *h_depth, const void *d_depth, const float *poses16, size_t n, const drf_score_options_t *opt, double *cost,
                   uint32_t *counts, double *score) {
    score_any(who, pair_of(nullptr, h_depth, nullptr, d_depth), poses16, n, opt, score_options, cost, nullptr, counts, score);
  }
  void score_colour_poses(const char *who, const uint8_t *h_bgr, const float *h_depth, const void *d_bgr, const void *d_depth, const float *poses16, size_t n,
                          const drf_score_colour_options_t *opt, double *cost, double *photo, uint32_t *counts, double *score) {
    score_any(who, pair_of(h_bgr, h_depth, d_bgr, d_depth), poses16, n, opt, score_colour_options, cost, photo, counts, score);
  }
  // returns what dr_last_error() says after a search that ran but found no pose (empty otherwise)
  std::string search_frame(const char *who, const float *h_depth, const void *d_depth, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot,
                           const drf_search_options_t *opt, const drf_track_options_t *topt, const drf_locate_options_t *lopt, float *pose16_out,
                           drf_search_result_t *res, double *all_scores) {
    return search_any(who, pair_of(nullptr, h_depth, nullptr, d_depth), anchors16, n_anchors, rotations9, n_rot, opt, search_options, topt, lopt, pose16_out, res, all_scores);
  }
  // The search with colour (DESIGN.md §7c "Searching with colour"): the colour score selects, the tracking is the pyramid's with
  // the frame's bgr on the pyramid's side, and the located float poses of the qualifying entries are scored once more, in one
  // plain-table launch, for the winner (pose_host.h search_colour_winner).
  std::string search_colour_frame(const char *who, const uint8_t *h_bgr, const float *h_depth, const void *d_bgr, const void *d_depth, const float *anchors16,
                                  size_t n_anchors, const double *rotations9, size_t n_rot, const drf_search_colour_options_t *opt,
                                  const drf_track_pyramid_options_t *topt, const drf_locate_options_t *lopt, float *pose16_out, drf_search_colour_result_t *res,
                                  double *all_scores) {
    return search_any(who, pair_of(h_bgr, h_depth, d_bgr, d_depth), anchors16, n_anchors, rotations9, n_rot, opt, search_colour_options, topt, lopt, pose16_out, res,
                      all_scores);
  }
  void search_stats(uint64_t out[8]) const {
    if (!out) fail(DR_ERR_ARG, "drf_search_stats: null argument");
    for (int i = 0; i < 8; ++i) out[i] = scorer_.stats[i];
  }
  void set_search_scope(int scope, size_t stage_capacity_blocks) { scorer_.set_scope(scope, stage_capacity_blocks); }
  void search_stage_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_search_stage_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = scorer_.stage_stats[i];
  }

 private:
  static constexpr SearchLattice kPlain = {{1, 1, 1}, {0, 0, 0}, 0.0, 1};  // drf_score_*_poses: candidate c is entry c of the table
  // the score calls: resolve is the family's option resolver (Opt: ScoreOpt, or ScoreColourOpt with photo)
  template <class Options, class Opt>
  void score_any(const char *who, const FramePair &in, const float *poses16, size_t n, const Options *opt, const char *(*resolve)(const Options *, float, float, Opt &),
                 double *cost, double *photo, uint32_t *counts, double *score) {
    scorer_.reset();
    if (!in.has(Opt::colour) || !poses16 || !(cost || photo || counts || score)) fail(DR_ERR_ARG, "%s: null argument", who);
    Opt so{};
    const char *bad = resolve(opt, core_.o.truncation_distance, core_.o.voxel_size, so);
    if (!bad && (n == 0 || n > kSearchMaxCandidates)) fail(DR_ERR_ARG, "%s: %zu poses (at least 1, at most 2^24)", who, n);
    with_score(who, bad, so.geo().step, std::min(n, scorer_.chunk_size()), in, Opt::colour, [&](const unsigned char *, const float *) {
      const std::vector<double> table = plain_table(who, poses16, n);
      scorer_.score(who, kPlain, table.data(), n, n, so, cost, photo, counts, score);
    });
  }
  // The searches (Opt: SearchOpt with drf_track_options_t and a drf_search_result_t; SearchColourOpt with
  // drf_track_pyramid_options_t and a drf_search_colour_result_t).  The family fixes the track options and the track side, whether
  // the frame's bgr is read, the room of the pose table and the winner rule.
  template <class Options, class Opt, class TrackOptions, class Result>
  std::string search_any(const char *who, const FramePair &in, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot, const Options *opt,
                         const char *(*resolve)(const Options *, float, float, Opt &), const TrackOptions *topt, const drf_locate_options_t *lopt, float *pose16_out,
                         Result *res, double *all_scores) {
    constexpr bool colour = Opt::colour;
    scorer_.reset();
    if (!in.has(colour) || !anchors16 || !rotations9 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    Opt so{};
    TrackPyramidOpt po{{}, 1, 0};
    LocateOpt lo;
    const char *bad = resolve(opt, core_.o.truncation_distance, core_.o.voxel_size, so);
    if constexpr (colour) {
      if (!bad) bad = track_pyramid_options(topt, core_.o.voxel_size, core_.o.width, core_.o.height, po);
    } else {
      if (!bad) bad = FrameTracker::track_options_of(topt, core_.o.voxel_size, po.c);
    }
    if (!bad) bad = locate_options(lopt, core_.o.truncation_distance, lo);
    const SearchLattice &L = so.search().L;
    const size_t entries = n_anchors * n_rot, n = bad ? 1 : search_count(n_anchors, n_rot, L);
    if (n == 0) fail(DR_ERR_ARG, "%s: %zu anchors x %zu rotations x %d x %d x %d offsets is no count of candidates (at least 1, at most 2^24)", who, n_anchors, n_rot,
                     L.N[0], L.N[1], L.N[2]);
    Result r;
    // with colour the table holds the search's entries, then the final re-score's poses
    with_score(who, bad, so.score().geo().step, colour ? std::max(entries, (size_t)DRF_SEARCH_MAX_TOP) : entries, in, colour, [&](const unsigned char *bgr, const float *depth) {
      std::vector<double> table;
      const std::string why = search_table(anchors16, n_anchors, rotations9, n_rot, core_.o.voxel_size, table);
      if (!why.empty()) fail(DR_ERR_ARG, "%s: %s", who, why.c_str());
      std::vector<double> cost(n), photo(colour ? n : 0), score(n);
      std::vector<uint32_t> counts(4 * n);
      scorer_.score(who, L, table.data(), entries, n, so.score(), cost.data(), photo.data(), counts.data(), score.data());
      if (all_scores) memcpy(all_scores, score.data(), n * 8);
      const FramePair frame = FramePair::device(bgr, depth);
      FrameTracker::TrackSide &side = colour ? tracker_.pyramid() : tracker_.geometric();
      search_refine(so, table.data(), search_select(score.data(), n, so.search().top_k), cost.data(), photo.data(), counts.data(), score.data(), n, core_.o.voxel_size,
                    [&](const float *p16, drf_align_result_t &tr) {
                      side.reset();
                      uint64_t last[5] = {0, 0, 0, 0, 0};
                      tracker_.track_levels(who, side, colour, po, frame, p16, tr, last);
                      scorer_.stats[4] += side.stats[4]; scorer_.stats[5] += side.stats[3];
                    },
                    [&](const float *p16, drf_align_result_t &lr) {
                      locator_.with_locate(who, nullptr, depth, p16, lopt, [&](const LocateOpt &l, auto &eval) { locate_loop(eval, map_motion(p16, core_.o.voxel_size), l, core_.o.voxel_size, lr); });
                      scorer_.stats[5] += locator_.locate_stats()[3];
                    },
                    [&](Result &rr, const int *qual, int nq) {
                      if constexpr (colour) {
                        return search_colour_winner(rr, qual, nq, [&](const float *poses16, size_t m, double *final_score, double *final_photo) {
                          const std::vector<double> located = plain_table(who, poses16, m);
                          scorer_.score(who, kPlain, located.data(), m, m, so.score(), nullptr, final_photo, nullptr, final_score, false);
                        });
                      } else {
                        return search_winner(rr, qual, nq);
                      }
                    },
                    pose16_out, r);
    });
    if (res) *res = r;
    if (r.status != DRF_ALIGN_LOST) return std::string();
    return std::string(who) + ": no candidate of the best " + std::to_string(r.n_entries) + " of " + std::to_string((unsigned long long)n) +
           " ended its tracking and its localisation with a pose (the best " + (colour ? "colour score" : "score") + " is " + std::to_string(r.entries[0].score) +
           " voxels per sample with " + std::to_string(r.entries[0].counts[1]) + " of " + std::to_string(r.entries[0].counts[0]) + " samples valid; " +
           std::to_string(streamer_.store().size()) + " blocks are in the host store); pose16_out is the best-scoring candidate";
  }
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
      scorer_.points(bgr, depth);
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
