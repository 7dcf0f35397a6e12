// pose_ops.h -- a camera pose from a frame, as components over FusionCore: drf_locate_*, drf_track_*, drf_track_colour_*,
// drf_track_pyramid_*, drf_track_exposure_* (the rules: pose_host.h; the kernels: locate_kernels.h, track_kernels.h,
// track_colour_kernels.h, track_pyramid_kernels.h, track_exposure_kernels.h, k_align_fold of align_kernels.h; DESIGN.md "Where the frame-pose code lives", "Where rendering and the
// frame pose live").  FramePose is what the families open with, written once; FrameLocator is the localisation with its scope over
// the map staging (render_ops.h MapStage) and the restaging rule (engine_host.h LocateStageCursor); FrameTracker the three tracking
// families, whose model render goes through MapRenderer's plan_render_call and render_passes.  Of the call order they only ask
// expect_integrate; the public render slots, their double buffers and the render statistics are not touched.  Everything runs on
// the integration stream.  Included by dr_fusion.hip after render_ops.h; search_ops.h composes the pose search from the two.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "fusion_core.h"
#include "fusion_host.h"
#include "map_ops.h"
#include "render_ops.h"
#include "stream_ops.h"

namespace dr {

// A (bgr, depth) image pair of the engine's camera as a tracking call is given it: both on the host, or both on the device.
// bgr null: the depth alone.
struct FramePair {
  const void *bgr, *depth;
  bool on_host;
  static FramePair host(const uint8_t *bgr, const float *depth) { return {bgr, depth, true}; }
  static FramePair device(const void *bgr, const void *depth) { return {bgr, depth, false}; }
  bool has(bool colour) const { return depth && (!colour || bgr); }  // the images a call with or without colour reads
};

// the sample grid of a call and what a launch over it needs; max_groups (step = 1) sizes the scratch once for every step
struct FrameGrid { LocateGrid lg; int total, groups; size_t max_groups; };

// What the families open with, written once, and what they share of the engine: the core, the streamer (the host store, settle)
// and the map-file transport (MapIo: the pinned pair behind evaluate).
struct FramePose {
  FramePose(FusionCore &core_, BlockStreamer &streamer_, MapIo &mio_) : core(core_), streamer(streamer_), mio(mio_) {}
  FusionCore &core;
  BlockStreamer &streamer;
  MapIo &mio;
  // frame_prologue: the refusals in their one order -- the options (bad_option: what the family's resolver returned), the call
  // order, blocks in the host store while streaming is off, the pose, the model pose (the *_system calls of the tracking) -- then
  // pending work settled.
  void frame_prologue(const char *who, const char *bad_option, const float *pose16, const float *model_pose16) const {
    if (bad_option) fail(DR_ERR_ARG, "%s: option %s is negative or not finite", who, bad_option);
    core.order.expect_integrate(who);
    if (!streamer.on() && !streamer.store().empty())
      fail(DR_ERR_PROTOCOL, "%s: %zu blocks are in the host store while streaming is off; bring them back with drf_stream_in_region first", who, streamer.store().size());
    if (const char *why = transform_pose_fault(pose16)) fail(DR_ERR_ARG, "%s: the pose %s", who, why);
    if (model_pose16)
      if (const char *why = transform_pose_fault(model_pose16)) fail(DR_ERR_ARG, "%s: the model pose %s", who, why);
    streamer.settle();  // behind any pending scan; the pinned buffers are idle and every eviction is in the host store
  }
  FrameGrid frame_grid(int step) const {
    const LocateGrid lg = locate_grid(core.o, step);
    return {lg, (int)locate_positions(lg), (int)locate_groups(lg), (core.npix + 511) / 512};
  }
};

// A depth frame located in the map this engine holds (the rule: pose_host.h locate_pixel / align_point; DESIGN.md §7c "Locating a
// depth frame in the map").  The map is read where it lives, through find_block; nothing of it is uploaded, changed or allocated.
class FrameLocator {
 public:
  FrameLocator(FramePose &frame, MapStage &stage) : frame_(frame), core_(frame.core), streamer_(frame.streamer), mio_(frame.mio), stage_(stage) {}
  // with_locate does what both calls share -- the prologue, device scratch that is sized once -- and hands body an evaluator:
  // k_map_locate + k_align_fold on core_.int_stream, 28 doubles and 4 counters back through the pinned pair.
  template <class Body>
  void with_locate(const char *who, const float *h_depth, const void *d_depth, const float *pose16, const drf_locate_options_t *opt, Body &&body) {
    locate_reset();
    LocateOpt lo;
    frame_.frame_prologue(who, locate_options(opt, core_.o.truncation_distance, lo), pose16, nullptr);
    const FrameGrid fg = frame_.frame_grid(lo.step);
    const LocateGrid &lg = fg.lg;
    const int total = fg.total, groups = fg.groups;
    double *partial = nullptr;
    unsigned long long *counts = nullptr;
    float *mine = nullptr;  // a host-given depth image
    carve(lc_buf_, core_.int_stream, [&](Carver &c) {
      partial = c.take<double>(fg.max_groups * 28);
      counts = c.take<unsigned long long>(4);
      mine = c.take<float>(core_.npix);
    });
    mio_.ensure(1);
    // Map scope (drf_set_locate_scope): the stored blocks an evaluation at the pose can read go through the map staging -- no
    // render reads it here: the call is legal only where a scan is, and the device is idle.  The cursor says how long a staging
    // serves the poses that follow, and what to stage when it no longer does; with an empty store or an empty selection nothing
    // is staged and the resident kernel is launched.
    const bool map_scope = locate_scope_ == DRF_LOCATE_MAP;
    double slack = locate_stage_slack(core_.o);
    if (const char *env = hook_env("DR_LOCATE_STAGE_SLACK")) slack = std::min(slack, std::max(0.0, atof(env)) * (double)core_.o.voxel_size);  // parity hook, in voxels
    LocateStageCursor cursor(streamer_.store(), core_.o, slack, stage_.capacity_for_locate());
    RenderStage sg{};
    bool staged = false;
    if (map_scope) {  // the refusal: decided at the first pose, before anything is evaluated
      float p16[16];
      locate_pose16(map_motion(pose16, core_.o.voxel_size), core_.o.voxel_size, p16);
      const LocateStageCursor::Step s = cursor.begin(p16);
      if (s.kind == LocateStageCursor::kTooMany)
        fail(DR_ERR_CAPACITY, "%s: the pose can read %zu stored blocks, the locate staging holds %zu (drf_set_locate_scope with a larger capacity, or drf_stream_in_region)",
             who, s.count, stage_.capacity_for_locate());
    }
    const float *depth = (const float *)d_depth;
    if (h_depth) {
      core_.upload_frame(nullptr, h_depth, nullptr, mine);
      depth = mine;
    }
    lc_stats_[0] = (uint64_t)total; lc_stats_[4] = lc_buf_.capacity(); lc_stats_[5] = streamer_.store().size();
    // the slot's flags go back to zero behind the evaluations that read it (they are on core_.int_stream)
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
    auto eval = [&](const AlignEval &e, double sums[28], uint64_t c4[4]) {
      if (map_scope) {
        float p16[16];
        locate_pose16(e.m, core_.o.voxel_size, p16);
        const LocateStageCursor::Step s = cursor.at(p16);
        if (s.kind == LocateStageCursor::kTooMany)
          fail(DR_ERR_CAPACITY, "%s: a pose of the refinement can read %zu stored blocks, the locate staging holds %zu (drf_set_locate_scope with a larger capacity, or drf_stream_in_region)",
               who, s.count, stage_.capacity_for_locate());
        if (s.kind == LocateStageCursor::kStage) {
          release(true);
          if (s.count) {
            sg = stage_.stage(cursor.keys());
            staged = true;
            ++ls_stats_[0]; ls_stats_[1] = std::max<uint64_t>(ls_stats_[1], s.count); ls_stats_[2] += s.count;
          }
        }
      }
      mio_.evaluate(partial, groups, counts, 4, sums, c4, [&] {
        if (staged) {
          stage_.wait_ready(core_.int_stream);
          hipLaunchKernelGGL(k_map_locate_staged, dim3(cdiv(groups, 4)), dim3(256), 0, core_.int_stream, core_.d, depth, lg, e, groups, total, partial, counts, sg);
        } else {
          hipLaunchKernelGGL(k_map_locate, dim3(cdiv(groups, 4)), dim3(256), 0, core_.int_stream, core_.d, depth, lg, e, groups, total, partial, counts);
        }
        DR_HIP(hipGetLastError());
      });
      lc_stats_[1] = c4[0]; lc_stats_[2] = c4[1]; ++lc_stats_[3];
      if (staged) ++ls_stats_[3];
    };
    try {
      body(lo, eval);
    } catch (...) {
      release(false);
      locate_reset();
      throw;
    }
    release(true);
  }
  void locate_system(const char *who, const float *h_depth, const void *d_depth, const float *pose16, const drf_locate_options_t *opt, double *sums,
                     uint64_t *counts) {
    locate_reset();
    if (!(h_depth || d_depth) || !pose16 || !sums || !counts) fail(DR_ERR_ARG, "%s: null argument", who);
    with_locate(who, h_depth, d_depth, pose16, opt, [&](const LocateOpt &lo, auto &eval) {
      double c_src[3];
      locate_centre_src(lo.centre_depth, core_.o.voxel_size, c_src);
      eval(align_eval(map_motion(pose16, core_.o.voxel_size), c_src, lo.a, core_.o.voxel_size), sums, counts);
    });
  }
  // returns what dr_last_error() says after a refinement that ran but found no pose (empty otherwise)
  std::string locate_frame(const char *who, const float *h_depth, const void *d_depth, const float *pose16, const drf_locate_options_t *opt, float *pose16_out,
                           drf_align_result_t *res) {
    locate_reset();
    if (!(h_depth || d_depth) || !pose16 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    drf_align_result_t r;
    uint64_t c4[4] = {0, 0, 0, 0};
    with_locate(who, h_depth, d_depth, pose16, opt, [&](const LocateOpt &lo, auto &eval) { locate_loop(eval, map_motion(pose16, core_.o.voxel_size), lo, core_.o.voxel_size, r, c4); });
    for (int i = 0; i < 16; ++i) pose16_out[i] = (float)r.T[i];
    if (res) *res = r;
    return no_pose_note(std::string(who) + ": the refinement", r,
                        ", " + std::to_string((unsigned long long)c4[2]) + " unobserved, " + std::to_string((unsigned long long)c4[3]) + " outside the band; " +
                            std::to_string(streamer_.store().size()) + " blocks are in the host store" +
                            (locate_scope_ == DRF_LOCATE_MAP ? ", " + std::to_string((unsigned long long)ls_stats_[1]) + " of them staged" : std::string()) + ")");
  }
  const uint64_t *locate_stats() const { return lc_stats_; }
  // DRF_LOCATE_RESIDENT: drf_locate_* read the pool (the default); DRF_LOCATE_MAP: the pool and the host store together.
  // stage_capacity_blocks bounds what one evaluation may stage (0 = the render's default); the staging holds the larger of the two needs.
  void set_locate_scope(int scope, size_t stage_capacity_blocks) {
    if (scope != DRF_LOCATE_RESIDENT && scope != DRF_LOCATE_MAP) fail(DR_ERR_ARG, "drf_set_locate_scope: unknown scope %d", scope);
    if (core_.order.render_pending()) fail(DR_ERR_PROTOCOL, "drf_set_locate_scope: a render is pending, call GetRenderResult first");
    locate_scope_ = scope;
    stage_.set_locate_need(stage_capacity_blocks, scope == DRF_LOCATE_MAP);
  }
  void locate_stage_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_locate_stage_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = ls_stats_[i];
  }

 private:
  void locate_reset() {
    for (auto &v : lc_stats_) v = 0;
    for (auto &v : ls_stats_) v = 0;
  }
  FramePose &frame_;
  FusionCore &core_;
  BlockStreamer &streamer_;
  MapIo &mio_;
  MapStage &stage_;
  DeviceBuf<unsigned char> lc_buf_;            // drf_locate_*: partial sums, counters and a host-given depth image (sized once)
  uint64_t lc_stats_[6] = {0, 0, 0, 0, 0, 0};  // drf_locate_stats
  int locate_scope_ = DRF_LOCATE_RESIDENT;     // drf_set_locate_scope
  uint64_t ls_stats_[4] = {0, 0, 0, 0};        // drf_locate_stage_stats
};

// A frame tracked against the ray-cast model: by its depth alone (drf_track_*; DESIGN.md §7c "Tracking a depth frame against the
// ray-cast model"), with the photometric term (drf_track_colour_*; "Tracking with colour"), coarse to fine (drf_track_reduce,
// drf_track_pyramid_*; "Tracking coarse to fine"), or with the frame's gain and offset beside the pose (drf_track_exposure_*;
// "Tracking under a change of exposure").  The rule: pose_host.h track_normal / track_point / track_colour_point /
// track_loop and track_level_grid / track_reduce_host / track_pyramid_schedule.  One path for the three families (what it
// guarantees: DESIGN.md "Where the frame-pose code lives").  Every launch is given its level, and level 0 is the single-level
// call (track_level_grid returns the grid itself), so drf_track_* and drf_track_colour_* are the schedule with one level; colour
// is a run-time flag.  What differs is the side -- tk_, tc_ or tp_: each family its own scratch, in its own layout, its own
// statistics and model render, so a call of one family leaves the others' statistics and buffers what they were -- and what each
// entry does itself: its null arguments, its options, its refusal texts.
class FrameTracker {
 public:
  FrameTracker(FramePose &frame, MapRenderer &renderer) : frame_(frame), core_(frame.core), streamer_(frame.streamer), mio_(frame.mio), renderer_(renderer) {}
  struct TrackSide {
    DeviceBuf<unsigned char> buf;             // sized once
    uint64_t stats[8] = {};                   // drf_track_stats / drf_track_colour_stats (the first six), drf_track_pyramid_stats
    uint64_t level[kTrackMaxLevels][4] = {};  // drf_track_pyramid_level_stats
    Render render{};                          // the *_frame call's full-resolution model render: core_.int_stream and pointers into buf
    void reset() { memset(stats, 0, sizeof stats); memset(level, 0, sizeof level); }
  };
  TrackSide &geometric() { return tk_; }  // drf_search_frame tracks its candidates on the side of drf_track_frame
  TrackSide &pyramid() { return tp_; }    // drf_search_colour_frame on the side of drf_track_pyramid_frame
  // The body of every *_frame call: the frame reduced once to every level above 0, then track_pyramid_schedule over track_loop;
  // po.levels = 1 is the single-level call.  r: level 0's result; last: the counters of its last evaluation.
  // x: null, or the exposure of drf_track_exposure_frame -- the solver's state beside the pose (pose_host.h ExposureState): it
  // carries from level to level, and an abandoned level hands on the one it started from.
  void track_levels(const char *who, TrackSide &s, bool colour, const TrackPyramidOpt &po, const FramePair &frame, const float *pose16, drf_align_result_t &r,
                    uint64_t last[5], ExposureState *x = nullptr) {
    with_track(who, s, colour, frame, po.c.t.step, [&](TrackCall &t) {
      for (int L = 1; L < po.levels; ++L) launch_reduce(t.b.depth, t.b.bgr, L, track_level_options(po, L).t.max_jump, t.b.pyr[L], t.b.pyr_bgr[L]);
      track_pyramid_schedule([&](int L, const float *p16, const TrackColourOpt &lo, drf_align_result_t &lr, uint64_t *lc, uint64_t *st2) {
        auto render = [&](const float *p) { track_render(t, L, lo, p); };
        auto eval = [&](const AlignEval &e, const float *mp16, double sums[28], uint64_t *c) {
          if (x) track_evaluate_exposure(t, L, lo, e, mp16, *x, sums, c);
          else track_evaluate(t, L, lo, e, mp16, sums, c);
        };
        if (x) {
          x->level_begin();
          track_loop<5>(render, eval, p16, lo.t, core_.o.voxel_size, lr, lc, st2, nullptr, x);
          if (L > 0 && (lr.status == DRF_ALIGN_LOST || lr.status == DRF_ALIGN_DEGENERATE)) x->level_abandoned();
        } else if (colour) {
          track_loop<5>(render, eval, p16, lo.t, core_.o.voxel_size, lr, lc, st2);
        } else {
          track_loop<4>(render, eval, p16, lo.t, core_.o.voxel_size, lr, lc, st2);
        }
      }, t.fg.lg, pose16, po, r, s.stats, s.level, last);
    });
  }
  // The single-level families: Options is drf_track_options_t (geometric: every bgr is null) or drf_track_colour_options_t.
  static const char *track_options_of(const drf_track_options_t *u, float voxel_size, TrackColourOpt &o) { o.photo_weight = 0.0f; return track_options(u, voxel_size, o.t); }
  static const char *track_options_of(const drf_track_colour_options_t *u, float voxel_size, TrackColourOpt &o) { return track_colour_options(u, voxel_size, o); }
  template <class Options>
  void track_system(const char *who, const FramePair &frame, const FramePair &model, const float *model_pose16, const float *pose16, const Options *opt, double *sums,
                    uint64_t *counts) {
    constexpr bool colour = std::is_same<Options, drf_track_colour_options_t>::value;
    TrackSide &s = colour ? tc_ : tk_;
    s.reset();
    if (!frame.has(colour) || !model.has(colour) || !model_pose16 || !pose16 || !sums || !counts) fail(DR_ERR_ARG, "%s: null argument", who);
    TrackPyramidOpt po{{}, 1, 0};
    frame_.frame_prologue(who, track_options_of(opt, core_.o.voxel_size, po.c), pose16, model_pose16);
    track_system_at(who, s, colour, 0, po, frame, model, model_pose16, pose16, sums, counts, colour ? 5 : 4);
  }
  template <class Options>
  std::string track_frame(const char *who, const FramePair &frame, const float *pose16, const Options *opt, float *pose16_out, drf_align_result_t *res) {
    constexpr bool colour = std::is_same<Options, drf_track_colour_options_t>::value;
    TrackSide &s = colour ? tc_ : tk_;
    s.reset();
    if (!frame.has(colour) || !pose16 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    TrackPyramidOpt po{{}, 1, 0};
    frame_.frame_prologue(who, track_options_of(opt, core_.o.voxel_size, po.c), pose16, nullptr);
    drf_align_result_t r;
    uint64_t last[5] = {0, 0, 0, 0, 0};
    track_levels(who, s, colour, po, frame, pose16, r, last);
    return track_note(who, s, r, last, colour ? ", " + std::to_string((unsigned long long)last[4]) + " with a colour term; " : std::string("; "), pose16_out, res);
  }
  const uint64_t *track_stats() const { return tk_.stats; }
  const uint64_t *track_colour_stats() const { return tc_.stats; }

  // The pyramid family: colour is decided by the images given (bgr null: the geometric kernels).
  // the reduction alone: a host pair through the scratch, or device images in place
  void track_reduce(const char *who, int level, float max_jump, const FramePair &in, void *bgr_out, void *depth_out) {
    tp_.reset();
    if (!in.depth || !depth_out || (in.bgr && !bgr_out)) fail(DR_ERR_ARG, "%s: null argument", who);
    if (!(max_jump >= 0.0f) || !std::isfinite(max_jump)) fail(DR_ERR_ARG, "%s: option max_jump is negative or not finite", who);
    if (!track_level_fits(core_.o.width, core_.o.height, level))
      fail(DR_ERR_ARG, "%s: level %d is outside 0..%d or below %d pixels on a side of the %dx%d camera", who, level, kTrackMaxLevels - 1, kTrackMinLevelSide, core_.o.height,
           core_.o.width);
    core_.order.expect_integrate(who);
    streamer_.settle();
    if (in.on_host) {
      const size_t nl = (size_t)(core_.o.width >> level) * (size_t)(core_.o.height >> level);
      TrackBufs b = track_spans(tp_);
      track_intake(b, in.bgr != nullptr, in);
      launch_reduce(b.depth, b.bgr, level, max_jump, b.model, b.model_bgr);  // the model's full-resolution spans hold any level
      DR_HIP(hipMemcpyAsync(depth_out, b.model, nl * 4, hipMemcpyDeviceToHost, core_.int_stream));
      if (in.bgr) DR_HIP(hipMemcpyAsync(bgr_out, b.model_bgr, nl * 3, hipMemcpyDeviceToHost, core_.int_stream));
    } else {
      launch_reduce((const float *)in.depth, (const unsigned char *)in.bgr, level, max_jump, (float *)depth_out, (unsigned char *)bgr_out);
    }
    DR_HIP(hipStreamSynchronize(core_.int_stream));
    tp_.stats[5] = tp_.buf.capacity();
  }
  // one evaluation at `level` (without colour counts[4] = 0)
  void track_pyramid_system(const char *who, int level, const FramePair &frame, const FramePair &model, const float *model_pose16, const float *pose16,
                            const drf_track_pyramid_options_t *opt, double *sums, uint64_t *counts) {
    tp_.reset();
    const bool colour = frame.bgr != nullptr;
    if (!frame.depth || !model.has(colour) || !model_pose16 || !pose16 || !sums || !counts) fail(DR_ERR_ARG, "%s: null argument", who);
    const TrackPyramidOpt po = track_pyramid_resolve(who, opt, &level);
    frame_.frame_prologue(who, nullptr, pose16, model_pose16);
    track_system_at(who, tp_, colour, level, po, frame, model, model_pose16, pose16, sums, counts, 5);
  }
  std::string track_pyramid_frame(const char *who, const FramePair &frame, const float *pose16, const drf_track_pyramid_options_t *opt, float *pose16_out,
                                  drf_align_result_t *res) {
    tp_.reset();
    if (!frame.depth || !pose16 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    const TrackPyramidOpt po = track_pyramid_resolve(who, opt, nullptr);
    frame_.frame_prologue(who, nullptr, pose16, nullptr);
    drf_align_result_t r;
    uint64_t last[5] = {0, 0, 0, 0, 0};
    track_levels(who, tp_, frame.bgr != nullptr, po, frame, pose16, r, last);
    return track_note(who, tp_, r, last,
                      "; " + std::to_string((unsigned long long)tp_.stats[6]) + " levels, " + std::to_string((unsigned long long)tp_.stats[7]) + " abandoned, ", pose16_out, res);
  }
  const uint64_t *track_pyramid_stats() const { return tp_.stats; }
  const uint64_t *track_pyramid_level_stats(int level) const {
    if (level < 0 || level >= kTrackMaxLevels) fail(DR_ERR_ARG, "drf_track_pyramid_level_stats: level %d is outside 0..%d", level, kTrackMaxLevels - 1);
    return tp_.level[level];
  }

  // The exposure family (DESIGN.md §7c "Tracking under a change of exposure"): the pyramid's calls with colour and the exposure in
  // the solver's state, on a side of their own.  The colour images are judged behind the options.
  void track_exposure_system(const char *who, int level, const FramePair &frame, const FramePair &model, const float *model_pose16, const float *pose16, double gain,
                             double offset, const drf_track_exposure_options_t *opt, double *sums, uint64_t *counts) {
    te_.reset();
    if (!frame.depth || !model.depth || !model_pose16 || !pose16 || !sums || !counts) fail(DR_ERR_ARG, "%s: null argument", who);
    const TrackExposureOpt xo = track_exposure_resolve(who, opt, &level);
    if (!frame.bgr || !model.bgr) fail(DR_ERR_ARG, "%s: bgr is null: the call needs the colour images", who);
    if (!std::isfinite(gain) || !std::isfinite(offset)) fail(DR_ERR_ARG, "%s: the exposure (%g, %g) is not finite", who, gain, offset);
    frame_.frame_prologue(who, nullptr, pose16, model_pose16);
    ExposureState x(xo);
    x.gain = gain; x.offset = offset;
    double pose_sums[28];
    track_system_at(who, te_, true, level, xo.p, frame, model, model_pose16, pose16, pose_sums, counts, 5, &x);
    memcpy(sums, pose_sums, sizeof pose_sums);
    memcpy(sums + 28, x.ext, sizeof x.ext);
  }
  std::string track_exposure_frame(const char *who, const FramePair &frame, const float *pose16, const drf_track_exposure_options_t *opt, float *pose16_out,
                                   drf_exposure_result_t *res) {
    te_.reset();
    if (!frame.depth || !pose16 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    const TrackExposureOpt xo = track_exposure_resolve(who, opt, nullptr);
    if (!frame.bgr) fail(DR_ERR_ARG, "%s: bgr is null: the call needs the colour image", who);
    frame_.frame_prologue(who, nullptr, pose16, nullptr);
    ExposureState x(xo);
    drf_align_result_t r;
    uint64_t last[5] = {0, 0, 0, 0, 0};
    track_levels(who, te_, true, xo.p, frame, pose16, r, last, &x);
    if (res) exposure_result(r, x, last, *res);
    return track_note(who, te_, r, last,
                      "; " + std::to_string((unsigned long long)te_.stats[6]) + " levels, " + std::to_string((unsigned long long)te_.stats[7]) + " abandoned, ", pose16_out, nullptr);
  }
  const uint64_t *track_exposure_stats() const { return te_.stats; }
  const uint64_t *track_exposure_level_stats(int level) const {
    if (level < 0 || level >= kTrackMaxLevels) fail(DR_ERR_ARG, "drf_track_exposure_level_stats: level %d is outside 0..%d", level, kTrackMaxLevels - 1);
    return te_.level[level];
  }

 private:
  // with_track does what the calls share behind the prologue -- device scratch that is sized once, the frame's intake, the
  // statistics reset when an exception passes -- and hands body the call: the spans and what track_launch_model, track_evaluate
  // (k_track or k_track_colour + k_align_fold on core_.int_stream; k_align_fold hands back four counters, the photometric terms added
  // leave through a pinned word) and track_render need.  The model's render goes through the renderer's one submit (render_passes)
  // on core_.int_stream into the scratch; the public render slots, the call order and the render statistics are not touched.
  struct TrackBufs {  // the spans; a layout leaves null what it does not have
    double *partial; unsigned long long *counts; int *flag; TrackPixel *map;
    float *model, *level, *Ym, *frame, *pyr[kTrackMaxLevels];  // the full-resolution model, its level, Ym, a host-given frame, the frame's levels >= 1
    unsigned char *model_bgr, *level_bgr, *frame_bgr, *pyr_bgr[kTrackMaxLevels];
    unsigned char *render_bgr; RayState *render_band;  // where the model's render puts its colour image and a banded render's ray state
    const float *depth; const unsigned char *bgr;      // the frame at full resolution: the caller's device images, or the spans a host frame went to
  };
  struct TrackCall { const char *who; TrackSide &s; bool colour; FrameGrid fg; TrackBufs b; };
  // The layouts (DESIGN.md "What the carver guarantees").  What of a render nobody reads once the model kernel runs may lie
  // in the bytes that kernel then overwrites with the model map: a banded render's per-pixel ray state in both single-level
  // layouts, and in the geometric one the colour image too (with colour k_track_model_colour reads it: it has the span model_bgr).
  // The pyramid's is sized for five levels with nothing aliased; the exposure's is the pyramid's with 45 doubles per group.
  TrackBufs track_spans(TrackSide &s) {
    TrackBufs b{};
    const size_t max_groups = frame_.frame_grid(1).max_groups;
    auto head = [&](Carver &c, size_t counters, size_t width = 28) {
      b.partial = c.take<double>(max_groups * width);
      b.counts = c.take<unsigned long long>(counters);  // four that k_align_fold hands back; with colour the fifth (and one unused)
      b.flag = c.take<int>(1);                          // the ray-cast's flag counter
      b.map = c.take<TrackPixel>(core_.npix, 32);            // the model map
    };
    if (&s == &tk_) {
      carve(s.buf, core_.int_stream, [&](Carver &c) {
        head(c, 4);
        b.model = c.take<float>(core_.npix);  // the model's depth: rendered, or a host-given one
        b.frame = c.take<float>(core_.npix);
        b.render_bgr = (unsigned char *)b.map;
        b.render_band = (RayState *)((unsigned char *)b.map + core_.npix * 8);
      });
    } else if (&s == &tc_) {
      carve(s.buf, core_.int_stream, [&](Carver &c) {
        head(c, 6);
        b.model = c.take<float>(core_.npix);
        b.Ym = c.take<float>(core_.npix);
        b.frame = c.take<float>(core_.npix);
        b.model_bgr = c.take<unsigned char>(core_.npix * 3);
        b.frame_bgr = c.take<unsigned char>(core_.npix * 3);
        b.render_bgr = b.model_bgr;
        b.render_band = (RayState *)b.map;
      });
    } else {
      auto level_pixels = [&](int L) { return std::max<size_t>(1, (size_t)(core_.o.width >> L) * (size_t)(core_.o.height >> L)); };
      carve(s.buf, core_.int_stream, [&](Carver &c) {
        head(c, 6, &s == &te_ ? 45 : 28);
        b.render_band = c.take<RayState>(core_.npix, 8);
        b.model = c.take<float>(core_.npix);
        b.level = c.take<float>(level_pixels(1));
        b.Ym = c.take<float>(core_.npix);
        b.frame = c.take<float>(core_.npix);
        for (int L = 1; L < kTrackMaxLevels; ++L) b.pyr[L] = c.take<float>(level_pixels(L));
        b.model_bgr = c.take<unsigned char>(core_.npix * 3);
        b.level_bgr = c.take<unsigned char>(level_pixels(1) * 3);
        b.frame_bgr = c.take<unsigned char>(core_.npix * 3);
        for (int L = 1; L < kTrackMaxLevels; ++L) b.pyr_bgr[L] = c.take<unsigned char>(level_pixels(L) * 3);
        b.render_bgr = b.model_bgr;
      });
    }
    return b;
  }
  // the frame: device images where they lie, or a host pair (without colour: the depth alone) through upload_frame into the spans
  void track_intake(TrackBufs &b, bool colour, const FramePair &frame) {
    b.depth = (const float *)frame.depth;
    b.bgr = (const unsigned char *)frame.bgr;
    if (!frame.on_host) return;
    core_.upload_frame((const uint8_t *)frame.bgr, (const float *)frame.depth, colour ? b.frame_bgr : nullptr, b.frame);
    b.depth = b.frame;
    b.bgr = colour ? b.frame_bgr : nullptr;
  }
  template <class Body>
  void with_track(const char *who, TrackSide &s, bool colour, const FramePair &frame, int step, Body &&body) {
    TrackCall t{who, s, colour, frame_.frame_grid(step), track_spans(s)};
    if (colour && !tc_fifth_) tc_fifth_ = core_.own.pinned<unsigned long long>(1);
    mio_.ensure(1);
    track_intake(t.b, colour, frame);
    s.stats[5] = s.buf.capacity();
    try {
      body(t);
    } catch (...) {
      s.reset();
      throw;
    }
  }
  void launch_reduce(const float *depth, const unsigned char *bgr, int L, float max_jump, float *depth_out, unsigned char *bgr_out) {
    const int WL = core_.o.width >> L, HL = core_.o.height >> L;
    const int threads = (WL * HL) << L;  // at most width * height
    hipLaunchKernelGGL(k_track_reduce, dim3(cdiv(threads, 256)), dim3(256), 0, core_.int_stream, depth, bgr, core_.o.width, WL, HL, L, max_jump, depth_out, bgr_out);
    DR_HIP(hipGetLastError());
  }
  // level L's model map (with colour: and Ym) from a full-resolution model pair, reduced to the level first above level 0.  The
  // geometric kernels never read bgr_m: in the geometric layout the render's colour image lies in the model map.
  void track_launch_model(const TrackCall &t, const float *depth_m, const unsigned char *bgr_m, int L, const TrackColourOpt &lo) {
    const LocateGrid lg = track_level_grid(t.fg.lg, L);
    if (L > 0) {
      launch_reduce(depth_m, t.colour ? bgr_m : nullptr, L, lo.t.max_jump, t.b.level, t.b.level_bgr);
      depth_m = t.b.level; bgr_m = t.b.level_bgr;
    }
    const int np = lg.W * lg.H;
    if (t.colour) hipLaunchKernelGGL(k_track_model_colour, dim3(cdiv(np, 256)), dim3(256), 0, core_.int_stream, depth_m, bgr_m, lg, lo.t.max_jump, t.b.map, t.b.Ym);
    else hipLaunchKernelGGL(k_track_model, dim3(cdiv(np, 256)), dim3(256), 0, core_.int_stream, depth_m, lg, lo.t.max_jump, t.b.map);
    DR_HIP(hipGetLastError());
  }
  // one evaluation of level L against the model map; c[5] with colour, c[4] without
  void track_evaluate(const TrackCall &t, int L, const TrackColourOpt &lo, const AlignEval &e, const float *model_pose16, double sums[28], uint64_t *c) {
    const TrackBufs &b = t.b;
    const LocateGrid lg = track_level_grid(t.fg.lg, L);
    const int total = (int)locate_positions(lg), groups = (int)locate_groups(lg);
    const float *fd = L == 0 ? b.depth : b.pyr[L];
    const unsigned char *fc = L == 0 ? b.bgr : b.pyr_bgr[L];
    const TrackModel tm = track_model(model_pose16, lo.t, core_.o.voxel_size, b.map);
    mio_.evaluate(b.partial, groups, b.counts, 4, sums, c, [&] {
      if (t.colour) {
        DR_HIP(hipMemsetAsync(b.counts + 4, 0, 8, core_.int_stream));
        hipLaunchKernelGGL(k_track_colour, dim3(cdiv(groups, 4)), dim3(256), 0, core_.int_stream, fd, fc, lg, e, tm, track_colour(lo, b.Ym), groups, total, b.partial, b.counts);
        DR_HIP(hipGetLastError());
        DR_HIP(hipMemcpyAsync(tc_fifth_, b.counts + 4, 8, hipMemcpyDeviceToHost, core_.int_stream));
      } else {
        hipLaunchKernelGGL(k_track, dim3(cdiv(groups, 4)), dim3(256), 0, core_.int_stream, fd, lg, e, tm, groups, total, b.partial, b.counts);
        DR_HIP(hipGetLastError());
      }
    });
    if (t.colour) c[4] = *tc_fifth_;
  }
  // one evaluation of level L under the exposure x: 45 sums and five counters back through the pair; the loop is handed the 28 of
  // the pose, the 17 others are left in x.ext for its step
  void track_evaluate_exposure(const TrackCall &t, int L, const TrackColourOpt &lo, const AlignEval &e, const float *model_pose16, ExposureState &x, double sums[28],
                               uint64_t c[5]) {
    const TrackBufs &b = t.b;
    const LocateGrid lg = track_level_grid(t.fg.lg, L);
    const int total = (int)locate_positions(lg), groups = (int)locate_groups(lg);
    const float *fd = L == 0 ? b.depth : b.pyr[L];
    const unsigned char *fc = L == 0 ? b.bgr : b.pyr_bgr[L];
    const TrackModel tm = track_model(model_pose16, lo.t, core_.o.voxel_size, b.map);
    double s45[45];
    mio_.evaluate_exposure(b.partial, groups, b.counts, s45, c, [&] {
      hipLaunchKernelGGL(k_track_exposure, dim3(cdiv(groups, 4)), dim3(256), 0, core_.int_stream, fd, fc, lg, e, tm, track_colour(lo, b.Ym), x.at(), groups, total, b.partial,
                         b.counts);
      DR_HIP(hipGetLastError());
    });
    memcpy(sums, s45, 28 * sizeof(double));
    memcpy(x.ext, s45 + 28, sizeof x.ext);
  }
  // the model of a *_frame round: the renderer's one submit at full resolution into the spans, then level L's model map
  void track_render(const TrackCall &t, int L, const TrackColourOpt &lo, const float *pose16) {
    Render &rd = t.s.render;
    if (!rd.cast) { rd.cast = core_.own.event(); rd.done = core_.own.event(); }
    rd.stream = core_.int_stream;
    rd.d_bgr = t.b.render_bgr;
    rd.d_band = t.b.render_band;
    rd.d_depth = t.b.model;
    rd.d_flag = t.b.flag;
    RenderStagePlan plan;
    RenderBandPlan bands;
    bool waited = false;
    const float *poses[1] = {pose16};
    renderer_.plan_render_call(t.who, poses, 1, plan, bands, waited);
    renderer_.render_passes(plan, bands, &rd, poses, 1, false);
    track_launch_model(t, t.b.model, t.b.model_bgr, L, lo);
  }
  // The body of every *_system call: one evaluation at `level` against a full-resolution model pair the caller gives, n counters
  // out.  A host-given model goes through upload_frame into the spans.  A device-given one is read in place by the single-level
  // calls and copied into the spans by the pyramid's: track_launch_model could read that one in place too, but the copy is part
  // of what drf_track_pyramid_system_device enqueues, and stays.
  void track_system_at(const char *who, TrackSide &s, bool colour, int level, const TrackPyramidOpt &po, const FramePair &frame, const FramePair &model,
                       const float *model_pose16, const float *pose16, double *sums, uint64_t *counts, int n, ExposureState *x = nullptr) {
    with_track(who, s, colour, frame, po.c.t.step, [&](TrackCall &t) {
      const TrackBufs &b = t.b;
      const TrackColourOpt lo = track_level_options(po, level);
      if (level > 0) launch_reduce(b.depth, b.bgr, level, lo.t.max_jump, b.pyr[level], b.pyr_bgr[level]);
      const float *depth_m = b.model;
      const unsigned char *bgr_m = b.model_bgr;
      if (model.on_host) {
        core_.upload_frame((const uint8_t *)model.bgr, (const float *)model.depth, colour ? b.model_bgr : nullptr, b.model, true);
      } else if (&s == &tp_) {
        DR_HIP(hipMemcpyAsync(b.model, model.depth, core_.npix * 4, hipMemcpyDeviceToDevice, core_.int_stream));
        if (colour) DR_HIP(hipMemcpyAsync(b.model_bgr, model.bgr, core_.npix * 3, hipMemcpyDeviceToDevice, core_.int_stream));
      } else {
        depth_m = (const float *)model.depth; bgr_m = (const unsigned char *)model.bgr;
      }
      track_launch_model(t, depth_m, bgr_m, level, lo);
      double c_src[3];
      locate_centre_src(lo.t.centre_depth, core_.o.voxel_size, c_src);
      uint64_t c[5] = {0, 0, 0, 0, 0};
      const AlignEval e = align_eval(map_motion(pose16, core_.o.voxel_size), c_src, lo.t.a, core_.o.voxel_size);
      if (x) track_evaluate_exposure(t, level, lo, e, model_pose16, *x, sums, c);
      else track_evaluate(t, level, lo, e, model_pose16, sums, c);
      for (int i = 0; i < n; ++i) counts[i] = c[i];
      s.stats[0] = (uint64_t)locate_positions(track_level_grid(t.fg.lg, level)); s.stats[1] = c[0]; s.stats[2] = c[1]; s.stats[3] = 1; s.stats[6] = 1;
      s.level[level][2] = 1; s.level[level][3] = c[1];
    });
  }
  // hands out the pose and returns what dr_last_error() says after a tracking that ran but found no pose (empty otherwise)
  std::string track_note(const char *who, const TrackSide &s, const drf_align_result_t &r, const uint64_t last[5], const std::string &own, float *pose16_out,
                         drf_align_result_t *res) {
    for (int i = 0; i < 16; ++i) pose16_out[i] = (float)r.T[i];
    if (res) *res = r;
    return no_pose_note(std::string(who) + ": the tracking", r,
                        ", " + std::to_string((unsigned long long)last[2]) + " unassociated, " + std::to_string((unsigned long long)last[3]) + " rejected" + own +
                            std::to_string((unsigned long long)s.stats[4]) + " renders; " + std::to_string(streamer_.store().size()) + " blocks are in the host store)");
  }
  // level null: drf_track_pyramid_frame; otherwise the level of a drf_track_pyramid_system, judged with the options.
  TrackPyramidOpt track_pyramid_resolve(const char *who, const drf_track_pyramid_options_t *opt, const int *level) {
    TrackPyramidOpt po;
    if (const char *bad = track_pyramid_options(opt, core_.o.voxel_size, core_.o.width, core_.o.height, po))
      fail(DR_ERR_ARG, "%s: option %s is negative, not finite or out of range (levels <= %d, every level at least %d pixels on a side)", who, bad, kTrackMaxLevels,
           kTrackMinLevelSide);
    if (level && !track_level_fits(core_.o.width, core_.o.height, *level))
      fail(DR_ERR_ARG, "%s: level %d is outside 0..%d or below %d pixels on a side of the %dx%d camera", who, *level, kTrackMaxLevels - 1, kTrackMinLevelSide, core_.o.height,
           core_.o.width);
    return po;
  }
  // level null: drf_track_exposure_frame; otherwise the level of a drf_track_exposure_system, judged with the options.
  TrackExposureOpt track_exposure_resolve(const char *who, const drf_track_exposure_options_t *opt, const int *level) {
    TrackExposureOpt xo;
    if (const char *bad = track_exposure_options(opt, core_.o.voxel_size, core_.o.width, core_.o.height, xo))
      fail(DR_ERR_ARG, "%s: option %s is negative, not finite or out of range (levels <= %d, every level at least %d pixels on a side; gain_min <= gain_init <= gain_max, |offset_init| <= 765)",
           who, bad, kTrackMaxLevels, kTrackMinLevelSide);
    if (level && !track_exposure_level_fits(core_.o.width, core_.o.height, *level))
      fail(DR_ERR_ARG, "%s: level %d is outside 0..%d or below %d pixels on a side of the %dx%d camera", who, *level, kTrackMaxLevels - 1, kTrackMinLevelSide, core_.o.height,
           core_.o.width);
    return xo;
  }

  FramePose &frame_;
  FusionCore &core_;
  BlockStreamer &streamer_;
  MapIo &mio_;
  MapRenderer &renderer_;
  TrackSide tk_, tc_, tp_, te_;             // drf_track_*, drf_track_colour_*, drf_track_reduce / drf_track_pyramid_*, drf_track_exposure_*: each its own scratch, statistics and model render (with_track)
  unsigned long long *tc_fifth_ = nullptr;  // pinned: the fifth counter of an evaluation with colour
};

}  // namespace dr
