// render_ops.h -- the ray-cast renders of DrFusion as two components over FusionCore (the kernels: raycast_kernels.h, k_publish in
// volume_kernels.h; the host rules: fusion_host.h; DESIGN.md §7c "Rendering the whole map", "Rendering beyond the staging").
// MapStage is the staging of host-stored blocks for the kernels that read them on the device; it has four readers -- map-scope
// renders, the tracking's model render (both through MapRenderer::render_passes), the locate scope (pose_ops.h FrameLocator) and the
// search scope (search_ops.h PoseScorer) -- and states its capacity rule and its slot release once.  MapRenderer owns the render slots, the one submit, the render scope, the
// depth bands, their statistics and the parity build's ray-cast switches.  Included by dr_fusion.hip after stream_ops.h.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>

#include "fusion_core.h"
#include "fusion_host.h"
#include "stream_ops.h"

namespace dr {

// rs_ carries [keys | voxels]; each of its two slots has a table and staged superblock flags of its own.  Everything that touches a
// slot on the device is ordered on rs_'s stream: copy, table clear, k_rs_build, and -- behind the readers of the slot -- k_rs_clear.
// Opened by the first staging, grown up to the larger need of its users.
class MapStage {
 public:
  MapStage(FusionCore &core, BlockStreamer &streamer) : core_(core), streamer_(streamer) {}
  // what its users may stage at a time, in blocks (0 = min(num_blocks, kStageBlocks)); the locate and the search scope count only
  // while they are on
  void set_render_need(size_t blocks) { rs_cap_req_ = blocks; }
  void set_locate_need(size_t blocks, bool on) { lc_cap_req_ = blocks; lc_on_ = on; }
  void set_search_need(size_t blocks, bool on) { sc_cap_req_ = blocks; sc_on_ = on; }
  size_t capacity_for_render() const { return rs_cap_req_ ? rs_cap_req_ : (size_t)std::min(core_.o.num_blocks, kStageBlocks); }
  size_t capacity_for_locate() const { return lc_cap_req_ ? lc_cap_req_ : (size_t)std::min(core_.o.num_blocks, kStageBlocks); }
  size_t capacity_for_search() const { return sc_cap_req_ ? sc_cap_req_ : (size_t)std::min(core_.o.num_blocks, kStageBlocks); }
  void ensure(size_t n) {
    if (!rs_.stream()) {
      rs_.open(core_.own);
      for (auto &f : rs_super_)
        for (int l = 0; l < kSuperLevels; ++l) f[l] = core_.own.device<unsigned char>((size_t)1 << (3 * (kGridBits - kSuperShift[l])), rs_.stream());
    }
    if (n <= rs_blocks_) return;
    size_t cap = capacity_for_render();  // the largest need of its three users
    if (lc_on_) cap = std::max(cap, capacity_for_locate());
    if (sc_on_) cap = std::max(cap, capacity_for_search());
    const size_t want = std::min(cap, std::max(2 * rs_blocks_, (n + 1023) & ~(size_t)1023));
    DR_HIP(hipDeviceSynchronize());  // no copy or kernel reads the old allocations
    rs_.reserve((want + 1) * 8 + want * 4096);
    for (auto &t : rs_table_) t.reserve(stage_table_slots(want), rs_.stream());
    rs_blocks_ = want;
  }
  // the stored blocks `keys` packed into the next slot, copied, indexed; the readers wait_ready() before they launch
  RenderStage stage(const std::vector<unsigned long long> &keys) {
    const size_t n = keys.size(), nk = (n + 1) & ~(size_t)1;  // voxels start 16-byte aligned
    ensure(n);
    unsigned char *h = rs_.next();
    streamer_.pack_stored(keys.data(), n, h, h + nk * 8);
    if (nk > n) memset(h + n * 8, 0xFF, 8);
    RenderStage sg{};
    sg.keys = (const unsigned long long *)rs_.dev();
    sg.vox = (const Voxel *)(rs_.dev() + nk * 8);
    sg.table = rs_table_[rs_.slot()].get(); sg.tmask = (unsigned)(stage_table_slots(n) - 1);
    sg.super[0] = rs_super_[rs_.slot()][0]; sg.super[1] = rs_super_[rs_.slot()][1];
    sg.n = (int)n;
    for (size_t k = 0; k < n; ++k) {
      int c[3]; unpack_key_host(keys[k], c);
      constexpr int G = 1 << (kGridBits - 1);
      for (int a = 0; a < 3; ++a) if (c[a] < -G || c[a] >= G) sg.far = 1;
    }
    rs_.copy(nk * 8 + n * 4096);
    DR_HIP(hipMemsetAsync(rs_table_[rs_.slot()].get(), 0, ((size_t)sg.tmask + 1) * 8, rs_.stream()));
    hipLaunchKernelGGL(k_rs_build, dim3(cdiv(sg.n, 256)), dim3(256), 0, rs_.stream(), sg.keys, sg.n, rs_table_[rs_.slot()].get(), sg.tmask,
                       rs_super_[rs_.slot()][0], rs_super_[rs_.slot()][1]);
    DR_HIP(hipGetLastError());
    rs_.record_ready();
    return sg;
  }
  // The current slot's release: its flags go back to zero, on the staging's stream.  The one launch of k_rs_clear.  The caller has
  // put the stream behind the slot's readers (wait_for their events) and asks hipGetLastError() behind it, each in its own way.
  void launch_clear(const RenderStage &sg) {
    hipLaunchKernelGGL(k_rs_clear, dim3(cdiv(sg.n, 256)), dim3(256), 0, rs_.stream(), sg.keys, sg.n, rs_super_[rs_.slot()][0], rs_super_[rs_.slot()][1]);
  }
  void wait_ready(hipStream_t consumer) { rs_.wait_ready(consumer); }  // a reader's stream behind the current slot's staging
  void wait_for(hipEvent_t e) { rs_.wait_for(e); }                     // the staging's stream behind a reader
  hipStream_t stream() const { return rs_.stream(); }
  hipEvent_t used() const { return rs_.used(); }  // the current slot's: for a reader with one event for all its kernels

 private:
  // slots of an open-addressing table over n staged blocks: a power of two, at least twice their number
  static size_t stage_table_slots(size_t n) { size_t s = 1024; while (s < 2 * n) s <<= 1; return s; }
  FusionCore &core_;
  BlockStreamer &streamer_;
  BlockStaging rs_;
  DeviceBuf<unsigned long long> rs_table_[2];  // per slot of rs_: the open-addressing table and the two staged superblock flag arrays
  unsigned char *rs_super_[2][2] = {};
  size_t rs_cap_req_ = 0, lc_cap_req_ = 0, sc_cap_req_ = 0, rs_blocks_ = 0;
  bool lc_on_ = false, sc_on_ = false;
};

// One render slot: a stream, the device images, the double-buffered pinned results, the two events.  MapRenderer owns the public
// ones; a tracking side fills one in over its scratch for its model render.
struct Render {
  hipStream_t stream;
  unsigned char *d_bgr, *h_bgr[2], *hd_bgr[2];   // hd_*: the pinned result buffers as the device addresses them
  float *d_depth, *h_depth[2], *hd_depth[2];
  int *d_flag;  // pixels the fast ray-caster handed to the literal pass
  RayState *d_band = nullptr;  // per-pixel state of a depth-banded render (allocated by the first one)
  hipEvent_t done, cast;  // result on the host / ray-cast kernels finished (the volume may be written again)
};

class MapRenderer {
 public:
  MapRenderer(FusionCore &core, BlockStreamer &streamer, MapStage &stage) : core_(core), streamer_(streamer), stage_(stage) {}
  // the render slots, on streams of the given priority (the engine's constructor); their cast events to core.casts
  void open(int priority) {
    for (int i = 0; i < core_.o.num_render_streams; ++i) {
      Render r;
      r.stream = core_.own.stream(priority);
      r.d_bgr = core_.own.device<unsigned char>(core_.npix * 3);
      r.d_depth = core_.own.device<float>(core_.npix);
      r.d_flag = core_.own.device<int>(4);
      for (int k = 0; k < 2; ++k) {  // double-buffered host results ("blocked"/"free", tsdf_volume.cu:846-872)
        r.h_bgr[k] = core_.own.pinned<unsigned char>(core_.npix * 3, &r.hd_bgr[k]);
        r.h_depth[k] = core_.own.pinned<float>(core_.npix, &r.hd_depth[k]);
      }
      r.done = core_.own.event();
      r.cast = core_.own.event();
      renders_.push_back(r);
      core_.casts.push_back(r.cast);
    }
  }
  int slots() const { return (int)renders_.size(); }
  // bench_sequence: the buffers NOT handed out last become the ones written, and one resident render on slot i
  void flip() { free_slot_ ^= 1; }
  void submit(int i, const Mat &P, hipEvent_t *timing) { submit_render(renders_[i], P, nullptr, timing); }

  // tsdf_volume.cu:634-700
  void render_async(const float *const *poses, int n) {
    // (a map that was loaded or merged may be rendered before its next scan: drf_load_map, drf_merge_map)
    core_.order.expect_render("Please call the functions like IntegrateScanAsync -> RenderAsync -> GetRenderResult.");
    if (n != (int)renders_.size()) fail(DR_ERR_PROTOCOL, "Can only render exactly as many poses as streams. Streams: %zu, Poses: %d.", renders_.size(), n);
    DR_HIP(hipSetDevice(core_.device));
    // map scope: the stored blocks these poses can read, decided before anything changes (DR_ERR_CAPACITY leaves all as it was)
    RenderStagePlan plan;
    RenderBandPlan bands;
    bool waited = false;
    if (render_scope_ == DRF_RENDER_MAP)
      for (int i = 0; i < n; ++i) if (!poses[i]) fail(DR_ERR_ARG, "RenderAsync: null pose");
    plan_render_call("RenderAsync", poses, n, plan, bands, waited);
    core_.order.render_begun();
    free_slot_ ^= 1;  // write into the buffers NOT handed out by the last GetRenderResult
    const PassStats ps = render_passes(plan, bands, renders_.data(), poses, n, true);
    render_stats_[0] = plan.keys.size(); render_stats_[1] = ps.total * (size_t)(8 + 4096);
    render_stats_[2] = (uint64_t)plan.whole; render_stats_[3] = waited ? 1 : 0;
    band_stats_[0] = ps.staged ? ps.passes : 0; band_stats_[1] = ps.largest; band_stats_[2] = ps.total; band_stats_[3] = bands.ok ? 1 : 0;
  }
  // What a render of these poses stages (drf_render_async, and drf_track_frame for its model): in the resident scope nothing; in
  // the map scope the union of the stored blocks in reach, or depth bands of it, or DR_ERR_CAPACITY before anything changes.
  void plan_render_call(const char *who, const float *const *poses, int n, RenderStagePlan &plan, RenderBandPlan &bands, bool &waited) {
    if (render_scope_ != DRF_RENDER_MAP) return;
    plan = plan_render(poses, n, waited);
    if (!render_stage_fits(plan, stage_.capacity_for_render())) {
      // depth bands (drf_set_render_bands): the union may exceed the staging as long as every band fits it
      if (render_bands_ >= 2) bands = plan_render_bands(streamer_.store(), core_.o, poses, n, stage_.capacity_for_render(), render_bands_);
      if (!bands.ok)
        fail(DR_ERR_CAPACITY, "%s: the poses can read %zu stored blocks, the render staging holds %zu (drf_set_render_scope%s)", who, plan.keys.size(),
             stage_.capacity_for_render(), render_bands_ >= 2 ? "; no plan of depth bands within drf_set_render_bands either" : "");
    }
#ifdef DR_PARITY_HOOKS
    if (!plan.keys.empty() && (raycast_v1_ || raycast_stats_ || raycast_sampler_ == 0))
      fail(DR_ERR_UNSUPPORTED, "%s: the superseded ray-cast generations have no staged form (DRF_RENDER_MAP with stored blocks in reach)", who);
#endif
  }
  // The planned render on the n streams of rs, pose i on rs[i]; handoff: the result goes to the host behind the last pass
  // (drf_render_async), otherwise it stays in rs[i]'s device buffers (drf_track_frame's model).
  struct PassStats { size_t passes, largest, total; bool staged; };
  PassStats render_passes(const RenderStagePlan &plan, const RenderBandPlan &bands, Render *rs, const float *const *poses, int n, bool handoff) {
    const bool staged = !plan.keys.empty();  // nothing to stage: exactly the resident launches
    // One pass stages the union; a banded render one depth band after the other.  The two slots of the staging alternate, so band
    // j + 1 is packed and copied while band j ray-casts; all render streams take a band together and share its staging.
    const size_t passes = bands.ok ? bands.keys.size() : 1;
    size_t largest = 0, total = 0;
    for (size_t j = 0; j < passes; ++j) {
      const std::vector<unsigned long long> &keys = bands.ok ? bands.keys[j] : plan.keys;
      largest = std::max(largest, keys.size());
      total += keys.size();
    }
    if (bands.ok) stage_.ensure(largest);  // (grown once, before the first band is in flight)
    for (size_t j = 0; j < passes; ++j) {
      RenderStage sg{};
      if (staged) sg = stage_.stage(bands.ok ? bands.keys[j] : plan.keys);
      RenderBand band{};
      band.z_hi = bands.ok ? bands.z[j + 1] : 0.0f;
      band.first = j == 0;
      for (int i = 0; i < n; ++i) {
        Mat P; memcpy(P.m, poses[i], 64);
        submit_render(rs[i], P, staged ? &sg : nullptr, nullptr, bands.ok ? &band : nullptr, handoff && j + 1 == passes);
      }
      if (staged) {  // behind every ray-cast that read the slot: its flags go back to zero
        for (int i = 0; i < n; ++i) stage_.wait_for(rs[i].cast);
        stage_.launch_clear(sg);
        DR_HIP(hipGetLastError());  // (per band: the launches of its ray-casts included)
      }
    }
    return PassStats{passes, largest, total, staged};
  }
  // Depth bands of map-scope renders: max_passes 0 or 1 = off (the default), 2..64 = a RenderAsync whose union exceeds the
  // staging may run in up to that many bands.
  void set_render_bands(int max_passes) {
    if (max_passes < 0 || max_passes > 64) fail(DR_ERR_ARG, "drf_set_render_bands: max_passes %d is not within 0..64", max_passes);
    if (core_.order.render_pending()) fail(DR_ERR_PROTOCOL, "drf_set_render_bands: a render is pending, call GetRenderResult first");
    render_bands_ = max_passes;
  }
  void render_band_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_render_band_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = band_stats_[i];
  }
  // DRF_RENDER_RESIDENT: renders read the pool (the default); DRF_RENDER_MAP: the pool and the host store together.
  // stage_capacity_blocks bounds the staging (0 = min(num_blocks, kStageBlocks)).
  void set_render_scope(int scope, size_t stage_capacity_blocks) {
    if (scope != DRF_RENDER_RESIDENT && scope != DRF_RENDER_MAP) fail(DR_ERR_ARG, "drf_set_render_scope: unknown scope %d", scope);
    if (core_.order.render_pending()) fail(DR_ERR_PROTOCOL, "drf_set_render_scope: a render is pending, call GetRenderResult first");
    render_scope_ = scope;
    stage_.set_render_need(stage_capacity_blocks);
  }
  void render_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_render_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = render_stats_[i];
  }
  // tsdf_volume.cu:702-737
  void get_render_result(uint8_t **bgr, float **depth, int n) {
    core_.order.expect(CallOrder::kGetRender, "Please call the functions in a loop: IntegrateScanAsync -> RenderAsync -> GetRenderResult.");
    if (n != (int)renders_.size()) fail(DR_ERR_ARG, "GetRenderResult: expected %zu outputs", renders_.size());
    core_.order.result_fetched();
    DR_HIP(hipSetDevice(core_.device));
    for (int i = 0; i < n; ++i) {
      DR_HIP(hipEventSynchronize(renders_[i].done));
      bgr[i] = renders_[i].h_bgr[free_slot_];
      depth[i] = renders_[i].h_depth[free_slot_];
    }
    core_.check_device_flags();
  }
  // Device-resident result of render stream i (the buffers GetRenderResult copies from): valid from GetRenderResult
  // until the next RenderAsync.  Lets a consumer on the same GPU (the coarse tracker's dense-depth hand-off) skip the
  // D2H + H2D round trip.
  void get_render_device(int i, const uint8_t **d_bgr, const float **d_depth) {
    if (i < 0 || i >= (int)renders_.size()) fail(DR_ERR_ARG, "get_render_device: stream %d of %zu", i, renders_.size());
    if (!core_.order.scan_may_come()) fail(DR_ERR_PROTOCOL, "get_render_device: call after GetRenderResult");
    if (d_bgr) *d_bgr = renders_[i].d_bgr;
    if (d_depth) *d_depth = renders_[i].d_depth;
  }
  // Test hook: the page-locked host copies of the last (back = 0) and the second-to-last (back = 1) ray-cast of render stream i that
  // bench_sequence wrote -- the second-to-last one ran BESIDE the allocation of the last scan (enqueue_scan), which is what a test of
  // that overlap has to look at.
  void bench_render_host(int i, int back, const uint8_t **bgr, const float **depth) {
    if (i < 0 || i >= (int)renders_.size() || back < 0 || back > 1) fail(DR_ERR_ARG, "bench_render_host: stream %d of %zu, back %d", i, renders_.size(), back);
    DR_HIP(hipSetDevice(core_.device));
    DR_HIP(hipDeviceSynchronize());
    const int slot = free_slot_ ^ back;
    if (bgr) *bgr = renders_[i].h_bgr[slot];
    if (depth) *depth = renders_[i].h_depth[slot];
  }

 private:
  // The product's ray-cast: the flag counter cleared, the two-round-trip sampler (SAMPLER 0: round 2's, parity build), the literal pass
  // for the pixels it flagged.  The staging is a trailing pack as in the kernels: none = resident, one RenderStage = staged, a
  // RenderBand behind it = one depth band of a staged render (the flag counter is cleared before the first band only).
  template <int SAMPLER, class... SG>
  void raycast_pass(hipStream_t st, unsigned char *d_bgr, float *d_depth, int *d_flag, const Mat &P, bool zero_flag, const SG &...stage) {
    constexpr bool STAGED = sizeof...(SG) != 0, BANDED = sizeof...(SG) == 2;
    const dim3 grid(8 * cdiv(cdiv((int)core_.npix, 64), 8)), block(64);
    if (zero_flag) hipLaunchKernelGGL(k_zero_int, dim3(1), dim3(1), 0, st, d_flag);
    FusionDev dv = core_.d;
    if (raycast_no_skip_) dv.super[0] = nullptr;  // DR_RAYCAST_NO_SKIP=1: every sample is looked up (A/B and parity hook)
    if (core_.d.fast_div) hipLaunchKernelGGL((k_raycast2<true, false, SAMPLER, STAGED, BANDED>), grid, block, 0, st, dv, P, d_bgr, d_depth, d_flag, (unsigned long long *)nullptr, stage...);
    else hipLaunchKernelGGL((k_raycast2<false, false, SAMPLER, STAGED, BANDED>), grid, block, 0, st, dv, P, d_bgr, d_depth, d_flag, (unsigned long long *)nullptr, stage...);
    hipLaunchKernelGGL((k_raycast_fix<STAGED, BANDED>), dim3(512), dim3(64), 0, st, core_.d, P, d_bgr, d_depth, d_flag, stage...);
  }
  // sg: the host blocks staged for this render (map scope with stored blocks in reach), nullptr = the resident kernels;
  // band: this launch is one depth band of the render (sg is then that band's staging)
  void launch_raycast(hipStream_t st, unsigned char *d_bgr, float *d_depth, int *d_flag, const Mat &P, const RenderStage *sg = nullptr,
                      const RenderBand *band = nullptr) {
#ifdef DR_PARITY_HOOKS  // the superseded generations have no staged form (plan_render_call refuses them)
    const dim3 grid(8 * cdiv(cdiv((int)core_.npix, 64), 8)), block(64);
    if (raycast_v1_) { hipLaunchKernelGGL(k_raycast, grid, block, 0, st, core_.d, P, d_bgr, d_depth); return; }
    if (raycast_stats_ && core_.d.fast_div) {  // DR_RAYCAST_STATS=1: a synchronous, counting launch of the same loop (prints to stderr)
      hipLaunchKernelGGL(k_zero_int, dim3(1), dim3(1), 0, st, d_flag);
      FusionDev dv = core_.d;
      if (raycast_no_skip_) dv.super[0] = nullptr;
      if (!d_rstats_) d_rstats_ = core_.own.device<unsigned long long>(32);
      DR_HIP(hipMemsetAsync(d_rstats_, 0, 32 * 8, st));
      hipLaunchKernelGGL((k_raycast2<true, true>), grid, block, 0, st, dv, P, d_bgr, d_depth, d_flag, d_rstats_);
      unsigned long long h[32];
      DR_HIP(hipMemcpyAsync(h, d_rstats_, sizeof h, hipMemcpyDeviceToHost, st));
      DR_HIP(hipStreamSynchronize(st));
      fprintf(stderr, "raycast stats: waves %llu  iterations/lane %.1f  longest ray %llu  mean wave-longest %.1f | per lane: missing-block samples %.1f, full samples %.1f, skip events %.2f (%.1f steps)\n  wave-longest histogram (x16):",
              h[7], (double)h[0] / (64.0 * h[7]), h[1], (double)h[2] / h[7], (double)h[3] / (64.0 * h[7]), (double)h[6] / (64.0 * h[7]), (double)h[4] / (64.0 * h[7]), (double)h[5] / (64.0 * h[7]));
      for (int i = 0; i < 24; ++i) fprintf(stderr, " %llu", h[8 + i]);
      fprintf(stderr, "\n");
      hipLaunchKernelGGL(k_raycast_fix<false>, dim3(512), dim3(64), 0, st, core_.d, P, d_bgr, d_depth, d_flag);
      return;
    }
    if (raycast_sampler_ == 0) return raycast_pass<0>(st, d_bgr, d_depth, d_flag, P, true);  // DR_RAYCAST_SAMPLER=0: the four-stage sampler of round 2
#endif
    if (band) raycast_pass<1>(st, d_bgr, d_depth, d_flag, P, band->first != 0, *sg, *band);
    else if (sg) raycast_pass<1>(st, d_bgr, d_depth, d_flag, P, true, *sg);
    else raycast_pass<1>(st, d_bgr, d_depth, d_flag, P, true);
  }
  // One render on its stream, behind the scan: ray-cast (sg: the staged host blocks it also reads, behind their staging), `cast`,
  // hand-off to the host (k_publish; DR_RENDER_D2H=copy, parity build: the two hipMemcpyAsync of round 2), `done`.
  // timing: three events around the ray-cast and the hand-off (bench_sequence).
  // band: one depth band of the render -- z_hi and `first` given, the stream's state filled in here; the hand-off follows the
  // last band only (`cast` is recorded behind every band: the staging stream waits for it before it takes the band's flags back).
  void submit_render(Render &r, const Mat &P, const RenderStage *sg, hipEvent_t *timing = nullptr, const RenderBand *band = nullptr, bool last = true) {
    if (!band || band->first) DR_HIP(hipStreamWaitEvent(r.stream, core_.int_done, 0));
    if (sg) stage_.wait_ready(r.stream);
    if (timing) DR_HIP(hipEventRecord(timing[0], r.stream));
    if (band) {
      if (!r.d_band) r.d_band = core_.own.device<RayState>(core_.npix);
      RenderBand b = *band;
      b.state = r.d_band;
      launch_raycast(r.stream, r.d_bgr, r.d_depth, r.d_flag, P, sg, &b);
    } else
      launch_raycast(r.stream, r.d_bgr, r.d_depth, r.d_flag, P, sg);
    if (timing) DR_HIP(hipEventRecord(timing[1], r.stream));
    DR_HIP(hipEventRecord(r.cast, r.stream));
    if (!last) return;
    if (render_copy_) {
      DR_HIP(hipMemcpyAsync(r.h_bgr[free_slot_], r.d_bgr, core_.npix * 3, hipMemcpyDeviceToHost, r.stream));
      DR_HIP(hipMemcpyAsync(r.h_depth[free_slot_], r.d_depth, core_.npix * 4, hipMemcpyDeviceToHost, r.stream));
    } else
      hipLaunchKernelGGL(k_publish, dim3(128), dim3(256), 0, r.stream, (const unsigned char *)r.d_depth, (unsigned char *)r.hd_depth[free_slot_], core_.npix * 4,
                         (const unsigned char *)r.d_bgr, r.hd_bgr[free_slot_], core_.npix * 3);
    if (timing) DR_HIP(hipEventRecord(timing[2], r.stream));
    DR_HIP(hipEventRecord(r.done, r.stream));
  }
  // The union of stored blocks the poses can read.  Blocks the last scan's eviction chain gathered are not in the store yet: only
  // a pose that could reach one (render_needs_fold) waits for the scan and folds them first.
  RenderStagePlan plan_render(const float *const *poses, int n, bool &waited) {
    if (streamer_.fold_if_reachable(poses, n)) waited = true;
    return plan_render_stage(streamer_.store(), core_.o, poses, n);
  }

  FusionCore &core_;
  BlockStreamer &streamer_;
  MapStage &stage_;
  // switches, read once here, every one through hook_env(): the parity build (-DDR_PARITY_HOOKS) alone reads them, the product library reads
  // none.  DR_RAYCAST_NO_SKIP: the empty-space skip's A/B switch, a run-time flag of the product's kernel.  Compiled into the parity
  // build only: the superseded generations -- the literal ray-caster, round 2's four-stage sampler, copy-engine result transfers,
  // statistics.
  bool raycast_no_skip_ = hook_env("DR_RAYCAST_NO_SKIP") != nullptr;
#ifdef DR_PARITY_HOOKS
  bool raycast_v1_ = hook_env("DR_RAYCAST_V1") != nullptr;
  int raycast_sampler_ = hook_env("DR_RAYCAST_SAMPLER") ? std::max(0, std::min(1, atoi(hook_env("DR_RAYCAST_SAMPLER")))) : (hook_env("DR_RAYCAST_UNSTAGED") ? 0 : 1);
  bool render_copy_ = hook_env("DR_RENDER_D2H") && !strcmp(hook_env("DR_RENDER_D2H"), "copy");
  bool raycast_stats_ = hook_env("DR_RAYCAST_STATS") != nullptr;     // measuring hook: iteration statistics of k_raycast2 on stderr
  unsigned long long *d_rstats_ = nullptr;
#else
  static constexpr bool render_copy_ = false;
#endif
  std::vector<Render> renders_;
  int free_slot_ = 0;
  int render_scope_ = DRF_RENDER_RESIDENT;
  uint64_t render_stats_[4] = {0, 0, 0, 0};
  int render_bands_ = 0;  // drf_set_render_bands
  uint64_t band_stats_[4] = {0, 0, 0, 0};
};

}  // namespace dr
