// dr_fusion.hip -- MI355X engine behind the DrFusion operator API (C ABI: include/dr_mi355x.h).
//
// The engine (FusionEngine: call order, scans, renders, the map file, locate and track) and the C ABI.  The volume's device code and the
// table of reference counterparts: volume_kernels.h.  What the engine lends its components: fusion_core.h (FusionCore); streaming:
// stream_ops.h (BlockStreamer); meshing and the incremental mesh: mesh_ops.h (MeshExtractor); the score stage of the pose search: search_ops.h
// (PoseScorer).  DESIGN.md "Where streaming and meshing live".
#include <cfloat>
#include <climits>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include <rocprim/rocprim.hpp>  // device radix sort (block keys) and exclusive scan (triangle offsets) of the mesh path

#include "dr_common.h"
#include "fusion_host.h"  // the host half of the map: block keys (kBS), reach bounds, host store, chunk planner
#include "hip_owner.h"    // HipOwner, DeviceBuf, PinnedBuf: what the engine takes from the runtime
#include "map_file.h"     // the map file: MapWriter, MapReader (host only)
#define DR_MC_CONST __device__ static const
#include "mc_tables.h"

#include "volume_kernels.h"   // Voxel, FusionDev, the block index, k_allocate .. k_integrate, k_zero_int, k_fold_counter, k_fill_keys, k_publish
#include "raycast_kernels.h"  // k_raycast2 / k_raycast_fix (k_raycast: parity build), resident and STAGED (map-scope renders)
namespace dr {

#include "stream_kernels.h"
#include "align_kernels.h"  // k_map_align / k_align_fold (drf_align_system, drf_align_map)
#include "locate_kernels.h"  // k_map_locate (drf_locate_system, drf_locate_frame)
#include "track_kernels.h"   // k_track_model, k_track (drf_track_system, drf_track_frame)
#include "track_colour_kernels.h"  // k_track_model_colour, k_track_colour (drf_track_colour_system, drf_track_colour_frame)
#include "track_pyramid_kernels.h"  // k_track_reduce (drf_track_reduce, drf_track_pyramid_system, drf_track_pyramid_frame)
#include "search_kernels.h"  // k_search_points, k_search_score (drf_score_poses, drf_search_frame)

}  // namespace dr
#include "mesh_kernels.h"
#include "mesh_update_kernels.h"
#include "map_ops.h"  // MapIo: what the map-file operations share; drf_transform_map / drf_align_* whole
#include "fusion_core.h"  // FusionCore: what the engine lends its components
#include "stream_ops.h"   // BlockStreamer
#include "mesh_ops.h"     // MeshExtractor
#include "search_ops.h"   // PoseScorer
namespace dr {

// cofactor inverse on the host in the reference's term order (matrix_utils.h:958-1083), fp32, no contraction
static void inverse4_host(const float *e, float *out) {
  float inv[16];
  auto t3 = [&](int a, int b, int c) { return e[a] * e[b] * e[c]; };
  inv[0] = t3(5, 10, 15) - t3(5, 11, 14) - t3(9, 6, 15) + t3(9, 7, 14) + t3(13, 6, 11) - t3(13, 7, 10);
  inv[4] = -t3(4, 10, 15) + t3(4, 11, 14) + t3(8, 6, 15) - t3(8, 7, 14) - t3(12, 6, 11) + t3(12, 7, 10);
  inv[8] = t3(4, 9, 15) - t3(4, 11, 13) - t3(8, 5, 15) + t3(8, 7, 13) + t3(12, 5, 11) - t3(12, 7, 9);
  inv[12] = -t3(4, 9, 14) + t3(4, 10, 13) + t3(8, 5, 14) - t3(8, 6, 13) - t3(12, 5, 10) + t3(12, 6, 9);
  inv[1] = -t3(1, 10, 15) + t3(1, 11, 14) + t3(9, 2, 15) - t3(9, 3, 14) - t3(13, 2, 11) + t3(13, 3, 10);
  inv[5] = t3(0, 10, 15) - t3(0, 11, 14) - t3(8, 2, 15) + t3(8, 3, 14) + t3(12, 2, 11) - t3(12, 3, 10);
  inv[9] = -t3(0, 9, 15) + t3(0, 11, 13) + t3(8, 1, 15) - t3(8, 3, 13) - t3(12, 1, 11) + t3(12, 3, 9);
  inv[13] = t3(0, 9, 14) - t3(0, 10, 13) - t3(8, 1, 14) + t3(8, 2, 13) + t3(12, 1, 10) - t3(12, 2, 9);
  inv[2] = t3(1, 6, 15) - t3(1, 7, 14) - t3(5, 2, 15) + t3(5, 3, 14) + t3(13, 2, 7) - t3(13, 3, 6);
  inv[6] = -t3(0, 6, 15) + t3(0, 7, 14) + t3(4, 2, 15) - t3(4, 3, 14) - t3(12, 2, 7) + t3(12, 3, 6);
  inv[10] = t3(0, 5, 15) - t3(0, 7, 13) - t3(4, 1, 15) + t3(4, 3, 13) + t3(12, 1, 7) - t3(12, 3, 5);
  inv[14] = -t3(0, 5, 14) + t3(0, 6, 13) + t3(4, 1, 14) - t3(4, 2, 13) - t3(12, 1, 6) + t3(12, 2, 5);
  inv[3] = -t3(1, 6, 11) + t3(1, 7, 10) + t3(5, 2, 11) - t3(5, 3, 10) - t3(9, 2, 7) + t3(9, 3, 6);
  inv[7] = t3(0, 6, 11) - t3(0, 7, 10) - t3(4, 2, 11) + t3(4, 3, 10) + t3(8, 2, 7) - t3(8, 3, 6);
  inv[11] = -t3(0, 5, 11) + t3(0, 7, 9) + t3(4, 1, 11) - t3(4, 3, 9) - t3(8, 1, 7) + t3(8, 3, 5);
  inv[15] = t3(0, 5, 10) - t3(0, 6, 9) - t3(4, 1, 10) + t3(4, 2, 9) + t3(8, 1, 6) - t3(8, 2, 5);
  const float det = e[0] * inv[0] + e[1] * inv[4] + e[2] * inv[8] + e[3] * inv[12];
  const float detr = 1.0f / det;
  for (int i = 0; i < 16; ++i) out[i] = inv[i] * detr;
}

// A (bgr, depth) image pair of the engine's camera as a tracking call is given it: both on the host, or both on the device.
// bgr null: the depth alone.
struct FramePair {
  const void *bgr, *depth;
  bool on_host;
  static FramePair host(const uint8_t *bgr, const float *depth) { return {bgr, depth, true}; }
  static FramePair device(const void *bgr, const void *depth) { return {bgr, depth, false}; }
  bool has(bool colour) const { return depth && (!colour || bgr); }  // the images a call with or without colour reads
};

// ------------------------------------------------------------------ engine
constexpr int kDefaultFusionPriority = 1;  // 0 least (the reference's), 1 normal (measured best in the TandemBackend loop), 2 greatest
class FusionEngine {
  struct Render {
    hipStream_t stream;
    unsigned char *d_bgr, *h_bgr[2], *hd_bgr[2];   // hd_*: the pinned result buffers as the device addresses them
    float *d_depth, *h_depth[2], *hd_depth[2];
    int *d_flag;  // pixels the fast ray-caster handed to the literal pass
    RayState *d_band = nullptr;  // per-pixel state of a depth-banded render (allocated by the first one)
    hipEvent_t done, cast;  // result on the host / ray-cast kernels finished (the volume may be written again)
  };

 public:
  FusionEngine(const drf_options_t &o, int device) : core_(o, device), streamer_(core_), mesher_(core_, streamer_), scorer_(core_), mio_(core_.own, device, o.voxel_size, (size_t)std::min(o.num_blocks, kStageBlocks)) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device) fail(DR_ERR_DEVICE, "DrFusion: no HIP device %d (found %d) -- the MI355X path has no CPU fallback", device, n);
    if (o.block_size != 8) fail(DR_ERR_UNSUPPORTED, "DrFusion: block_size must be 8 (got %d)", o.block_size);
    if (o.num_blocks >= (1 << 30) - 1) fail(DR_ERR_UNSUPPORTED, "DrFusion: num_blocks must be below 2^30 - 1 (got %d)", o.num_blocks);
    if (o.height <= 0 || o.width <= 0 || o.num_blocks <= 0 || o.num_buckets <= 0 || o.bucket_size <= 0 || o.num_render_streams < 0)
      fail(DR_ERR_ARG, "DrFusion: invalid options");
    DR_HIP(hipSetDevice(core_.device));
    // Stream priority of the integrate and render streams.  The reference creates them at the LEAST priority with a note that
    // higher may be better (tsdf_volume.cu:64-70).  DR_FUSION_PRIORITY=low|normal|high selects it here; see DESIGN.md
    // "TandemBackend loop" for the measurement behind the default.
    int least, greatest;
    DR_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    int lo = kDefaultFusionPriority == 2 ? greatest : (kDefaultFusionPriority == 1 ? 0 : least);
    if (const char *e = getenv("DR_FUSION_PRIORITY")) lo = !strcmp(e, "high") ? greatest : (!strcmp(e, "normal") ? 0 : (!strcmp(e, "low") ? least : lo));
    core_.int_stream = mio_.stream = core_.own.stream(lo);
    core_.npix = (size_t)o.height * o.width;
    size_t cap = 1024;
    const size_t want = std::max((size_t)o.num_buckets * (size_t)o.bucket_size, (size_t)2 * o.num_blocks);
    while (cap < want) cap <<= 1;
    core_.d.o = o;
    core_.d.keys = core_.own.device<unsigned long long>(cap);
    core_.d.vals = core_.own.device<int>(cap);
    // -1 everywhere: an insert publishes the key (CAS) BEFORE it stores the pool index, so a concurrent reader -- the ray-cast of scan k
    // beside the allocation of scan k + 1 (enqueue_scan) -- may match a key whose value is not there yet; it then reads -1 = absent, which
    // is the state the block was in a moment ago (its voxels are still all unobserved: the same ray-cast result either way)
    DR_HIP(hipMemsetAsync(core_.d.vals, 0xFF, cap * sizeof(int), core_.int_stream));
    core_.d.cmask = (unsigned)(cap - 1);
    core_.d.blk_key = core_.own.device<unsigned long long>(o.num_blocks);
    core_.d.vox = core_.own.device<Voxel>((size_t)o.num_blocks * 512, core_.int_stream);  // hash_table.cu:28-32
    core_.d.n_alloc = core_.own.device<int>(4, core_.int_stream);
    core_.d.err = core_.d.n_alloc + 1;
    core_.d.cnt = core_.own.device<unsigned long long>(8, core_.int_stream);
    core_.d.sd = core_.own.device<float>(core_.npix);
    core_.d.pix = core_.own.device<PixRec>(core_.npix);
    for (int l = 0; l < kSuperLevels; ++l) core_.d.super[l] = core_.own.device<unsigned char>((size_t)1 << (3 * (kGridBits - kSuperShift[l])), core_.int_stream);
    core_.d.present = core_.own.device<unsigned>((size_t)1 << (3 * kPresentBits - 5), core_.int_stream);
    core_.d.grid = core_.own.device<int>((size_t)1 << (3 * kGridBits), core_.int_stream);
    core_.d.req = core_.own.device<unsigned>(o.num_blocks);
    core_.d.req_count = core_.own.device<int>(4, core_.int_stream);
    core_.d.vis_count = core_.d.req_count + 1;
    core_.d.vis = core_.own.device<int>(o.num_blocks);
    core_.d.wg_upd = core_.own.device<unsigned>(65536);
    setup_fast_div();
    hipLaunchKernelGGL(k_fill_keys, dim3(1024), dim3(256), 0, core_.int_stream, core_.d.keys, cap);
    d_bgr_in_ = core_.own.device<unsigned char>(core_.npix * 3);
    d_depth_in_ = core_.own.device<float>(core_.npix);
    h_bgr_in_ = core_.own.pinned<unsigned char>(core_.npix * 3);
    h_depth_in_ = core_.own.pinned<float>(core_.npix);
    // 12 workgroups per CU: enough to keep every SIMD's 4 resident waves busy, few enough that the blocks being worked on
    // at any moment are neighbours in the pool (sweep on the bench map: 1024 / 3072 / 4096 / 6144 / 8192 / 16384
    // workgroups -> 0.341 / 0.327 / 0.329 / 0.363 / 0.443 / 0.697 ms per scan)
    integrate_grid_ = std::min(cdiv(o.num_blocks, 4), 3072);
    if (const char *e = hook_env("DR_INT_GRID")) integrate_grid_ = std::min(65536, std::max(1, atoi(e)));  // tuning hook
    core_.int_done = core_.own.event();
    for (int i = 0; i < o.num_render_streams; ++i) {
      Render r;
      r.stream = core_.own.stream(lo);
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
    DR_HIP(hipStreamSynchronize(core_.int_stream));
  }
  ~FusionEngine() {  // the device idle before the growable scratch goes; core_.own (declared first, so released last) frees the rest
    (void)hipSetDevice(core_.device);
    (void)hipDeviceSynchronize();
  }

  // tsdf_volume.cu:515-598
  void integrate_scan_async(const uint8_t *bgr, const float *depth, const float *pose16) {
    if (!bgr || !depth || !pose16) fail(DR_ERR_ARG, "IntegrateScanAsync: null argument");
    expect(kIntegrate, "Please call the functions like Integration -> RenderAsync -> GetRenderResults.");
    if (!streamer_.on() && !streamer_.store().empty()) fail(DR_ERR_PROTOCOL, "IntegrateScanAsync: %zu blocks are in the host store while streaming is off; bring them back with drf_stream_in_region first", streamer_.store().size());
    next_ = kRender; loaded_ = false;
    DR_HIP(hipSetDevice(core_.device));
    const float depth_bound = streamer_.on() ? max_valid_depth(depth, core_.npix, core_.o.min_sensor_depth, core_.o.max_sensor_depth) : 0.0f;
    scan_between_streaming(pose16, depth_bound, [&] {
      memcpy(h_bgr_in_, bgr, core_.npix * 3);
      memcpy(h_depth_in_, depth, core_.npix * 4);
      DR_HIP(hipMemcpyAsync(d_bgr_in_, h_bgr_in_, core_.npix * 3, hipMemcpyHostToDevice, core_.int_stream));
      DR_HIP(hipMemcpyAsync(d_depth_in_, h_depth_in_, core_.npix * 4, hipMemcpyHostToDevice, core_.int_stream));
      // the ray-casts read the volume; their result copies do not (the reference waits for the copies, tsdf_volume.cu:553-556)
      enqueue_scan(d_bgr_in_, d_depth_in_, pose16, true);
    });
  }
  // One scan: the previous scan's use of the pinned buffers awaited, blocks streamed in before and out after, core_.int_done behind it
  template <class Enqueue> void scan_between_streaming(const float *pose16, float depth_bound, Enqueue enqueue) {
    DR_HIP(hipEventSynchronize(core_.int_done));
    if (streamer_.on()) streamer_.stream_before_scan(pose16, depth_bound);
    enqueue();
    if (streamer_.on()) streamer_.stream_after_scan(pose16);
    DR_HIP(hipEventRecord(core_.int_done, core_.int_stream));
  }
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
#ifdef DR_PARITY_HOOKS  // the superseded generations have no staged form (render_async refuses them)
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
    if (sg) rs_.wait_ready(r.stream);
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
  // tsdf_volume.cu:634-700
  void render_async(const float *const *poses, int n) {
    // (a map that was loaded or merged may be rendered before its next scan: drf_load_map, drf_merge_map)
    if (!(loaded_ && next_ == kIntegrate)) expect(kRender, "Please call the functions like IntegrateScanAsync -> RenderAsync -> GetRenderResult.");
    if (n != (int)renders_.size()) fail(DR_ERR_PROTOCOL, "Can only render exactly as many poses as streams. Streams: %zu, Poses: %d.", renders_.size(), n);
    DR_HIP(hipSetDevice(core_.device));
    // map scope: the stored blocks these poses can read, decided before anything changes (DR_ERR_CAPACITY leaves all as it was)
    RenderStagePlan plan;
    RenderBandPlan bands;
    bool waited = false;
    if (render_scope_ == DRF_RENDER_MAP) {
      for (int i = 0; i < n; ++i) if (!poses[i]) fail(DR_ERR_ARG, "RenderAsync: null pose");
      plan_render_call("RenderAsync", poses, n, plan, bands, waited);
    }
    next_ = kGetRender;
    free_slot_ ^= 1;  // write into the buffers NOT handed out by the last GetRenderResult
    const PassStats ps = render_passes(plan, bands, renders_.data(), poses, n, true);
    render_stats_[0] = plan.keys.size(); render_stats_[1] = ps.total * (size_t)(8 + 4096);
    render_stats_[2] = (uint64_t)plan.whole; render_stats_[3] = waited ? 1 : 0;
    band_stats_[0] = ps.staged ? ps.passes : 0; band_stats_[1] = ps.largest; band_stats_[2] = ps.total; band_stats_[3] = bands.ok ? 1 : 0;
  }
  // What a map-scope render of these poses stages (drf_render_async, and drf_track_frame for its model): the union of the stored
  // blocks in reach, or depth bands of it, or DR_ERR_CAPACITY before anything changes.
  void plan_render_call(const char *who, const float *const *poses, int n, RenderStagePlan &plan, RenderBandPlan &bands, bool &waited) {
    plan = plan_render(poses, n, waited);
    if (!render_stage_fits(plan, rs_capacity())) {
      // depth bands (drf_set_render_bands): the union may exceed the staging as long as every band fits it
      if (render_bands_ >= 2) bands = plan_render_bands(streamer_.store(), core_.o, poses, n, rs_capacity(), render_bands_);
      if (!bands.ok)
        fail(DR_ERR_CAPACITY, "%s: the poses can read %zu stored blocks, the render staging holds %zu (drf_set_render_scope%s)", who, plan.keys.size(), rs_capacity(),
             render_bands_ >= 2 ? "; no plan of depth bands within drf_set_render_bands either" : "");
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
    // One pass stages the union; a banded render one depth band after the other.  The two slots of rs_ alternate, so band j + 1 is
    // packed and copied while band j ray-casts; all render streams take a band together and share its staging.
    const size_t passes = bands.ok ? bands.keys.size() : 1;
    size_t largest = 0, total = 0;
    for (size_t j = 0; j < passes; ++j) {
      const std::vector<unsigned long long> &keys = bands.ok ? bands.keys[j] : plan.keys;
      largest = std::max(largest, keys.size());
      total += keys.size();
    }
    if (bands.ok) ensure_render_staging(largest);  // (grown once, before the first band is in flight)
    for (size_t j = 0; j < passes; ++j) {
      RenderStage sg{};
      if (staged) sg = stage_render(bands.ok ? bands.keys[j] : plan.keys);
      RenderBand band{};
      band.z_hi = bands.ok ? bands.z[j + 1] : 0.0f;
      band.first = j == 0;
      for (int i = 0; i < n; ++i) {
        Mat P; memcpy(P.m, poses[i], 64);
        submit_render(rs[i], P, staged ? &sg : nullptr, nullptr, bands.ok ? &band : nullptr, handoff && j + 1 == passes);
      }
      if (staged) {  // behind every ray-cast that read the slot: its flags go back to zero
        for (int i = 0; i < n; ++i) rs_.wait_for(rs[i].cast);
        hipLaunchKernelGGL(k_rs_clear, dim3(cdiv(sg.n, 256)), dim3(256), 0, rs_.stream(), sg.keys, sg.n, rs_super_[rs_.slot()][0], rs_super_[rs_.slot()][1]);
        DR_HIP(hipGetLastError());  // (per band: the launches of its ray-casts included)
      }
    }
    return PassStats{passes, largest, total, staged};
  }
  // Depth bands of map-scope renders: max_passes 0 or 1 = off (the default), 2..64 = a RenderAsync whose union exceeds the
  // staging may run in up to that many bands.
  void set_render_bands(int max_passes) {
    if (max_passes < 0 || max_passes > 64) fail(DR_ERR_ARG, "drf_set_render_bands: max_passes %d is not within 0..64", max_passes);
    if (next_ == kGetRender) fail(DR_ERR_PROTOCOL, "drf_set_render_bands: a render is pending, call GetRenderResult first");
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
    if (next_ == kGetRender) fail(DR_ERR_PROTOCOL, "drf_set_render_scope: a render is pending, call GetRenderResult first");
    render_scope_ = scope;
    rs_cap_req_ = stage_capacity_blocks;
  }
  void render_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_render_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = render_stats_[i];
  }
  // tsdf_volume.cu:702-737
  void get_render_result(uint8_t **bgr, float **depth, int n) {
    expect(kGetRender, "Please call the functions in a loop: IntegrateScanAsync -> RenderAsync -> GetRenderResult.");
    if (n != (int)renders_.size()) fail(DR_ERR_ARG, "GetRenderResult: expected %zu outputs", renders_.size());
    next_ = kIntegrate;
    DR_HIP(hipSetDevice(core_.device));
    for (int i = 0; i < n; ++i) {
      DR_HIP(hipEventSynchronize(renders_[i].done));
      bgr[i] = renders_[i].h_bgr[free_slot_];
      depth[i] = renders_[i].h_depth[free_slot_];
    }
    check_device_flags();
  }
  // Device-resident result of render stream i (the buffers GetRenderResult copies from): valid from GetRenderResult
  // until the next RenderAsync.  Lets a consumer on the same GPU (the coarse tracker's dense-depth hand-off) skip the
  // D2H + H2D round trip.
  void get_render_device(int i, const uint8_t **d_bgr, const float **d_depth) {
    if (i < 0 || i >= (int)renders_.size()) fail(DR_ERR_ARG, "get_render_device: stream %d of %zu", i, renders_.size());
    if (next_ != kIntegrate) fail(DR_ERR_PROTOCOL, "get_render_device: call after GetRenderResult");
    if (d_bgr) *d_bgr = renders_[i].d_bgr;
    if (d_depth) *d_depth = renders_[i].d_depth;
  }
  // Test hook: the page-locked host copies of the last (back = 0) and the second-to-last (back = 1) ray-cast of render stream i that
  // bench_sequence wrote -- the second-to-last one ran BESIDE the allocation of the last scan (enqueue_scan), which is what a test of
  // that overlap has to look at.
  void bench_render_host(int i, int back, const uint8_t **bgr, const float **depth) {
    no_bench_while_streaming("drf_bench_render_host");
    if (i < 0 || i >= (int)renders_.size() || back < 0 || back > 1) fail(DR_ERR_ARG, "bench_render_host: stream %d of %zu, back %d", i, renders_.size(), back);
    DR_HIP(hipSetDevice(core_.device));
    DR_HIP(hipDeviceSynchronize());
    const int slot = free_slot_ ^ back;
    if (bgr) *bgr = renders_[i].h_bgr[slot];
    if (depth) *depth = renders_[i].h_depth[slot];
  }
  void synchronize() {
    DR_HIP(hipSetDevice(core_.device));
    DR_HIP(hipDeviceSynchronize());
    check_device_flags();
  }
  void stats(uint64_t out[4]) {
    DR_HIP(hipSetDevice(core_.device));
    DR_HIP(hipDeviceSynchronize());
    unsigned long long c[4];
    DR_HIP(hipMemcpy(c, core_.d.cnt, 32, hipMemcpyDeviceToHost));
    out[0] = (uint64_t)core_.pool_blocks(); out[1] = c[3]; out[2] = c[1]; out[3] = c[2];
  }
  // blocks k_integrate has read since the engine was created (one 4 KB read each, whether or not any voxel of the block was updated): with
  // `updated_total` this gives the kernel's HBM bytes exactly -- 4096 x visited + 8 x updated -- for the counter calibration in DESIGN.md
  uint64_t visited_blocks() {
    DR_HIP(hipSetDevice(core_.device));
    DR_HIP(hipDeviceSynchronize());
    unsigned long long v = 0;
    DR_HIP(hipMemcpy(&v, core_.d.cnt + 4, 8, hipMemcpyDeviceToHost));
    return v;
  }
  void export_blocks(int max_blocks, int32_t *coords, uint8_t *voxels, int *n) {
    DR_HIP(hipSetDevice(core_.device));
    DR_HIP(hipDeviceSynchronize());
    const int na = std::min(core_.pool_blocks(), max_blocks);
    std::vector<unsigned long long> keys(na);
    DR_HIP(hipMemcpy(keys.data(), core_.d.blk_key, (size_t)na * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < na; ++i) unpack_key_host(keys[i], coords + 3 * i);
    DR_HIP(hipMemcpy(voxels, core_.d.vox, (size_t)na * 4096, hipMemcpyDeviceToHost));
    if (n) *n = na;
  }
  void fast_div_status(int *enabled, unsigned long long *mismatches) const { if (enabled) *enabled = core_.d.fast_div; if (mismatches) *mismatches = fast_div_mismatches_; }
  void test_combine(size_t n, const uint8_t *a, const uint8_t *b, int max_weight, uint8_t *out) {
    DR_HIP(hipSetDevice(core_.device));
    DeviceBuf<Voxel> da, db, dout;
    da.reserve(n, core_.int_stream); db.reserve(n, core_.int_stream); dout.reserve(n, core_.int_stream);
    DR_HIP(hipMemcpy(da.get(), a, n * 8, hipMemcpyHostToDevice));
    DR_HIP(hipMemcpy(db.get(), b, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_combine, dim3(2048), dim3(256), 0, core_.int_stream, da.get(), db.get(), dout.get(), n, max_weight);
    DR_HIP(hipStreamSynchronize(core_.int_stream));
    DR_HIP(hipMemcpy(out, dout.get(), n * 8, hipMemcpyDeviceToHost));
  }
  // ---- marching cubes and the incremental mesh: mesh_ops.h.  The refusals in their order: null arguments, the call order, "pending"
  void extract_mesh_async(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "ExtractMeshAsync: null argument");
    expect(kIntegrate, "Please call this functions after GetRenderResult.");
    mesher_.extract_mesh_async(lower, upper);
  }
  void get_mesh_sync(size_t num_max, size_t *num, float *vert, float *cols) {
    expect(kIntegrate, "Please call this functions after GetRenderResult.");
    mesher_.get_mesh_sync(num_max, num, vert, cols);
  }
  void extract_mesh_update_async(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "drf_extract_mesh_update_async: null argument");
    expect(kIntegrate, "Please call this functions after GetRenderResult.");
    mesher_.extract_mesh_update_async(lower, upper);
  }
  MeshExtractor &mesh() { return mesher_; }  // the entry points no call order guards (the C ABI below)

  // bench path: inputs already resident in HBM
  void integrate_device(const void *d_bgr, const void *d_depth, const float *pose16) {
    DR_HIP(hipSetDevice(core_.device));
    if (streamer_.on()) {  // the depths are on the device: bound the scan by max_sensor_depth
      if (!d_bgr || !d_depth || !pose16) fail(DR_ERR_ARG, "drf_integrate_device: null argument");
      return scan_between_streaming(pose16, core_.o.max_sensor_depth, [&] { enqueue_scan((const unsigned char *)d_bgr, (const float *)d_depth, pose16); });
    }
    if (!streamer_.store().empty()) fail(DR_ERR_PROTOCOL, "drf_integrate_device: blocks are in the host store while streaming is off");
    enqueue_scan((const unsigned char *)d_bgr, (const float *)d_depth, pose16);
  }
  void no_bench_while_streaming(const char *what) {
    if (streamer_.on() || !streamer_.store().empty()) fail(DR_ERR_UNSUPPORTED, "%s: not available while streaming is on or the host store holds blocks", what);
  }
  void bench_integrate(const void *d_bgr, const void *d_depth, const float *poses, int nscans, float *ms, float *kernel_ms) {
    no_bench_while_streaming("drf_bench_integrate");
    DR_HIP(hipSetDevice(core_.device));
    std::vector<hipEvent_t> ev(2 * (size_t)nscans + 2);
    for (auto &e : ev) DR_HIP(hipEventCreate(&e));
    DR_HIP(hipEventRecord(ev[0], core_.int_stream));
    for (int s = 0; s < nscans; ++s) {
      kernel_events_[0] = ev[2 + 2 * s]; kernel_events_[1] = ev[3 + 2 * s];
      enqueue_scan((const unsigned char *)d_bgr + (size_t)s * core_.npix * 3, (const float *)d_depth + (size_t)s * core_.npix, poses + 16 * s);
    }
    kernel_events_[0] = kernel_events_[1] = nullptr;
    DR_HIP(hipEventRecord(ev[1], core_.int_stream));
    DR_HIP(hipStreamSynchronize(core_.int_stream));
    float t = 0, k = 0;
    DR_HIP(hipEventElapsedTime(&t, ev[0], ev[1]));
    for (int s = 0; s < nscans; ++s) { float q = 0; DR_HIP(hipEventElapsedTime(&q, ev[2 + 2 * s], ev[3 + 2 * s])); k += q; }
    for (auto &e : ev) (void)hipEventDestroy(e);
    if (ms) *ms = t;
    if (kernel_ms) *kernel_ms = k;
    check_device_flags();
  }

  // BASELINE configs[3] loop (dr_debug_example.cpp:78-162: GetRenderResult(k-1) / IntegrateScanAsync(k) / RenderAsync(k) per
  // frame, map growing) over `n` frames whose inputs are resident in HBM: allocate + integrate on the integration stream,
  // then -- render != 0 -- one ray-cast per render stream from the frame's own pose with the D2H of its result into the
  // pinned double buffers, ordered by the same events as the operator path.  ms[0] = first allocate .. last copy
  // (hipEvents), ms[1..4] = sums of the allocate / integrate / ray-cast / D2H intervals, ms[5] = host wall clock.
  void bench_sequence(const void *d_bgr, const void *d_depth, const float *poses, int n, int render, float ms[6]) {
    no_bench_while_streaming("drf_bench_sequence");
    if (!d_bgr || !d_depth || !poses || !ms || n <= 0) fail(DR_ERR_ARG, "bench_sequence: bad argument");
    expect(kIntegrate, "bench_sequence starts where IntegrateScanAsync may be called.");
    DR_HIP(hipSetDevice(core_.device));
    const int nr = render ? (int)renders_.size() : 0;
    const size_t per = 4 + (size_t)3 * nr;
    std::vector<hipEvent_t> ev(per * n);
    for (auto &e : ev) DR_HIP(hipEventCreate(&e));
    DR_HIP(hipDeviceSynchronize());
    const auto t0 = std::chrono::steady_clock::now();
    for (int s = 0; s < n; ++s) {
      hipEvent_t *e = &ev[per * s];
      DR_HIP(hipEventRecord(e[0], core_.int_stream));
      kernel_events_[0] = e[1]; kernel_events_[1] = e[2]; kernel_events_[2] = e[3];
      // (the voxel update waits for the previous frame's ray-casts inside enqueue_scan; allocation, commit and cull run beside them)
      enqueue_scan((const unsigned char *)d_bgr + (size_t)s * core_.npix * 3, (const float *)d_depth + (size_t)s * core_.npix, poses + 16 * s, true);
      kernel_events_[0] = kernel_events_[1] = kernel_events_[2] = nullptr;
      DR_HIP(hipEventRecord(core_.int_done, core_.int_stream));
      free_slot_ ^= 1;
      for (int i = 0; i < nr; ++i) {
        Mat P; memcpy(P.m, poses + 16 * s, 64);
        submit_render(renders_[i], P, nullptr, e + 4 + 3 * i);
      }
    }
    DR_HIP(hipDeviceSynchronize());
    ms[5] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int k = 0; k < 5; ++k) ms[k] = 0.f;
    float q = 0.f;
    hipEvent_t last = nr ? ev[per * (n - 1) + 6 + 3 * (nr - 1)] : ev[per * (n - 1) + 2];
    DR_HIP(hipEventElapsedTime(&ms[0], ev[0], last));
    for (int s = 0; s < n; ++s) {
      hipEvent_t *e = &ev[per * s];
      DR_HIP(hipEventElapsedTime(&q, e[0], e[3])); ms[1] += q;  // allocate + commit + cull (may run beside the previous frame's ray-cast)
      DR_HIP(hipEventElapsedTime(&q, e[1], e[2])); ms[2] += q;  // k_integrate alone
      for (int i = 0; i < nr; ++i) {
        DR_HIP(hipEventElapsedTime(&q, e[4 + 3 * i], e[5 + 3 * i])); ms[3] += q;
        DR_HIP(hipEventElapsedTime(&q, e[5 + 3 * i], e[6 + 3 * i])); ms[4] += q;
      }
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    check_device_flags();
  }

  // ---- streaming: stream_ops.h ----
  void stream_out_region(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "drf_stream_out_region: null argument");
    expect(kIntegrate, "drf_stream_out_region: call it where IntegrateScanAsync may be called.");
    streamer_.stream_out_region(lower, upper);
  }
  void stream_in_region(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "drf_stream_in_region: null argument");
    expect(kIntegrate, "drf_stream_in_region: call it where IntegrateScanAsync may be called.");
    streamer_.stream_in_region(lower, upper);
  }
  BlockStreamer &streaming() { return streamer_; }  // the entry points no call order guards (the C ABI below)

  // ---- the map file (include/dr_mi355x.h "map files"; DESIGN.md §7c "Saving and loading the map") ----
  // Resident and stored blocks merged in ascending key order, chunk by chunk: k_map_gather writes a chunk's resident blocks
  // straight into one of two pinned buffers while the host copies the stored ones into their positions of it, appends the
  // other buffer to the file and folds it into the checksum.  Folds pending evictions first; beyond that nothing changes.
  void save_map(const char *path, size_t chunk_blocks) {
    if (!path) fail(DR_ERR_ARG, "drf_save_map: null argument");
    expect(kIntegrate, "drf_save_map: call it where IntegrateScanAsync may be called.");
    streamer_.settle();
    const int nres = core_.pool_blocks();
    std::vector<unsigned long long> res((size_t)nres);
    sort_resident(nres, res);
    const std::vector<unsigned long long> sto = streamer_.store().sorted_keys();
    const size_t n = res.size() + sto.size();
    std::vector<unsigned long long> keys;
    std::vector<unsigned char> stored;
    keys.reserve(n); stored.reserve(n);
    const BlockRange all{{INT_MIN, INT_MIN, INT_MIN}, {INT_MAX, INT_MAX, INT_MAX}};
    for_each_in_range(res, sto, all, [&](unsigned long long key, bool st) { keys.push_back(key); stored.push_back(st ? 1 : 0); });
    const size_t chunk = mio_.chunk(chunk_blocks, n), nc = (n + chunk - 1) / chunk;
    // per chunk the resident blocks rb[c] .. rb[c + 1] of the sorted pairs; each one's position within its chunk
    std::vector<size_t> rb(nc + 1, 0);
    std::vector<int> dst;
    dst.reserve((size_t)nres);
    for (size_t i = 0; i < n; ++i)
      if (!stored[i]) { ++rb[i / chunk + 1]; dst.push_back((int)(i % chunk)); }
    for (size_t c = 0; c < nc; ++c) rb[c + 1] += rb[c];
    if (nres > 0) DR_HIP(hipMemcpy(mio_.dst.get(), dst.data(), (size_t)nres * 4, hipMemcpyHostToDevice));
    mio_.ensure(chunk);
    std::string err;
    MapWriter w;
    if (!w.open(path, core_.o.voxel_size, keys.data(), n, err)) fail(DR_ERR_IO, "drf_save_map: %s", err.c_str());
    mio_.write_chunks(
        "drf_save_map", w, n, chunk,
        [&](size_t c) {  // chunk c's resident blocks into the current buffer; nothing is launched for none
          const int m = (int)(rb[c + 1] - rb[c]);
          if (m == 0) return;
          hipLaunchKernelGGL(k_map_gather, dim3(std::min(cdiv(m, 4), 1024)), dim3(256), 0, core_.int_stream, core_.d.vox, mio_.slot.get() + rb[c], mio_.dst.get() + rb[c], m,
                             (uint4 *)mio_.pair.dev());
          DR_HIP(hipGetLastError());
        },
        [&](size_t c, unsigned char *h) {  // and the stored ones, while that kernel runs
          const size_t b = c * chunk, m = std::min(chunk, n - b);
          for (size_t i = 0; i < m; ++i)
            if (stored[b + i]) memcpy(h + i * 4096, streamer_.store().get(keys[b + i]), 4096);
        });
  }
  // The file validated as a whole first, then its blocks placed: into the pool in the keys' order (streaming off; k_in_place
  // reads one pinned buffer while the host reads the file into the other) or into the host store (streaming on).  A failure
  // leaves the map empty.
  void load_map(const char *path, size_t chunk_blocks) {
    if (!path) fail(DR_ERR_ARG, "drf_load_map: null argument");
    expect(kIntegrate, "drf_load_map: call it where IntegrateScanAsync may be called.");
    const bool pending = streamer_.eviction_pending();
    streamer_.settle();
    const int nres = core_.pool_blocks();
    if (pending || nres != 0 || !streamer_.store().empty())
      fail(DR_ERR_PROTOCOL, "drf_load_map: the map is not empty (%d resident blocks, %zu in the host store%s)", nres, streamer_.store().size(), pending ? ", an eviction was pending" : "");
    std::string err;
    MapReader rd;
    mio_.open_reader("drf_load_map", path, rd);
    const uint64_t n = rd.blocks();
    const bool to_store = streamer_.on();
    if (to_store ? n > (uint64_t)streamer_.host_capacity() : n > (uint64_t)core_.o.num_blocks)
      fail(DR_ERR_CAPACITY, "drf_load_map: %llu blocks do not fit in the %s (%llu)", (unsigned long long)n, to_store ? "host store" : "pool",
           (unsigned long long)(to_store ? streamer_.host_capacity() : (size_t)core_.o.num_blocks));
    mesher_.force_full_update();
    if (n == 0) { loaded_ = true; return; }
    const std::vector<unsigned long long> &keys = rd.keys();
    const size_t chunk = mio_.chunk(chunk_blocks, (size_t)n);
    mio_.ensure(chunk);
    bool ok;
    if (to_store) {  // the next scan's stream_before_scan brings in what lies within the radius
      ok = mio_.read_chunks(rd, chunk, err, [&](size_t b, size_t m, const unsigned char *h, const unsigned char *) {
        for (size_t i = 0; i < m; ++i) streamer_.store().put(keys[b + i], h + i * 4096);
      });
    } else {  // k_in_place reads one pinned buffer while the host reads the file into the other
      mio_.keys.reserve((size_t)n, core_.int_stream);
      DR_HIP(hipMemcpy(mio_.keys.get(), keys.data(), (size_t)n * 8, hipMemcpyHostToDevice));
      core_.wait_casts();  // blocks are added
      ok = mio_.read_chunks(rd, chunk, err, [&](size_t b, size_t m, const unsigned char *, const unsigned char *d) {
        hipLaunchKernelGGL(k_in_place, dim3(std::min(cdiv((int)m, 4), 1024)), dim3(256), 0, core_.int_stream, core_.d, mio_.keys.get() + b, (const uint4 *)d, (int)m);
        hipLaunchKernelGGL(k_in_finish, dim3(1), dim3(64), 0, core_.int_stream, core_.d.n_alloc, (int)m);
        DR_HIP(hipGetLastError());
      });
      DR_HIP(hipStreamSynchronize(core_.int_stream));
    }
    if (!ok) {
      clear_map();
      fail(DR_ERR_IO, "drf_load_map: %s", err.c_str());
    }
    loaded_ = true;
  }

  // A map file merged into the map (the rule: fusion_host.h merge_voxel).  The file validated and every block classified against
  // the map (plan_merge) before anything changes; then chunk by chunk through the two pinned buffers: k_map_merge combines the
  // blocks whose key is resident in place, k_in_place_at appends the new ones (streaming off) while the host combines the
  // chunk's stored blocks into the store, puts the new ones there (streaming on) and reads the next chunk.  A file that changes
  // under the second pass leaves a mixture of merged and untouched blocks (DR_ERR_IO; merge_stats tells how far it got).
  void merge_map(const char *path, size_t chunk_blocks) {
    if (!path) fail(DR_ERR_ARG, "drf_merge_map: null argument");
    expect(kIntegrate, "drf_merge_map: call it where IntegrateScanAsync may be called.");
    streamer_.settle();
    std::string err;
    MapReader rd;
    mio_.open_reader("drf_merge_map", path, rd);
    const size_t n = (size_t)rd.blocks();
    const std::vector<unsigned long long> &keys = rd.keys();
    const int nres = core_.pool_blocks();
    std::vector<unsigned long long> res((size_t)nres);
    std::vector<int> slots((size_t)nres);
    sort_resident(nres, res);
    if (nres > 0) DR_HIP(hipMemcpy(slots.data(), mio_.slot.get(), (size_t)nres * 4, hipMemcpyDeviceToHost));
    const size_t chunk = mio_.chunk(chunk_blocks, n);
    const MergePlan p = plan_merge(res, slots, streamer_.store().sorted_keys(), keys, chunk);
    const bool to_store = streamer_.on();
    const size_t n_add = p.add_key.size(), n_res = p.res_slot.size();
    if (to_store ? streamer_.store().size() + n_add > streamer_.host_capacity() : (size_t)nres + n_add > (size_t)core_.o.num_blocks)
      fail(DR_ERR_CAPACITY, "drf_merge_map: %zu new blocks do not fit in the %s (%zu of %llu in use)", n_add, to_store ? "host store" : "pool",
           to_store ? streamer_.store().size() : (size_t)nres, (unsigned long long)(to_store ? streamer_.host_capacity() : (size_t)core_.o.num_blocks));
    for (auto &v : mg_stats_) v = 0;
    mg_stats_[0] = n;
    mesher_.force_full_update();
    if (n == 0) { loaded_ = true; return; }
    mio_.ensure(chunk);
    // the per-chunk index lists, in the sort's buffers (their contents are on the host now)
    const size_t n_dev = to_store ? 0 : n_add;
    mio_.slot_in.reserve(std::max<size_t>(n_res, 1), core_.int_stream); mio_.slot.reserve(std::max<size_t>(n_res, 1), core_.int_stream);
    mio_.dst.reserve(std::max<size_t>(n_dev, 1), core_.int_stream); mio_.keys.reserve(std::max<size_t>(n_dev, 1), core_.int_stream);
    mg_counts_.reserve(2, core_.int_stream);
    if (n_res > 0) {
      DR_HIP(hipMemcpy(mio_.slot_in.get(), p.res_src.data(), n_res * 4, hipMemcpyHostToDevice));
      DR_HIP(hipMemcpy(mio_.slot.get(), p.res_slot.data(), n_res * 4, hipMemcpyHostToDevice));
    }
    if (n_dev > 0) {
      DR_HIP(hipMemcpy(mio_.dst.get(), p.add_src.data(), n_dev * 4, hipMemcpyHostToDevice));
      DR_HIP(hipMemcpy(mio_.keys.get(), p.add_key.data(), n_dev * 8, hipMemcpyHostToDevice));
    }
    DR_HIP(hipMemset(mg_counts_.get(), 0, 16));
    core_.wait_casts();  // blocks change
    const unsigned char W = (unsigned char)core_.o.max_sdf_weight;
    uint64_t host_counts[2] = {0, 0};
    const bool ok = mio_.read_chunks(rd, chunk, err, [&](size_t b, size_t, const unsigned char *h, const unsigned char *d) {
      const size_t c = b / chunk;
      const int mr = (int)(p.rb[c + 1] - p.rb[c]), ma = to_store ? 0 : (int)(p.ab[c + 1] - p.ab[c]);
      if (mr > 0)
        hipLaunchKernelGGL(k_map_merge, dim3(std::min(cdiv(mr, 4), 1024)), dim3(256), 0, core_.int_stream, core_.d.vox, mio_.slot_in.get() + p.rb[c], mio_.slot.get() + p.rb[c], mr,
                           (const uint4 *)d, W, mg_counts_.get());
      if (ma > 0) {
        hipLaunchKernelGGL(k_in_place_at, dim3(std::min(cdiv(ma, 4), 1024)), dim3(256), 0, core_.int_stream, core_.d, mio_.keys.get() + p.ab[c], mio_.dst.get() + p.ab[c],
                           (const uint4 *)d, ma);
        hipLaunchKernelGGL(k_in_finish, dim3(1), dim3(64), 0, core_.int_stream, core_.d.n_alloc, ma);
      }
      if (mr > 0 || ma > 0) DR_HIP(hipGetLastError());
      // the host half of the chunk, from the same buffer, while the kernels read it
      for (size_t i = p.sb[c]; i < p.sb[c + 1]; ++i) merge_block(streamer_.store().get_mut(p.sto_key[i]), h + (size_t)p.sto_src[i] * 4096, W, host_counts);
      if (to_store)
        for (size_t i = p.ab[c]; i < p.ab[c + 1]; ++i) streamer_.store().put(p.add_key[i], h + (size_t)p.add_src[i] * 4096);
      mg_stats_[1] += p.ab[c + 1] - p.ab[c]; mg_stats_[2] += (uint64_t)mr; mg_stats_[3] += p.sb[c + 1] - p.sb[c];
    });
    DR_HIP(hipStreamSynchronize(core_.int_stream));
    unsigned long long dev_counts[2];
    DR_HIP(hipMemcpy(dev_counts, mg_counts_.get(), 16, hipMemcpyDeviceToHost));
    mg_stats_[4] = host_counts[0] + dev_counts[0]; mg_stats_[5] = host_counts[1] + dev_counts[1];
    if (!ok) fail(DR_ERR_IO, "drf_merge_map: %s (the blocks merged so far stay merged: drf_merge_stats)", err.c_str());
    loaded_ = true;
  }
  const uint64_t *merge_stats() const { return mg_stats_; }

  // Operations on map files alone (map_ops.h: map_transform, map_align_system, map_align).  The engine lends mio_ -- its device,
  // core_.int_stream, the pinned pair, voxel_size -- and states where in its call order they may run; its own map is neither read nor changed.
  void transform_map(const char *src, const float *T16, const char *dst, size_t chunk_blocks) {
    map_transform(mio_, src, T16, dst, chunk_blocks, [&] { expect_integrate("drf_transform_map"); });
  }
  const uint64_t *transform_stats() const { return mio_.xf_stats; }
  void align_system(const char *src, const char *ref, const float *T16, const drf_align_options_t *opt, double *sums, uint64_t *counts) {
    map_align_system(mio_, src, ref, T16, opt, sums, counts, [&](const char *who) { expect_integrate(who); });
  }
  // returns what dr_last_error() says after a registration that ran but found no pose (empty otherwise)
  std::string align_map(const char *src, const char *ref, const float *T16, const drf_align_options_t *opt, float *T16_out, drf_align_result_t *res) {
    return map_align(mio_, src, ref, T16, opt, T16_out, res, [&](const char *who) { expect_integrate(who); });
  }
  const uint64_t *align_stats() const { return mio_.al_stats; }

  // ---- a camera pose from a frame: drf_locate_*, drf_track_*, drf_track_colour_*, drf_track_pyramid_* (the rules: pose_host.h;
  // DESIGN.md "Where the frame-pose code lives").  What the families open with, written once.  frame_prologue: the refusals in their one order --
  // the options (bad_option: what the family's resolver returned), the call order, blocks in the host store while streaming is
  // off, the pose, the model pose (the *_system calls of the tracking) -- then pending work settled.
  void frame_prologue(const char *who, const char *bad_option, const float *pose16, const float *model_pose16) {
    if (bad_option) fail(DR_ERR_ARG, "%s: option %s is negative or not finite", who, bad_option);
    expect_integrate(who);
    if (!streamer_.on() && !streamer_.store().empty())
      fail(DR_ERR_PROTOCOL, "%s: %zu blocks are in the host store while streaming is off; bring them back with drf_stream_in_region first", who, streamer_.store().size());
    if (const char *why = transform_pose_fault(pose16)) fail(DR_ERR_ARG, "%s: the pose %s", who, why);
    if (model_pose16)
      if (const char *why = transform_pose_fault(model_pose16)) fail(DR_ERR_ARG, "%s: the model pose %s", who, why);
    streamer_.settle();  // behind any pending scan; the pinned buffers are idle and every eviction is in the host store
  }
  // the sample grid of a call and what a launch over it needs; max_groups (step = 1) sizes the scratch once for every step
  struct FrameGrid { LocateGrid lg; int total, groups; size_t max_groups; };
  FrameGrid frame_grid(int step) const {
    const LocateGrid lg = locate_grid(core_.o, step);
    return {lg, (int)locate_positions(lg), (int)locate_groups(lg), (core_.npix + 511) / 512};
  }
  // A host image pair, or a depth image alone (d_bgr null), through the scan's pinned input buffers into scratch.  again: the
  // buffers carry this call's frame, which must have left them first.
  void upload_frame(const uint8_t *h_bgr, const float *h_depth, unsigned char *d_bgr, float *d_depth, bool again = false) {
    if (again) DR_HIP(hipStreamSynchronize(core_.int_stream));
    if (d_bgr) memcpy(h_bgr_in_, h_bgr, core_.npix * 3);
    memcpy(h_depth_in_, h_depth, core_.npix * 4);
    if (d_bgr) DR_HIP(hipMemcpyAsync(d_bgr, h_bgr_in_, core_.npix * 3, hipMemcpyHostToDevice, core_.int_stream));
    DR_HIP(hipMemcpyAsync(d_depth, h_depth_in_, core_.npix * 4, hipMemcpyHostToDevice, core_.int_stream));
  }

  // A depth frame located in the map this engine holds (the rule: pose_host.h locate_pixel / align_point; DESIGN.md §7c "Locating a
  // depth frame in the map").  The map is read where it lives, through find_block; nothing of it is uploaded, changed or allocated.
  // with_locate does what both calls share -- the prologue, device scratch that is sized once -- and hands body an evaluator:
  // k_map_locate + k_align_fold on core_.int_stream, 28 doubles and 4 counters back through the pinned pair.
  template <class Body>
  void with_locate(const char *who, const float *h_depth, const void *d_depth, const float *pose16, const drf_locate_options_t *opt, Body &&body) {
    locate_reset();
    LocateOpt lo;
    frame_prologue(who, locate_options(opt, core_.o.truncation_distance, lo), pose16, nullptr);
    const FrameGrid fg = frame_grid(lo.step);
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
    // Map scope (drf_set_locate_scope): the stored blocks an evaluation at the pose can read go through the render's staging, rs_
    // -- no render reads it here: the call is legal only where a scan is, and the device is idle.  A staging serves the poses that
    // follow while locate_stage_serves says so; a pose beyond that selects and stages again.  With an empty store or an empty
    // selection nothing is staged and the resident kernel is launched.
    const bool map_scope = locate_scope_ == DRF_LOCATE_MAP && !streamer_.store().empty();
    double slack = locate_stage_slack(core_.o);
    if (const char *env = hook_env("DR_LOCATE_STAGE_SLACK")) slack = std::min(slack, std::max(0.0, atof(env)) * (double)core_.o.voxel_size);  // parity hook, in voxels
    std::vector<unsigned long long> keys;  // the selection at sel_pose
    float sel_pose[16];
    RenderStage sg{};
    bool staged = false, selected = false;
    if (map_scope) {  // the refusal: decided at the first pose, before anything is evaluated
      locate_pose16(map_motion(pose16, core_.o.voxel_size), core_.o.voxel_size, sel_pose);
      keys = select_locate_blocks(streamer_.store(), core_.o, sel_pose);
      if (keys.size() > lc_capacity())
        fail(DR_ERR_CAPACITY, "%s: the pose can read %zu stored blocks, the locate staging holds %zu (drf_set_locate_scope with a larger capacity, or drf_stream_in_region)",
             who, keys.size(), lc_capacity());
    }
    const float *depth = (const float *)d_depth;
    if (h_depth) {
      upload_frame(nullptr, h_depth, nullptr, mine);
      depth = mine;
    }
    lc_stats_[0] = (uint64_t)total; lc_stats_[4] = lc_buf_.capacity(); lc_stats_[5] = streamer_.store().size();
    // the slot's flags go back to zero behind the evaluations that read it (they are on core_.int_stream)
    auto release = [&](bool may_throw) {
      if (!staged) return;
      staged = false;
      hipError_t err = hipEventRecord(rs_.used(), core_.int_stream);
      if (err == hipSuccess) err = hipStreamWaitEvent(rs_.stream(), rs_.used(), 0);
      if (err == hipSuccess) {
        hipLaunchKernelGGL(k_rs_clear, dim3(cdiv(sg.n, 256)), dim3(256), 0, rs_.stream(), sg.keys, sg.n, rs_super_[rs_.slot()][0], rs_super_[rs_.slot()][1]);
        err = hipGetLastError();
      }
      if (may_throw) DR_HIP(err);
    };
    auto eval = [&](const AlignEval &e, double sums[28], uint64_t c4[4]) {
      if (map_scope) {
        float p16[16];
        locate_pose16(e.m, core_.o.voxel_size, p16);
        if (selected && !locate_stage_serves(core_.o, sel_pose, p16, slack)) {
          keys = select_locate_blocks(streamer_.store(), core_.o, p16);
          if (keys.size() > lc_capacity())
            fail(DR_ERR_CAPACITY, "%s: a pose of the refinement can read %zu stored blocks, the locate staging holds %zu (drf_set_locate_scope with a larger capacity, or drf_stream_in_region)",
                 who, keys.size(), lc_capacity());
          memcpy(sel_pose, p16, sizeof p16);
          selected = false;
        }
        if (!selected) {
          release(true);
          if (!keys.empty()) {
            sg = stage_render(keys);
            staged = true;
            ++ls_stats_[0]; ls_stats_[1] = std::max<uint64_t>(ls_stats_[1], keys.size()); ls_stats_[2] += keys.size();
          }
          selected = true;
        }
      }
      mio_.evaluate(partial, groups, counts, 4, sums, c4, [&] {
        if (staged) {
          rs_.wait_ready(core_.int_stream);
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
  // stage_capacity_blocks bounds what one evaluation may stage (0 = the render's default); rs_ holds the larger of the two needs.
  void set_locate_scope(int scope, size_t stage_capacity_blocks) {
    if (scope != DRF_LOCATE_RESIDENT && scope != DRF_LOCATE_MAP) fail(DR_ERR_ARG, "drf_set_locate_scope: unknown scope %d", scope);
    if (next_ == kGetRender) fail(DR_ERR_PROTOCOL, "drf_set_locate_scope: a render is pending, call GetRenderResult first");
    locate_scope_ = scope;
    lc_cap_req_ = stage_capacity_blocks;
  }
  void locate_stage_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_locate_stage_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = ls_stats_[i];
  }

  // A frame tracked against the ray-cast model: by its depth alone (drf_track_*; DESIGN.md §7c "Tracking a depth frame against the
  // ray-cast model"), with the photometric term (drf_track_colour_*; "Tracking with colour"), or coarse to fine (drf_track_reduce,
  // drf_track_pyramid_*; "Tracking coarse to fine").  The rule: pose_host.h track_normal / track_point / track_colour_point /
  // track_loop and track_level_grid / track_reduce_host / track_pyramid_schedule.  One path for the three families (what it
  // guarantees: DESIGN.md "Where the frame-pose code lives").  Every launch is given its level, and level 0 is the single-level
  // call (track_level_grid returns the grid itself), so drf_track_* and drf_track_colour_* are the schedule with one level; colour
  // is a run-time flag.  What differs is the side -- tk_, tc_ or tp_: each family its own scratch, in its own layout, its own
  // statistics and model render, so a call of one family leaves the others' statistics and buffers what they were -- and what each
  // entry does itself: its null arguments, its options, its refusal texts.
  // with_track does what the calls share behind the prologue -- device scratch that is sized once, the frame's intake, the
  // statistics reset when an exception passes -- and hands body the call: the spans and what track_launch_model, track_evaluate
  // (k_track or k_track_colour + k_align_fold on core_.int_stream; k_align_fold hands back four counters, the photometric terms added
  // leave through a pinned word) and track_render need.  The model's render goes through the engine's one submit (render_passes)
  // on core_.int_stream into the scratch; renders_, free_slot_, next_ and the render statistics are not touched.
  struct TrackSide {
    DeviceBuf<unsigned char> buf;             // sized once
    uint64_t stats[8] = {};                   // drf_track_stats / drf_track_colour_stats (the first six), drf_track_pyramid_stats
    uint64_t level[kTrackMaxLevels][4] = {};  // drf_track_pyramid_level_stats
    Render render{};                          // the *_frame call's full-resolution model render: core_.int_stream and pointers into buf
    void reset() { memset(stats, 0, sizeof stats); memset(level, 0, sizeof level); }
  };
  struct TrackBufs {  // the spans; a layout leaves null what it does not have
    double *partial; unsigned long long *counts; int *flag; TrackPixel *map;
    float *model, *level, *Ym, *frame, *pyr[kTrackMaxLevels];  // the full-resolution model, its level, Ym, a host-given frame, the frame's levels >= 1
    unsigned char *model_bgr, *level_bgr, *frame_bgr, *pyr_bgr[kTrackMaxLevels];
    unsigned char *render_bgr; RayState *render_band;  // where the model's render puts its colour image and a banded render's ray state
    const float *depth; const unsigned char *bgr;      // the frame at full resolution: the caller's device images, or the spans a host frame went to
  };
  struct TrackCall { const char *who; TrackSide &s; bool colour; FrameGrid fg; TrackBufs b; };
  // The three layouts (DESIGN.md "What the carver guarantees").  What of a render nobody reads once the model kernel runs may lie
  // in the bytes that kernel then overwrites with the model map: a banded render's per-pixel ray state in both single-level
  // layouts, and in the geometric one the colour image too (with colour k_track_model_colour reads it: it has the span model_bgr).
  // The pyramid's is sized for five levels with nothing aliased.
  TrackBufs track_spans(TrackSide &s) {
    TrackBufs b{};
    const size_t max_groups = frame_grid(1).max_groups;
    auto head = [&](Carver &c, size_t counters) {
      b.partial = c.take<double>(max_groups * 28);
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
        head(c, 6);
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
    upload_frame((const uint8_t *)frame.bgr, (const float *)frame.depth, colour ? b.frame_bgr : nullptr, b.frame);
    b.depth = b.frame;
    b.bgr = colour ? b.frame_bgr : nullptr;
  }
  template <class Body>
  void with_track(const char *who, TrackSide &s, bool colour, const FramePair &frame, int step, Body &&body) {
    TrackCall t{who, s, colour, frame_grid(step), track_spans(s)};
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
  // the model of a *_frame round: the engine's one submit at full resolution into the spans, then level L's model map
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
    if (render_scope_ == DRF_RENDER_MAP) plan_render_call(t.who, poses, 1, plan, bands, waited);
    render_passes(plan, bands, &rd, poses, 1, false);
    track_launch_model(t, t.b.model, t.b.model_bgr, L, lo);
  }
  // The body of every *_system call: one evaluation at `level` against a full-resolution model pair the caller gives, n counters
  // out.  A host-given model goes through upload_frame into the spans.  A device-given one is read in place by the single-level
  // calls and copied into the spans by the pyramid's: track_launch_model could read that one in place too, but the copy is part
  // of what drf_track_pyramid_system_device enqueues, and stays.
  void track_system_at(const char *who, TrackSide &s, bool colour, int level, const TrackPyramidOpt &po, const FramePair &frame, const FramePair &model,
                       const float *model_pose16, const float *pose16, double *sums, uint64_t *counts, int n) {
    with_track(who, s, colour, frame, po.c.t.step, [&](TrackCall &t) {
      const TrackBufs &b = t.b;
      const TrackColourOpt lo = track_level_options(po, level);
      if (level > 0) launch_reduce(b.depth, b.bgr, level, lo.t.max_jump, b.pyr[level], b.pyr_bgr[level]);
      const float *depth_m = b.model;
      const unsigned char *bgr_m = b.model_bgr;
      if (model.on_host) {
        upload_frame((const uint8_t *)model.bgr, (const float *)model.depth, colour ? b.model_bgr : nullptr, b.model, true);
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
      track_evaluate(t, level, lo, align_eval(map_motion(pose16, core_.o.voxel_size), c_src, lo.t.a, core_.o.voxel_size), model_pose16, sums, c);
      for (int i = 0; i < n; ++i) counts[i] = c[i];
      s.stats[0] = (uint64_t)locate_positions(track_level_grid(t.fg.lg, level)); s.stats[1] = c[0]; s.stats[2] = c[1]; s.stats[3] = 1; s.stats[6] = 1;
      s.level[level][2] = 1; s.level[level][3] = c[1];
    });
  }
  // The body of every *_frame call: the frame reduced once to every level above 0, then track_pyramid_schedule over track_loop;
  // po.levels = 1 is the single-level call.  r: level 0's result; last: the counters of its last evaluation.
  void track_levels(const char *who, TrackSide &s, bool colour, const TrackPyramidOpt &po, const FramePair &frame, const float *pose16, drf_align_result_t &r,
                    uint64_t last[5]) {
    with_track(who, s, colour, frame, po.c.t.step, [&](TrackCall &t) {
      for (int L = 1; L < po.levels; ++L) launch_reduce(t.b.depth, t.b.bgr, L, track_level_options(po, L).t.max_jump, t.b.pyr[L], t.b.pyr_bgr[L]);
      track_pyramid_schedule([&](int L, const float *p16, const TrackColourOpt &lo, drf_align_result_t &lr, uint64_t *lc, uint64_t *st2) {
        auto render = [&](const float *p) { track_render(t, L, lo, p); };
        auto eval = [&](const AlignEval &e, const float *mp16, double sums[28], uint64_t *c) { track_evaluate(t, L, lo, e, mp16, sums, c); };
        if (colour) track_loop<5>(render, eval, p16, lo.t, core_.o.voxel_size, lr, lc, st2);
        else track_loop<4>(render, eval, p16, lo.t, core_.o.voxel_size, lr, lc, st2);
      }, t.fg.lg, pose16, po, r, s.stats, s.level, last);
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
    frame_prologue(who, track_options_of(opt, core_.o.voxel_size, po.c), pose16, model_pose16);
    track_system_at(who, s, colour, 0, po, frame, model, model_pose16, pose16, sums, counts, colour ? 5 : 4);
  }
  template <class Options>
  std::string track_frame(const char *who, const FramePair &frame, const float *pose16, const Options *opt, float *pose16_out, drf_align_result_t *res) {
    constexpr bool colour = std::is_same<Options, drf_track_colour_options_t>::value;
    TrackSide &s = colour ? tc_ : tk_;
    s.reset();
    if (!frame.has(colour) || !pose16 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    TrackPyramidOpt po{{}, 1, 0};
    frame_prologue(who, track_options_of(opt, core_.o.voxel_size, po.c), pose16, nullptr);
    drf_align_result_t r;
    uint64_t last[5] = {0, 0, 0, 0, 0};
    track_levels(who, s, colour, po, frame, pose16, r, last);
    return track_note(who, s, r, last, colour ? ", " + std::to_string((unsigned long long)last[4]) + " with a colour term; " : std::string("; "), pose16_out, res);
  }
  const uint64_t *track_stats() const { return tk_.stats; }
  const uint64_t *track_colour_stats() const { return tc_.stats; }

  // The pyramid family: colour is decided by the images given (bgr null: the geometric kernels).
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
  // the reduction alone: a host pair through the scratch, or device images in place
  void track_reduce(const char *who, int level, float max_jump, const FramePair &in, void *bgr_out, void *depth_out) {
    tp_.reset();
    if (!in.depth || !depth_out || (in.bgr && !bgr_out)) fail(DR_ERR_ARG, "%s: null argument", who);
    if (!(max_jump >= 0.0f) || !std::isfinite(max_jump)) fail(DR_ERR_ARG, "%s: option max_jump is negative or not finite", who);
    if (!track_level_fits(core_.o.width, core_.o.height, level))
      fail(DR_ERR_ARG, "%s: level %d is outside 0..%d or below %d pixels on a side of the %dx%d camera", who, level, kTrackMaxLevels - 1, kTrackMinLevelSide, core_.o.height,
           core_.o.width);
    expect_integrate(who);
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
    frame_prologue(who, nullptr, pose16, model_pose16);
    track_system_at(who, tp_, colour, level, po, frame, model, model_pose16, pose16, sums, counts, 5);
  }
  std::string track_pyramid_frame(const char *who, const FramePair &frame, const float *pose16, const drf_track_pyramid_options_t *opt, float *pose16_out,
                                  drf_align_result_t *res) {
    tp_.reset();
    if (!frame.depth || !pose16 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    const TrackPyramidOpt po = track_pyramid_resolve(who, opt, nullptr);
    frame_prologue(who, nullptr, pose16, nullptr);
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

  // A depth frame found in the map from many poses (the rule: pose_host.h score_point / search_candidate / search_refine; DESIGN.md
  // §7c "Searching a pose lattice").  The score stage is scorer_'s (search_ops.h: k_search_points once, k_search_score in chunks, the
  // resident map through find_block); what the engine adds is its call order -- frame_prologue -- the frame's
  // intake, and the refinement: track_levels and with_locate + locate_loop as drf_track_frame and drf_locate_frame run them, on the
  // device image the score read.  Nothing of the map, the public render buffers or the streaming state is written.
  template <class Body>
  void with_score(const char *who, const char *bad_option, int step, size_t table_entries, const float *h_depth, const void *d_depth, Body &&body) {
    static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    frame_prologue(who, bad_option, identity, nullptr);  // the call's poses are many: body refuses them, each by its index
    float *mine = scorer_.prepare(step, table_entries);
    const float *depth = (const float *)d_depth;
    if (h_depth) {
      upload_frame(nullptr, h_depth, nullptr, mine);
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
    if (!bad) bad = track_options_of(topt, core_.o.voxel_size, po.c);
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
      search_refine(so, table.data(), search_select(score.data(), n, so.top_k), cost.data(), counts.data(), score.data(), n, core_.o.voxel_size,
                    [&](const float *p16, drf_align_result_t &tr) {
                      tk_.reset();
                      uint64_t last[5] = {0, 0, 0, 0, 0};
                      track_levels(who, tk_, false, po, frame, p16, tr, last);
                      scorer_.stats[4] += tk_.stats[4]; scorer_.stats[5] += tk_.stats[3];
                    },
                    [&](const float *p16, drf_align_result_t &lr) {
                      with_locate(who, nullptr, depth, p16, lopt, [&](const LocateOpt &l, auto &eval) { locate_loop(eval, map_motion(p16, core_.o.voxel_size), l, core_.o.voxel_size, lr); });
                      scorer_.stats[5] += lc_stats_[3];
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
  enum Next { kIntegrate, kRender, kGetRender };
  // the resident order: (blk_key, slot) pairs sorted by key, as mesh_tables sorts the keys -- the keys to res, keys and slots
  // left in mio_.keys / mio_.slot (drf_save_map, drf_merge_map)
  void sort_resident(int nres, std::vector<unsigned long long> &res) {
    if (nres <= 0) return;
    std::vector<int> iota((size_t)nres);
    for (int i = 0; i < nres; ++i) iota[i] = i;
    mio_.keys.reserve((size_t)nres, core_.int_stream); mio_.slot_in.reserve((size_t)nres, core_.int_stream);
    mio_.slot.reserve((size_t)nres, core_.int_stream); mio_.dst.reserve((size_t)nres, core_.int_stream);
    DR_HIP(hipMemcpy(mio_.slot_in.get(), iota.data(), (size_t)nres * 4, hipMemcpyHostToDevice));
    size_t tb = 0;
    DR_HIP(rocprim::radix_sort_pairs(nullptr, tb, core_.d.blk_key, mio_.keys.get(), mio_.slot_in.get(), mio_.slot.get(), (size_t)nres, 0, 63, core_.int_stream));
    mio_.tmp.reserve(std::max<size_t>(tb, 256), core_.int_stream);  // (never null: a null scratch is rocprim's size query)
    tb = mio_.tmp.capacity();
    DR_HIP(rocprim::radix_sort_pairs(mio_.tmp.get(), tb, core_.d.blk_key, mio_.keys.get(), mio_.slot_in.get(), mio_.slot.get(), (size_t)nres, 0, 63, core_.int_stream));
    DR_HIP(hipMemcpyAsync(res.data(), mio_.keys.get(), (size_t)nres * 8, hipMemcpyDeviceToHost, core_.int_stream));
    DR_HIP(hipStreamSynchronize(core_.int_stream));
  }
  // a load that failed half way: pool, block index and host store as a new engine has them (the counters were not touched)
  void clear_map() {
    streamer_.store() = HostBlockStore();
    const int placed = core_.pool_blocks();
    if (placed == 0) return;
    const size_t cap = (size_t)core_.d.cmask + 1;
    DR_HIP(hipMemsetAsync(core_.d.vals, 0xFF, cap * sizeof(int), core_.int_stream));
    hipLaunchKernelGGL(k_fill_keys, dim3(1024), dim3(256), 0, core_.int_stream, core_.d.keys, cap);
    DR_HIP(hipMemsetAsync(core_.d.vox, 0, (size_t)placed * 4096, core_.int_stream));
    for (int l = 0; l < kSuperLevels; ++l) DR_HIP(hipMemsetAsync(core_.d.super[l], 0, (size_t)1 << (3 * (kGridBits - kSuperShift[l])), core_.int_stream));
    DR_HIP(hipMemsetAsync(core_.d.present, 0, ((size_t)1 << (3 * kPresentBits - 5)) * sizeof(unsigned), core_.int_stream));
    DR_HIP(hipMemsetAsync(core_.d.grid, 0, ((size_t)1 << (3 * kGridBits)) * sizeof(int), core_.int_stream));
    DR_HIP(hipMemsetAsync(core_.d.n_alloc, 0, 4 * sizeof(int), core_.int_stream));
    DR_HIP(hipStreamSynchronize(core_.int_stream));
  }
  // slots of an open-addressing table over n staged blocks: a power of two, at least twice their number
  static size_t stage_table_slots(size_t n) { size_t s = 1024; while (s < 2 * n) s <<= 1; return s; }
  // ---- the render scope (DRF_RENDER_MAP; DESIGN.md §7c "Rendering the whole map") ----
  size_t rs_capacity() const { return rs_cap_req_ ? rs_cap_req_ : (size_t)std::min(core_.o.num_blocks, kStageBlocks); }
  size_t lc_capacity() const { return lc_cap_req_ ? lc_cap_req_ : (size_t)std::min(core_.o.num_blocks, kStageBlocks); }
  void locate_reset() {
    for (auto &v : lc_stats_) v = 0;
    for (auto &v : ls_stats_) v = 0;
  }
  // The union of stored blocks the poses can read.  Blocks the last scan's eviction chain gathered are not in the store yet: only
  // a pose that could reach one (render_needs_fold) waits for the scan and folds them first.
  RenderStagePlan plan_render(const float *const *poses, int n, bool &waited) {
    if (streamer_.fold_if_reachable(poses, n)) waited = true;
    return plan_render_stage(streamer_.store(), core_.o, poses, n);
  }
  // rs_ carries [keys | voxels]; each of its two slots has a table and staged superblock flags of its own.  Everything that touches a
  // slot on the device is ordered on rs_'s stream: copy, table clear, k_rs_build, and -- behind the cast events of the renders that
  // read it -- k_rs_clear.
  void ensure_render_staging(size_t n) {
    if (!rs_.stream()) {
      rs_.open(core_.own);
      for (auto &f : rs_super_)
        for (int l = 0; l < kSuperLevels; ++l) f[l] = core_.own.device<unsigned char>((size_t)1 << (3 * (kGridBits - kSuperShift[l])), rs_.stream());
    }
    if (n <= rs_blocks_) return;
    const size_t cap = locate_scope_ == DRF_LOCATE_MAP ? std::max(rs_capacity(), lc_capacity()) : rs_capacity();  // the larger need of its two users
    const size_t want = std::min(cap, std::max(2 * rs_blocks_, (n + 1023) & ~(size_t)1023));
    DR_HIP(hipDeviceSynchronize());  // no copy or kernel reads the old allocations
    rs_.reserve((want + 1) * 8 + want * 4096);
    for (auto &t : rs_table_) t.reserve(stage_table_slots(want), rs_.stream());
    rs_blocks_ = want;
  }
  RenderStage stage_render(const std::vector<unsigned long long> &keys) {
    const size_t n = keys.size(), nk = (n + 1) & ~(size_t)1;  // voxels start 16-byte aligned
    ensure_render_staging(n);
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
  void expect(Next want, const char *msg) {
    static const char *names[] = {"IntegrateScanAsync", "RenderAsync", "GetRenderResult"};
    if (next_ != want) fail(DR_ERR_PROTOCOL, "%s You should have called %s", msg, names[next_]);
  }
  void expect_integrate(const char *who) { expect(kIntegrate, (std::string(who) + ": call it where IntegrateScanAsync may be called.").c_str()); }
  // allocate -> integrate on core_.int_stream, no host round trip: the number of allocated blocks lives on the
  // device, so the integrate grid is fixed (a few workgroups per CU) and strides over [0, *n_alloc).
  // wait_renders: order the voxel UPDATE behind the ray-casts of the previous scan (they read the voxels).  The allocation pass, the
  // commit and the cull of this scan do not wait: they only turn absent blocks into present, EMPTY ones (zero voxels, weight 0), write
  // the per-pixel records and the visible list -- a ray that meets such a block mid-flight takes the same step as through an absent one
  // (weight 0 either way; the empty-space skip is conservative in both states), so a ray-cast of scan k that runs beside the allocation
  // of scan k + 1 returns the same image bit for bit, and a quarter of the scan (0.08 of 0.46 ms at 5 mm) leaves the critical path.
  void enqueue_scan(const unsigned char *d_bgr, const float *d_depth, const float *pose16, bool wait_renders = false) {
    Mat T, Ti;
    memcpy(T.m, pose16, 64);
    inverse4_host(T.m, Ti.m);
    mesher_.record_scan(Ti);
    hipLaunchKernelGGL(k_allocate, dim3(cdiv((int)core_.npix, 256)), dim3(256), 0, core_.int_stream, core_.d, d_bgr, d_depth, T);
    hipLaunchKernelGGL(k_alloc_commit, dim3(64), dim3(256), 0, core_.int_stream, core_.d);
    hipLaunchKernelGGL(k_cull, dim3(512), dim3(256), 0, core_.int_stream, core_.d, Ti);
    if (kernel_events_[2]) DR_HIP(hipEventRecord(kernel_events_[2], core_.int_stream));  // timing hook: end of allocate + commit + cull
    if (wait_renders) core_.wait_casts();
    if (kernel_events_[0]) DR_HIP(hipEventRecord(kernel_events_[0], core_.int_stream));  // timing hooks: [0]..[1] brackets k_integrate alone
    hipLaunchKernelGGL(k_integrate, dim3(integrate_grid_), dim3(256), 0, core_.int_stream, core_.d, d_bgr, d_depth, T, Ti);
    if (kernel_events_[1]) DR_HIP(hipEventRecord(kernel_events_[1], core_.int_stream));
    hipLaunchKernelGGL(k_fold_counter, dim3(1), dim3(256), 0, core_.int_stream, core_.d.cnt, core_.d.req_count, core_.d.wg_upd, integrate_grid_);
    DR_HIP(hipGetLastError());
  }
  // Correctly rounded reciprocals of the three per-engine divisors, each checked against IEEE division over all 2^32
  // dividends (see div_exact); DR_FUSION_IEEE_DIV=1 forces the IEEE sequences (A/B and fallback testing).
  static float rcp_rn(float b) { return (float)(1.0 / (double)b); }  // double rounding cannot bite: 1/b is never within 2^-49 of a float midpoint
  void setup_fast_div() {
    core_.d.vs_rcp = rcp_rn(core_.o.voxel_size); core_.d.fx_rcp = rcp_rn(core_.o.fx); core_.d.fy_rcp = rcp_rn(core_.o.fy);
    core_.d.fast_div = 0;
    if (hook_env("DR_FUSION_IEEE_DIV")) return;
    DeviceBuf<unsigned long long> counter;  // freed when the check is done
    counter.reserve(1, core_.int_stream);
    unsigned long long *bad = counter.get(), h = 0;
    DR_HIP(hipMemsetAsync(bad, 0, 8, core_.int_stream));
    const float b[3] = {core_.o.voxel_size, core_.o.fx, core_.o.fy}, y[3] = {core_.d.vs_rcp, core_.d.fx_rcp, core_.d.fy_rcp};
    for (int k = 0; k < 3; ++k)
      if (b[k] > 0.0f && b[k] < 1e30f) hipLaunchKernelGGL(k_verify_fast_div, dim3(4096), dim3(256), 0, core_.int_stream, b[k], y[k], bad);
      else h = 1;
    DR_HIP(hipMemcpyAsync(&fast_div_mismatches_, bad, 8, hipMemcpyDeviceToHost, core_.int_stream));
    DR_HIP(hipStreamSynchronize(core_.int_stream));
    fast_div_mismatches_ += h;
    core_.d.fast_div = fast_div_mismatches_ == 0 ? 1 : 0;
  }
  void check_device_flags() {
    int f[4];
    DR_HIP(hipMemcpy(f, core_.d.n_alloc, 16, hipMemcpyDeviceToHost));
    if (f[1] || f[2]) fail(DR_ERR_CAPACITY, "DrFusion: block pool exhausted (num_blocks=%d) or block coordinate out of range", core_.o.num_blocks);
  }

  FusionCore core_;          // first: its HipOwner is released after every other member
  BlockStreamer streamer_;   // the host store, evictions, stream-in (stream_ops.h)
  MeshExtractor mesher_;     // extraction, the map pass, the incremental mesh (mesh_ops.h)
  PoseScorer scorer_;        // the score stage of drf_score_poses / drf_search_frame and their statistics (search_ops.h)
  hipEvent_t kernel_events_[3] = {nullptr, nullptr, nullptr};
  unsigned char *d_bgr_in_ = nullptr, *h_bgr_in_ = nullptr;
  float *d_depth_in_ = nullptr, *h_depth_in_ = nullptr;
  int integrate_grid_ = 4096;
  unsigned long long fast_div_mismatches_ = 0;
  // switches, read once here, every one through hook_env(): the parity build (-DDR_PARITY_HOOKS) alone reads them, the product library reads
  // none.  DR_RAYCAST_NO_SKIP: the empty-space skip's A/B switch, a run-time flag of the product's kernel, and DR_FUSION_IEEE_DIV
  // (setup_fast_div): the IEEE-division instances, which the product takes only when the exact fast division fails its check.  Compiled
  // into the parity build only: the superseded generations -- the literal ray-caster, round 2's four-stage sampler, copy-engine result
  // transfers, statistics.
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
  Next next_ = kIntegrate;
  bool loaded_ = false;  // the map came from drf_load_map / drf_merge_map and no scan followed yet: RenderAsync is legal where IntegrateScanAsync is
  // render scope: staging opened by the first map-scope render that has stored blocks in reach, grown up to rs_capacity()
  BlockStaging rs_;
  DeviceBuf<unsigned long long> rs_table_[2];  // per slot of rs_: the open-addressing table and the two staged superblock flag arrays
  unsigned char *rs_super_[2][2] = {};
  int render_scope_ = DRF_RENDER_RESIDENT;
  size_t rs_cap_req_ = 0, rs_blocks_ = 0;
  uint64_t render_stats_[4] = {0, 0, 0, 0};
  int render_bands_ = 0;  // drf_set_render_bands
  uint64_t band_stats_[4] = {0, 0, 0, 0};
  // map file transport (map_ops.h; allocated with the first use): two pinned chunk buffers, the sorted (key, slot) pairs
  MapIo mio_;
  DeviceBuf<unsigned long long> mg_counts_;  // drf_merge_map: voxels of case 2 and case 3 counted by k_map_merge
  uint64_t mg_stats_[6] = {0, 0, 0, 0, 0, 0};  // drf_merge_stats
  DeviceBuf<unsigned char> lc_buf_;            // drf_locate_*: partial sums, counters and a host-given depth image (sized once)
  uint64_t lc_stats_[6] = {0, 0, 0, 0, 0, 0};  // drf_locate_stats
  TrackSide tk_, tc_, tp_;                     // drf_track_*, drf_track_colour_*, drf_track_reduce / drf_track_pyramid_*: each its own scratch, statistics and model render (with_track)
  unsigned long long *tc_fifth_ = nullptr;     // pinned: the fifth counter of an evaluation with colour
  int locate_scope_ = DRF_LOCATE_RESIDENT;     // drf_set_locate_scope
  size_t lc_cap_req_ = 0;
  uint64_t ls_stats_[4] = {0, 0, 0, 0};        // drf_locate_stage_stats
};

}  // namespace dr

// ==================================================================== C ABI
using dr::guarded;
struct drf_s {
  std::unique_ptr<dr::FusionEngine> e;
};
// every C-ABI entry point goes through this: a NULL handle is an argument error, not a crash
static inline dr::FusionEngine *eng(drf_s *h) {
  if (!h || !h->e) dr::fail(DR_ERR_ARG, "NULL handle");
  return h->e.get();
}
// A search for a pose (drf_align_map, drf_*_frame): DEGENERATE and LOST are results, not failures -- DR_OK, with the reason, the note
// call() returns, where a failure's message would be.
template <class Call>
static int guarded_note(Call &&call) {
  std::string note;
  const int rc = guarded([&] { note = call(); });
  if (rc == DR_OK && !note.empty()) dr::last_error_slot() = note;
  return rc;
}
// the six statistics of an operation's last call, through the engine's getter
static int stats6(drf_s *h, const char *who, uint64_t *out, const uint64_t *(dr::FusionEngine::*get)() const) {
  return guarded([&] {
    if (!out) dr::fail(DR_ERR_ARG, "%s: null argument", who);
    const uint64_t *s = (eng(h)->*get)();
    for (int i = 0; i < 6; ++i) out[i] = s[i];
  });
}

extern "C" {

int drf_create(const drf_options_t *opt, int device, drf_t **out) {
  return guarded([&] {
    if (!opt || !out) dr::fail(DR_ERR_ARG, "drf_create: null argument");
    auto *h = new drf_s();
    try { h->e.reset(new dr::FusionEngine(*opt, device)); } catch (...) { delete h; throw; }
    *out = h;
  });
}
void drf_destroy(drf_t *h) { delete h; }
int drf_integrate_scan_async(drf_t *h, const uint8_t *bgr, const float *depth, const float *pose16) {
  return guarded([&] { eng(h)->integrate_scan_async(bgr, depth, pose16); });
}
int drf_render_async(drf_t *h, const float *const *poses16, int n) { return guarded([&] { eng(h)->render_async(poses16, n); }); }
int drf_get_render_result(drf_t *h, uint8_t **bgr, float **depth, int n) { return guarded([&] { eng(h)->get_render_result(bgr, depth, n); }); }
int drf_extract_mesh_async(drf_t *h, const float *lower, const float *upper) {
  return guarded([&] { eng(h)->extract_mesh_async(lower, upper); });
}
int drf_get_mesh_sync(drf_t *h, size_t num_max, size_t *num, float *vert, float *cols) {
  return guarded([&] { eng(h)->get_mesh_sync(num_max, num, vert, cols); });
}
int drf_mesh_num_triangles(drf_t *h, size_t *ntri) {
  return guarded([&] { if (!ntri) dr::fail(DR_ERR_ARG, "drf_mesh_num_triangles: null argument"); *ntri = eng(h)->mesh().mesh_num_triangles(); });
}
int drf_save_mesh(drf_t *h, const char *filename, const float *lower, const float *upper) {
  return guarded([&] { eng(h)->mesh().save_mesh(filename, lower, upper); });
}
int drf_get_render_device(drf_t *h, int stream, const uint8_t **d_bgr, const float **d_depth) {
  return guarded([&] { eng(h)->get_render_device(stream, d_bgr, d_depth); });
}
int drf_synchronize(drf_t *h) { return guarded([&] { eng(h)->synchronize(); }); }
int drf_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->stats(out); }); }
int drf_export_blocks(drf_t *h, int max_blocks, int32_t *coords, uint8_t *voxels, int *n) {
  return guarded([&] { eng(h)->export_blocks(max_blocks, coords, voxels, n); });
}
int drf_fast_div_status(drf_t *h, int *enabled, uint64_t *mismatches) {
  return guarded([&] { unsigned long long m = 0; eng(h)->fast_div_status(enabled, &m); if (mismatches) *mismatches = m; });
}
int drf_test_combine(drf_t *h, size_t n, const uint8_t *a, const uint8_t *b, int max_weight, uint8_t *out) {
  return guarded([&] { if (!a || !b || !out) dr::fail(DR_ERR_ARG, "drf_test_combine: null argument"); eng(h)->test_combine(n, a, b, max_weight, out); });
}
int drf_integrate_device(drf_t *h, const void *d_bgr, const void *d_depth, const float *pose16) {
  return guarded([&] { eng(h)->integrate_device(d_bgr, d_depth, pose16); });
}
int dr_device_alloc(int device, size_t bytes, void **dptr) {
  return guarded([&] { DR_HIP(hipSetDevice(device)); DR_HIP(dr::device_alloc(dptr, bytes, "dr_device_alloc")); });
}
int dr_device_free(void *dptr) { return guarded([&] { DR_HIP(dr::device_free(dptr)); }); }
// The guarded allocator's switch and its check (dr_common.h, guard_host.h): parity build only.
int dr_guard_set(size_t guard_bytes) {
  return guarded([&] {
#ifndef DR_PARITY_HOOKS
    (void)guard_bytes;
    dr::fail(DR_ERR_UNSUPPORTED, "dr_guard_set: guarded allocation is built into the parity library (libdr_mi355x_hooks.so, -DDR_PARITY_HOOKS) only");
#else
    if (guard_bytes % dr::guard::kGranule) dr::fail(DR_ERR_ARG, "dr_guard_set: the guard size must be a multiple of %zu bytes (0: off)", dr::guard::kGranule);
    dr::guard::Registry &r = dr::guard::registry();
    std::lock_guard<std::mutex> lk(r.mu);
    r.guard_bytes = guard_bytes;
#endif
  });
}
int dr_guard_check(uint64_t out[4], char *report, size_t cap) {
  return guarded([&] {
#ifndef DR_PARITY_HOOKS
    (void)out; (void)report; (void)cap;
    dr::fail(DR_ERR_UNSUPPORTED, "dr_guard_check: guarded allocation is built into the parity library (libdr_mi355x_hooks.so, -DDR_PARITY_HOOKS) only");
#else
    if (!out) dr::fail(DR_ERR_ARG, "dr_guard_check: null argument");
    dr::guard::Registry &r = dr::guard::registry();
    std::lock_guard<std::mutex> lk(r.mu);
    std::vector<dr::guard::Violation> all = r.sticky;
    uint64_t bytes = 0;
    if (!r.live.empty()) DR_HIP(hipDeviceSynchronize());
    for (auto &kv : r.live) { dr::guard::scan_entry(kv.first, kv.second, all); bytes += kv.second.bytes; }
    out[0] = r.live.size(); out[1] = r.since_clear; out[2] = all.size(); out[3] = bytes;
    dr::guard::report(all, report, cap);
#endif
  });
}
int dr_guard_clear(void) {
  return guarded([&] {
#ifndef DR_PARITY_HOOKS
    dr::fail(DR_ERR_UNSUPPORTED, "dr_guard_clear: guarded allocation is built into the parity library (libdr_mi355x_hooks.so, -DDR_PARITY_HOOKS) only");
#else
    dr::guard::Registry &r = dr::guard::registry();
    std::lock_guard<std::mutex> lk(r.mu);
    r.sticky.clear();
    r.since_clear = 0;
#endif
  });
}
int dr_memcpy_h2d(void *dptr, const void *src, size_t bytes) { return guarded([&] { DR_HIP(hipMemcpy(dptr, src, bytes, hipMemcpyHostToDevice)); }); }
int dr_memcpy_d2d(void *dst, const void *src, size_t bytes) {
  // a device-to-device hipMemcpy may return before the copy has run, and the engines' streams are non-blocking:
  // synchronise so that whatever the caller enqueues next (on any stream) sees the data
  return guarded([&] {
    hipPointerAttribute_t at;  // synchronise the device that owns the destination, not whichever is current on this thread --
    int prev = -1;             // and leave the caller's current device as it was (a helper must not move a host thread between GPUs)
    (void)hipGetDevice(&prev);
    const bool moved = hipPointerGetAttributes(&at, dst) == hipSuccess && at.device != prev;
    if (moved) DR_HIP(hipSetDevice(at.device));
    const hipError_t e1 = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice);
    const hipError_t e2 = e1 == hipSuccess ? hipDeviceSynchronize() : e1;
    if (moved && prev >= 0) (void)hipSetDevice(prev);
    DR_HIP(e2);
  });
}
int dr_memcpy_d2h(void *dst, const void *dptr, size_t bytes) { return guarded([&] { DR_HIP(hipMemcpy(dst, dptr, bytes, hipMemcpyDeviceToHost)); }); }
int drf_bench_sequence(drf_t *h, const void *d_bgr, const void *d_depth, const float *poses16, int nframes, int render, float ms[6]) {
  return guarded([&] { eng(h)->bench_sequence(d_bgr, d_depth, poses16, nframes, render, ms); });
}
int drf_visited_blocks(drf_t *h, uint64_t *total) {
  return guarded([&] { if (!total) dr::fail(DR_ERR_ARG, "drf_visited_blocks: null pointer"); *total = eng(h)->visited_blocks(); });
}
int drf_bench_render_host(drf_t *h, int stream, int back, const uint8_t **bgr, const float **depth) {
  return guarded([&] { eng(h)->bench_render_host(stream, back, bgr, depth); });
}
int drf_bench_integrate(drf_t *h, const void *d_bgr, const void *d_depth, const float *poses16, int nscans, float *ms, float *kernel_ms) {
  return guarded([&] { eng(h)->bench_integrate(d_bgr, d_depth, poses16, nscans, ms, kernel_ms); });
}
int drf_streaming_min_radius(const drf_options_t *o, float *radius) {
  return guarded([&] {
    if (!o || !radius) dr::fail(DR_ERR_ARG, "drf_streaming_min_radius: null argument");
    if (!dr::stream_options_ok(*o)) dr::fail(DR_ERR_ARG, "drf_streaming_min_radius: invalid options (voxel_size, fx, fy, max_sensor_depth must be > 0, width and height > 0)");
    *radius = dr::streaming_min_radius(*o);
  });
}
int drf_set_streaming(drf_t *h, float radius, size_t host_capacity_blocks) {
  return guarded([&] { eng(h)->streaming().set_streaming(radius, host_capacity_blocks); });
}
int drf_stream_out_region(drf_t *h, const float lower[3], const float upper[3]) {
  return guarded([&] { eng(h)->stream_out_region(lower, upper); });
}
int drf_stream_in_region(drf_t *h, const float lower[3], const float upper[3]) {
  return guarded([&] { eng(h)->stream_in_region(lower, upper); });
}
int drf_streaming_stats(drf_t *h, uint64_t out[6]) {
  return guarded([&] { if (!out) dr::fail(DR_ERR_ARG, "drf_streaming_stats: null argument"); eng(h)->streaming().streaming_stats(out); });
}
int drf_export_host_blocks(drf_t *h, int max_blocks, int32_t *coords, uint8_t *voxels, int *n) {
  return guarded([&] { eng(h)->streaming().export_host_blocks(max_blocks, coords, voxels, n); });
}
int drf_map_info(const char *path, float *voxel_size, uint64_t *n_blocks) {
  return guarded([&] {
    if (!path || !voxel_size || !n_blocks) dr::fail(DR_ERR_ARG, "drf_map_info: null argument");
    std::string err;
    if (!dr::map_file_info(path, voxel_size, n_blocks, err)) dr::fail(DR_ERR_IO, "drf_map_info: %s", err.c_str());
  });
}
int drf_save_map(drf_t *h, const char *path, size_t chunk_blocks) { return guarded([&] { eng(h)->save_map(path, chunk_blocks); }); }
int drf_load_map(drf_t *h, const char *path, size_t chunk_blocks) { return guarded([&] { eng(h)->load_map(path, chunk_blocks); }); }
int drf_merge_map(drf_t *h, const char *path, size_t chunk_blocks) { return guarded([&] { eng(h)->merge_map(path, chunk_blocks); }); }
int drf_merge_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_merge_stats", out, &dr::FusionEngine::merge_stats); }
int drf_transform_map(drf_t *h, const char *src_path, const float T16[16], const char *dst_path, size_t chunk_blocks) {
  return guarded([&] { eng(h)->transform_map(src_path, T16, dst_path, chunk_blocks); });
}
int drf_transform_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_transform_stats", out, &dr::FusionEngine::transform_stats); }
int drf_align_system(drf_t *h, const char *src_path, const char *ref_path, const float T16[16], const drf_align_options_t *opt, double sums[28],
                     uint64_t counts[3]) {
  return guarded([&] { eng(h)->align_system(src_path, ref_path, T16, opt, sums, counts); });
}
int drf_align_map(drf_t *h, const char *src_path, const char *ref_path, const float T_init16[16], const drf_align_options_t *opt, float T16_out[16],
                  drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->align_map(src_path, ref_path, T_init16, opt, T16_out, res); });
}
int drf_align_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_align_stats", out, &dr::FusionEngine::align_stats); }
int drf_locate_system(drf_t *h, const float *depth, const float pose16[16], const drf_locate_options_t *opt, double sums[28], uint64_t counts[4]) {
  return guarded([&] { eng(h)->locate_system("drf_locate_system", depth, nullptr, pose16, opt, sums, counts); });
}
int drf_locate_system_device(drf_t *h, const void *d_depth, const float pose16[16], const drf_locate_options_t *opt, double sums[28], uint64_t counts[4]) {
  return guarded([&] { eng(h)->locate_system("drf_locate_system_device", nullptr, d_depth, pose16, opt, sums, counts); });
}
int drf_locate_frame(drf_t *h, const float *depth, const float pose_init16[16], const drf_locate_options_t *opt, float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->locate_frame("drf_locate_frame", depth, nullptr, pose_init16, opt, pose16_out, res); });
}
int drf_locate_frame_device(drf_t *h, const void *d_depth, const float pose_init16[16], const drf_locate_options_t *opt, float pose16_out[16],
                            drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->locate_frame("drf_locate_frame_device", nullptr, d_depth, pose_init16, opt, pose16_out, res); });
}
int drf_locate_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_locate_stats", out, &dr::FusionEngine::locate_stats); }
using dr::FramePair;
int drf_track_system(drf_t *h, const float *depth, const float *model_depth, const float model_pose16[16], const float pose16[16], const drf_track_options_t *opt,
                     double sums[28], uint64_t counts[4]) {
  return guarded([&] {
    eng(h)->track_system("drf_track_system", FramePair::host(nullptr, depth), FramePair::host(nullptr, model_depth), model_pose16, pose16, opt, sums, counts);
  });
}
int drf_track_system_device(drf_t *h, const void *d_depth, const void *d_model_depth, const float model_pose16[16], const float pose16[16],
                            const drf_track_options_t *opt, double sums[28], uint64_t counts[4]) {
  return guarded([&] {
    eng(h)->track_system("drf_track_system_device", FramePair::device(nullptr, d_depth), FramePair::device(nullptr, d_model_depth), model_pose16, pose16, opt, sums, counts);
  });
}
int drf_track_frame(drf_t *h, const float *depth, const float pose_init16[16], const drf_track_options_t *opt, float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_frame("drf_track_frame", FramePair::host(nullptr, depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_frame_device(drf_t *h, const void *d_depth, const float pose_init16[16], const drf_track_options_t *opt, float pose16_out[16],
                           drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_frame("drf_track_frame_device", FramePair::device(nullptr, d_depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_track_stats", out, &dr::FusionEngine::track_stats); }
int drf_track_colour_system(drf_t *h, const uint8_t *bgr, const float *depth, const uint8_t *model_bgr, const float *model_depth, const float model_pose16[16],
                            const float pose16[16], const drf_track_colour_options_t *opt, double sums[28], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track_system("drf_track_colour_system", FramePair::host(bgr, depth), FramePair::host(model_bgr, model_depth), model_pose16, pose16, opt, sums, counts);
  });
}
int drf_track_colour_system_device(drf_t *h, const void *d_bgr, const void *d_depth, const void *d_model_bgr, const void *d_model_depth, const float model_pose16[16],
                                   const float pose16[16], const drf_track_colour_options_t *opt, double sums[28], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track_system("drf_track_colour_system_device", FramePair::device(d_bgr, d_depth), FramePair::device(d_model_bgr, d_model_depth), model_pose16, pose16, opt, sums,
                         counts);
  });
}
int drf_track_colour_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float pose_init16[16], const drf_track_colour_options_t *opt, float pose16_out[16],
                           drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_frame("drf_track_colour_frame", FramePair::host(bgr, depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_colour_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float pose_init16[16], const drf_track_colour_options_t *opt,
                                  float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_frame("drf_track_colour_frame_device", FramePair::device(d_bgr, d_depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_colour_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_track_colour_stats", out, &dr::FusionEngine::track_colour_stats); }
int drf_track_reduce(drf_t *h, int level, float max_jump, const uint8_t *bgr, const float *depth, uint8_t *bgr_out, float *depth_out) {
  return guarded([&] { eng(h)->track_reduce("drf_track_reduce", level, max_jump, FramePair::host(bgr, depth), bgr_out, depth_out); });
}
int drf_track_reduce_device(drf_t *h, int level, float max_jump, const void *d_bgr, const void *d_depth, void *d_bgr_out, void *d_depth_out) {
  return guarded([&] { eng(h)->track_reduce("drf_track_reduce_device", level, max_jump, FramePair::device(d_bgr, d_depth), d_bgr_out, d_depth_out); });
}
int drf_track_pyramid_system(drf_t *h, int level, const uint8_t *bgr, const float *depth, const uint8_t *model_bgr, const float *model_depth,
                             const float model_pose16[16], const float pose16[16], const drf_track_pyramid_options_t *opt, double sums[28], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track_pyramid_system("drf_track_pyramid_system", level, FramePair::host(bgr, depth), FramePair::host(model_bgr, model_depth), model_pose16, pose16, opt, sums,
                                 counts);
  });
}
int drf_track_pyramid_system_device(drf_t *h, int level, const void *d_bgr, const void *d_depth, const void *d_model_bgr, const void *d_model_depth,
                                    const float model_pose16[16], const float pose16[16], const drf_track_pyramid_options_t *opt, double sums[28],
                                    uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track_pyramid_system("drf_track_pyramid_system_device", level, FramePair::device(d_bgr, d_depth), FramePair::device(d_model_bgr, d_model_depth), model_pose16,
                                 pose16, opt, sums, counts);
  });
}
int drf_track_pyramid_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float pose_init16[16], const drf_track_pyramid_options_t *opt,
                            float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_pyramid_frame("drf_track_pyramid_frame", FramePair::host(bgr, depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_pyramid_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float pose_init16[16], const drf_track_pyramid_options_t *opt,
                                   float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_pyramid_frame("drf_track_pyramid_frame_device", FramePair::device(d_bgr, d_depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_pyramid_stats(drf_t *h, uint64_t out[8]) {
  return guarded([&] {
    if (!out) dr::fail(DR_ERR_ARG, "drf_track_pyramid_stats: null argument");
    const uint64_t *s = eng(h)->track_pyramid_stats();
    for (int i = 0; i < 8; ++i) out[i] = s[i];
  });
}
int drf_track_pyramid_level_stats(drf_t *h, int level, uint64_t out[4]) {
  return guarded([&] {
    if (!out) dr::fail(DR_ERR_ARG, "drf_track_pyramid_level_stats: null argument");
    const uint64_t *s = eng(h)->track_pyramid_level_stats(level);
    for (int i = 0; i < 4; ++i) out[i] = s[i];
  });
}
int drf_score_poses(drf_t *h, const float *depth, const float *poses16, size_t n, const drf_score_options_t *opt, double *cost, uint32_t *counts, double *score) {
  return guarded([&] { eng(h)->score_poses("drf_score_poses", depth, nullptr, poses16, n, opt, cost, counts, score); });
}
int drf_score_poses_device(drf_t *h, const void *d_depth, const float *poses16, size_t n, const drf_score_options_t *opt, double *cost, uint32_t *counts,
                           double *score) {
  return guarded([&] { eng(h)->score_poses("drf_score_poses_device", nullptr, d_depth, poses16, n, opt, cost, counts, score); });
}
int drf_search_frame(drf_t *h, const float *depth, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot, const drf_search_options_t *opt,
                     const drf_track_options_t *track_opt, const drf_locate_options_t *locate_opt, float pose16_out[16], drf_search_result_t *res, double *all_scores) {
  return guarded_note([&] {
    return eng(h)->search_frame("drf_search_frame", depth, nullptr, anchors16, n_anchors, rotations9, n_rot, opt, track_opt, locate_opt, pose16_out, res, all_scores);
  });
}
int drf_search_frame_device(drf_t *h, const void *d_depth, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot,
                            const drf_search_options_t *opt, const drf_track_options_t *track_opt, const drf_locate_options_t *locate_opt, float pose16_out[16],
                            drf_search_result_t *res, double *all_scores) {
  return guarded_note([&] {
    return eng(h)->search_frame("drf_search_frame_device", nullptr, d_depth, anchors16, n_anchors, rotations9, n_rot, opt, track_opt, locate_opt, pose16_out, res,
                                all_scores);
  });
}
int drf_search_stats(drf_t *h, uint64_t out[8]) { return guarded([&] { eng(h)->search_stats(out); }); }
int drf_set_locate_scope(drf_t *h, int scope, size_t stage_capacity_blocks) { return guarded([&] { eng(h)->set_locate_scope(scope, stage_capacity_blocks); }); }
int drf_locate_stage_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->locate_stage_stats(out); }); }
int drf_set_render_scope(drf_t *h, int scope, size_t stage_capacity_blocks) { return guarded([&] { eng(h)->set_render_scope(scope, stage_capacity_blocks); }); }
int drf_render_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->render_stats(out); }); }
int drf_set_render_bands(drf_t *h, int max_passes) { return guarded([&] { eng(h)->set_render_bands(max_passes); }); }
int drf_render_band_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->render_band_stats(out); }); }
int drf_set_mesh_scope(drf_t *h, int scope) { return guarded([&] { eng(h)->mesh().set_mesh_scope(scope); }); }
int drf_mesh_stats(drf_t *h, uint64_t out[3]) { return guarded([&] { eng(h)->mesh().mesh_stats(out); }); }
int drf_extract_mesh_update_async(drf_t *h, const float *lower, const float *upper) {
  return guarded([&] { eng(h)->extract_mesh_update_async(lower, upper); });
}
int drf_mesh_update_size(drf_t *h, size_t *nblk, size_t *ntri, int *full) { return guarded([&] { eng(h)->mesh().mesh_update_size(nblk, ntri, full); }); }
int drf_get_mesh_update_sync(drf_t *h, size_t max_blocks, size_t num_max, size_t *nblk, int32_t *coords, uint64_t *first, size_t *num,
                             float *vert, float *cols, int *full) {
  return guarded([&] { eng(h)->mesh().get_mesh_update_sync(max_blocks, num_max, nblk, coords, first, num, vert, cols, full); });
}
int drf_mesh_update_reset(drf_t *h) { return guarded([&] { eng(h)->mesh().force_full_update(); }); }
int drf_mesh_update_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->mesh().mesh_update_stats(out); }); }

}  // extern "C"
