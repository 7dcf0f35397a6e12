// dr_fusion.hip -- MI355X engine behind the DrFusion operator API (C ABI: include/dr_mi355x.h).
//
// The engine (FusionEngine: scans, the bench hooks, the map file, and in front of its components the checks that must precede their
// bodies) and the C ABI.  The volume's device code and the table of reference counterparts: volume_kernels.h.  What the engine lends
// its components: fusion_core.h (FusionCore, with the call order: engine_host.h CallOrder); streaming: stream_ops.h (BlockStreamer);
// meshing and the incremental mesh: mesh_ops.h (MeshExtractor); the staging of stored blocks and the renders: render_ops.h (MapStage,
// MapRenderer); a pose from a frame: pose_ops.h (FramePose, FrameLocator, FrameTracker); the pose search: search_ops.h (PoseScorer,
// PoseSearch).  DESIGN.md "Where streaming and meshing live", "Where rendering and the frame pose live".
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
#include "track_exposure_kernels.h"  // k_track_exposure, k_exposure_fold (drf_track_exposure_system, drf_track_exposure_frame)
#include "search_kernels.h"  // k_search_points, k_search_score (drf_score_poses, drf_search_frame) and their colour forms (drf_score_colour_poses, drf_search_colour_frame)

}  // namespace dr
#include "mesh_kernels.h"
#include "mesh_update_kernels.h"
#include "map_ops.h"  // MapIo: what the map-file operations share; drf_transform_map / drf_align_* whole
#include "fusion_core.h"  // FusionCore: what the engine lends its components
#include "stream_ops.h"   // BlockStreamer
#include "mesh_ops.h"     // MeshExtractor
#include "render_ops.h"   // MapStage, MapRenderer
#include "pose_ops.h"     // FramePose, FrameLocator, FrameTracker
#include "search_ops.h"   // PoseScorer, PoseSearch
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

// ------------------------------------------------------------------ engine
constexpr int kDefaultFusionPriority = 1;  // 0 least (the reference's), 1 normal (measured best in the TandemBackend loop), 2 greatest
class FusionEngine {
 public:
  FusionEngine(const drf_options_t &o, int device)
      : core_(o, device), streamer_(core_), mesher_(core_, streamer_), mio_(core_.own, device, o.voxel_size, (size_t)std::min(o.num_blocks, kStageBlocks)),
        stage_(core_, streamer_), renderer_(core_, streamer_, stage_), frame_(core_, streamer_, mio_), locator_(frame_, stage_), tracker_(frame_, renderer_),
        search_(frame_, tracker_, locator_, stage_) {
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
    core_.d_bgr_in = core_.own.device<unsigned char>(core_.npix * 3);
    core_.d_depth_in = core_.own.device<float>(core_.npix);
    core_.h_bgr_in = core_.own.pinned<unsigned char>(core_.npix * 3);
    core_.h_depth_in = core_.own.pinned<float>(core_.npix);
    // 12 workgroups per CU: enough to keep every SIMD's 4 resident waves busy, few enough that the blocks being worked on
    // at any moment are neighbours in the pool (sweep on the bench map: 1024 / 3072 / 4096 / 6144 / 8192 / 16384
    // workgroups -> 0.341 / 0.327 / 0.329 / 0.363 / 0.443 / 0.697 ms per scan)
    integrate_grid_ = std::min(cdiv(o.num_blocks, 4), 3072);
    if (const char *e = hook_env("DR_INT_GRID")) integrate_grid_ = std::min(65536, std::max(1, atoi(e)));  // tuning hook
    core_.int_done = core_.own.event();
    renderer_.open(lo);  // the render slots
    DR_HIP(hipStreamSynchronize(core_.int_stream));
  }
  ~FusionEngine() {  // the device idle before the growable scratch goes; core_.own (declared first, so released last) frees the rest
    (void)hipSetDevice(core_.device);
    (void)hipDeviceSynchronize();
  }

  // tsdf_volume.cu:515-598
  void integrate_scan_async(const uint8_t *bgr, const float *depth, const float *pose16) {
    if (!bgr || !depth || !pose16) fail(DR_ERR_ARG, "IntegrateScanAsync: null argument");
    core_.order.expect(CallOrder::kIntegrate, "Please call the functions like Integration -> RenderAsync -> GetRenderResults.");
    if (!streamer_.on() && !streamer_.store().empty()) fail(DR_ERR_PROTOCOL, "IntegrateScanAsync: %zu blocks are in the host store while streaming is off; bring them back with drf_stream_in_region first", streamer_.store().size());
    core_.order.scan_begun();
    DR_HIP(hipSetDevice(core_.device));
    const float depth_bound = streamer_.on() ? max_valid_depth(depth, core_.npix, core_.o.min_sensor_depth, core_.o.max_sensor_depth) : 0.0f;
    scan_between_streaming(pose16, depth_bound, [&] {
      core_.upload_frame(bgr, depth, core_.d_bgr_in, core_.d_depth_in);
      // the ray-casts read the volume; their result copies do not (the reference waits for the copies, tsdf_volume.cu:553-556)
      enqueue_scan(core_.d_bgr_in, core_.d_depth_in, pose16, true);
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
  // ---- the renders and the staging of stored blocks: render_ops.h ----
  MapRenderer &render() { return renderer_; }
  void bench_render_host(int i, int back, const uint8_t **bgr, const float **depth) {
    no_bench_while_streaming("drf_bench_render_host");
    renderer_.bench_render_host(i, back, bgr, depth);
  }
  void synchronize() {
    DR_HIP(hipSetDevice(core_.device));
    DR_HIP(hipDeviceSynchronize());
    core_.check_device_flags();
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
    core_.order.expect(CallOrder::kIntegrate, "Please call this functions after GetRenderResult.");
    mesher_.extract_mesh_async(lower, upper);
  }
  void get_mesh_sync(size_t num_max, size_t *num, float *vert, float *cols) {
    core_.order.expect(CallOrder::kIntegrate, "Please call this functions after GetRenderResult.");
    mesher_.get_mesh_sync(num_max, num, vert, cols);
  }
  void extract_mesh_update_async(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "drf_extract_mesh_update_async: null argument");
    core_.order.expect(CallOrder::kIntegrate, "Please call this functions after GetRenderResult.");
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
    core_.check_device_flags();
  }

  // BASELINE configs[3] loop (dr_debug_example.cpp:78-162: GetRenderResult(k-1) / IntegrateScanAsync(k) / RenderAsync(k) per
  // frame, map growing) over `n` frames whose inputs are resident in HBM: allocate + integrate on the integration stream,
  // then -- render != 0 -- one ray-cast per render stream from the frame's own pose with the D2H of its result into the
  // pinned double buffers, ordered by the same events as the operator path.  ms[0] = first allocate .. last copy
  // (hipEvents), ms[1..4] = sums of the allocate / integrate / ray-cast / D2H intervals, ms[5] = host wall clock.
  void bench_sequence(const void *d_bgr, const void *d_depth, const float *poses, int n, int render, float ms[6]) {
    no_bench_while_streaming("drf_bench_sequence");
    if (!d_bgr || !d_depth || !poses || !ms || n <= 0) fail(DR_ERR_ARG, "bench_sequence: bad argument");
    core_.order.expect(CallOrder::kIntegrate, "bench_sequence starts where IntegrateScanAsync may be called.");
    DR_HIP(hipSetDevice(core_.device));
    const int nr = render ? renderer_.slots() : 0;
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
      renderer_.flip();
      for (int i = 0; i < nr; ++i) {
        Mat P; memcpy(P.m, poses + 16 * s, 64);
        renderer_.submit(i, P, e + 4 + 3 * i);
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
    core_.check_device_flags();
  }

  // ---- streaming: stream_ops.h ----
  void stream_out_region(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "drf_stream_out_region: null argument");
    core_.order.expect(CallOrder::kIntegrate, "drf_stream_out_region: call it where IntegrateScanAsync may be called.");
    streamer_.stream_out_region(lower, upper);
  }
  void stream_in_region(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "drf_stream_in_region: null argument");
    core_.order.expect(CallOrder::kIntegrate, "drf_stream_in_region: call it where IntegrateScanAsync may be called.");
    streamer_.stream_in_region(lower, upper);
  }
  BlockStreamer &streaming() { return streamer_; }  // the entry points no call order guards (the C ABI below)

  // ---- the map file (include/dr_mi355x.h "map files"; DESIGN.md §7c "Saving and loading the map") ----
  // Resident and stored blocks merged in ascending key order, chunk by chunk: k_map_gather writes a chunk's resident blocks
  // straight into one of two pinned buffers while the host copies the stored ones into their positions of it, appends the
  // other buffer to the file and folds it into the checksum.  Folds pending evictions first; beyond that nothing changes.
  void save_map(const char *path, size_t chunk_blocks) {
    if (!path) fail(DR_ERR_ARG, "drf_save_map: null argument");
    core_.order.expect(CallOrder::kIntegrate, "drf_save_map: call it where IntegrateScanAsync may be called.");
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
    core_.order.expect(CallOrder::kIntegrate, "drf_load_map: call it where IntegrateScanAsync may be called.");
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
    if (n == 0) { core_.order.map_loaded(); return; }
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
    core_.order.map_loaded();
  }

  // A map file merged into the map (the rule: fusion_host.h merge_voxel).  The file validated and every block classified against
  // the map (plan_merge) before anything changes; then chunk by chunk through the two pinned buffers: k_map_merge combines the
  // blocks whose key is resident in place, k_in_place_at appends the new ones (streaming off) while the host combines the
  // chunk's stored blocks into the store, puts the new ones there (streaming on) and reads the next chunk.  A file that changes
  // under the second pass leaves a mixture of merged and untouched blocks (DR_ERR_IO; merge_stats tells how far it got).
  void merge_map(const char *path, size_t chunk_blocks) {
    if (!path) fail(DR_ERR_ARG, "drf_merge_map: null argument");
    core_.order.expect(CallOrder::kIntegrate, "drf_merge_map: call it where IntegrateScanAsync may be called.");
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
    if (n == 0) { core_.order.map_loaded(); return; }
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
    core_.order.map_loaded();
  }
  const uint64_t *merge_stats() const { return mg_stats_; }

  // Operations on map files alone (map_ops.h: map_transform, map_align_system, map_align).  The engine lends mio_ -- its device,
  // core_.int_stream, the pinned pair, voxel_size -- and states where in its call order they may run; its own map is neither read nor changed.
  void transform_map(const char *src, const float *T16, const char *dst, size_t chunk_blocks) {
    map_transform(mio_, src, T16, dst, chunk_blocks, [&] { core_.order.expect_integrate("drf_transform_map"); });
  }
  const uint64_t *transform_stats() const { return mio_.xf_stats; }
  void align_system(const char *src, const char *ref, const float *T16, const drf_align_options_t *opt, double *sums, uint64_t *counts) {
    map_align_system(mio_, src, ref, T16, opt, sums, counts, [&](const char *who) { core_.order.expect_integrate(who); });
  }
  // returns what dr_last_error() says after a registration that ran but found no pose (empty otherwise)
  std::string align_map(const char *src, const char *ref, const float *T16, const drf_align_options_t *opt, float *T16_out, drf_align_result_t *res) {
    return map_align(mio_, src, ref, T16, opt, T16_out, res, [&](const char *who) { core_.order.expect_integrate(who); });
  }
  const uint64_t *align_stats() const { return mio_.al_stats; }

  // ---- a camera pose from a frame: pose_ops.h, search_ops.h (their null arguments and the call order are the components' own) ----
  FrameLocator &locate() { return locator_; }
  FrameTracker &track() { return tracker_; }
  PoseSearch &search() { return search_; }
  const uint64_t *locate_stats() const { return locator_.locate_stats(); }
  const uint64_t *track_stats() const { return tracker_.track_stats(); }
  const uint64_t *track_colour_stats() const { return tracker_.track_colour_stats(); }

 private:
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

  FusionCore core_;          // first: its HipOwner is released after every other member
  BlockStreamer streamer_;   // the host store, evictions, stream-in (stream_ops.h)
  MeshExtractor mesher_;     // extraction, the map pass, the incremental mesh (mesh_ops.h)
  // map file transport (map_ops.h; allocated with the first use): two pinned chunk buffers, the sorted (key, slot) pairs
  MapIo mio_;
  MapStage stage_;           // stored blocks staged for the kernels that read them: renders, the tracking's model, the locate scope (render_ops.h)
  MapRenderer renderer_;     // the render slots, the one submit, render scope and depth bands (render_ops.h)
  FramePose frame_;          // what the pose families open with (pose_ops.h)
  FrameLocator locator_;     // drf_locate_* and the locate scope (pose_ops.h)
  FrameTracker tracker_;     // drf_track_*, drf_track_colour_*, drf_track_reduce / drf_track_pyramid_*, drf_track_exposure_* (pose_ops.h)
  PoseSearch search_;        // drf_score_poses / drf_search_frame over the score stage, the tracker and the locator (search_ops.h)
  hipEvent_t kernel_events_[3] = {nullptr, nullptr, nullptr};
  int integrate_grid_ = 4096;
  unsigned long long fast_div_mismatches_ = 0;  // setup_fast_div; DR_FUSION_IEEE_DIV (parity build) forces the IEEE-division instances
  DeviceBuf<unsigned long long> mg_counts_;  // drf_merge_map: voxels of case 2 and case 3 counted by k_map_merge
  uint64_t mg_stats_[6] = {0, 0, 0, 0, 0, 0};  // drf_merge_stats
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
int drf_render_async(drf_t *h, const float *const *poses16, int n) { return guarded([&] { eng(h)->render().render_async(poses16, n); }); }
int drf_get_render_result(drf_t *h, uint8_t **bgr, float **depth, int n) { return guarded([&] { eng(h)->render().get_render_result(bgr, depth, n); }); }
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
  return guarded([&] { eng(h)->render().get_render_device(stream, d_bgr, d_depth); });
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
  return guarded([&] { eng(h)->locate().locate_system("drf_locate_system", depth, nullptr, pose16, opt, sums, counts); });
}
int drf_locate_system_device(drf_t *h, const void *d_depth, const float pose16[16], const drf_locate_options_t *opt, double sums[28], uint64_t counts[4]) {
  return guarded([&] { eng(h)->locate().locate_system("drf_locate_system_device", nullptr, d_depth, pose16, opt, sums, counts); });
}
int drf_locate_frame(drf_t *h, const float *depth, const float pose_init16[16], const drf_locate_options_t *opt, float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->locate().locate_frame("drf_locate_frame", depth, nullptr, pose_init16, opt, pose16_out, res); });
}
int drf_locate_frame_device(drf_t *h, const void *d_depth, const float pose_init16[16], const drf_locate_options_t *opt, float pose16_out[16],
                            drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->locate().locate_frame("drf_locate_frame_device", nullptr, d_depth, pose_init16, opt, pose16_out, res); });
}
int drf_locate_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_locate_stats", out, &dr::FusionEngine::locate_stats); }
using dr::FramePair;
int drf_track_system(drf_t *h, const float *depth, const float *model_depth, const float model_pose16[16], const float pose16[16], const drf_track_options_t *opt,
                     double sums[28], uint64_t counts[4]) {
  return guarded([&] {
    eng(h)->track().track_system("drf_track_system", FramePair::host(nullptr, depth), FramePair::host(nullptr, model_depth), model_pose16, pose16, opt, sums, counts);
  });
}
int drf_track_system_device(drf_t *h, const void *d_depth, const void *d_model_depth, const float model_pose16[16], const float pose16[16],
                            const drf_track_options_t *opt, double sums[28], uint64_t counts[4]) {
  return guarded([&] {
    eng(h)->track().track_system("drf_track_system_device", FramePair::device(nullptr, d_depth), FramePair::device(nullptr, d_model_depth), model_pose16, pose16, opt, sums, counts);
  });
}
int drf_track_frame(drf_t *h, const float *depth, const float pose_init16[16], const drf_track_options_t *opt, float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track().track_frame("drf_track_frame", FramePair::host(nullptr, depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_frame_device(drf_t *h, const void *d_depth, const float pose_init16[16], const drf_track_options_t *opt, float pose16_out[16],
                           drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track().track_frame("drf_track_frame_device", FramePair::device(nullptr, d_depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_track_stats", out, &dr::FusionEngine::track_stats); }
int drf_track_colour_system(drf_t *h, const uint8_t *bgr, const float *depth, const uint8_t *model_bgr, const float *model_depth, const float model_pose16[16],
                            const float pose16[16], const drf_track_colour_options_t *opt, double sums[28], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track().track_system("drf_track_colour_system", FramePair::host(bgr, depth), FramePair::host(model_bgr, model_depth), model_pose16, pose16, opt, sums, counts);
  });
}
int drf_track_colour_system_device(drf_t *h, const void *d_bgr, const void *d_depth, const void *d_model_bgr, const void *d_model_depth, const float model_pose16[16],
                                   const float pose16[16], const drf_track_colour_options_t *opt, double sums[28], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track().track_system("drf_track_colour_system_device", FramePair::device(d_bgr, d_depth), FramePair::device(d_model_bgr, d_model_depth), model_pose16, pose16, opt, sums,
                         counts);
  });
}
int drf_track_colour_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float pose_init16[16], const drf_track_colour_options_t *opt, float pose16_out[16],
                           drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track().track_frame("drf_track_colour_frame", FramePair::host(bgr, depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_colour_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float pose_init16[16], const drf_track_colour_options_t *opt,
                                  float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track().track_frame("drf_track_colour_frame_device", FramePair::device(d_bgr, d_depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_colour_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_track_colour_stats", out, &dr::FusionEngine::track_colour_stats); }
int drf_track_reduce(drf_t *h, int level, float max_jump, const uint8_t *bgr, const float *depth, uint8_t *bgr_out, float *depth_out) {
  return guarded([&] { eng(h)->track().track_reduce("drf_track_reduce", level, max_jump, FramePair::host(bgr, depth), bgr_out, depth_out); });
}
int drf_track_reduce_device(drf_t *h, int level, float max_jump, const void *d_bgr, const void *d_depth, void *d_bgr_out, void *d_depth_out) {
  return guarded([&] { eng(h)->track().track_reduce("drf_track_reduce_device", level, max_jump, FramePair::device(d_bgr, d_depth), d_bgr_out, d_depth_out); });
}
int drf_track_pyramid_system(drf_t *h, int level, const uint8_t *bgr, const float *depth, const uint8_t *model_bgr, const float *model_depth,
                             const float model_pose16[16], const float pose16[16], const drf_track_pyramid_options_t *opt, double sums[28], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track().track_pyramid_system("drf_track_pyramid_system", level, FramePair::host(bgr, depth), FramePair::host(model_bgr, model_depth), model_pose16, pose16, opt, sums,
                                 counts);
  });
}
int drf_track_pyramid_system_device(drf_t *h, int level, const void *d_bgr, const void *d_depth, const void *d_model_bgr, const void *d_model_depth,
                                    const float model_pose16[16], const float pose16[16], const drf_track_pyramid_options_t *opt, double sums[28],
                                    uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track().track_pyramid_system("drf_track_pyramid_system_device", level, FramePair::device(d_bgr, d_depth), FramePair::device(d_model_bgr, d_model_depth), model_pose16,
                                 pose16, opt, sums, counts);
  });
}
int drf_track_pyramid_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float pose_init16[16], const drf_track_pyramid_options_t *opt,
                            float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track().track_pyramid_frame("drf_track_pyramid_frame", FramePair::host(bgr, depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_pyramid_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float pose_init16[16], const drf_track_pyramid_options_t *opt,
                                   float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track().track_pyramid_frame("drf_track_pyramid_frame_device", FramePair::device(d_bgr, d_depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_pyramid_stats(drf_t *h, uint64_t out[8]) {
  return guarded([&] {
    if (!out) dr::fail(DR_ERR_ARG, "drf_track_pyramid_stats: null argument");
    const uint64_t *s = eng(h)->track().track_pyramid_stats();
    for (int i = 0; i < 8; ++i) out[i] = s[i];
  });
}
int drf_track_pyramid_level_stats(drf_t *h, int level, uint64_t out[4]) {
  return guarded([&] {
    if (!out) dr::fail(DR_ERR_ARG, "drf_track_pyramid_level_stats: null argument");
    const uint64_t *s = eng(h)->track().track_pyramid_level_stats(level);
    for (int i = 0; i < 4; ++i) out[i] = s[i];
  });
}
int drf_track_exposure_system(drf_t *h, int level, const uint8_t *bgr, const float *depth, const uint8_t *model_bgr, const float *model_depth,
                              const float model_pose16[16], const float pose16[16], double gain, double offset, const drf_track_exposure_options_t *opt,
                              double sums[45], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track().track_exposure_system("drf_track_exposure_system", level, FramePair::host(bgr, depth), FramePair::host(model_bgr, model_depth), model_pose16, pose16, gain,
                                          offset, opt, sums, counts);
  });
}
int drf_track_exposure_system_device(drf_t *h, int level, const void *d_bgr, const void *d_depth, const void *d_model_bgr, const void *d_model_depth,
                                     const float model_pose16[16], const float pose16[16], double gain, double offset, const drf_track_exposure_options_t *opt,
                                     double sums[45], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track().track_exposure_system("drf_track_exposure_system_device", level, FramePair::device(d_bgr, d_depth), FramePair::device(d_model_bgr, d_model_depth),
                                          model_pose16, pose16, gain, offset, opt, sums, counts);
  });
}
int drf_track_exposure_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float pose_init16[16], const drf_track_exposure_options_t *opt,
                             float pose16_out[16], drf_exposure_result_t *res) {
  return guarded_note([&] { return eng(h)->track().track_exposure_frame("drf_track_exposure_frame", FramePair::host(bgr, depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_exposure_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float pose_init16[16], const drf_track_exposure_options_t *opt,
                                    float pose16_out[16], drf_exposure_result_t *res) {
  return guarded_note([&] { return eng(h)->track().track_exposure_frame("drf_track_exposure_frame_device", FramePair::device(d_bgr, d_depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_exposure_stats(drf_t *h, uint64_t out[8]) {
  return guarded([&] {
    if (!out) dr::fail(DR_ERR_ARG, "drf_track_exposure_stats: null argument");
    const uint64_t *s = eng(h)->track().track_exposure_stats();
    for (int i = 0; i < 8; ++i) out[i] = s[i];
  });
}
int drf_track_exposure_level_stats(drf_t *h, int level, uint64_t out[4]) {
  return guarded([&] {
    if (!out) dr::fail(DR_ERR_ARG, "drf_track_exposure_level_stats: null argument");
    const uint64_t *s = eng(h)->track().track_exposure_level_stats(level);
    for (int i = 0; i < 4; ++i) out[i] = s[i];
  });
}
int drf_score_poses(drf_t *h, const float *depth, const float *poses16, size_t n, const drf_score_options_t *opt, double *cost, uint32_t *counts, double *score) {
  return guarded([&] { eng(h)->search().score_poses("drf_score_poses", depth, nullptr, poses16, n, opt, cost, counts, score); });
}
int drf_score_poses_device(drf_t *h, const void *d_depth, const float *poses16, size_t n, const drf_score_options_t *opt, double *cost, uint32_t *counts,
                           double *score) {
  return guarded([&] { eng(h)->search().score_poses("drf_score_poses_device", nullptr, d_depth, poses16, n, opt, cost, counts, score); });
}
int drf_search_frame(drf_t *h, const float *depth, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot, const drf_search_options_t *opt,
                     const drf_track_options_t *track_opt, const drf_locate_options_t *locate_opt, float pose16_out[16], drf_search_result_t *res, double *all_scores) {
  return guarded_note([&] {
    return eng(h)->search().search_frame("drf_search_frame", depth, nullptr, anchors16, n_anchors, rotations9, n_rot, opt, track_opt, locate_opt, pose16_out, res, all_scores);
  });
}
int drf_search_frame_device(drf_t *h, const void *d_depth, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot,
                            const drf_search_options_t *opt, const drf_track_options_t *track_opt, const drf_locate_options_t *locate_opt, float pose16_out[16],
                            drf_search_result_t *res, double *all_scores) {
  return guarded_note([&] {
    return eng(h)->search().search_frame("drf_search_frame_device", nullptr, d_depth, anchors16, n_anchors, rotations9, n_rot, opt, track_opt, locate_opt, pose16_out, res,
                                all_scores);
  });
}
int drf_search_stats(drf_t *h, uint64_t out[8]) { return guarded([&] { eng(h)->search().search_stats(out); }); }
int drf_score_colour_poses(drf_t *h, const uint8_t *bgr, const float *depth, const float *poses16, size_t n, const drf_score_colour_options_t *opt, double *cost,
                           double *photo, uint32_t *counts, double *score) {
  return guarded([&] { eng(h)->search().score_colour_poses("drf_score_colour_poses", bgr, depth, nullptr, nullptr, poses16, n, opt, cost, photo, counts, score); });
}
int drf_score_colour_poses_device(drf_t *h, const void *d_bgr, const void *d_depth, const float *poses16, size_t n, const drf_score_colour_options_t *opt,
                                  double *cost, double *photo, uint32_t *counts, double *score) {
  return guarded([&] { eng(h)->search().score_colour_poses("drf_score_colour_poses_device", nullptr, nullptr, d_bgr, d_depth, poses16, n, opt, cost, photo, counts, score); });
}
int drf_search_colour_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot,
                            const drf_search_colour_options_t *opt, const drf_track_pyramid_options_t *track_opt, const drf_locate_options_t *locate_opt,
                            float pose16_out[16], drf_search_colour_result_t *res, double *all_scores) {
  return guarded_note([&] {
    return eng(h)->search().search_colour_frame("drf_search_colour_frame", bgr, depth, nullptr, nullptr, anchors16, n_anchors, rotations9, n_rot, opt, track_opt, locate_opt,
                                                pose16_out, res, all_scores);
  });
}
int drf_search_colour_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float *anchors16, size_t n_anchors, const double *rotations9,
                                   size_t n_rot, const drf_search_colour_options_t *opt, const drf_track_pyramid_options_t *track_opt,
                                   const drf_locate_options_t *locate_opt, float pose16_out[16], drf_search_colour_result_t *res, double *all_scores) {
  return guarded_note([&] {
    return eng(h)->search().search_colour_frame("drf_search_colour_frame_device", nullptr, nullptr, d_bgr, d_depth, anchors16, n_anchors, rotations9, n_rot, opt, track_opt,
                                                locate_opt, pose16_out, res, all_scores);
  });
}
int drf_set_search_scope(drf_t *h, int scope, size_t stage_capacity_blocks) { return guarded([&] { eng(h)->search().set_search_scope(scope, stage_capacity_blocks); }); }
int drf_search_stage_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->search().search_stage_stats(out); }); }
int drf_set_locate_scope(drf_t *h, int scope, size_t stage_capacity_blocks) { return guarded([&] { eng(h)->locate().set_locate_scope(scope, stage_capacity_blocks); }); }
int drf_locate_stage_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->locate().locate_stage_stats(out); }); }
int drf_set_render_scope(drf_t *h, int scope, size_t stage_capacity_blocks) { return guarded([&] { eng(h)->render().set_render_scope(scope, stage_capacity_blocks); }); }
int drf_render_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->render().render_stats(out); }); }
int drf_set_render_bands(drf_t *h, int max_passes) { return guarded([&] { eng(h)->render().set_render_bands(max_passes); }); }
int drf_render_band_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->render().render_band_stats(out); }); }
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
