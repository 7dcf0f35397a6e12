// dr_mvsnet.hip -- MI355X engine behind the DrMvsnet operator API (C ABI: include/dr_mi355x.h).
//
// Replaces tandem/libdr/dr_mvsnet/src/dr_mvsnet.cpp (libtorch TorchScript interpreter + cuDNN)
// with a fixed launch plan of hand-written gfx950 kernels (conv_mfma.h, mvs_kernels.h; launchers: mvs_launch.h; host logic: mvs_host.h):
//   CallAsync   dr_mvsnet.cpp:125-283  -> MvsEngine::stage_inputs + worker thread
//   forward     dr_mvsnet.cpp:285-331  -> MvsEngine::forward (cva_mvsnet.py:98-184 as ~75 launches)
//   GetResult   dr_mvsnet.cpp:95-107   -> drm_get_result
// The threading contract is the reference's: one worker thread, one mutex, two condition variables;
// CallAsync blocks only while the previous input is still unprocessed.
#include <atomic>
#include <memory>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is bound with dlopen when a communicator is asked for

#include "conv_mfma.h"
#include "mvs_host.h"
#include "mvs_launch.h"
#ifdef DR_PARITY_HOOKS  // conv11 + prob in one launch: built twice in round 5, correct, slower than the two-kernel path (profiles/r05_tail.txt): parity build only
#include "tail_kernels.h"
#endif
#include "fn_front.h"
#include "fn_head3.h"

namespace dr {

std::string &last_error_slot() {
  thread_local std::string s;
  return s;
}

// An instance no plan asks for (DR_CONV_A_INSTANCES: its tiles are PT = 2's at half the work per wave) but one the library has always carried: instantiated
// here so that the library's set of kernels does not depend on how launch_conv's dispatcher is written.
template __global__ void k_conv_a<4, 1, 1>(const ConvArgs a);

// ------------------------------------------------------------------ engine
struct DevTensor {
  float *d = nullptr;
  int D = 0, H = 0, W = 0, C = 0;
  int pad = 0;  // zero border (pixels) around every H x W plane in memory; H and W stay the logical size
  int split = 0;  // 16: stored as C / 16 consecutive (D,H,W,16) sub-tensors (stage 1's cost volume: each 16-channel pass of conv0 then reads whole records)
  size_t n() const { return (size_t)D * (H + 2 * pad) * (W + 2 * pad) * C; }         // floats in memory
  float *interior() const { return d + ((size_t)pad * (W + 2 * pad) + pad) * C; }    // first logical pixel
};

struct Op {
  enum Kind { PREPROCESS, CONV, SKIPUP, PROB, COSTVOL, REGRESS, EDGE, HIST, SCAN, APPLY, BORDERFIX, TAIL, FRONT, HEAD3 } kind;
  const float *p0 = nullptr, *p1 = nullptr, *p3 = nullptr, *p4 = nullptr;
  float *p2 = nullptr;
  int d0 = 0, d1 = 0, d2 = 0;
  std::string name;
  ConvLaunch conv;
#ifdef DR_PARITY_HOOKS
  TailArgs tail{};                        // TAIL only: conv11 + prob in one launch (tail_kernels.h)
#endif
  FrontArgs front{};                      // FRONT only: preprocess + conv0.0 + conv0.1 in one launch (fn_front.h)
  Head3Args head3{};                      // HEAD3 only: FeatureNet's folded stage-3 head in one launch (fn_head3.h)
  PreprocessArgs pre{};                   // PREPROCESS only
  std::function<ConvLaunch(int)> replan;  // CONV only: build candidate `rank` of the planner's ranking
  std::string sig;                        // CONV only: layer signature in conv_tuned.h's column order
  int ncand = 0;
  int stage = 0, shift = 0, bits = 0;
  double flops = 0, bytes = 0;
};

// RCCL, bound lazily (drm_comm_*): an engine that never view-shards does not need the library, and inside a PyTorch
// process the same librccl.so.1 that torch.distributed loaded is picked up (one RCCL per process).
struct Rccl {
  void *lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclReduce) Reduce = nullptr;
  decltype(&ncclBroadcast) Broadcast = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;  // optional (reporting only)
  static Rccl &get() {
    static Rccl r;
    static std::mutex m;
    std::lock_guard<std::mutex> g(m);
    if (!r.lib) {
      // DR_RCCL_LIB: bind this library instead (tests/test_view_shard_gpu.py runs two ranks on one GPU against a
      // shared-memory stand-in, tests/cpp/rccl_stub.cpp: RCCL itself refuses two ranks on one device)
      if (const char *e = getenv("DR_RCCL_LIB")) r.lib = dlopen(e, RTLD_NOW | RTLD_GLOBAL);
      else
      for (const char *n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if ((r.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
      if (!r.lib) fail(DR_ERR_UNSUPPORTED, "RCCL not found (librccl.so.1): %s", dlerror());
      r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
      r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
      r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
      r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(r.lib, "ncclAllReduce"));
      r.Reduce = reinterpret_cast<decltype(r.Reduce)>(dlsym(r.lib, "ncclReduce"));
      r.Broadcast = reinterpret_cast<decltype(r.Broadcast)>(dlsym(r.lib, "ncclBroadcast"));
      r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
      r.CommCount = reinterpret_cast<decltype(r.CommCount)>(dlsym(r.lib, "ncclCommCount"));
      if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllReduce || !r.Reduce || !r.Broadcast || !r.GetErrorString) {
        r.lib = nullptr;
        fail(DR_ERR_UNSUPPORTED, "RCCL: missing symbols in librccl");
      }
    }
    return r;
  }
  void check(ncclResult_t e, const char *what) const {
    if (e != ncclSuccess) fail(DR_ERR_DEVICE, "RCCL %s: %s", what, GetErrorString(e));
  }
};

static const char *conv_kind_name(const ConvLaunch &c) { return conv_family_name(conv_family(c)); }

class MvsEngine {
 public:
  MvsEngine(const char *path, int device) : device_(device), blob_(load_blob(path)) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device) fail(DR_ERR_DEVICE, "DrMvsnet: no HIP device %d (found %d) -- the MI355X path has no CPU fallback", device, n);
    DR_HIP(hipSetDevice(device_));
    DR_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    // Both streams are created HERE, whether the side stream will be used or not: the runtime (ROCm 7.2, four hardware queues by default) gives a new stream the
    // least-shared queue, and with two streams per engine the main streams of four engines land on four different queues (tools/ubench/stream_queues.hip shows
    // the mapping; one stream per engine puts the fourth engine on the third one's queue: 535 instead of 580 depth maps/s, profiles/r06_queues_side_stream.txt).
    DR_HIP(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking));
    for (auto *e : {&ev_fork_, &ev_feat2_, &ev_feat3_}) DR_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    side_enabled_ = sw_.side_stream;
    std::vector<float> lut(256);
    for (int i = 0; i < 256; ++i) lut[i] = (float)((double)(float)i / 255.0);
    lut_ = consts_.upload(lut);
    DR_HIP(hipHostMalloc((void **)&march_err_, sizeof(int), hipHostMallocDefault));  // pinned, device-visible: k_conv_m raises it when a ring wait gives up
    *march_err_ = 0;
    worker_ = std::thread(&MvsEngine::loop, this);
  }
  ~MvsEngine() {
    {
      std::unique_lock<std::mutex> lk(mu_);
      done_cv_.wait(lk, [&] { return !unprocessed_; });
      running_ = false;
      input_cv_.notify_all();
    }
    worker_.join();
    (void)hipSetDevice(device_);
    (void)hipStreamSynchronize(stream_);
    if (comm_) { Rccl::get().CommDestroy(comm_); comm_ = nullptr; }
    release();
    for (float *&h : h_out_) if (h) (void)hipHostFree(h);
    if (h_in_) (void)hipHostFree(h_in_);
    if (ev_h2d_) (void)hipEventDestroy(ev_h2d_);
    if (march_err_) (void)hipHostFree(march_err_);
    if (fc_flag_) (void)hipHostFree(fc_flag_);
    if (up_stream_) { (void)hipStreamSynchronize(up_stream_); (void)hipEventDestroy(ev_hits_); (void)hipStreamDestroy(up_stream_); }
    (void)hipStreamSynchronize(side_);
    for (auto e : {ev_fork_, ev_feat2_, ev_feat3_}) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(side_);
    (void)hipStreamDestroy(stream_);
  }

  // --- reference-API surface -------------------------------------------------------------------
  void call_async(int H, int W, int V, int ref, const uint8_t *const *bgrs, const float *K9, const float *const *c2ws,
                  float dmin, float dmax, float disc) {
    check_args(H, W, V, ref, bgrs, K9, c2ws);
    std::unique_lock<std::mutex> lk(mu_);  // held by the worker for the whole forward (dr_mvsnet.cpp:84-92)
    done_cv_.wait(lk, [&] { return !unprocessed_; });
    stage_inputs(H, W, V, ref, bgrs, K9, c2ws, dmin, dmax, disc, true);
    unprocessed_ = true;
    input_cv_.notify_all();
  }
  bool ready() { return !unprocessed_; }
  void wait() {
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return !unprocessed_; });
    rethrow_worker_error();
  }
  void get_result(float *depth, float *conf, float *depth_dense, float *conf_dense) {
    std::unique_lock<std::mutex> lk(mu_);
    const float *src = take_result(lk);
    const size_t n = (size_t)H_ * W_;
    copier_.run([=] { memcpy(depth_dense, src + 2 * n, n * 4); memcpy(conf_dense, src + 3 * n, n * 4); });  // two maps each
    memcpy(depth, src, n * 4); memcpy(conf, src + n, n * 4);
    copier_.wait();
  }
  // The same result WITHOUT the 4.9 MB host copy: pointers into the page-locked block the device wrote it to.  Two blocks alternate,
  // so the maps stay valid while the NEXT call is processed and die when the call after that one starts.
  void get_result_view(const float **depth, const float **conf, const float **depth_dense, const float **conf_dense) {
    std::unique_lock<std::mutex> lk(mu_);
    const float *src = take_result(lk);
    const size_t n = (size_t)H_ * W_;
    if (depth) *depth = src;
    if (conf) *conf = src + n;
    if (depth_dense) *depth_dense = src + 2 * n;
    if (conf_dense) *conf_dense = src + 3 * n;
  }

  // --- key-frame feature cache (extension; see build_fn1) ----------------------------------------
  void set_feature_cache(int capacity) {
    if (capacity < 0 || capacity > 64) fail(DR_ERR_ARG, "drm_set_feature_cache: capacity %d out of range (0 = off, up to 64 key frames)", capacity);
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return !unprocessed_; });
    if (capacity == fcache_cap_) return;
    fcache_cap_ = capacity;
    if (H_) {  // a configured engine is re-planned: the entries are sized for the window shape
      DR_HIP(hipSetDevice(device_));
      const int H = H_, W = W_, V = V_;
      H_ = W_ = V_ = 0;
      configure(H, W, V);
      has_output_ = false;
    }
  }
  void feature_cache_stats(uint64_t out[6]) {
    std::unique_lock<std::mutex> lk(mu_);
    out[0] = fc_.hits; out[1] = fc_.misses; out[2] = fc_.batch_windows; out[3] = fc_.collisions; out[4] = fn1_ok_ ? 1 : 0; out[5] = (uint64_t)fc_.size();
  }

  // --- device-resident hooks -------------------------------------------------------------------
  void upload(int H, int W, int V, int ref, const uint8_t *const *bgrs, const float *K9, const float *const *c2ws,
              float dmin, float dmax, float disc) {
    check_args(H, W, V, ref, bgrs, K9, c2ws);
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return !unprocessed_; });
    stage_inputs(H, W, V, ref, bgrs, K9, c2ws, dmin, dmax, disc);
    DR_HIP(hipStreamSynchronize(stream_));
  }
  void forward_n(int iters, float *ms) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    DR_HIP(hipSetDevice(device_));
    InFlight windows(device_, false);  // (several engines driven through this hook at once count as windows in flight, like CallAsync's)
    hipEvent_t e0, e1;
    DR_HIP(hipEventCreate(&e0)); DR_HIP(hipEventCreate(&e1));
    DR_HIP(hipEventRecord(e0, stream_));
    for (int i = 0; i < iters; ++i) forward(nullptr);
    DR_HIP(hipEventRecord(e1, stream_));
    DR_HIP(hipStreamSynchronize(stream_));
    float t = 0;
    DR_HIP(hipEventElapsedTime(&t, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    cache_mismatch_recovered();
    check_march();
    if (ms) *ms = t;
  }
  // Time the first `k` candidates of every convolution layer's plan ranking in place (hipEvents, layer alone on the
  // stream) and keep the fastest.  Different candidates tile and order the fp32 accumulation differently, so results
  // move at the 1e-7 level; a tuned engine is therefore only bit-reproducible against an equally tuned one.
  // Returns the summed layer time before / after (ms).
  void autotune(int k, float *before_ms, float *after_ms) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    if (comm_ && shard_nsrc_) fail(DR_ERR_PROTOCOL, "autotune(): not on a view-sharded engine (tune the unsharded plan)");
    DR_HIP(hipSetDevice(device_));
    hipEvent_t e0, e1;
    DR_HIP(hipEventCreate(&e0)); DR_HIP(hipEventCreate(&e1));
    auto time_launch = [&](const ConvLaunch &c) {
      for (int i = 0; i < 2; ++i) launch_conv(c, stream_);
      DR_HIP(hipEventRecord(e0, stream_));
      for (int i = 0; i < 8; ++i) launch_conv(c, stream_);
      DR_HIP(hipEventRecord(e1, stream_));
      DR_HIP(hipEventSynchronize(e1));
      float t = 0;
      DR_HIP(hipEventElapsedTime(&t, e0, e1));
      return t / 8;
    };
    double t_before = 0, t_after = 0;
    const bool print = sw_.conv_print > 0;
    const char *only = sw_.autotune_only.empty() ? nullptr : sw_.autotune_only.c_str();
    for (Op &o : ops_) {
      if (o.kind != Op::CONV || !o.replan || (only && o.name.find(only) == std::string::npos)) continue;
      const float t0 = time_launch(o.conv);
      float best = t0;
      int best_rank = 0;
      ConvLaunch best_c = o.conv;
      for (int r = 1; r < std::min(k, o.ncand); ++r) {
        const ConvLaunch c = o.replan(r);
        const float t = time_launch(c);
        if (sw_.conv_print > 1)
          fprintf(stderr, "  cand %-12s rank %2d %s<%d,%d,%d> tile %dx%dx%d lds %zu KB grid %u: %.4f ms\n", o.name.c_str(), r, conv_kind_name(c), c.ci, c.ct, c.pt,
                  c.args.TZ, c.args.TY, c.args.TXT * 16, c.lds_bytes >> 10, c.grid.x, t);
        if (t < best * 0.98f) { best = t; best_rank = r; best_c = c; }
      }
      if (print) fprintf(stderr, "autotune %-12s model %.4f ms %s<%d,%d,%d> tile %dx%dx%d -> rank %d %.4f ms %s<%d,%d,%d> tile %dx%dx%d\n", o.name.c_str(), t0,
                         conv_kind_name(o.conv), o.conv.ci, o.conv.ct, o.conv.pt, o.conv.args.TZ, o.conv.args.TY, o.conv.args.TXT * 16, best_rank, best,
                         conv_kind_name(best_c), best_c.ci, best_c.ct, best_c.pt, best_c.args.TZ, best_c.args.TY, best_c.args.TXT * 16);
      if (print && best_rank != 0)
        fprintf(stderr, "TUNED    {%s,   %d, %d, %d, %d, %d, %d, %d},  // %s %.4f -> %.4f ms\n", o.sig.c_str(), best_c.ci, best_c.ct, best_c.pt, best_c.args.TZ,
                best_c.args.TY, best_c.args.TXT, (int)conv_family(best_c), o.name.c_str(), t0, best);
      o.conv = best_c;
      t_before += t0; t_after += best;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    DR_HIP(hipStreamSynchronize(stream_));
    check_march();
    if (before_ms) *before_ms = (float)t_before;
    if (after_ms) *after_ms = (float)t_after;
    if (fn1_ok_ && !match_fn1()) { fn1_ok_ = false; fc_.fast = false; }  // (the feature cache's single-view plan follows the batch plan's instances, or stands down)
  }

  // ---- view sharding hooks (SURVEY 8e / BASELINE configs[2]; no reference counterpart) ----
  // Phase p = 0..3 of the uploaded window: [.. cost volume 1] [regularise 1 .. cost volume 2] [.. cost volume 3]
  // [regularise 3 .. edge filter].  Between phases the host sum-reduces "volume<p+1>" over the ranks.
  void set_view_shard(int nsrc_total) {
    std::unique_lock<std::mutex> lk(mu_);
    if (nsrc_total < 0 || nsrc_total > kMaxSrc) fail(DR_ERR_ARG, "set_view_shard: %d source views unsupported (0..%d)", nsrc_total, kMaxSrc);
    shard_nsrc_ = nsrc_total;
  }
  // The view-shard collective inside the engine: with a communicator set, every cost-volume launch of a sharded window
  // is followed -- on the engine's stream, no host round trip -- by an in-place RCCL sum all-reduce of that volume over
  // the ranks, so drm_forward / CallAsync run the whole sharded depth map as one stream of work; FeatureNet's stage-2/3
  // heads on the side stream and the reduce of stage 1 overlap.  (The host-driven protocol of forward_phase stays as
  // the test double: RCCL refuses two ranks on one device, gloo can emulate them.)
  void comm_init(int rank, int world, const void *unique_id) {
    std::unique_lock<std::mutex> lk(mu_);
    if (comm_) fail(DR_ERR_PROTOCOL, "comm_init: a communicator is already set");
    if (!unique_id || rank < 0 || rank >= world) fail(DR_ERR_ARG, "comm_init: bad rank %d of %d", rank, world);
    Rccl &r = Rccl::get();
    DR_HIP(hipSetDevice(device_));
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof id);
    r.check(r.CommInitRank(&comm_, world, id, rank), "ncclCommInitRank");
    comm_world_ = world;
    comm_rank_ = rank;
  }
  // ranks RCCL itself reports for the engine's communicator (ncclCommCount): what bench.py prints next to the sharded figure, so that a
  // driver record shows how many GPUs the collective really spanned.  0: no communicator; -1: the bound library has no ncclCommCount.
  int comm_count() {
    std::unique_lock<std::mutex> lk(mu_);
    if (!comm_) return 0;
    Rccl &r = Rccl::get();
    if (!r.CommCount) return -1;
    int n = 0;
    r.check(r.CommCount(comm_, &n), "ncclCommCount");
    return n;
  }
  void comm_destroy() {
    std::unique_lock<std::mutex> lk(mu_);
    if (!comm_) return;
    (void)hipSetDevice(device_);
    (void)hipStreamSynchronize(stream_);
    Rccl::get().CommDestroy(comm_);
    comm_ = nullptr;
    comm_world_ = 0;
  }
  void forward_phase(int phase) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    if (phase < 0 || phase > 3) fail(DR_ERR_ARG, "forward_phase: phase must be 0..3");
    DR_HIP(hipSetDevice(device_));
    std::vector<size_t> cut{0};
    for (size_t i = 0; i < ops_.size(); ++i) if (ops_[i].kind == Op::COSTVOL) cut.push_back(i + 1);
    cut.push_back(ops_.size());
    phase_mode_ = true;  // the caller reduces between phases
    try { forward(nullptr, cut[phase], cut[phase + 1]); } catch (...) { phase_mode_ = false; throw; }
    phase_mode_ = false;
    DR_HIP(hipStreamSynchronize(stream_));
    check_march();
  }
  void device_tensor(const char *name, void **dptr, size_t *n) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    const DevTensor &t = T(name);
    if (dptr) *dptr = t.d;
    if (n) *n = t.n();
  }
  void download(float *depth, float *conf, float *depth_dense, float *conf_dense) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    DR_HIP(hipSetDevice(device_));
    const size_t n = (size_t)H_ * W_ * 4;
    DR_HIP(hipMemcpyAsync(depth, T("depth").d, n, hipMemcpyDeviceToHost, stream_));
    DR_HIP(hipMemcpyAsync(conf, T("confidence").d, n, hipMemcpyDeviceToHost, stream_));
    DR_HIP(hipMemcpyAsync(depth_dense, T("depth3").d, n, hipMemcpyDeviceToHost, stream_));
    DR_HIP(hipMemcpyAsync(conf_dense, T("conf3").d, n, hipMemcpyDeviceToHost, stream_));
    DR_HIP(hipStreamSynchronize(stream_));
    check_march();
  }
  void get_tensor(const char *name, float *out, size_t n_max, size_t *n, int dims[4]) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    DR_HIP(hipSetDevice(device_));
    const DevTensor &t = T(name);
    const size_t logical = (size_t)t.D * t.H * t.W * t.C;
    if (n) *n = logical;
    if (dims) { dims[0] = t.D; dims[1] = t.H; dims[2] = t.W; dims[3] = t.C; }
    if (out) {
      if (logical > n_max) fail(DR_ERR_ARG, "get_tensor(%s): need %zu floats, have %zu", name, logical, n_max);
      DR_HIP(hipStreamSynchronize(stream_));
      check_march();
      if (t.split) {  // split tensor: sub-tensor k, strided into channels [k * split, (k + 1) * split) of the logical (D, H, W, C) block
        const size_t npos = (size_t)t.D * t.H * t.W;
        for (int k = 0; k < t.C / t.split; ++k)
          DR_HIP(hipMemcpy2D(out + (size_t)k * t.split, (size_t)t.C * 4, t.d + (size_t)k * npos * t.split, (size_t)t.split * 4, (size_t)t.split * 4, npos, hipMemcpyDeviceToHost));
      } else if (!t.pad) DR_HIP(hipMemcpy(out, t.d, logical * 4, hipMemcpyDeviceToHost));
      else  // bordered tensor: the caller gets the logical (D, H, W, C) block
        for (int z = 0; z < t.D; ++z)
          DR_HIP(hipMemcpy2D(out + (size_t)z * t.H * t.W * t.C, (size_t)t.W * t.C * 4, t.interior() + (size_t)z * (t.H + 2 * t.pad) * (t.W + 2 * t.pad) * t.C,
                             (size_t)(t.W + 2 * t.pad) * t.C * 4, (size_t)t.W * t.C * 4, t.H, hipMemcpyDeviceToHost));
    }
  }
  void profile(std::string &names, std::vector<float> &ms) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    if (comm_ && shard_nsrc_) fail(DR_ERR_PROTOCOL, "profile(): a view-sharded engine enqueues collectives -- every rank would have to profile in lockstep");
    DR_HIP(hipSetDevice(device_));
    forward(nullptr);  // warm
    std::vector<hipEvent_t> ev(ops_.size() + 1);
    for (auto &e : ev) DR_HIP(hipEventCreate(&e));
    forward(&ev);
    DR_HIP(hipStreamSynchronize(stream_));
    check_march();
    names.clear(); ms.clear();
    for (size_t i = 0; i < ops_.size(); ++i) {
      float t = 0;
      DR_HIP(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
      ms.push_back(t);
      const Op &o = ops_[i];
      char kn[64] = "misc";
      if (o.kind == Op::CONV) conv_instance_name(o.conv, kn, sizeof kn);
      else if (o.kind == Op::COSTVOL) choose_costvol(costvol_shape(cv_[o.stage - 1]), sw_, o.stage).name(kn, sizeof kn);
      else if (o.kind == Op::PROB) choose_prob(prob_shape(pr_[o.stage - 1]), sw_, o.stage).name(kn, sizeof kn);
#ifdef DR_PARITY_HOOKS
      else if (o.kind == Op::TAIL) snprintf(kn, sizeof kn, o.tail.wmf ? "k_tail_m<%d>" : "k_tail<%d>", std::max(3, tail_nout(o.tail.QY, o.tail.QX)));
#endif
      else if (o.kind == Op::REGRESS) snprintf(kn, sizeof kn, "k_regress");
      else if (o.kind == Op::PREPROCESS) snprintf(kn, sizeof kn, "k_preprocess");
      else if (o.kind == Op::FRONT) snprintf(kn, sizeof kn, "k_fn_front");
      else if (o.kind == Op::HEAD3) snprintf(kn, sizeof kn, "k_fn_head3");
      else if (o.kind == Op::SKIPUP) snprintf(kn, sizeof kn, "k_skip_up<%d>", o.stage);
      else if (o.kind == Op::BORDERFIX) snprintf(kn, sizeof kn, "k_out3_border");
      else snprintf(kn, sizeof kn, "k_filter");
      char line[256];
      snprintf(line, sizeof line, "%s\t%s\t%.6e\t%.6e\n", o.name.c_str(), kn, o.flops, o.bytes);
      names += line;
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
  }
  void work(double *flops, double *bytes) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    double f = 0, b = 0;
    for (auto &o : ops_) { f += o.flops; b += o.bytes; }
    if (flops) *flops = f;
    if (bytes) *bytes = b;
  }

 private:
  // ---------------------------------------------------------------- plumbing
  void check_args(int H, int W, int V, int ref, const uint8_t *const *bgrs, const float *K9, const float *const *c2ws) {
    if (!bgrs || !K9 || !c2ws) fail(DR_ERR_ARG, "CallAsync: null pointer argument");
    const int vmin = shard_nsrc_ ? 1 : 2;  // a view-shard rank may hold the reference view only
    if (V < vmin || V > kMaxSrc + 1) fail(DR_ERR_ARG, "CallAsync: view_num=%d unsupported (%d..%d)", V, vmin, kMaxSrc + 1);
    if (ref < 0 || ref >= V) fail(DR_ERR_ARG, "CallAsync: ref_index=%d out of range", ref);
    if (H <= 0 || W <= 0 || H % 32 || W % 32) fail(DR_ERR_ARG, "CallAsync: height/width must be positive multiples of 32 (got %dx%d)", H, W);
    for (int i = 0; i < V - 1; ++i) for (int j = i + 1; j < V; ++j)
      if (bgrs[i] == bgrs[j] || c2ws[i] == c2ws[j])
        fail(DR_ERR_ARG, "ERROR: In Call Async passing the same data for index %d and %d", i, j);  // dr_mvsnet.cpp:153-160
  }
  void require_config() { if (!H_) fail(DR_ERR_PROTOCOL, "no window uploaded yet"); }
  void rethrow_worker_error() {
    if (!worker_error_.empty()) { std::string e = worker_error_; worker_error_.clear(); fail(DR_ERR_DEVICE, "%s", e.c_str()); }
  }
  // GetResult's first half: waits for the window, rethrows what its worker threw and hands the pinned block of four maps out ONCE
  const float *take_result(std::unique_lock<std::mutex> &lk) {
    done_cv_.wait(lk, [&] { return !unprocessed_; });
    rethrow_worker_error();
    if (!has_output_) fail(DR_ERR_PROTOCOL, "Output should be valid. Maybe you called GetResult more than once?");
    has_output_ = false;
    return h_out_[out_cur_];
  }
  // windows whose kernels are enqueued or running, per device, over all engines of the process (forward() forks onto its side stream only when it is alone)
  static std::atomic<int> &windows_in_flight(int device) {
    static std::atomic<int> n[16];
    return n[device & 15];
  }
  struct InFlight {
    int dev;
    InFlight(int d, bool counted_already) : dev(d) { if (!counted_already) windows_in_flight(dev).fetch_add(1, std::memory_order_relaxed); }
    ~InFlight() { windows_in_flight(dev).fetch_sub(1, std::memory_order_relaxed); }
  };
  void loop() {  // dr_mvsnet.cpp:83-93
    std::unique_lock<std::mutex> lk(mu_);
    while (running_) {
      if (unprocessed_) {
        try {
          DR_HIP(hipSetDevice(device_));
          InFlight window(device_, prelaunched_);  // (counted from here, or from CallAsync's own launch, to the end of this block)
          if (prelaunched_) prelaunched_ = false;  // (CallAsync enqueued this window's forward itself: stage_inputs)
          else forward(nullptr);
          const int blk = out_cur_ ^ 1;  // the block the previous result does NOT live in (drm_get_result_view: that one may still be read)
          publish(blk);
          if (cache_mismatch_recovered()) publish(blk);  // a cache hit that was a key collision: the window ran again without the cache; publish THAT result
          check_march();
          out_cur_ = blk;
          has_output_ = true;
        } catch (const std::exception &e) { worker_error_ = e.what(); }
        unprocessed_ = false;
        done_cv_.notify_all();
      }
      input_cv_.wait(lk, [&] { return unprocessed_ || !running_; });
    }
  }

  // the four result maps into pinned block `blk`, and the wait for them
  void publish(int blk) {
    const size_t n = (size_t)H_ * W_ * 4;
    float *ho = h_out_[blk];
    if (sw_.d2h_copy) {  // DR_MVS_D2H=copy: the four copy-engine transfers of round 2 (A/B hook)
      DR_HIP(hipMemcpyAsync(ho, filt_.depth, n, hipMemcpyDeviceToHost, stream_));
      DR_HIP(hipMemcpyAsync(ho + n / 4, filt_.conf, n, hipMemcpyDeviceToHost, stream_));
      DR_HIP(hipMemcpyAsync(ho + 2 * (n / 4), filt_.depth3, n, hipMemcpyDeviceToHost, stream_));
      DR_HIP(hipMemcpyAsync(ho + 3 * (n / 4), filt_.conf3, n, hipMemcpyDeviceToHost, stream_));
    } else launch_publish4(filt_.depth, filt_.conf, filt_.depth3, filt_.conf3, h_out_dev_[blk], n / 16, stream_);
    DR_HIP(hipStreamSynchronize(stream_));
  }

  DevTensor &T(const std::string &name) {
    auto it = tensors_.find(tprefix_.empty() ? name : tprefix_ + name);
    if (it == tensors_.end()) fail(DR_ERR_ARG, "unknown tensor '%s'", name.c_str());
    return it->second;
  }
  DevTensor &alloc(const std::string &name, int D, int H, int W, int C, int pad = 0) {
    DevTensor t; t.D = D; t.H = H; t.W = W; t.C = C; t.pad = pad;
    const std::string key = tprefix_.empty() ? name : tprefix_ + name;  // (the single-view FeatureNet of the feature cache builds into its own names)
    t.d = dalloc<float>(t.n(), key.c_str());
    if (pad) DR_HIP(hipMemset(t.d, 0, t.n() * 4));  // the border is written once, here; producers only touch the interior
    tensors_[key] = t;
    return tensors_[key];
  }
  void release() {
    for (auto &kv : tensors_) dfree(kv.second.d);
    tensors_.clear();
    ops_.clear();
    ops1_.clear(); fcache_.clear(); fc_.clear(); fn1_ok_ = false; fc_.fast = fc_.fill = false;  // (a new window shape evicts everything: the entries' buffers are in misc_)
    plan_arena_.reset();
    for (void *p : misc_) dfree(p);
    misc_.clear();
  }

  // ---------------------------------------------------------------- layer construction
  // FeatureNet's skip connection (1x1 conv + bias + nearest-upsampled coarser level) on the streaming kernel k_skip_up;
  // DR_SKIP_ON_CONV=1 keeps it on the MFMA convolution kernel (A/B hook, and the path for other channel counts).
  DevTensor &add_skip(const std::string &opname, const std::string &wname, const DevTensor &in, const std::string &outname, const DevTensor &coarse) {
    const HostTensor &w = blob_.at(wname + ".weight");
    // (measured at 640x480x7: stage 3, Cin = 8: 0.141 -> 0.108 ms; stage 2, Cin = 16, a quarter of the pixels and twice the
    // weights per lane: 0.038 -> 0.073 ms, so that one stays where it was)
    if (!kParityHooks || sw_.skip_on_conv || w.dims[0] != 32 || w.dims[1] != in.C || in.C != 8 || coarse.C != 32 ||
        coarse.H * 2 != in.H || coarse.W * 2 != in.W)
      return add_conv(opname, wname, "", true, false, in, outname, 1, 1, 1, 1, 1, 1, false, CONV_NORMAL, &coarse, 2);
    DevTensor &out = alloc(outname, in.D, in.H, in.W, 32);
    Op o; o.kind = Op::SKIPUP; o.name = opname;
    o.p0 = in.d; o.p1 = plan_arena_->upload(w.data); o.p2 = out.d; o.d0 = in.D; o.d1 = in.H; o.d2 = in.W; o.stage = in.C;
    o.p3 = plan_arena_->upload(blob_.at(wname + ".bias").data); o.p4 = coarse.d;
    o.flops = 2.0 * in.C * 32 * in.n() / in.C; o.bytes = 4.0 * (in.n() + coarse.n() + out.n());
    ops_.push_back(o);
    return out;
  }
  // Adds one convolution layer (possibly several launches) to the plan; returns the output tensor.
  DevTensor &add_conv(const std::string &opname, const std::string &wname, const std::string &bnname, bool conv_bias, bool relu,
                      const DevTensor &in, const std::string &outname, int k3d, int kh, int kw, int sd, int sh, int sw,
                      bool transposed, ConvMode mode, const DevTensor *add, int add_mode, const ConvFuse *fz = nullptr, int out_pad = 0) {
    const HostTensor &w = blob_.at(wname + ".weight");
    ConvLayer L;
    L.transposed = transposed;
    const int c_out = transposed ? w.dims[1] : w.dims[0], c_in_real = transposed ? w.dims[0] : w.dims[1];
    L.Cout = c_out; L.Cin = in.C;
    L.kd = k3d; L.kh = kh; L.kw = kw; L.sd = sd; L.sh = sh; L.sw = sw; L.relu = relu; L.out_pad = out_pad;
    std::vector<float> padded;
    if (c_in_real != in.C) {  // RGB -> RGB0: zero-pad the input-channel axis of the weights
      if (transposed || c_in_real > in.C) fail(DR_ERR_ARG, "%s: channel mismatch", opname.c_str());
      padded = pad_cin(w.data, c_out, c_in_real, in.C, k3d * kh * kw);
      L.weight = padded.data();
    } else L.weight = w.data.data();
    if (!bnname.empty()) fold_bn(blob_, bnname, c_out, L.scale, L.bias);
    else if (conv_bias) L.bias = blob_.at(wname + ".bias").data;
    ConvPlanOut P0;  // dims first
    {
      auto cz = axis_classes(k3d, sd, transposed, in.D), cy = axis_classes(kh, sh, transposed, in.H), cx = axis_classes(kw, sw, transposed, in.W);
      P0.outD = transposed ? in.D * sd : cz[0].npos; P0.outH = transposed ? in.H * sh : cy[0].npos; P0.outW = transposed ? in.W * sw : cx[0].npos;
    }
    DevTensor &out = alloc(outname, P0.outD, P0.outH, P0.outW, c_out, out_pad);
    emit_conv(opname, L, mode, in, out, add ? add->d : nullptr, add_mode, add ? (add_mode == 2 ? add->n() : out.n()) : 0, fz);
    return out;
  }
  // Plans layer L (in -> out, both existing tensors) and appends its launch(es) to the op list.
  void emit_conv(const std::string &opname, const ConvLayer &L, ConvMode mode, const DevTensor &in, DevTensor &out, const float *add_d, int add_mode,
                 size_t add_n, const ConvFuse *fz = nullptr) {
    const int k3d = L.kd, kh = L.kh, kw = L.kw;
    ConvFuse fzc{};
    if (fz) fzc = *fz;
    const bool fused = fz != nullptr;
    ConvPlanOut P = plan_conv(L, mode, in.d, in.D, in.H, in.W, in.C, out.interior(), add_d, add_mode, *plan_arena_, 0, fz, in.split);
    // the autotuner re-plans this layer with another candidate of the cost model's ranking (weights are kept alive)
    auto keep = std::make_shared<std::vector<float>>(L.weight, L.weight + (size_t)L.Cout * L.Cin * k3d * kh * kw);
    ConvLayer Lc = L;
    const float *in_d = in.d;
    float *out_d = out.interior();
    const int iD = in.D, iH = in.H, iW = in.W, iC = in.C, iS = in.split, ncand = P.ncand;
    auto replan = [this, keep, Lc, mode, in_d, iD, iH, iW, iC, iS, out_d, add_d, add_mode, fzc, fused](int rank) mutable {
      Lc.weight = keep->data();
      return plan_conv(Lc, mode, in_d, iD, iH, iW, iC, out_d, add_d, add_mode, *plan_arena_, rank, fused ? &fzc : nullptr, iS).launches.at(0);
    };
    int idx = 0;
    for (auto &cl : P.launches) {
      Op o; o.kind = Op::CONV; o.conv = cl; o.name = opname + (P.launches.size() > 1 ? "." + std::to_string(idx) : "");
      if (P.launches.size() == 1) {
        o.replan = replan; o.ncand = ncand;
        char sig[160];
        snprintf(sig, sizeof sig, "%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d", L.Cin, L.Cout, k3d, kh, kw, L.sd, L.sh, L.sw, L.transposed ? 1 : (L.up2 ? 1 + L.up2 : 0),
                 (int)mode + (fused ? 8 : 0) + (iS ? 16 : 0), iD, iH, iW);
        o.sig = sig;
      }
      o.flops = cl.flops;
      if (idx == 0) o.bytes = 4.0 * ((fused ? in.n() / in.C * fzc.cin + in.n() / 4 : in.n()) + out.n() + add_n);
      if (fused) o.flops += 2.0 * fzc.cin * in.C * (in.n() / in.C);
      ops_.push_back(o);
      ++idx;
    }
  }
  // FeatureNet's first block: u8 BGR -> RGB0 / 255, conv0.0 (3 -> 8), conv0.1 (8 -> 8), both 3x3 + BN + ReLU (module.py:461-470).  One launch
  // (k_fn_front, fn_front.h) when the weights have that shape; DR_FN_FRONT=0, the bf16x3 mode and any other shape keep the three launches.
  // the fused FeatureNet kernels need 55 KB / 133.5 KB of dynamic LDS per workgroup: plan them only where the device grants that much to one
  // workgroup (on a part with less the launch would be rejected in every forward while the multi-launch forms still exist)
  bool lds_fits(size_t bytes) const {
    int optin = 0;
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, device_) != hipSuccess || optin <= 0) {
      (void)hipGetLastError();
      if (hipDeviceGetAttribute(&optin, hipDeviceAttributeMaxSharedMemoryPerBlock, device_) != hipSuccess) { (void)hipGetLastError(); return false; }
    }
    return (size_t)optin >= bytes;
  }
  DevTensor &front_block(const std::string &fn, int V, int H, int W) {
    const HostTensor &wa = blob_.at(fn + "conv0.0.conv.weight"), &wb = blob_.at(fn + "conv0.1.conv.weight");
    const bool shape_ok = wa.dims.size() == 4 && wa.dims[0] == 8 && wa.dims[1] == 3 && wa.dims[2] == 3 && wa.dims[3] == 3 &&
                          wb.dims.size() == 4 && wb.dims[0] == 8 && wb.dims[1] == 8 && wb.dims[2] == 3 && wb.dims[3] == 3;
    const bool fits32 = (double)V * H * W * 32.0 < 2147483648.0 && ((uintptr_t)d_bgr_ & 3) == 0;  // (the kernel addresses both tensors with 32-bit byte offsets from an aligned base)
    if (!sw_.fn_front || conv_bf3_policy() || !shape_ok || !fits32 || !lds_fits(kFrontLdsBytes)) {
      DevTensor &img = alloc("image", V, H, W, 4);
      { Op o; o.kind = Op::PREPROCESS; o.name = "preprocess"; o.bytes = (double)V * H * W * (3 + 16); o.pre = {d_bgr_, reinterpret_cast<float4 *>(img.d), lut_, (size_t)V * H * W}; ops_.push_back(o); }
      DevTensor &c3a = cbr2("fn.conv0.0", fn + "conv0.0", img, 3, 1, CONV_XPAIR);
      return cbr2("fn.conv0.1", fn + "conv0.1", c3a, 3, 1, CONV_XPAIR);
    }
    DevTensor &c3 = alloc("fn.conv0.1", V, H, W, 8);
    Op o; o.kind = Op::FRONT; o.name = "fn.front";
    FrontArgs &a = o.front;
    a.bgr = d_bgr_; a.lut = lut_; a.out = c3.d;
    a.w1 = reinterpret_cast<const float4 *>(plan_arena_->upload(front_pack(wa.data.data(), 3, 4)));
    a.w2 = reinterpret_cast<const float4 *>(plan_arena_->upload(front_pack(wb.data.data(), 8, 8)));
    auto affine = [&](const std::string &bn) {  // 16 scales, 16 biases: XPAIR row r = 8 * (x of the pair) + channel
      std::vector<float> sc, bi, sb(32);
      fold_bn(blob_, bn, 8, sc, bi);
      for (int r = 0; r < 16; ++r) { sb[r] = sc[r & 7]; sb[16 + r] = bi[r & 7]; }
      return plan_arena_->upload(sb);
    };
    a.sb1 = affine(fn + "conv0.0.bn"); a.sb2 = affine(fn + "conv0.1.bn");
    a.V = V; a.H = H; a.W = W;
    a.tilesY = cdiv(H, kFrontTY); a.tilesX = cdiv(W, kFrontTXP); a.ntiles = V * a.tilesY * a.tilesX;
    o.flops = 2.0 * V * H * W * 9.0 * (4 * 8 + 8 * 8);  // (as the planner counts the two layers: RGB0 has four channels)
    o.bytes = (double)V * H * W * (3 + 32);
    ops_.push_back(o);
    return c3;
  }
  DevTensor &cbr2(const std::string &name, const std::string &p, const DevTensor &in, int k, int s, ConvMode m) {
    return add_conv(name, p + ".conv", p + ".bn", false, true, in, name, 1, k, k, 1, s, s, false, m, nullptr, 0);
  }
  DevTensor &cbr3(const std::string &name, const std::string &p, const DevTensor &in, int sd, int shw, ConvMode m) {
    return add_conv(name, p + ".conv", p + ".bn", false, true, in, name, 3, 3, 3, sd, shw, shw, false, m, nullptr, 0);
  }
  DevTensor &dbr3(const std::string &name, const std::string &p, const DevTensor &in, int sd, const DevTensor &skip) {
    return add_conv(name, p + ".conv", p + ".bn", false, true, in, name, 3, 3, 3, sd, 2, 2, true, CONV_NORMAL, &skip, 1);
  }

  // (Re)builds the whole plan for a new window shape.  The engine keeps H_ = W_ = V_ = 0 ("not configured") until the
  // plan is complete: if anything below throws (out of memory, unsupported depth_num, missing tensor) everything
  // allocated so far is released and the next call starts from scratch instead of running a half-built plan.
  void configure(int H, int W, int V) {
    if (H == H_ && W == W_ && V == V_) return;
    DR_HIP(hipStreamSynchronize(stream_));
    release();
    H_ = W_ = V_ = 0;
    memset(cv_, 0, sizeof cv_);
    memset(rg_, 0, sizeof rg_);
    memset(pr_, 0, sizeof pr_);
    try {
      build_plan(H, W, V);
    } catch (...) {
      release();
      throw;
    }
    H_ = H; W_ = W; V_ = V;
  }
  // FeatureNet for a batch of V views (module.py:461-531): appends its launches to ops_ and records which of them may run on the side stream
  void build_featurenet(int V, int H, int W) {
    const std::string fn = "feature_net.";
    DevTensor &c3 = front_block(fn, V, H, W);
    DevTensor &c2a = cbr2("fn.conv1.0", fn + "conv1.0", c3, 5, 2, CONV_NORMAL);
    DevTensor &c2b = cbr2("fn.conv1.1", fn + "conv1.1", c2a, 3, 1, CONV_NORMAL);
    DevTensor &c2 = cbr2("fn.conv1.2", fn + "conv1.2", c2b, 3, 1, CONV_NORMAL);
    DevTensor &c1a = cbr2("fn.conv2.0", fn + "conv2.0", c2, 5, 2, CONV_NORMAL);
    DevTensor &c1b = cbr2("fn.conv2.1", fn + "conv2.1", c1a, 3, 1, CONV_NORMAL);
    DevTensor &c1 = cbr2("fn.conv2.2", fn + "conv2.2", c1b, 3, 1, CONV_NORMAL);
    // feature maps handed to the cost volume carry a one-pixel zero border (k_costvol2); DR_COSTVOL_V1=1: the unpadded layout + k_costvol
    const int fpad = sw_.costvol_v1 ? 0 : 1;
    add_conv("fn.out1", fn + "out.stage1", "", false, false, c1, "feat1", 1, 1, 1, 1, 1, 1, false, CONV_NORMAL, nullptr, 0, nullptr, fpad);
    fork_lo_ = ops_.size();
    DevTensor &i2 = add_skip("fn.skip2", fn + "skip.stage2", c2, "inter2", c1);
    add_conv("fn.out2", fn + "out.stage2", "", false, false, i2, "feat2", 1, 3, 3, 1, 1, 1, false, CONV_NORMAL, nullptr, 0, nullptr, fpad);
    feat2_op_ = ops_.size() - 1;
    // stage 3: skip.stage3 (1x1, 8 -> 32, + upsampled inter2) is computed inside out.stage3's staging step -- the
    // 32-channel full-resolution tensor between them (275 MB at 640x480x7) is never written or read.  DR_NO_SKIP_FUSION=1: the two-kernel path.
    const HostTensor &w3 = blob_.at(fn + "skip.stage3.weight");
    const HostTensor &wo3 = blob_.at(fn + "out.stage3.weight");
    // out.stage3 is linear in inter3 = up(inter2) + skip.stage3(c3) (no BatchNorm, no ReLU, no bias: module.py:480-485,524-529), so it
    // is evaluated as   conv3x3(c3; Wout . Wskip)  +  conv3x3(up(inter2); Wout)  +  (Wout . bskip, corrected at the image border):
    // an 8 -> 8 XPAIR layer at full resolution (composed weights), two 2 x 3-tap phase layers over inter2 at HALF resolution that
    // add their rows in place (ConvLayer::up2: the upsampled tensor never exists), and a border kernel.  11.0 GFLOP become 6.9, the
    // 275 MB inter3 and the skip staging disappear, and all three convolutions run on the persistent kernels (0.22 -> 0.13 ms).
    // feat3 then differs from the literal order by fp32 reassociation (2e-6 of its range).  DR_OUT3_FOLDED=0: the fused-skip form.
    if (sw_.out3_folded && !sw_.no_skip_fusion && !sw_.skip_on_conv && w3.dims[0] == 32 && w3.dims[1] == 8 && c3.C == 8 &&
        i2.C == 32 && wo3.dims[0] == 8 && wo3.dims[1] == 32 && i2.H * 2 == c3.H && i2.W * 2 == c3.W) {
      const Out3Fold fold = compose_out3(wo3.data, w3.data, blob_.at(fn + "skip.stage3.bias").data);
      const std::vector<float> &wa = fold.wa, &T = fold.T, &bint = fold.bint;
      DevTensor &f3 = alloc("feat3", c3.D, c3.H, c3.W, 8, fpad);
      if (sw_.fn_head3 && !conv_bf3_policy() && (double)f3.n() * 4.0 < 2147483648.0 && (double)i2.n() * 4.0 < 2147483648.0 && lds_fits(kH3LdsBytes)) {  // one launch: the three terms meet in one accumulator (fn_head3.h)
        Op o; o.kind = Op::HEAD3; o.name = "fn.head3";
        Head3Args &a = o.head3;
        a.c0 = c3.d; a.i2 = i2.d;
        a.wa = reinterpret_cast<const float4 *>(plan_arena_->upload(h3_pack_a(wa.data())));
        a.wb = reinterpret_cast<const float4 *>(plan_arena_->upload(h3_pack_b(wo3.data.data())));
        std::vector<float> b16(16);
        for (int r = 0; r < 16; ++r) b16[r] = bint[r & 7];
        a.bias16 = plan_arena_->upload(b16); a.T = plan_arena_->upload(T);
        a.out = f3.interior(); a.V = c3.D; a.H = c3.H; a.W = c3.W;
        a.out_row = (f3.W + 2 * f3.pad) * 8; a.out_plane = (f3.H + 2 * f3.pad) * a.out_row;
        a.tilesY = cdiv(c3.H, kH3TY); a.tilesX = cdiv(c3.W, kH3TXP); a.ntiles = c3.D * a.tilesY * a.tilesX;
        o.flops = 2.0 * c3.D * c3.H * c3.W * (9.0 * 8 * 8 + 4.0 * 32 * 8);  // (as the four launches count them: 9 taps of the composed layer, 2 x 2 half-resolution pixels per output pixel)
        o.bytes = 4.0 * (c3.n() + i2.n() + (double)c3.D * c3.H * c3.W * 8);
        ops_.push_back(o);
      } else {
      ConvLayer LA; LA.Cin = 8; LA.Cout = 8; LA.kd = 1; LA.kh = 3; LA.kw = 3; LA.weight = wa.data(); LA.bias = bint; LA.out_pad = fpad;
      emit_conv("fn.out3a", LA, CONV_XPAIR, c3, f3, nullptr, 0, 0);
      for (int py = 0; py < 2; ++py) {
        ConvLayer LB; LB.Cin = 32; LB.Cout = 8; LB.kd = 1; LB.kh = 3; LB.kw = 3; LB.weight = wo3.data.data(); LB.up2 = 1 + py; LB.out_pad = fpad;
        emit_conv(py ? "fn.out3c" : "fn.out3b", LB, CONV_NORMAL, i2, f3, f3.interior(), 1, f3.n() / 2);
      }
      Op o; o.kind = Op::BORDERFIX; o.name = "fn.out3d"; o.p2 = f3.interior(); o.p1 = plan_arena_->upload(T); o.d0 = c3.D; o.d1 = c3.H; o.d2 = c3.W;
      o.stage = fpad; o.bytes = 64.0 * c3.D * (c3.H + c3.W);
      ops_.push_back(o);
      }
    } else
    if (!sw_.no_skip_fusion && !sw_.skip_on_conv && kParityHooks && w3.dims[0] == 32 && w3.dims[1] == 8 && c3.C == 8 && i2.C == 32 &&
        i2.H * 2 == c3.H && i2.W * 2 == c3.W) {  // (parity build only: the fused-skip kernel instances are not in the product library)
      ConvFuse fz{c3.d, plan_arena_->upload(w3.data), plan_arena_->upload(blob_.at(fn + "skip.stage3.bias").data), i2.d, 8};
      DevTensor virt; virt.D = c3.D; virt.H = c3.H; virt.W = c3.W; virt.C = 32; virt.d = nullptr;  // inter3 exists in LDS only
      add_conv("fn.out3", fn + "out.stage3", "", false, false, virt, "feat3", 1, 3, 3, 1, 1, 1, false, CONV_XPAIR, nullptr, 0, &fz, fpad);
    } else {
      DevTensor &i3 = add_skip("fn.skip3", fn + "skip.stage3", c3, "inter3", i2);
      add_conv("fn.out3", fn + "out.stage3", "", false, false, i3, "feat3", 1, 3, 3, 1, 1, 1, false, CONV_XPAIR, nullptr, 0, nullptr, fpad);
    }
    fork_hi_ = ops_.size();
  }

  // ---------------------------------------------------------------- key-frame feature cache (drm_set_feature_cache)
  // In TANDEM six of a window's seven images were in the previous window (FullSystem.cpp:1162-1171 re-sends frameHessians[i]->image_bgr), and
  // FeatureNet is per image.  With the cache on, the engine keeps feat1..3 (and the u8 image) of the last `capacity` images; a window whose images
  // are all cached but at most ONE runs FeatureNet on that one view (its own single-view plan, the same kernel instances as the batch plan) and the
  // plane sweep reads every view's features where the cache holds them (CostVolArgs::vfeat): 15 launches over 7 views become 11 over one.
  //  * identity: a 128-bit key over a sample of the image (first / last 64 bytes + 512 evenly spaced 8-byte words) finds the entry; the hit is then
  //    made EXACT on the device -- every uploaded image is compared byte for byte with the entry's copy (k_verify_image), and a difference (a key
  //    collision) drops the whole cache and runs the window again without it, before any result leaves the engine;
  //  * windows with two or more uncached images (the first one, a reset) take the batch path and fill the cache from its outputs;
  //  * same bits with the cache on and off: the single-view plan is built from the batch plan's own choices (kernel family, channel pass, tiles per wave)
  //    -- the products and their order per output value do not depend on the tile shape or the batch size (tests: test_feature_cache_is_bit_identical);
  //  * OFF by default and in every leg of bench.py that feeds `value` / `single_window_ms` (they repeat one window: every image would hit).
  struct FnOut { size_t op; int stage; size_t offset; };  // launch `op` of the single-view plan stores into feat<stage + 1> at this float offset
  struct FcBuffers { float *feat[3] = {nullptr, nullptr, nullptr}; uint8_t *bgr = nullptr; };  // entry e of the index (fc_, mvs_host.h): its three bordered feature maps and its image
  static bool same_instance(const ConvLaunch &a, const ConvLaunch &b) {
    return a.async == b.async && a.ci == b.ci && a.ct == b.ct && a.pt == b.pt && a.fz == b.fz && a.bf3 == b.bf3 && a.nup == b.nup && a.ncw == b.ncw &&
           a.march.wino == b.march.wino && a.march.rm == b.march.rm;
  }
  void build_fn1(int H, int W) {
    fn1_ok_ = false; ops1_.clear(); fcache_.clear(); fc_.clear();
    if (ops_.empty() || ops_[0].kind != Op::FRONT || sw_.costvol_v1 || shard_nsrc_) return;  // (the single-view plan patches k_fn_front's image pointer per call)
    const size_t lo = fork_lo_, hi = fork_hi_, f2 = feat2_op_;
    std::vector<Op> batch;
    batch.swap(ops_);
    tprefix_ = "c1.";
    try { build_featurenet(1, H, W); } catch (...) { tprefix_.clear(); ops_.swap(batch); fork_lo_ = lo; fork_hi_ = hi; feat2_op_ = f2; throw; }
    tprefix_.clear();
    ops1_.swap(ops_); ops_.swap(batch);
    fork_lo_ = lo; fork_hi_ = hi; feat2_op_ = f2;
    if (!match_fn1()) { ops1_.clear(); return; }
    // the entries: three bordered feature maps + the image, per cached key frame
    const size_t img_bytes = (size_t)H * W * 3;
    fcache_.resize(fcache_cap_); fc_.resize(fcache_cap_);
    for (FcBuffers &e : fcache_) {
      for (int s = 0; s < 3; ++s) {
        const DevTensor &t = T("c1.feat" + std::to_string(s + 1));
        e.feat[s] = dalloc<float>(t.n()); misc_.push_back(e.feat[s]);
        DR_HIP(hipMemset(e.feat[s], 0, t.n() * 4));  // (the zero border is written once, here: the producers store interior pixels only)
      }
      e.bgr = dalloc<uint8_t>(img_bytes + 16); misc_.push_back(e.bgr);
    }
    if (!fc_flag_) { DR_HIP(hipHostMalloc((void **)&fc_flag_, sizeof(int), hipHostMallocDefault)); *fc_flag_ = 0; }
    if (!up_stream_) { DR_HIP(hipStreamCreateWithFlags(&up_stream_, hipStreamNonBlocking)); DR_HIP(hipEventCreateWithFlags(&ev_hits_, hipEventDisableTiming)); }
    // the single-view plan writes its three outputs straight into the entry of the image it runs on: which launches store into feat1..3, and where
    fn1_out_.clear();
    for (size_t i = 0; i < ops1_.size(); ++i) {
      Op &o = ops1_[i];
      float *out = o.kind == Op::CONV ? o.conv.args.out : (o.kind == Op::HEAD3 ? o.head3.out : nullptr);
      for (int s = 0; s < 3 && out; ++s) {
        const DevTensor &t = T("c1.feat" + std::to_string(s + 1));
        if (out >= t.d && out < t.d + t.n()) fn1_out_.push_back({i, s, (size_t)(out - t.d)});
      }
    }
    if (fn1_out_.size() != 3) { ops1_.clear(); fcache_.clear(); fc_.clear(); return; }
    fn1_ok_ = true;
  }
  // every launch of the single-view plan becomes the batch plan's own kernel instance for that layer (the planner ranks candidates by a cost model that sees
  // the batch size; the arithmetic of an instance does not)
  bool match_fn1() {
    for (Op &o : ops1_) {
      const Op *b = nullptr;
      for (size_t i = 0; i < fork_hi_ && i < ops_.size(); ++i) if (ops_[i].name == o.name) b = &ops_[i];
      if (!b || b->kind != o.kind) return false;
      if (o.kind == Op::FRONT || o.kind == Op::HEAD3) continue;
      if (o.kind != Op::CONV) return false;
      if (same_instance(o.conv, b->conv)) continue;
      if (!o.replan) return false;
      bool found = false;
      for (int r = 0; r < o.ncand && !found; ++r) {
        const ConvLaunch c = o.replan(r);
        if (same_instance(c, b->conv)) { o.conv = c; found = true; }
      }
      if (!found) return false;
    }
    return true;
  }
  // decides, for the window being staged, which views the cache answers (FeatureIndex::plan); the guards that need engine state are here
  void plan_cache_use(int H, int W, int V, const uint8_t *const *bgrs, const int *order) {
    fc_.stand_down();
    if (!fn1_ok_ || shard_nsrc_ || comm_ || phase_mode_) return;  // (a view-shard rank computes its own views every time)
    for (int s = 1; s <= 3; ++s)
      if (choose_costvol(costvol_shape(cv_[s - 1]), sw_, s).family != CostVolChoice::V5) return;  // (only k_costvol5 reads the views by pointer)
    uint64_t keys[kMaxSrc + 1][2];
    for (int v = 0; v < V; ++v) image_key(bgrs[order[v]], (size_t)H * W * 3, H, W, keys[v]);
    fc_.plan(V, keys);
    // where the plane sweep finds each view
    for (int s = 0; s < 3; ++s)
      for (int v = 0; v < V; ++v)
        if (fc_.fast) cv_[s].vfeat[v] = fcache_[fc_.slot[v]].feat[s];
  }
  void launch_fn_op(const Op &o, hipStream_t st) {
    if (o.kind == Op::CONV) launch_conv(o.conv, st);
    else if (o.kind == Op::FRONT) launch_fn_front(o.front, st);
    else if (o.kind == Op::HEAD3) launch_fn_head3(o.head3, st);
    else fail(DR_ERR_UNSUPPORTED, "feature cache: op kind %d in the single-view plan", (int)o.kind);
  }
  // one launch: the hits compared with their entries' images, the new image filed in its entry
  void enqueue_cache_io() {
    const size_t img_bytes = (size_t)H_ * W_ * 3;
    CacheIoArgs io{};
    for (int v = 0; v < V_; ++v) {
      io.img[v] = reinterpret_cast<const uint4 *>(d_bgr_ + v * img_bytes);
      io.entry[v] = reinterpret_cast<uint4 *>(fcache_[fc_.slot[v]].bgr);
    }
    io.miss = fc_.miss; io.flag = fc_flag_dev(); io.n16 = img_bytes / 16;
    launch_cache_io(io, V_, stream_);
  }
  // fast path of a forward: verify the hits, FeatureNet on the one uncached view, its outputs (and image) into the entry
  void forward_cached_features() {
    const size_t img_bytes = (size_t)H_ * W_ * 3;
    if (!defer_cache_io_) enqueue_cache_io();
    if (fc_.miss >= 0) {
      const FcBuffers &e = fcache_[fc_.slot[fc_.miss]];
      for (const FnOut &p : fn1_out_) {
        Op &o = ops1_[p.op];
        (o.kind == Op::CONV ? o.conv.args.out : o.head3.out) = e.feat[p.stage] + p.offset;
      }
      // (the heads on the side stream, as the batch path runs them, were measured: device time 1.821 -> 1.825 ms, the sliding loop x 1.10 instead of x 1.12-1.15 --
      // two cross-stream waits cost what the overlap of three small launches wins; not kept)
      for (Op &o : ops1_) {
        if (o.kind == Op::FRONT) o.front.bgr = d_bgr_ + fc_.miss * img_bytes;
        launch_fn_op(o, stream_);
      }
      fc_.set_valid(fc_.slot[fc_.miss]);
    }
  }
  // batch path with the cache on: every view's features (and image) into its entry, behind the forward that produced them
  void fill_cache_from_batch() {
    const size_t img_bytes = (size_t)H_ * W_ * 3;
    for (int v = 0; v < V_; ++v) {
      const FcBuffers &e = fcache_[fc_.slot[v]];
      if (fc_.valid(fc_.slot[v])) continue;
      for (int s = 0; s < 3; ++s) {
        const DevTensor &t = T("feat" + std::to_string(s + 1));
        const size_t n1 = t.n() / t.D;
        DR_HIP(hipMemcpyAsync(e.feat[s], t.d + v * n1, n1 * 4, hipMemcpyDeviceToDevice, stream_));
      }
      DR_HIP(hipMemcpyAsync(e.bgr, d_bgr_ + v * img_bytes, img_bytes, hipMemcpyDeviceToDevice, stream_));
      fc_.set_valid(fc_.slot[v]);
    }
  }
  int *fc_flag_dev() { int *d = nullptr; DR_HIP(hipHostGetDevicePointer((void **)&d, fc_flag_, 0)); return d; }
  // after a stream synchronise: a hit that was not one (key collision).  The cache is dropped and the staged window runs again on the batch path.
  bool cache_mismatch_recovered() {
    if (!fc_flag_ || !*fc_flag_) return false;
    *fc_flag_ = 0;
    ++fc_.collisions;
    fc_.invalidate_all();
    fc_.fast = false; fc_.fill = false;
    for (int s = 0; s < 3; ++s) set_batch_vfeat(s);
    forward(nullptr);
    DR_HIP(hipStreamSynchronize(stream_));
    return true;
  }
  void set_batch_vfeat(int s) {
    const DevTensor &t = T("feat" + std::to_string(s + 1));
    for (int v = 0; v < V_ && v <= kMaxSrc; ++v) cv_[s].vfeat[v] = t.d + (size_t)v * (t.n() / t.D);
  }

  void build_plan(int H, int W, int V) {
    plan_arena_.reset(new DeviceArena());
    plan_arena_->err_flag = march_err_;
    for (float *&h : h_out_) if (h) { (void)hipHostFree(h); h = nullptr; }
    if (h_in_) { (void)hipHostFree(h_in_); h_in_ = nullptr; }
    for (int b = 0; b < 2; ++b) {
      DR_HIP(hipHostMalloc((void **)&h_out_[b], (size_t)H * W * 16, hipHostMallocDefault));
      DR_HIP(hipHostGetDevicePointer((void **)&h_out_dev_[b], h_out_[b], 0));
    }
    has_output_ = false;
    DR_HIP(hipHostMalloc((void **)&h_in_, (size_t)V * H * W * 3, hipHostMallocDefault));
    d_bgr_ = dalloc<uint8_t>((size_t)V * H * W * 3 + 16); misc_.push_back(d_bgr_);  // (+16: k_fn_front fetches a pixel as the two aligned words around it)
    d_state_ = dalloc<unsigned>(16); misc_.push_back(d_state_);   // four 4-word slots (the fused-scan form keeps one per level)
    d_hist_ = dalloc<unsigned>(3 * 2048); misc_.push_back(d_hist_);  // one histogram per level (the k_scan form uses the first only)
    DR_HIP(hipMemset(d_hist_, 0, 3 * 2048 * 4));
    DR_HIP(hipMemset(d_state_, 0, 16 * 4));

    build_featurenet(V, H, W);
    if (fcache_cap_ > 0) build_fn1(H, W);

    for (int s = 1; s <= 3; ++s) {
      const int sc = 1 << (3 - s), h = H / sc, w = W / sc, D = blob_.depth_num[s - 1], C = 32 >> (s - 1);
      if (!(D == 4 || D % 8 == 0)) fail(DR_ERR_UNSUPPORTED, "depth_num[%d]=%d must be 4 or a multiple of 8", s - 1, D);
      const std::string S = std::to_string(s), cr = "cost_regularization_net.stage" + S + ".", pre = "s" + S + ".";
      DevTensor &vol = alloc("volume" + S, D, h, w, C);
      if (C == 32 && sw_.vol_split && !conv_bf3_policy()) vol.split = 16;  // (the bf16 x 3 mode stages through its own kernel: one tensor)
      {
        Op o; o.kind = Op::COSTVOL; o.stage = s; o.name = pre + "costvol";
        o.bytes = 4.0 * ((double)V * h * w * C + vol.n());
        o.flops = (double)(V - 1) * D * h * w * (3.0 * C + 2.0 * C + 8.0 * C);  // diff^2, gate dot, weighted accumulate, 4-tap lerp
        ops_.push_back(o);
      }
      const bool four = D == 4;
      DevTensor &c0 = cbr3(pre + "conv0", cr + "conv0", vol, 1, 1, CONV_XPAIR);
      DevTensor &k1 = cbr3(pre + "conv1", cr + "conv1", c0, 2, 2, CONV_NORMAL);
      DevTensor &k2 = cbr3(pre + "conv2", cr + "conv2", k1, 1, 1, CONV_NORMAL);
      DevTensor &k3 = cbr3(pre + "conv3", cr + "conv3", k2, 2, 2, CONV_NORMAL);
      DevTensor &k4 = cbr3(pre + "conv4", cr + "conv4", k3, 1, 1, CONV_NORMAL);
      DevTensor &k5 = cbr3(pre + "conv5", cr + "conv5", k4, four ? 1 : 2, 2, CONV_NORMAL);
      DevTensor &k6 = cbr3(pre + "conv6", cr + "conv6", k5, 1, 1, CONV_NORMAL);
      DevTensor &x7 = dbr3(pre + "conv7", cr + "conv7", k6, four ? 1 : 2, k4);
      DevTensor &x9 = dbr3(pre + "conv9", cr + "conv9", x7, 2, k2);
#ifdef DR_PARITY_HOOKS
      const HostTensor &w11 = blob_.at(cr + "conv11.conv.weight");
      const HostTensor &wpr = blob_.at(cr + "prob.weight");
      const bool tail = sw_.tail_fused && !sw_.prob_on_conv && !conv_bf3_policy() && w11.dims.size() == 5 && w11.dims[0] == 16 && w11.dims[1] == 8 && w11.dims[2] == 3 &&
                        w11.dims[3] == 3 && w11.dims[4] == 3 && x9.C == 16 && c0.C == 8 && x9.D * 2 == D && x9.H * 2 == h && x9.W * 2 == w && wpr.dims[0] == 1 && wpr.dims[1] == 8;
      if (tail) {
        // conv11 (ConvTranspose3d 16 -> 8 + BN + ReLU, + conv0) and prob (8 -> 1) in one z-marching launch: the 8-channel full-resolution tensor
        // between them (78.6 MB at stages 2 and 3) is never written or read (tail_kernels.h)
        std::vector<float> sc, bi;
        fold_bn(blob_, cr + "conv11.bn", 8, sc, bi);
        sc.insert(sc.end(), bi.begin(), bi.end());
        DevTensor &lg = alloc("logits" + S, D, h, w, 1);
        Op o; o.kind = Op::TAIL; o.stage = s; o.name = pre + "tail";
        TailArgs &t = o.tail;
        t.x = x9.d; t.skip = c0.d; t.out = lg.d; t.D = D; t.h = h; t.w = w;
        t.wd = plan_arena_->upload(tail_pack_deconv(w11.data.data()));
        t.sb = plan_arena_->upload(sc);
        t.wp = plan_arena_->upload(tail_pack_prob(wpr.data.data()));
        const bool mf = sw_.tail_fused == 1;
        t.wmf = mf ? plan_arena_->upload(tail_pack_deconv_mfma(w11.data.data())) : nullptr;
        tail_set_tile(t, sw_.tail_qy, sw_.tail_zchunk, mf);
        const double N = (double)D * h * w;
        o.flops = 2.0 * 3.375 * 16 * 8 * N + 2.0 * 216 * N;  // the algorithmic MACs of both layers (halo recomputation not counted)
        o.bytes = 4.0 * (x9.n() + c0.n() + lg.n());
        ops_.push_back(o);
      } else
#endif
      {
      DevTensor &x11 = dbr3(pre + "conv11", cr + "conv11", x9, 2, c0);
      if (sw_.prob_on_conv && w % 8 == 0) {
        // A/B hook: the Cout = 1 head as 8 x-shifts per column on the MFMA kernel (CONV_X8, 50 % of the rows carry work);
        // measured against k_prob in profiles/r02_experiments.txt
        add_conv(pre + "prob", cr + "prob", "", false, false, x11, "logits" + S, 3, 3, 3, 1, 1, 1, false, CONV_X8, nullptr, 0);
      } else {
        DevTensor &lg = alloc("logits" + S, D, h, w, 1);
        Op o; o.kind = Op::PROB; o.stage = s; o.name = pre + "prob";
        pr_[s - 1] = {x11.d, plan_arena_->upload(prob_taps(blob_.at(cr + "prob.weight").data)), lg.d, D, h, w};
        o.flops = 2.0 * 216 * D * h * w; o.bytes = 4.0 * (x11.n() + lg.n());
        ops_.push_back(o);
      }
      }
      alloc("depth" + S, 1, h, w, 1);
      alloc("conf" + S, 1, h, w, 1);
      { Op o; o.kind = Op::REGRESS; o.stage = s; o.name = pre + "regress"; o.bytes = 4.0 * ((double)D * h * w + 2.0 * h * w); o.flops = 8.0 * D * h * w; ops_.push_back(o); }
    }
    filt_ = {T("depth3").d, T("conf3").d, alloc("edge", 1, H, W, 1).d, alloc("depth", 1, H, W, 1).d, alloc("confidence", 1, H, W, 1).d, d_state_, d_hist_,
             H * W, H, W, sw_.hist_blocks, sw_.filter_fused};
    { Op o; o.kind = Op::EDGE; o.name = "filter.edge"; o.bytes = 8.0 * H * W; ops_.push_back(o); }
    const int *shifts = kSelectShift, *bits = kSelectBits;
    for (int i = 0; i < 3; ++i) {
      Op o; o.kind = Op::HIST; o.shift = shifts[i]; o.bits = bits[i]; o.stage = i; o.d0 = i ? shifts[i - 1] : 0; o.d1 = i ? bits[i - 1] : 0;
      o.name = "filter.hist" + std::to_string(i); o.bytes = 4.0 * H * W; ops_.push_back(o);
      if (sw_.filter_fused) continue;  // (the scan of level i is the prologue of the next kernel: mvs_kernels.h k_hist_s / k_apply_s)
      Op q; q.kind = Op::SCAN; q.shift = shifts[i]; q.bits = bits[i]; q.name = "filter.scan" + std::to_string(i); ops_.push_back(q);
    }
    { Op o; o.kind = Op::APPLY; o.name = "filter.apply"; o.shift = shifts[2]; o.bits = bits[2]; o.bytes = 20.0 * H * W; ops_.push_back(o); }
  }

  // Copies the window into pinned memory in model order [ref, others] (dr_mvsnet.cpp:190-197), enqueues
  // the H2D copy and derives every per-call kernel parameter.  Caller holds mu_.
  void stage_inputs(int H, int W, int V, int ref, const uint8_t *const *bgrs, const float *K9, const float *const *c2ws,
                    float dmin, float dmax, float disc, bool may_prelaunch = false) {
    DR_HIP(hipSetDevice(device_));
    configure(H, W, V);
    const size_t img_bytes = (size_t)H * W * 3;
    const WindowGeometry geo = plan_geometry(H, W, V, ref, K9, c2ws, dmin, dmax, disc, blob_, shard_nsrc_);  // cameras, plane ranges, filter rank (mvs_host.h)
    const int *order = geo.order;  // model order [ref, others]
    // view by view: the copy engine moves view v to the device while the host gathers view v + 1 into the pinned block (one 6.45 MB
    // transfer behind seven memcpys cost their sum: 0.3 + 0.2 ms at 640 x 480 x 7 on the operator boundary's critical path)
    // Images that already live in page-locked memory (drm_host_alloc, hipHostMalloc, hipHostRegister) go to the device straight from
    // where they are -- no gather into the pinned block, which is the 0.3-0.4 ms memcpy on the operator boundary's critical path; the
    // call still returns only when the copies have completed ("inputs are copied before return": the caller may reuse its buffers).
    // "Page-locked" is decided for the WHOLE image, not for its first byte: the allocation (or registered range) the first byte lies in has
    // to contain all img_bytes of it -- an image that starts inside a hipHostRegister'ed range and runs past its end takes the staging path.
    bool pinned = true;
    for (int v = 0; v < V && pinned; ++v) {
      hipPointerAttribute_t at;
      hipDeviceptr_t base = nullptr;
      size_t span = 0;
      if (hipPointerGetAttributes(&at, bgrs[v]) != hipSuccess || at.type != hipMemoryTypeHost || !at.devicePointer ||
          hipMemGetAddressRange(&base, &span, (hipDeviceptr_t)at.devicePointer) != hipSuccess) {
        (void)hipGetLastError();
        pinned = false;
      } else {
        const char *lo = (const char *)base, *p = (const char *)at.devicePointer;
        pinned = p >= lo && p + img_bytes <= lo + span;
      }
    }
    for (int s = 1; s <= 3; ++s) {
      const StageGeometry &g = geo.stage[s - 1];
      const int sc = 1 << (3 - s), h = H / sc, w = W / sc, D = g.D, C = 32 >> (s - 1);
      const std::string S = std::to_string(s);
      const DevTensor &feat = T("feat" + S), &vol = T("volume" + S);
      CostVolArgs &a = cv_[s - 1];
      memset(&a, 0, sizeof a);
      a.feat = feat.d; a.fpad = feat.pad;
      a.vol = vol.d; a.split = vol.split;
      a.V = V; a.h = h; a.w = w;
      a.view_aggregation = blob_.view_aggregation;
      a.dchunk = costvol_dchunk(s, D, a.view_aggregation, a.fpad, sw_);
      a.nsrc_f = g.nsrc_f;
      memcpy(a.M, g.M, sizeof a.M);
      PlaneArgs &p = a.planes;
      p.D = D; p.dmin = g.dmin; p.interval = g.interval;
      p.half_range = g.half_range; p.full_range = g.full_range;
      if (s > 1) { p.prev = T("depth" + std::to_string(s - 1)).d; p.hp = h / 2; p.wp = w / 2; }
      if (blob_.view_aggregation) {
        const GateFold gf = fold_gate(blob_, s, C);
        memcpy(a.gw, gf.gw, sizeof a.gw);
        a.gA1 = gf.gA1; a.gB1 = gf.gB1; a.gA2 = gf.gA2; a.gB2 = gf.gB2;
      }
      RegressArgs &r = rg_[s - 1];
      r.logits = T("logits" + S).d;
      r.depth = T("depth" + S).d;
      r.conf = T("conf" + S).d;
      r.planes = p; r.h = h; r.w = w;
    }
    for (int s = 0; s < 3; ++s) set_batch_vfeat(s);
    if (fcache_cap_ > 0) plan_cache_use(H, W, V, bgrs, order);
    filter_rank_ = geo.filter_rank;
    prelaunched_ = false;
    // PRELAUNCH (CallAsync with the feature cache answering the window): the device needs ONE image -- the new one -- to start; the other six are only compared
    // with their cache entries, which can happen last.  So the new image goes up first, the helper thread stages and uploads the rest on a second stream, and
    // THIS thread enqueues the whole forward meanwhile; the comparison (k_cache_io) is enqueued behind it once the uploads are in flight.  The device starts
    // ~0.3 ms earlier in TandemBackend's loop (it idles while a window is staged); the call still returns only when every image has been copied.
    if (may_prelaunch && fc_.fast && up_stream_) {
      auto up_one = [&, pinned](int v, hipStream_t st) {
        const uint8_t *src = bgrs[order[v]];
        if (!pinned) { memcpy(h_in_ + v * img_bytes, src, img_bytes); src = h_in_ + v * img_bytes; }
        DR_HIP(hipMemcpyAsync(d_bgr_ + v * img_bytes, src, img_bytes, hipMemcpyHostToDevice, st));
      };
      const int miss = fc_.miss;
      if (miss >= 0) {
        up_one(miss, stream_);
        if (pinned) {  // (read in place from the caller's page-locked image: waited for before the call returns)
          if (!ev_h2d_) DR_HIP(hipEventCreateWithFlags(&ev_h2d_, hipEventDisableTiming));
          DR_HIP(hipEventRecord(ev_h2d_, stream_));
        }
      }
      copier_.run([&, miss] {
        DR_HIP(hipSetDevice(device_));
        for (int v = 0; v < V; ++v) if (v != miss) up_one(v, up_stream_);
        DR_HIP(hipEventRecord(ev_hits_, up_stream_));
      });
      struct Count {  // this window counts as in flight from here; the worker's InFlight takes the count over once prelaunched_ is set
        std::atomic<int> &n; bool handed_over = false;
        explicit Count(std::atomic<int> &a) : n(a) { n.fetch_add(1, std::memory_order_relaxed); }
        ~Count() { if (!handed_over) n.fetch_sub(1, std::memory_order_relaxed); }
      } count(windows_in_flight(device_));
      try {
        defer_cache_io_ = true;
        forward(nullptr);
        defer_cache_io_ = false;
      } catch (...) { defer_cache_io_ = false; copier_.wait_quiet(); throw; }
      copier_.wait();
      DR_HIP(hipStreamWaitEvent(stream_, ev_hits_, 0));
      enqueue_cache_io();
      if (pinned) {  // uploaded in place from the caller's page-locked images: they must have been read before the call returns
        DR_HIP(hipEventSynchronize(ev_hits_));
        if (miss >= 0) DR_HIP(hipEventSynchronize(ev_h2d_));
      }
      prelaunched_ = true;
      count.handed_over = true;
    } else {
    auto upload_views = [&, pinned](int v0) {  // views v0, v0 + 2, ...: gather into the staging block (unless page-locked already), then the copy engine
        DR_HIP(hipSetDevice(device_));
        for (int v = v0; v < V; v += 2) {
          const uint8_t *src = bgrs[order[v]];
          if (!pinned) { memcpy(h_in_ + v * img_bytes, src, img_bytes); src = h_in_ + v * img_bytes; }
          DR_HIP(hipMemcpyAsync(d_bgr_ + v * img_bytes, src, img_bytes, hipMemcpyHostToDevice, stream_));
        }
      };
      if (!pinned) {
        copier_.run([&] { upload_views(1); });  // the helper thread takes every other view
        try { upload_views(0); } catch (...) { copier_.wait_quiet(); throw; }  // (the job refers to this frame's locals)
        copier_.wait();
      } else {
        upload_views(1);
        upload_views(0);
      }
      if (pinned) {
        if (!ev_h2d_) DR_HIP(hipEventCreateWithFlags(&ev_h2d_, hipEventDisableTiming));
        DR_HIP(hipEventRecord(ev_h2d_, stream_));
        DR_HIP(hipEventSynchronize(ev_h2d_));
      }

    }
  }

  // Enqueue one complete forward on stream_ (or the ops [first, last) of it).  ev (optional): ops_.size()+1 events
  // for per-op timing.
  //
  // A whole forward (no per-op events, no range) forks: the FeatureNet heads that only stages 2 and 3 need
  // (fn.skip2, fn.out2, fn.skip3, fn.out3 -- 0.5 ms at 640x480) run on a side stream under stage 1's cost volume and
  // regularisation, whose coarse UNet levels leave most CUs idle; stage 2 / 3's cost volume waits for feat2 / feat3.
  // The next forward's main-stream work is ordered after those waits, so the side stream never runs ahead of a reader.
  void forward(std::vector<hipEvent_t> *ev, size_t first = 0, size_t last = ~(size_t)0) {
    if ((fc_.fast || fc_.fill) && !(first == 0 && last >= ops_.size())) {  // a partial forward (phases, one op) cannot skip FeatureNet: the window goes back to the batch path
      fc_.fast = fc_.fill = false;
      for (int s = 0; s < 3; ++s) set_batch_vfeat(s);
    }
    const bool cached = fc_.fast;  // FeatureNet answered by the feature cache: its ops are skipped
    // ... unless other engines of this process have windows in flight on the device: their kernels already fill the idle CUs, and a second stream per
    // engine only adds queue contention (4 engines: 580 depth maps/s without the fork against 570 with it, profiles/r06_queues_side_stream.txt; alone: 2.150 ms
    // with it against 2.165).  Same kernels in the same per-stream order either way: the result does not depend on it.
    const bool alone = windows_in_flight(device_).load(std::memory_order_relaxed) <= 1;
    const bool fork = side_enabled_ && alone && !ev && first == 0 && last >= ops_.size() && fork_lo_ < fork_hi_ && !cached;
    if (cached) forward_cached_features();
    // view shard, reduce-to-root form: between a stage's cost volume and its regression only rank 0 works
    const bool rooted = comm_ && shard_nsrc_ && !phase_mode_ && !sw_.shard_allreduce;
    bool idle_stage = false;
    size_t i = 0;
    for (const Op &o : ops_) {
      if (ev) DR_HIP(hipEventRecord((*ev)[i], stream_));
      ++i;
      if (i - 1 < first || i - 1 >= last) continue;
      if (cached && i - 1 < fork_hi_) continue;
      if (idle_stage && o.kind != Op::REGRESS) continue;  // (CostRegNet and prob of this stage run on rank 0 only)
      const bool on_side = fork && i - 1 >= fork_lo_ && i - 1 < fork_hi_;
      if (fork && i - 1 == fork_lo_) { DR_HIP(hipEventRecord(ev_fork_, stream_)); DR_HIP(hipStreamWaitEvent(side_, ev_fork_, 0)); }
      if (fork && o.kind == Op::COSTVOL && o.stage == 2) DR_HIP(hipStreamWaitEvent(stream_, ev_feat2_, 0));
      if (fork && o.kind == Op::COSTVOL && o.stage == 3) DR_HIP(hipStreamWaitEvent(stream_, ev_feat3_, 0));
      const hipStream_t st = on_side ? side_ : stream_;
      switch (o.kind) {
        case Op::PREPROCESS: launch_preprocess(o.pre, st); break;
        case Op::CONV: launch_conv(o.conv, st); break;
        case Op::BORDERFIX: launch_out3_border(o.p2, o.p1, o.d0, o.d1, o.d2, o.stage, st); break;
        case Op::SKIPUP: launch_skip_up(o.p0, o.p1, o.p3, o.p4, o.p2, o.d0, o.d1, o.d2, st); break;
        case Op::PROB: launch_prob(pr_[o.stage - 1], rg_[o.stage - 1], sw_, o.stage, st); break;
        case Op::TAIL: launch_tail_op(o, st); break;
        case Op::FRONT: launch_fn_front(o.front, st); break;
        case Op::HEAD3: launch_fn_head3(o.head3, st); break;
        case Op::COSTVOL: {
          const CostVolArgs &a = cv_[o.stage - 1];
          // a view-shard rank that holds the reference view only: its partial volume is the empty sum (the kernels return without storing)
          if (a.V - 1 <= 0) { const DevTensor &vol = T("volume" + std::to_string(o.stage)); DR_HIP(hipMemsetAsync(vol.d, 0, vol.n() * 4, st)); }
          launch_costvol(a, sw_, o.stage, st);
          if (comm_ && shard_nsrc_ && !phase_mode_) {  // view shard: sum the partial volumes of all ranks, in place, in stream order
            const DevTensor &vol = T("volume" + std::to_string(o.stage));
            Rccl &r = Rccl::get();
            if (rooted) {
              r.check(r.Reduce(vol.d, vol.d, vol.n(), ncclFloat, ncclSum, 0, comm_, st), "ncclReduce");
              idle_stage = comm_rank_ != 0;
            } else r.check(r.AllReduce(vol.d, vol.d, vol.n(), ncclFloat, ncclSum, comm_, st), "ncclAllReduce");
          }
          break;
        }
        case Op::REGRESS: {
          // (where the stage's PROB op ran k_prob2_regress, the regression is done: the same choice function says so here and there)
          const ProbArgs &pr = pr_[o.stage - 1];
          const bool done = pr.x && choose_prob(prob_shape(pr), sw_, o.stage).regresses();
          if (!idle_stage && !done) launch_regress(rg_[o.stage - 1], sw_, st);
          if (rooted) {  // the stage's depth map goes back to every rank: stage s + 1 centres its hypotheses on it; stage 3's
            Rccl &c = Rccl::get();  // depth and confidence are the result (the edge filter then runs on every rank: 0.08 ms)
            const DevTensor &dep = T("depth" + std::to_string(o.stage));
            c.check(c.Broadcast(dep.d, dep.d, dep.n(), ncclFloat, 0, comm_, st), "ncclBroadcast");
            if (o.stage == 3) {
              const DevTensor &cf = T("conf3");
              c.check(c.Broadcast(cf.d, cf.d, cf.n(), ncclFloat, 0, comm_, st), "ncclBroadcast");
            }
            idle_stage = false;
          }
          break;
        }
        case Op::EDGE: launch_edge(filt_, filter_rank_, st); break;
        case Op::HIST: launch_hist(filt_, o.stage, o.d0, o.d1, o.shift, o.bits, st); break;
        case Op::SCAN: launch_scan(filt_, o.shift, o.bits, st); break;
        case Op::APPLY: launch_apply(filt_, o.shift, o.bits, st); break;
      }
      // the side stream's results are published after whichever op ends them (fn.out2; the LAST op of the fork range: a
      // convolution in the fused-skip form, the border kernel in the folded form) -- independent of the op kind
      if (on_side && i - 1 == feat2_op_) DR_HIP(hipEventRecord(ev_feat2_, side_));
      if (on_side && i - 1 == fork_hi_ - 1) DR_HIP(hipEventRecord(ev_feat3_, side_));
    }
    if (fc_.fill && first == 0 && last >= ops_.size()) fill_cache_from_batch();
    if (ev) DR_HIP(hipEventRecord((*ev)[i], stream_));
    DR_HIP(hipGetLastError());
  }

  void launch_tail_op([[maybe_unused]] const Op &o, [[maybe_unused]] hipStream_t st) {
#ifdef DR_PARITY_HOOKS
    launch_tail(o.tail, st);
#endif  // (the product plans no TAIL op)
  }
  hipStream_t side_ = nullptr;
  hipEvent_t ev_fork_ = nullptr, ev_feat2_ = nullptr, ev_feat3_ = nullptr;
  bool side_enabled_ = true;
  size_t fork_lo_ = 0, fork_hi_ = 0, feat2_op_ = 0;  // ops [fork_lo_, fork_hi_) = fn.skip2 .. fn.out3
  // key-frame feature cache (build_fn1 .. set_batch_vfeat)
  int fcache_cap_ = 0;             // entries (0: off, the default)
  std::vector<FcBuffers> fcache_;  // the entries' device buffers, parallel to the index
  FeatureIndex fc_;                // which entry answers which view of the staged window; LRU; counters (mvs_host.h)
  std::vector<Op> ops1_;           // FeatureNet for ONE view
  std::vector<FnOut> fn1_out_;
  std::string tprefix_;            // tensor-name prefix while ops1_ is built
  bool fn1_ok_ = false;            // the single-view plan exists and matches the batch plan's instances
  int *fc_flag_ = nullptr;         // page-locked: raised by k_cache_io
  hipStream_t up_stream_ = nullptr;  // uploads of the images the cache answers (prelaunch, stage_inputs)
  hipEvent_t ev_hits_ = nullptr;
  bool prelaunched_ = false;       // the staged window's forward is already on the stream (the worker only publishes)
  bool defer_cache_io_ = false;    // ... and its image comparison follows once the uploads are in flight

  const MvsSwitches sw_;  // read once, here
#ifdef DR_PARITY_HOOKS
  static constexpr bool kParityHooks = true;
#else
  static constexpr bool kParityHooks = false;
#endif
  int device_;
  int *march_err_ = nullptr;
  // called after a stream synchronise: a marching convolution that gave up a wait leaves garbage behind -- report it, never return it
  void check_march() {
    if (march_err_ && *march_err_) { const int c = *march_err_; *march_err_ = 0; fail(DR_ERR_DEVICE, "k_conv_m: a ring wait gave up (code %d): the LDS producer/consumer protocol stalled", c); }
  }
  Blob blob_;
  hipStream_t stream_ = nullptr;
  DeviceArena consts_;
  const float *lut_ = nullptr;
  std::unique_ptr<DeviceArena> plan_arena_;
  std::map<std::string, DevTensor> tensors_;
  std::vector<Op> ops_;
  std::vector<void *> misc_;
  CostVolArgs cv_[3];
  RegressArgs rg_[3];
  ProbArgs pr_[3];    // per stage; x == nullptr where the plan has no PROB op
  FilterArgs filt_{};
  uint8_t *d_bgr_ = nullptr, *h_in_ = nullptr;
  float *h_out_[2] = {nullptr, nullptr}, *h_out_dev_[2] = {nullptr, nullptr};  // two pinned result blocks (4 maps each), used alternately, and the addresses the device uses for them
  int out_cur_ = 0;                // the block the last result is in
  hipEvent_t ev_h2d_ = nullptr;    // completion of a window uploaded straight from the caller's page-locked images
  unsigned *d_state_ = nullptr, *d_hist_ = nullptr;
  unsigned filter_rank_ = 0;
  int H_ = 0, W_ = 0, V_ = 0;
  int shard_nsrc_ = 0;  // > 0: view-shard rank, cost-volume divisor = source views of the whole window
  ncclComm_t comm_ = nullptr;  // view-shard communicator (drm_comm_init); the volumes are reduced in stream order when set
  int comm_world_ = 0, comm_rank_ = 0;
  // Collective form of a sharded forward (MvsSwitches::shard_allreduce).  Default: the partial volumes are REDUCED to rank 0, which
  // alone regularises and regresses the stage, and the stage's depth map (what the next stage's hypotheses hang on: 77 / 307 /
  // 1229 KB) is BROADCAST back -- (n-1)/n x 354 MB over xGMI per depth map instead of the all-reduce's 2(n-1)/n, and no redundant
  // CostRegNet on the other ranks.  DR_SHARD_ALLREDUCE=1: round 2's form (sum all-reduce, every rank
  // regularises redundantly; no broadcast).
  bool phase_mode_ = false;

  std::thread worker_;
  HostCopier copier_;
  std::mutex mu_;
  std::condition_variable input_cv_, done_cv_;
  bool running_ = true;
  std::atomic<bool> unprocessed_{false};  // read without the lock by ready() (dr_mvsnet.cpp:54 does the same with a plain bool)
  bool has_output_ = false;
  std::string worker_error_;
};

}  // namespace dr

// ==================================================================== C ABI
using dr::guarded;
struct drm_s {
  std::unique_ptr<dr::MvsEngine> e;
};
// every C-ABI entry point goes through this: a NULL handle is an argument error, not a crash
static inline dr::MvsEngine *eng(drm_s *h) {
  if (!h || !h->e) dr::fail(DR_ERR_ARG, "NULL handle");
  return h->e.get();
}

extern "C" {

const char *dr_last_error(void) { return dr::last_error_slot().c_str(); }
const char *dr_version(void) { return "dr_mi355x 0.1 gfx950"; }

int drm_create(const char *weights_path, int device, drm_t **out) {
  return guarded([&] {
    if (!weights_path || !out) dr::fail(DR_ERR_ARG, "drm_create: null argument");
    auto *h = new drm_s();
    try { h->e.reset(new dr::MvsEngine(weights_path, device)); } catch (...) { delete h; throw; }
    *out = h;
  });
}
void drm_destroy(drm_t *h) { delete h; }
int drm_set_feature_cache(drm_t *h, int capacity) { return guarded([&] { eng(h)->set_feature_cache(capacity); }); }
int drm_feature_cache_stats(drm_t *h, uint64_t out[6]) {
  return guarded([&] { if (!out) dr::fail(DR_ERR_ARG, "drm_feature_cache_stats: null argument"); eng(h)->feature_cache_stats(out); });
}
int drm_call_async(drm_t *h, int height, int width, int view_num, int ref_index, const uint8_t *const *bgrs, const float *K9,
                   const float *const *c2ws, float depth_min, float depth_max, float discard_percentage) {
  return guarded([&] { eng(h)->call_async(height, width, view_num, ref_index, bgrs, K9, c2ws, depth_min, depth_max, discard_percentage); });
}
int drm_ready(drm_t *h) { return (h && h->e && h->e->ready()) ? 1 : 0; }
int drm_wait(drm_t *h) { return guarded([&] { eng(h)->wait(); }); }
int drm_get_result(drm_t *h, float *depth, float *confidence, float *depth_dense, float *confidence_dense) {
  return guarded([&] { eng(h)->get_result(depth, confidence, depth_dense, confidence_dense); });
}
int drm_get_result_view(drm_t *h, const float **depth, const float **confidence, const float **depth_dense, const float **confidence_dense) {
  return guarded([&] { eng(h)->get_result_view(depth, confidence, depth_dense, confidence_dense); });
}
void *drm_host_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
void drm_host_free(void *p) { if (p) (void)hipHostFree(p); }
int drm_upload(drm_t *h, int height, int width, int view_num, int ref_index, const uint8_t *const *bgrs, const float *K9,
               const float *const *c2ws, float depth_min, float depth_max, float discard_percentage) {
  return guarded([&] { eng(h)->upload(height, width, view_num, ref_index, bgrs, K9, c2ws, depth_min, depth_max, discard_percentage); });
}
int drm_forward(drm_t *h, int iters, float *ms_total) { return guarded([&] { eng(h)->forward_n(iters, ms_total); }); }
int drm_autotune(drm_t *h, int max_candidates, float *before_ms, float *after_ms) {
  return guarded([&] { eng(h)->autotune(max_candidates, before_ms, after_ms); });
}
int drm_set_view_shard(drm_t *h, int nsrc_total) { return guarded([&] { eng(h)->set_view_shard(nsrc_total); }); }
int drm_forward_phase(drm_t *h, int phase) { return guarded([&] { eng(h)->forward_phase(phase); }); }
int drm_comm_available(void) { return guarded([&] { (void)dr::Rccl::get(); }); }
int drm_comm_unique_id(uint8_t id[128]) {
  return guarded([&] {
    if (!id) dr::fail(DR_ERR_ARG, "drm_comm_unique_id: null argument");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    dr::Rccl &r = dr::Rccl::get();
    ncclUniqueId u;
    r.check(r.GetUniqueId(&u), "ncclGetUniqueId");
    memcpy(id, &u, 128);
  });
}
int drm_comm_init(drm_t *h, int rank, int world, const uint8_t id[128]) { return guarded([&] { eng(h)->comm_init(rank, world, id); }); }
int drm_comm_destroy(drm_t *h) { return guarded([&] { eng(h)->comm_destroy(); }); }
int drm_comm_count(drm_t *h, int *nranks) {
  return guarded([&] { if (!nranks) dr::fail(DR_ERR_ARG, "drm_comm_count: null pointer"); *nranks = eng(h)->comm_count(); });
}
int drm_device_tensor(drm_t *h, const char *name, void **dptr, size_t *nfloats) {
  return guarded([&] { if (!name) dr::fail(DR_ERR_ARG, "drm_device_tensor: null name"); eng(h)->device_tensor(name, dptr, nfloats); });
}
int drm_download(drm_t *h, float *depth, float *confidence, float *depth_dense, float *confidence_dense) {
  return guarded([&] { eng(h)->download(depth, confidence, depth_dense, confidence_dense); });
}
int drm_get_stage_output(drm_t *h, int stage, float *depth, float *confidence) {
  return guarded([&] {
    if (stage < 1 || stage > 3) dr::fail(DR_ERR_ARG, "stage must be 1..3");
    size_t n; int dims[4];
    eng(h)->get_tensor(("depth" + std::to_string(stage)).c_str(), nullptr, 0, &n, dims);
    eng(h)->get_tensor(("depth" + std::to_string(stage)).c_str(), depth, n, &n, dims);
    eng(h)->get_tensor(("conf" + std::to_string(stage)).c_str(), confidence, n, &n, dims);
  });
}
int drm_get_tensor(drm_t *h, const char *name, float *out, size_t n_max, size_t *n, int dims[4]) {
  return guarded([&] { eng(h)->get_tensor(name, out, n_max, n, dims); });
}
int drm_profile(drm_t *h, char *names, size_t names_cap, float *ms, int cap, int *count) {
  return guarded([&] {
    std::string nm; std::vector<float> t;
    eng(h)->profile(nm, t);
    if (count) *count = (int)t.size();
    if (names && names_cap) { strncpy(names, nm.c_str(), names_cap - 1); names[names_cap - 1] = 0; }
    for (int i = 0; i < (int)t.size() && i < cap; ++i) ms[i] = t[i];
  });
}
int drm_work(drm_t *h, double *flops, double *bytes) { return guarded([&] { eng(h)->work(flops, bytes); }); }

int drm_debug_conv(int device, const float *in, int D, int H, int W, int Cin, const float *weight, int Cout, int kd, int kh, int kw,
                   int sd, int sh, int sw, int transposed, const float *scale, const float *bias, int relu, const float *add,
                   int add_up2, float *out, int out_dims[3]) {
  return guarded([&] {
    using namespace dr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device) fail(DR_ERR_DEVICE, "no HIP device %d", device);
    DR_HIP(hipSetDevice(device));
    DeviceArena arena;
    arena.err_flag = arena.upload(std::vector<int>(1, 0));
    ConvLayer L;
    L.Cin = Cin; L.Cout = Cout; L.kd = kd; L.kh = kh; L.kw = kw; L.sd = sd; L.sh = sh; L.sw = sw;
    L.transposed = transposed == 1; L.weight = weight; L.relu = relu != 0;
    const bool up2 = transposed == 2;  // test hook for ConvLayer::up2: both row parities, one launch each
    if (scale) L.scale.assign(scale, scale + Cout);
    if (bias) L.bias.assign(bias, bias + Cout);
    const ConvMode mode = (!transposed && sw == 1 && Cout == 8) ? CONV_XPAIR : ((!transposed && sw == 1 && Cout == 1) ? CONV_X8 : CONV_NORMAL);
    auto cz = axis_classes(kd, sd, L.transposed, D), cy = axis_classes(kh, sh, L.transposed, H), cx = axis_classes(kw, sw, L.transposed, W);
    const int oD = L.transposed ? D * sd : cz[0].npos, oH = L.transposed ? H * sh : (up2 ? 2 * H : cy[0].npos), oW = L.transposed ? W * sw : (up2 ? 2 * W : cx[0].npos);
    std::vector<float> hin(in, in + (size_t)D * H * W * Cin);
    float *d_in = arena.upload(hin);
    const size_t on = (size_t)oD * oH * oW * Cout;
    // the output starts as the poison pattern (guard_host.h), not as zeros: a position no launch writes is a NaN the caller sees
    float poison; memcpy(&poison, &guard::kWord, 4);
    float *d_out = arena.upload(std::vector<float>(on, poison));
    float *d_add = nullptr;
    if (add) {
      const size_t an = add_up2 ? (size_t)oD * (oH / 2) * (oW / 2) * Cout : on;
      std::vector<float> ha(add, add + an);
      d_add = arena.upload(ha);
    }
    // DR_CONV_RANK (test hook): build the rank-th candidate of the planner's ranking instead of its first choice
    const char *rk = getenv("DR_CONV_RANK");
    ConvPlanOut P;
    for (int py = 0; py < (up2 ? 2 : 1); ++py) {
      L.up2 = up2 ? 1 + py : 0;
      P = plan_conv(L, mode, d_in, D, H, W, Cin, d_out, d_add, add_up2 ? 2 : 1, arena, rk ? atoi(rk) : 0);
      for (auto &cl : P.launches) launch_conv(cl, nullptr);
    }
    DR_HIP(hipDeviceSynchronize());
    DR_HIP(hipGetLastError());
    int march_err = 0;
    DR_HIP(hipMemcpy(&march_err, arena.err_flag, sizeof(int), hipMemcpyDeviceToHost));
    if (march_err) fail(DR_ERR_DEVICE, "k_conv_m: a ring wait gave up (code %d)", march_err);
    if (getenv("DR_CONV_PRINT")) {
      const ConvLaunch &c = P.launches.at(0);
      fprintf(stderr, "debug_conv: %s<%d,%d,%d> nup %d tile %dx%dx%d lds %zu grid %ux%u (%d candidates)%s\n", *conv_kind_name(c) ? conv_kind_name(c) : (c.bf3 ? "bf16x3" : "sync"), c.ci, c.ct, c.pt,
              c.nup, c.args.TZ, c.args.TY, c.args.TXT * 16, c.lds_bytes, c.grid.x, c.grid.z, P.ncand,
              c.args.class_loop ? ", class loop" : (conv_family(c) == CONV_FAM_WINOMARCH ? (c.march.wino == 2 ? ", scatter order" : ", gather order") : ""));
    }
    DR_HIP(hipMemcpy(out, d_out, on * 4, hipMemcpyDeviceToHost));
    if (out_dims) { out_dims[0] = oD; out_dims[1] = oH; out_dims[2] = oW; }
  });
}

/* Kernel unit-test hook for k_tail (tail_kernels.h): conv11 (ConvTranspose3d 16 -> 8, k 3, s 2, p 1, op 1; folded BN scale / bias; ReLU; + skip) followed by prob
 * (Conv3d 8 -> 1, k 3, p 1).  x: (D/2, h/2, w/2, 16), skip: (D, h, w, 8) channels-last; w_deconv (16, 8, 3, 3, 3), w_prob (1, 8, 3, 3, 3) torch layouts;
 * qy: quad rows of the tile (0: chosen by size), zchunk: depth planes per workgroup (0: chosen), form: 1 = k_tail_m (matrix pipe), 0 = k_tail.  out: (D, h, w) logits. */
int drm_debug_tail(int device, const float *x, const float *skip, const float *w_deconv, const float *scale8, const float *bias8, const float *w_prob, int D, int h,
                   int w, int qy, int zchunk, int form, float *out) {
  return guarded([&] {
    using namespace dr;
#ifndef DR_PARITY_HOOKS
    fail(DR_ERR_UNSUPPORTED, "drm_debug_tail: k_tail / k_tail_m are built into the parity library (libdr_mi355x_hooks.so, -DDR_PARITY_HOOKS) only");
#else
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device) fail(DR_ERR_DEVICE, "no HIP device %d", device);
    if (D <= 0 || h <= 0 || w <= 0 || (D | h | w) & 1) fail(DR_ERR_ARG, "drm_debug_tail: output dims must be positive and even");
    DR_HIP(hipSetDevice(device));
    DeviceArena arena;
    TailArgs t{};
    t.x = arena.upload(std::vector<float>(x, x + (size_t)(D / 2) * (h / 2) * (w / 2) * 16));
    t.skip = arena.upload(std::vector<float>(skip, skip + (size_t)D * h * w * 8));
    t.wd = arena.upload(tail_pack_deconv(w_deconv));
    std::vector<float> sb(scale8, scale8 + 8);
    sb.insert(sb.end(), bias8, bias8 + 8);
    t.sb = arena.upload(sb);
    t.wp = arena.upload(tail_pack_prob(w_prob));
    float poison; memcpy(&poison, &guard::kWord, 4);  // (guard_host.h: a position the launch does not write stays a NaN)
    float *d_out = arena.upload(std::vector<float>((size_t)D * h * w, poison));
    t.out = d_out; t.D = D; t.h = h; t.w = w;
    const bool mf = form == 1;  // 1: k_tail_m (matrix pipe), else k_tail (vector pipe)
    t.wmf = mf ? arena.upload(tail_pack_deconv_mfma(w_deconv)) : nullptr;
    tail_set_tile(t, qy, zchunk, mf);
    launch_tail(t, nullptr);
    DR_HIP(hipDeviceSynchronize());
    DR_HIP(hipGetLastError());
    DR_HIP(hipMemcpy(out, d_out, (size_t)D * h * w * 4, hipMemcpyDeviceToHost));
#endif
  });
}

/* ---- kernel unit-test hooks for the regression and the edge filter (include/dr_mi355x.h).  Every buffer comes from a DeviceArena (the guarded allocator of
 * the parity build sees it), outputs start as the poison word, the switches are the engine's (MvsSwitches, read from the environment), and every launch goes
 * through the launcher the engine calls (mvs_launch.h): the kernel an input reaches is the one the engine would run on it. */
static void debug_device(int device, const char *who) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0) dr::fail(DR_ERR_DEVICE, "%s: no HIP device %d", who, device);
  DR_HIP(hipSetDevice(device));
}
static float *debug_poison(dr::DeviceArena &arena, size_t n) {
  float poison; memcpy(&poison, &dr::guard::kWord, 4);  // (guard_host.h: a position no launch writes stays a NaN)
  return arena.upload(std::vector<float>(n, poison));
}
static void debug_check_planes(const char *who, int D, int h, int w, const float *prev, int hp, int wp) {
  if (D <= 0 || h <= 0 || w <= 0 || D > 4096 || (long long)D * h * w > (1ll << 28)) dr::fail(DR_ERR_ARG, "%s: D, h, w must be positive (D <= 4096, D h w <= 2^28)", who);
  // up2_bilinear reads prev at rows <= (h - 1) / 2 and columns <= (w - 1) / 2: the previous stage's map is exactly half the size
  if (prev && (hp <= 0 || wp <= 0 || h != 2 * hp || w != 2 * wp)) dr::fail(DR_ERR_ARG, "%s: prev must be (h / 2, w / 2)", who);
}
static dr::RegressArgs debug_regress_args(dr::DeviceArena &arena, const float *d_logits, int D, int h, int w, const float *prev, int hp, int wp, float dmin,
                                          float interval, float half_range, float full_range) {
  dr::RegressArgs r{};
  r.logits = d_logits;
  r.depth = debug_poison(arena, (size_t)h * w);
  r.conf = debug_poison(arena, (size_t)h * w);
  r.planes.prev = prev ? arena.upload(std::vector<float>(prev, prev + (size_t)hp * wp)) : nullptr;
  r.planes.hp = prev ? hp : 0; r.planes.wp = prev ? wp : 0;
  r.planes.D = D; r.planes.dmin = dmin; r.planes.interval = interval;
  r.planes.half_range = half_range; r.planes.full_range = full_range;
  r.h = h; r.w = w;
  return r;
}
static void debug_regress_name(char *out, size_t cap, int D, const dr::MvsSwitches &sw) {
  const int d = dr::choose_regress(D, sw);
  if (d) snprintf(out, cap, "k_regress_r<%d>", d);
  else snprintf(out, cap, "k_regress");
}

int drm_debug_regress(int device, const float *logits, int D, int h, int w, const float *prev, int hp, int wp, float dmin, float interval, float half_range,
                      float full_range, float *depth_out, float *conf_out, char kernel_name_out[64]) {
  return guarded([&] {
    using namespace dr;
    if (!logits || !depth_out || !conf_out) fail(DR_ERR_ARG, "drm_debug_regress: null pointer");
    debug_check_planes("drm_debug_regress", D, h, w, prev, hp, wp);
    debug_device(device, "drm_debug_regress");
    const MvsSwitches sw;  // read from the environment, as the engine's
    DeviceArena arena;
    const size_t hw = (size_t)h * w;
    const float *d_logits = arena.upload(std::vector<float>(logits, logits + (size_t)D * hw));
    const RegressArgs r = debug_regress_args(arena, d_logits, D, h, w, prev, hp, wp, dmin, interval, half_range, full_range);
    launch_regress(r, sw, nullptr);
    DR_HIP(hipDeviceSynchronize());
    DR_HIP(hipGetLastError());
    DR_HIP(hipMemcpy(depth_out, r.depth, hw * 4, hipMemcpyDeviceToHost));
    DR_HIP(hipMemcpy(conf_out, r.conf, hw * 4, hipMemcpyDeviceToHost));
    if (kernel_name_out) debug_regress_name(kernel_name_out, 64, D, sw);
  });
}

int drm_debug_prob_regress(int device, const float *x11, const float *w_prob, int D, int h, int w, const float *prev, int hp, int wp, float dmin, float interval,
                           float half_range, float full_range, float *logits_out, float *depth_out, float *conf_out, char kernel_name_out[64]) {
  return guarded([&] {
    using namespace dr;
    if (!x11 || !w_prob || !logits_out || !depth_out || !conf_out) fail(DR_ERR_ARG, "drm_debug_prob_regress: null pointer");
    debug_check_planes("drm_debug_prob_regress", D, h, w, prev, hp, wp);
    debug_device(device, "drm_debug_prob_regress");
    const MvsSwitches sw;
    DeviceArena arena;
    const size_t hw = (size_t)h * w;
    ProbArgs p{};
    p.x = arena.upload(std::vector<float>(x11, x11 + (size_t)D * hw * 8));
    p.wt = arena.upload(prob_taps(std::vector<float>(w_prob, w_prob + 8 * 27)));
    p.out = debug_poison(arena, (size_t)D * hw);
    p.D = D; p.h = h; p.w = w;
    const RegressArgs r = debug_regress_args(arena, p.out, D, h, w, prev, hp, wp, dmin, interval, half_range, full_range);
    const int stage = 3;  // (choose_prob asks for a stage 1..3 and nothing else of it)
    const ProbChoice k = choose_prob(prob_shape(p), sw, stage);
    launch_prob(p, r, sw, stage, nullptr);
    if (!k.regresses()) launch_regress(r, sw, nullptr);
    DR_HIP(hipDeviceSynchronize());
    DR_HIP(hipGetLastError());
    DR_HIP(hipMemcpy(logits_out, p.out, (size_t)D * hw * 4, hipMemcpyDeviceToHost));
    DR_HIP(hipMemcpy(depth_out, r.depth, hw * 4, hipMemcpyDeviceToHost));
    DR_HIP(hipMemcpy(conf_out, r.conf, hw * 4, hipMemcpyDeviceToHost));
    if (kernel_name_out) {
      k.name(kernel_name_out, 64);
      if (!k.regresses()) {  // two launches: "k_prob2<1>+k_regress_r<8>"
        const size_t n = strlen(kernel_name_out);
        kernel_name_out[n] = '+';
        debug_regress_name(kernel_name_out + n + 1, 64 - n - 1, D, sw);
      }
    }
  });
}

int drm_debug_edge_filter(int device, const float *depth, const float *conf, int H, int W, const float *edge_in, unsigned rank, float *edge_out, float *depth_out,
                          float *conf_out, unsigned *thr_bits_out) {
  return guarded([&] {
    using namespace dr;
    if (!depth || !conf || !edge_out || !depth_out || !conf_out || !thr_bits_out) fail(DR_ERR_ARG, "drm_debug_edge_filter: null pointer");
    if (H <= 0 || W <= 0 || (long long)H * W > (1ll << 28)) fail(DR_ERR_ARG, "drm_debug_edge_filter: H, W must be positive, H W <= 2^28");
    const size_t n = (size_t)H * W;
    if (rank >= n) fail(DR_ERR_ARG, "drm_debug_edge_filter: rank %u of %zu values", rank, n);
    debug_device(device, "drm_debug_edge_filter");
    const MvsSwitches sw;
    DeviceArena arena;
    FilterArgs f{};
    f.depth3 = arena.upload(std::vector<float>(depth, depth + n));
    f.conf3 = arena.upload(std::vector<float>(conf, conf + n));
    f.edge = debug_poison(arena, n);
    f.depth = debug_poison(arena, n);
    f.conf = debug_poison(arena, n);
    f.state = arena.upload(std::vector<unsigned>(16, 0u));        // as the engine's: four 4-word slots, zero
    f.hist = arena.upload(std::vector<unsigned>(3 * 2048, 0u));   // one zeroed histogram per level
    f.n = (int)n; f.H = H; f.W = W;
    f.hist_blocks = sw.hist_blocks; f.fused = sw.filter_fused;
    // the EDGE, HIST x 3, (SCAN x 3,) APPLY sequence of MvsEngine::configure
    launch_edge(f, rank, nullptr);
    if (edge_in) DR_HIP(hipMemcpyAsync(f.edge, edge_in, n * 4, hipMemcpyHostToDevice, nullptr));  // in stream order: behind the edge kernel, before level 0
    for (int i = 0; i < 3; ++i) {
      launch_hist(f, i, i ? kSelectShift[i - 1] : 0, i ? kSelectBits[i - 1] : 0, kSelectShift[i], kSelectBits[i], nullptr);
      if (!f.fused) launch_scan(f, kSelectShift[i], kSelectBits[i], nullptr);
    }
    launch_apply(f, kSelectShift[2], kSelectBits[2], nullptr);
    DR_HIP(hipDeviceSynchronize());
    DR_HIP(hipGetLastError());
    DR_HIP(hipMemcpy(edge_out, f.edge, n * 4, hipMemcpyDeviceToHost));
    DR_HIP(hipMemcpy(depth_out, f.depth, n * 4, hipMemcpyDeviceToHost));
    DR_HIP(hipMemcpy(conf_out, f.conf, n * 4, hipMemcpyDeviceToHost));
    // the threshold: word [3] of the select's state -- of the last slot in the fused form (one slot per level, mvs_kernels.h), of the only slot otherwise
    DR_HIP(hipMemcpy(thr_bits_out, f.state + (f.fused ? 3 * 4 + 3 : 3), 4, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
