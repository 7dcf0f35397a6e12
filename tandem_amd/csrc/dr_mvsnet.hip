// dr_mvsnet.hip -- MI355X engine behind the DrMvsnet operator API (C ABI: include/dr_mi355x.h).
//
// Replaces tandem/libdr/dr_mvsnet/src/dr_mvsnet.cpp (libtorch TorchScript interpreter + cuDNN)
// with a fixed launch plan of hand-written gfx950 kernels (conv_mfma.h, mvs_kernels.h; launchers: mvs_launch.h; host logic: mvs_host.h; the plan: mvs_plan.h):
//   CallAsync   dr_mvsnet.cpp:125-283  -> MvsEngine::stage_inputs (WindowStager, mvs_stage.h) + worker thread
//   forward     dr_mvsnet.cpp:285-331  -> MvsEngine::forward (cva_mvsnet.py:98-184 as ~75 launches; what each op gets: ForwardCursor, mvs_engine_host.h)
//   GetResult   dr_mvsnet.cpp:95-107   -> drm_get_result (ResultSlots, mvs_engine_host.h)
// The key-frame feature cache is FeatureCacheDev (mvs_cache.h), the view shard and its RCCL binding ViewShard (mvs_shard.h).
// The threading contract is the reference's: one worker thread, one mutex, two condition variables;
// CallAsync blocks only while the previous input is still unprocessed.
#include <memory>

#include "mvs_stage.h"  // WindowStager; through it mvs_cache.h, mvs_engine_host.h and mvs_plan.h (the kernels and their launchers, MvsPlan, HipOwner)
#include "mvs_shard.h"

namespace dr {

std::string &last_error_slot() {
  thread_local std::string s;
  return s;
}

// An instance no plan asks for (DR_CONV_A_INSTANCES: its tiles are PT = 2's at half the work per wave) but one the library has always carried: instantiated
// here so that the library's set of kernels does not depend on how launch_conv's dispatcher is written.
template __global__ void k_conv_a<4, 1, 1>(const ConvArgs a);

// ------------------------------------------------------------------ engine
static const char *conv_kind_name(const ConvLaunch &c) { return conv_family_name(conv_family(c)); }

class MvsEngine {
 public:
  MvsEngine(const char *path, int device) : device_(device), blob_(load_blob(path)) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device) fail(DR_ERR_DEVICE, "DrMvsnet: no HIP device %d (found %d) -- the MI355X path has no CPU fallback", device, n);
    DR_HIP(hipSetDevice(device_));
    stream_ = own_.stream_plain();
    // Both streams are created HERE, whether the side stream will be used or not: the runtime (ROCm 7.2, four hardware queues by default) gives a new stream the
    // least-shared queue, and with two streams per engine the main streams of four engines land on four different queues (tools/ubench/stream_queues.hip shows
    // the mapping; one stream per engine puts the fourth engine on the third one's queue: 535 instead of 580 depth maps/s, profiles/r06_queues_side_stream.txt).
    side_ = own_.stream_plain();
    for (auto *e : {&ev_fork_, &ev_feat2_, &ev_feat3_}) *e = own_.event();
    std::vector<float> lut(256);
    for (int i = 0; i < 256; ++i) lut[i] = (float)((double)(float)i / 255.0);
    lut_ = consts_.upload(lut);
    march_err_ = own_.pinned<int>(1);  // pinned, device-visible: k_conv_m raises it when a ring wait gives up
    *march_err_ = 0;
    worker_ = std::thread(&MvsEngine::loop, this);
  }
  ~MvsEngine() {
    {
      std::unique_lock<std::mutex> lk(mu_);
      done_cv_.wait(lk, [&] { return !slots_.unprocessed(); });
      running_ = false;
      input_cv_.notify_all();
    }
    worker_.join();
    (void)hipSetDevice(device_);
    (void)hipStreamSynchronize(stream_);
    shard_.comm_destroy();
  }

  // --- reference-API surface -------------------------------------------------------------------
  void call_async(int H, int W, int V, int ref, const uint8_t *const *bgrs, const float *K9, const float *const *c2ws,
                  float dmin, float dmax, float disc) {
    check_args(H, W, V, ref, bgrs, K9, c2ws);
    std::unique_lock<std::mutex> lk(mu_);  // held by the worker for the whole forward (dr_mvsnet.cpp:84-92)
    done_cv_.wait(lk, [&] { return !slots_.unprocessed(); });
    stage_inputs(H, W, V, ref, bgrs, K9, c2ws, dmin, dmax, disc, true);
    slots_.submit();
    input_cv_.notify_all();
  }
  bool ready() { return !slots_.unprocessed(); }
  void wait() {
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return !slots_.unprocessed(); });
    slots_.rethrow();
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
    done_cv_.wait(lk, [&] { return !slots_.unprocessed(); });
    if (capacity == cache_.capacity()) return;
    cache_.set_capacity(capacity);
    if (H_) {  // a configured engine is re-planned: the entries are sized for the window shape
      DR_HIP(hipSetDevice(device_));
      replan(H_, W_, V_);
    }
  }
  void feature_cache_stats(uint64_t out[6]) {
    std::unique_lock<std::mutex> lk(mu_);
    cache_.stats(out);
  }

  // --- device-resident hooks -------------------------------------------------------------------
  void upload(int H, int W, int V, int ref, const uint8_t *const *bgrs, const float *K9, const float *const *c2ws,
              float dmin, float dmax, float disc) {
    check_args(H, W, V, ref, bgrs, K9, c2ws);
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return !slots_.unprocessed(); });
    stage_inputs(H, W, V, ref, bgrs, K9, c2ws, dmin, dmax, disc);
    DR_HIP(hipStreamSynchronize(stream_));
  }
  void forward_n(int iters, float *ms) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    DR_HIP(hipSetDevice(device_));
    WindowTicket windows(device_);  // (several engines driven through this hook at once count as windows in flight, like CallAsync's)
    HipOwner timing;  // (two events: gone with the scope on every way out of it)
    const hipEvent_t e0 = timing.event(hipEventDefault), e1 = timing.event(hipEventDefault);
    DR_HIP(hipEventRecord(e0, stream_));
    for (int i = 0; i < iters; ++i) forward(nullptr);
    DR_HIP(hipEventRecord(e1, stream_));
    DR_HIP(hipStreamSynchronize(stream_));
    float t = 0;
    DR_HIP(hipEventElapsedTime(&t, e0, e1));
    cache_.mismatch_recovered([&] { forward(nullptr); });
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
    if (shard_.collective()) fail(DR_ERR_PROTOCOL, "autotune(): not on a view-sharded engine (tune the unsharded plan)");
    DR_HIP(hipSetDevice(device_));
    HipOwner timing;
    const hipEvent_t e0 = timing.event(hipEventDefault), e1 = timing.event(hipEventDefault);
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
    for (Op &o : plan_->ops) {
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
    DR_HIP(hipStreamSynchronize(stream_));
    check_march();
    if (before_ms) *before_ms = (float)t_before;
    if (after_ms) *after_ms = (float)t_after;
    cache_.follow_tuned_plan();
  }

  // ---- view sharding hooks (SURVEY 8e / BASELINE configs[2]; no reference counterpart) ----
  // Phase p = 0..3 of the uploaded window: [.. cost volume 1] [regularise 1 .. cost volume 2] [.. cost volume 3]
  // [regularise 3 .. edge filter].  Between phases the host sum-reduces "volume<p+1>" over the ranks.
  void set_view_shard(int nsrc_total) {
    std::unique_lock<std::mutex> lk(mu_);
    shard_.set_nsrc(nsrc_total);
  }
  // the communicator of the view-shard collective inside the engine (ViewShard, mvs_shard.h)
  void comm_init(int rank, int world, const void *unique_id) {
    std::unique_lock<std::mutex> lk(mu_);
    shard_.comm_init(device_, rank, world, unique_id);
  }
  int comm_count() {
    std::unique_lock<std::mutex> lk(mu_);
    return shard_.comm_count();
  }
  void comm_destroy() {
    std::unique_lock<std::mutex> lk(mu_);
    if (!shard_.has_comm()) return;
    (void)hipSetDevice(device_);
    (void)hipStreamSynchronize(stream_);
    shard_.comm_destroy();
  }
  void forward_phase(int phase) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    if (phase < 0 || phase > 3) fail(DR_ERR_ARG, "forward_phase: phase must be 0..3");
    DR_HIP(hipSetDevice(device_));
    const std::vector<Op> &ops = plan_->ops;
    std::vector<size_t> cut{0};
    for (size_t i = 0; i < ops.size(); ++i) if (ops[i].kind == Op::COSTVOL) cut.push_back(i + 1);
    cut.push_back(ops.size());
    {
      FlagScope phase_mode(shard_.phase_flag());  // the caller reduces between phases
      forward(nullptr, cut[phase], cut[phase + 1]);
    }
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
    if (shard_.collective()) fail(DR_ERR_PROTOCOL, "profile(): a view-sharded engine enqueues collectives -- every rank would have to profile in lockstep");
    DR_HIP(hipSetDevice(device_));
    forward(nullptr);  // warm
    const std::vector<Op> &ops = plan_->ops;
    HipOwner timing;
    std::vector<hipEvent_t> ev(ops.size() + 1);
    for (auto &e : ev) e = timing.event(hipEventDefault);
    forward(&ev);
    DR_HIP(hipStreamSynchronize(stream_));
    check_march();
    names.clear(); ms.clear();
    for (size_t i = 0; i < ops.size(); ++i) {
      float t = 0;
      DR_HIP(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
      ms.push_back(t);
      const Op &o = ops[i];
      char kn[64], line[256];
      op_kernel_name(o, *plan_, win_, sw_, kn, sizeof kn);
      snprintf(line, sizeof line, "%s\t%s\t%.6e\t%.6e\n", o.name.c_str(), kn, o.flops, o.bytes);
      names += line;
    }
  }
  void work(double *flops, double *bytes) {
    std::unique_lock<std::mutex> lk(mu_);
    require_config();
    double f = 0, b = 0;
    for (auto &o : plan_->ops) { f += o.flops; b += o.bytes; }
    if (flops) *flops = f;
    if (bytes) *bytes = b;
  }

 private:
  // ---------------------------------------------------------------- plumbing
  void check_args(int H, int W, int V, int ref, const uint8_t *const *bgrs, const float *K9, const float *const *c2ws) {
    if (!bgrs || !K9 || !c2ws) fail(DR_ERR_ARG, "CallAsync: null pointer argument");
    const int vmin = shard_.nsrc() ? 1 : 2;  // a view-shard rank may hold the reference view only
    if (V < vmin || V > kMaxSrc + 1) fail(DR_ERR_ARG, "CallAsync: view_num=%d unsupported (%d..%d)", V, vmin, kMaxSrc + 1);
    if (ref < 0 || ref >= V) fail(DR_ERR_ARG, "CallAsync: ref_index=%d out of range", ref);
    if (H <= 0 || W <= 0 || H % 32 || W % 32) fail(DR_ERR_ARG, "CallAsync: height/width must be positive multiples of 32 (got %dx%d)", H, W);
    for (int i = 0; i < V - 1; ++i) for (int j = i + 1; j < V; ++j)
      if (bgrs[i] == bgrs[j] || c2ws[i] == c2ws[j])
        fail(DR_ERR_ARG, "ERROR: In Call Async passing the same data for index %d and %d", i, j);  // dr_mvsnet.cpp:153-160
  }
  void require_config() { if (!H_) fail(DR_ERR_PROTOCOL, "no window uploaded yet"); }
  // GetResult's first half: waits for the window, rethrows what its worker threw and hands the pinned block of four maps out ONCE
  const float *take_result(std::unique_lock<std::mutex> &lk) {
    done_cv_.wait(lk, [&] { return !slots_.unprocessed(); });
    return plan_->h_out[slots_.take()];
  }
  void loop() {  // dr_mvsnet.cpp:83-93
    std::unique_lock<std::mutex> lk(mu_);
    while (running_) {
      if (slots_.unprocessed()) {
        try {
          const bool prelaunched = (bool)parked_;  // (CallAsync enqueued this window's forward itself: stage_inputs)
          WindowTicket window = WindowTicket::take(parked_, device_);  // (counted from here, or from CallAsync's own launch, to the end of this block)
          DR_HIP(hipSetDevice(device_));
          if (!prelaunched) forward(nullptr);
          const int blk = slots_.next_block();
          publish(blk);
          if (cache_.mismatch_recovered([&] { forward(nullptr); })) publish(blk);  // a cache hit that was a key collision: the window ran again without the cache; publish THAT result
          check_march();
          slots_.done(blk);
        } catch (const std::exception &e) { slots_.failed(e.what()); }
        done_cv_.notify_all();
      }
      input_cv_.wait(lk, [&] { return slots_.unprocessed() || !running_; });
    }
  }

  // the four result maps into pinned block `blk`, and the wait for them
  void publish(int blk) {
    const size_t n = (size_t)H_ * W_ * 4;
    launch_publish4(plan_->filt.depth, plan_->filt.conf, plan_->filt.depth3, plan_->filt.conf3, plan_->h_out_dev[blk], n / 16, stream_);
    DR_HIP(hipStreamSynchronize(stream_));
  }

  DevTensor &T(const std::string &name) { return plan_->T(name); }  // (callers have a plan: require_config, or they run inside a forward)

  // (Re)builds the whole plan for a new window shape: the old one goes first (two plans never exist side by side), and the engine keeps
  // H_ = W_ = V_ = 0 ("not configured") and no plan until the new one is complete.  If the builder throws (out of memory, unsupported
  // depth_num, missing tensor) what it had allocated is gone with it, and the next call starts from scratch instead of running a half-built plan.
  void configure(int H, int W, int V) {
    if (H == H_ && W == W_ && V == V_) return;
    replan(H, W, V);
  }
  // ... and for the shape the engine has, when what the plan is built from changed (the feature cache's capacity)
  void replan(int H, int W, int V) {
    DR_HIP(hipStreamSynchronize(stream_));
    plan_.reset();
    cache_.release();
    H_ = W_ = V_ = 0;
    slots_.drop();  // (the result blocks were the old plan's)
    memset(win_.cv, 0, sizeof win_.cv);
    memset(win_.rg, 0, sizeof win_.rg);
    std::unique_ptr<MvsPlan> plan = MvsPlanBuilder{blob_, sw_, device_, lut_, march_err_, H, W, V, shard_.nsrc(), cache_.capacity()}.build();
    cache_.attach(*plan);
    plan_ = std::move(plan);
    H_ = H; W_ = W; V_ = V;
  }

  // Takes the window to the device in model order [ref, others] and derives every per-call kernel parameter (WindowStager); decides what
  // the feature cache answers.  A window that CallAsync may enqueue itself (the cache answers it) leaves its ticket parked for the worker.  Caller holds mu_.
  void stage_inputs(int H, int W, int V, int ref, const uint8_t *const *bgrs, const float *K9, const float *const *c2ws,
                    float dmin, float dmax, float disc, bool may_prelaunch = false) {
    DR_HIP(hipSetDevice(device_));
    configure(H, W, V);
    const WindowGeometry geo = plan_geometry(H, W, V, ref, K9, c2ws, dmin, dmax, disc, blob_, shard_.nsrc());  // cameras, plane ranges, filter rank (mvs_host.h)
    stager_.begin(H, W, V, bgrs, geo.order);
    stager_.fill_args(H, W, V, geo, blob_);
    cache_.to_batch_path();
    if (cache_.capacity() > 0) cache_.plan_use(H, W, V, bgrs, geo.order, shard_.excludes_cache());
    win_.filter_rank = geo.filter_rank;
    if (may_prelaunch && cache_.can_prelaunch()) parked_ = stager_.prelaunch(cache_, [&] { forward(nullptr); });
    else stager_.upload_all();
  }

  // Enqueue one complete forward on stream_ (or the ops [first, last) of it).  ev (optional): plan_->ops.size()+1 events
  // for per-op timing.  What each op gets -- its stream, the fork's events, the view shard's collectives -- is ForwardCursor's answer
  // (mvs_engine_host.h); this is the loop that executes it.
  //
  // A whole forward (no per-op events, no range) forks: the FeatureNet heads that only stages 2 and 3 need
  // (fn.skip2, fn.out2, fn.skip3, fn.out3 -- 0.5 ms at 640x480) run on a side stream under stage 1's cost volume and
  // regularisation, whose coarse UNet levels leave most CUs idle; stage 2 / 3's cost volume waits for feat2 / feat3.
  // The next forward's main-stream work is ordered after those waits, so the side stream never runs ahead of a reader.
  void forward(std::vector<hipEvent_t> *ev, size_t first = 0, size_t last = ~(size_t)0) {
    const ForwardRange range{first, last, plan_->ops.size()};
    if ((cache_.fast() || cache_.fill()) && !range.whole()) cache_.to_batch_path();  // a partial forward (phases, one op) cannot skip FeatureNet
    const bool cached = cache_.fast();  // FeatureNet answered by the feature cache: its ops are skipped
    // ... unless other engines of this process have windows in flight on the device: their kernels already fill the idle CUs, and a second stream per
    // engine only adds queue contention (4 engines: 580 depth maps/s without the fork against 570 with it, profiles/r06_queues_side_stream.txt; alone: 2.150 ms
    // with it against 2.165).  Same kernels in the same per-stream order either way: the result does not depend on it.
    const bool alone = windows_in_flight(device_).load(std::memory_order_relaxed) <= 1;
    ForwardCursor cursor({range, ev != nullptr, alone, sw_.side_stream, cached, plan_->fork_lo, plan_->fork_hi, plan_->feat2_op,
                          shard_.form(sw_), shard_.rank(), shard_.phase_mode(),
                          {win_.cv[0].V - 1 > 0, win_.cv[1].V - 1 > 0, win_.cv[2].V - 1 > 0}});
    if (cached) cache_.forward_cached_features();
    size_t i = 0;
    for (const Op &o : plan_->ops) {
      if (ev) DR_HIP(hipEventRecord((*ev)[i], stream_));
      const ForwardCursor::Step s = cursor.at(i++, o.kind == Op::COSTVOL, o.kind == Op::REGRESS, o.stage);
      if (s.skip) continue;
      if (s.open_fork) { DR_HIP(hipEventRecord(ev_fork_, stream_)); DR_HIP(hipStreamWaitEvent(side_, ev_fork_, 0)); }
      if (s.wait_feat2) DR_HIP(hipStreamWaitEvent(stream_, ev_feat2_, 0));
      if (s.wait_feat3) DR_HIP(hipStreamWaitEvent(stream_, ev_feat3_, 0));
      const hipStream_t st = s.side ? side_ : stream_;
      // a view-shard rank that holds the reference view only: its partial volume is the empty sum (the kernels return without storing)
      if (s.zero_volume) { const DevTensor &vol = T("volume" + std::to_string(o.stage)); DR_HIP(hipMemsetAsync(vol.d, 0, vol.n() * 4, st)); }
      if (s.launch) launch_op(o, *plan_, win_, sw_, st);
      // view shard: sum the partial volumes of all ranks, in place, in stream order
      if (s.reduce) shard_.reduce(T("volume" + std::to_string(o.stage)), st);
      if (s.all_reduce) shard_.all_reduce(T("volume" + std::to_string(o.stage)), st);
      // the stage's depth map goes back to every rank: stage s + 1 centres its hypotheses on it; stage 3's depth and
      // confidence are the result (the edge filter then runs on every rank: 0.08 ms)
      if (s.broadcast_depth) shard_.broadcast(T("depth" + std::to_string(o.stage)), st);
      if (s.broadcast_conf3) shard_.broadcast(T("conf3"), st);
      // the side stream's results are published after whichever op ends them (fn.out2; the LAST op of the fork range: a
      // convolution in the fused-skip form, the border kernel in the folded form) -- independent of the op kind
      if (s.record_feat2) DR_HIP(hipEventRecord(ev_feat2_, side_));
      if (s.record_feat3) DR_HIP(hipEventRecord(ev_feat3_, side_));
    }
    if (cache_.fill() && cursor.whole()) cache_.fill_from_batch();
    if (ev) DR_HIP(hipEventRecord((*ev)[i], stream_));
    DR_HIP(hipGetLastError());
  }

  const MvsSwitches sw_;  // read once, here
  int device_;
  Blob blob_;
  // (declared in the order that lets go backwards: the plan's buffers first, then the constants, then own_'s pinned words, events and streams)
  HipOwner own_;
  hipStream_t stream_ = nullptr, side_ = nullptr;
  hipEvent_t ev_fork_ = nullptr, ev_feat2_ = nullptr, ev_feat3_ = nullptr;
  int *march_err_ = nullptr;
  DeviceArena consts_;
  const float *lut_ = nullptr;
  std::unique_ptr<MvsPlan> plan_;  // of the window shape H_ x W_ x V_ (mvs_plan.h); null while the engine is not configured
  WindowArgs win_{};               // of the staged window (stage_inputs)
  // called after a stream synchronise: a marching convolution that gave up a wait leaves garbage behind -- report it, never return it
  void check_march() {
    if (march_err_ && *march_err_) { const int c = *march_err_; *march_err_ = 0; fail(DR_ERR_DEVICE, "k_conv_m: a ring wait gave up (code %d): the LDS producer/consumer protocol stalled", c); }
  }
  int H_ = 0, W_ = 0, V_ = 0;
  // the parts: what they take from the runtime is own_'s, so they hold nothing that outlives the members above
  const MvsCore core_{sw_, device_, own_, stream_, plan_, win_, H_, W_, V_};
  FeatureCacheDev cache_{core_};  // the key-frame feature cache (the single-view plan and the entries' buffers are the plan's)
  ViewShard shard_;               // source-view total, communicator, collectives, phase mode
  WindowTicket parked_;           // of a window whose forward CallAsync enqueued itself (the worker only publishes)

  std::thread worker_;
  HostCopier copier_;
  WindowStager stager_{core_, copier_};
  std::mutex mu_;
  std::condition_variable input_cv_, done_cv_;
  bool running_ = true;
  ResultSlots slots_;  // unprocessed / has output / which result block / the worker's error
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
    // the EDGE, HIST x 3, (SCAN x 3,) APPLY sequence of the plan (mvs_plan.h)
    launch_edge(f, rank, nullptr);
    if (edge_in) DR_HIP(hipMemcpyAsync(f.edge, edge_in, n * 4, hipMemcpyHostToDevice, nullptr));  // in stream order: behind the edge kernel, before level 0
    for (int i = 0; i < 3; ++i) {
      launch_hist(f, i, nullptr);
      if (!f.fused) launch_scan(f, i, nullptr);
    }
    launch_apply(f, nullptr);
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
