// mvs_cache.h -- the key-frame feature cache on the device (included by dr_mvsnet.hip; drm_set_feature_cache): FeatureCacheDev over the
// index (FeatureIndex, mvs_host.h) and the plan's single-view ops and entry buffers (mvs_plan.h).
//
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
#pragma once
#include "mvs_engine_host.h"
#include "mvs_plan.h"

namespace dr {

class FeatureCacheDev {
 public:
  explicit FeatureCacheDev(const MvsCore &c) : c_(c) {}

  int capacity() const { return cap_; }  // entries (0: off, the default)
  // a configured engine is then re-planned by its caller: the entries are sized for the window shape
  void set_capacity(int capacity) { cap_ = capacity; }
  // the plan goes: a new window shape evicts everything (the entries' buffers are the plan's)
  void release() { fc_.clear(); fn1_ok_ = false; fc_.fast = fc_.fill = false; }
  // the new plan has the cache's single-view plan: what it needs of the engine, with its first use
  void attach(const MvsPlan &plan) {
    if (plan.ops1.empty()) return;
    if (!flag_) { flag_ = c_.own.pinned<int>(1); *flag_ = 0; }
    if (!up_stream_) { up_stream_ = c_.own.stream_plain(); ev_hits_ = c_.own.event(); }
    fc_.resize(cap_);
    fn1_ok_ = true;
  }
  // after autotune: the single-view plan follows the batch plan's instances, or stands down
  void follow_tuned_plan() {
    if (fn1_ok_ && !c_.plan->match_fn1()) { fn1_ok_ = false; fc_.fast = false; }
  }
  void stats(uint64_t out[6]) const {
    out[0] = fc_.hits; out[1] = fc_.misses; out[2] = fc_.batch_windows; out[3] = fc_.collisions; out[4] = fn1_ok_ ? 1 : 0; out[5] = (uint64_t)fc_.size();
  }

  bool fast() const { return fc_.fast; }  // FeatureNet of the staged window is answered by the cache: at most one view, miss(), is computed
  bool fill() const { return fc_.fill; }  // the staged window runs as a batch whose outputs fill the entries
  int miss() const { return fc_.miss; }
  // the staged window's forward may be enqueued while its cached images are still on their way up (WindowStager::prelaunch)
  bool can_prelaunch() const { return fc_.fast && up_stream_; }
  hipStream_t up_stream() const { return up_stream_; }  // uploads of the images the cache answers
  hipEvent_t ev_hits() const { return ev_hits_; }
  bool &defer_io() { return defer_io_; }  // up (FlagScope): the forward's image comparison follows once the uploads are in flight

  // back to the batch path: the staged window computes every view and the plane sweep reads the batch's feature maps
  void to_batch_path() {
    fc_.fast = fc_.fill = false;
    for (int s = 0; s < 3; ++s) set_batch_vfeat(s);
  }
  // decides, for the window being staged, which views the cache answers (FeatureIndex::plan); the guards that need engine state are here
  void plan_use(int H, int W, int V, const uint8_t *const *bgrs, const int *order, bool sharded) {
    fc_.stand_down();
    if (!fn1_ok_ || sharded) return;  // (a view-shard rank computes its own views every time)
    for (int s = 1; s <= 3; ++s)
      if (choose_costvol(costvol_shape(c_.win.cv[s - 1]), c_.sw, s).family != CostVolChoice::V5) return;  // (only k_costvol5 reads the views by pointer)
    uint64_t keys[kMaxSrc + 1][2];
    for (int v = 0; v < V; ++v) image_key(bgrs[order[v]], (size_t)H * W * 3, H, W, keys[v]);
    fc_.plan(V, keys);
    // where the plane sweep finds each view
    for (int s = 0; s < 3; ++s)
      for (int v = 0; v < V; ++v)
        if (fc_.fast) c_.win.cv[s].vfeat[v] = c_.plan->fcache[fc_.slot[v]].feat[s];
  }
  // one launch: the hits compared with their entries' images, the new image filed in its entry
  void enqueue_io() {
    const size_t img_bytes = (size_t)c_.H * c_.W * 3;
    CacheIoArgs io{};
    for (int v = 0; v < c_.V; ++v) {
      io.img[v] = reinterpret_cast<const uint4 *>(c_.plan->d_bgr + v * img_bytes);
      io.entry[v] = reinterpret_cast<uint4 *>(c_.plan->fcache[fc_.slot[v]].bgr);
    }
    io.miss = fc_.miss; io.flag = flag_dev(); io.n16 = img_bytes / 16;
    launch_cache_io(io, c_.V, c_.stream);
  }
  // fast path of a forward: verify the hits, FeatureNet on the one uncached view, its outputs (and image) into the entry
  void forward_cached_features() {
    const size_t img_bytes = (size_t)c_.H * c_.W * 3;
    MvsPlan &plan = *c_.plan;
    if (!defer_io_) enqueue_io();
    if (fc_.miss >= 0) {
      const FcBuffers &e = plan.fcache[fc_.slot[fc_.miss]];
      for (const FnOut &p : plan.fn1_out) {
        Op &o = plan.ops1[p.op];
        (o.kind == Op::CONV ? o.conv.args.out : o.head3.out) = e.feat[p.stage] + p.offset;
      }
      // (the heads on the side stream, as the batch path runs them, were measured: device time 1.821 -> 1.825 ms, the sliding loop x 1.10 instead of x 1.12-1.15 --
      // two cross-stream waits cost what the overlap of three small launches wins; not kept)
      for (Op &o : plan.ops1) {
        if (o.kind == Op::FRONT) o.front.bgr = plan.d_bgr + fc_.miss * img_bytes;
        if (o.kind != Op::CONV && o.kind != Op::FRONT && o.kind != Op::HEAD3) fail(DR_ERR_UNSUPPORTED, "feature cache: op kind %d in the single-view plan", (int)o.kind);
        launch_op(o, plan, c_.win, c_.sw, c_.stream);
      }
      fc_.set_valid(fc_.slot[fc_.miss]);
    }
  }
  // batch path with the cache on: every view's features (and image) into its entry, behind the forward that produced them
  void fill_from_batch() {
    const size_t img_bytes = (size_t)c_.H * c_.W * 3;
    for (int v = 0; v < c_.V; ++v) {
      const FcBuffers &e = c_.plan->fcache[fc_.slot[v]];
      if (fc_.valid(fc_.slot[v])) continue;
      for (int s = 0; s < 3; ++s) {
        const DevTensor &t = c_.plan->T("feat" + std::to_string(s + 1));
        const size_t n1 = t.n() / t.D;
        DR_HIP(hipMemcpyAsync(e.feat[s], t.d + v * n1, n1 * 4, hipMemcpyDeviceToDevice, c_.stream));
      }
      DR_HIP(hipMemcpyAsync(e.bgr, c_.plan->d_bgr + v * img_bytes, img_bytes, hipMemcpyDeviceToDevice, c_.stream));
      fc_.set_valid(fc_.slot[v]);
    }
  }
  // after a stream synchronise: a hit that was not one (key collision).  The cache is dropped and the staged window runs again on the batch path.
  template <class Forward>
  bool mismatch_recovered(Forward forward) {
    if (!flag_ || !*flag_) return false;
    *flag_ = 0;
    ++fc_.collisions;
    fc_.invalidate_all();
    to_batch_path();
    forward();
    DR_HIP(hipStreamSynchronize(c_.stream));
    return true;
  }

 private:
  int *flag_dev() { int *d = nullptr; DR_HIP(hipHostGetDevicePointer((void **)&d, flag_, 0)); return d; }
  void set_batch_vfeat(int s) {
    const DevTensor &t = c_.plan->T("feat" + std::to_string(s + 1));
    for (int v = 0; v < c_.V && v <= kMaxSrc; ++v) c_.win.cv[s].vfeat[v] = t.d + (size_t)v * (t.n() / t.D);
  }

  const MvsCore c_;
  int cap_ = 0;
  FeatureIndex fc_;                  // which entry answers which view of the staged window; LRU; counters (mvs_host.h)
  bool fn1_ok_ = false;              // the single-view plan exists and matches the batch plan's instances
  int *flag_ = nullptr;              // page-locked: raised by k_cache_io
  hipStream_t up_stream_ = nullptr;
  hipEvent_t ev_hits_ = nullptr;
  bool defer_io_ = false;
};

}  // namespace dr
