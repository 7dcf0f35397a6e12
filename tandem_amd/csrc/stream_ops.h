// stream_ops.h -- BlockStreamer: the streaming of voxel blocks between the device pool and the host store (DESIGN.md "Streaming voxel
// blocks"; the kernels: stream_kernels.h, the host rules: fusion_host.h).  It owns the host store and the reach balls, the eviction
// chain in flight, the pinned and device staging (allocated with the first drf_set_streaming(radius > 0) or region call) and the
// statistics; the engine lends it FusionCore.  Everything runs on the integration stream.  Included by dr_fusion.hip after fusion_core.h.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "fusion_core.h"
#include "fusion_host.h"

namespace dr {

class BlockStreamer {
 public:
  explicit BlockStreamer(FusionCore &core) : core_(core) {}
  // ---- what the rest of the engine asks ----
  bool on() const { return st_radius_ > 0.0f; }
  float radius() const { return st_radius_; }
  size_t host_capacity() const { return st_host_cap_; }  // of the host store, in blocks
  HostBlockStore &store() { return store_; }             // drf_load_map and drf_merge_map fill it, a failed load empties it
  const HostBlockStore &store() const { return store_; }
  bool eviction_pending() const { return ev_pending_; }  // an eviction chain awaits folding
  // every pending eviction folded into the host store, the device idle
  void settle() {
    DR_HIP(hipSetDevice(core_.device));
    DR_HIP(hipDeviceSynchronize());
    fold_evicted();
  }
  // n stored blocks as the staging kernels read them: their keys to kdst, their voxels (4096 bytes each, in the keys' order) to vdst
  void pack_stored(const unsigned long long *keys, size_t n, void *kdst, unsigned char *vdst) const {
    memcpy(kdst, keys, n * 8);
    for (size_t k = 0; k < n; ++k) memcpy(vdst + k * 4096, store_.get(keys[k]), 4096);
  }
  // Automatic mode, before k_allocate: fold the previous scan's evictions, bring back every stored block whose centre lies
  // within the radius of this scan's camera centre.  No launch and no wait when nothing comes in.
  void stream_before_scan(const float *pose16, float depth_bound) {
    DR_HIP(hipStreamSynchronize(core_.int_stream));
    fold_evicted();
    double p[3];
    camera_centre(pose16, p);
    std::vector<unsigned long long> in;
    store_.query_sphere(p, st_radius_, core_.o.voxel_size, in);
    double r = stream_reach(core_.o, depth_bound);
    if (!in.empty()) {
      DR_HIP(hipEventRecord(st_ev_[0], core_.int_stream));
      upload(in);
      DR_HIP(hipEventRecord(st_ev_[1], core_.int_stream));
      st_timed_ |= 1;
      r = std::max(r, (double)st_radius_);
    }
    reach_.add(p, r);
  }
  // After the scan: select resident blocks beyond radius + hysteresis, unless the host can tell that there are none -- every
  // block centre lies in one of the reach balls, so if none of them reaches beyond radius + hysteresis of p nothing is launched.
  void stream_after_scan(const float *pose16) {
    double p[3];
    camera_centre(pose16, p);
    const double lim = (double)st_radius_ + hysteresis();
    const int cap = (int)std::min((size_t)st_cap_, host_free());
    st_scan_done_ = true;
    if (reach_.farthest(p) <= lim || cap == 0) return;
    F3 pf; pf.x = (float)p[0]; pf.y = (float)p[1]; pf.z = (float)p[2];
    const float r2 = (float)(lim * lim);
    DR_HIP(hipEventRecord(st_ev_[2], core_.int_stream));
    launch_eviction(pf, r2, pf, pf, 0, cap);
    DR_HIP(hipEventRecord(st_ev_[3], core_.int_stream));
    st_timed_ |= 2;
    ev_auto_ = true;
    memcpy(ev_p_, p, sizeof p);
  }
  // A render of these poses reads the host store.  Blocks the last scan's eviction chain gathered are not in it yet: only a pose that
  // could reach one (render_needs_fold) waits for the scan and folds them first.  true: it waited.
  bool fold_if_reachable(const float *const *poses, int n) {
    if (!ev_pending_) return false;
    bool far = !ev_auto_;
    for (int i = 0; i < n && !far; ++i) far = render_needs_fold(core_.o, poses[i], ev_p_, (double)st_radius_);
    if (!far) return false;
    DR_HIP(hipEventSynchronize(core_.int_done));
    fold_evicted();
    return true;
  }
  // ---- the entry points, behind the engine's null-argument and call-order checks ----
  void set_streaming(float radius, size_t host_capacity_blocks) {
    if (!(radius >= 0.0f) || !std::isfinite(radius)) fail(DR_ERR_ARG, "drf_set_streaming: radius must be finite and >= 0 (got %g)", radius);
    const float rmin = streaming_min_radius(core_.o);
    if (radius > 0.0f && radius < rmin) fail(DR_ERR_ARG, "drf_set_streaming: radius %g is below drf_streaming_min_radius = %g", radius, rmin);
    settle();
    if (!store_.empty()) fail(DR_ERR_PROTOCOL, "drf_set_streaming: the host store holds %zu blocks; bring them back with drf_stream_in_region first", store_.size());
    if (radius > 0.0f) ensure_staging();
    st_radius_ = radius;
    st_host_cap_ = host_capacity_blocks ? host_capacity_blocks : (size_t)-1;
    reach_.reset();
    // blocks integrated before now are bounded by nothing the host knows: the first scan runs the selection pass
    const double origin[3] = {0.0, 0.0, 0.0};
    if (radius > 0.0f) reach_.push(origin, HUGE_VAL);
  }
  void stream_out_region(const float *lower, const float *upper) {
    settle();
    ensure_staging();
    F3 lo, hi, p{0.f, 0.f, 0.f};
    lo.x = lower[0]; lo.y = lower[1]; lo.z = lower[2]; hi.x = upper[0]; hi.y = upper[1]; hi.z = upper[2];
    // count first: a region that does not fit in the host store moves nothing
    launch_eviction(p, 0.0f, lo, hi, 1, 0);  // (cap = 0 gathers nothing: no chain is pending behind it)
    DR_HIP(hipStreamSynchronize(core_.int_stream));
    const size_t want = (size_t)sd_.h_out[1];
    if (want > host_free()) fail(DR_ERR_CAPACITY, "drf_stream_out_region: %zu blocks do not fit in the host store (%zu free)", want, host_free());
    for (;;) {
      launch_eviction(p, 0.0f, lo, hi, 1, st_cap_);
      DR_HIP(hipStreamSynchronize(core_.int_stream));
      const bool more = sd_.h_out[1] > sd_.h_out[0];
      fold_evicted();
      if (!more) break;
    }
  }
  void stream_in_region(const float *lower, const float *upper) {
    settle();
    std::vector<unsigned long long> keys;
    double bl[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, bh[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    store_.for_each([&](unsigned long long k, const uint8_t *) {
      int c[3]; unpack_key_host(k, c);
      for (int a = 0; a < 3; ++a) {
        const float org = blk_origin_host(c[a], core_.o.voxel_size);
        if (!(org >= lower[a] && org <= upper[a])) return;
      }
      keys.push_back(k);
      for (int a = 0; a < 3; ++a) { bl[a] = std::min(bl[a], blk_centre_host(c[a], core_.o.voxel_size)); bh[a] = std::max(bh[a], blk_centre_host(c[a], core_.o.voxel_size)); }
    });
    if (keys.empty()) return;
    upload(keys);  // checks the pool's free room before anything moves
    DR_HIP(hipStreamSynchronize(core_.int_stream));
    if (st_radius_ > 0.0f) {  // the ball around the uploaded centres bounds them for the selection skip
      double c[3], r = 0.0;
      for (int a = 0; a < 3; ++a) { c[a] = 0.5 * (bl[a] + bh[a]); r += (bh[a] - bl[a]) * (bh[a] - bl[a]); }
      reach_.push(c, 0.5 * std::sqrt(r) + core_.o.voxel_size);
    }
  }
  // out: resident blocks, blocks in the host store, blocks streamed out / in (totals), bytes moved, last scan's streaming time (us)
  void streaming_stats(uint64_t out[6]) {
    settle();
    out[0] = (uint64_t)core_.pool_blocks(); out[1] = store_.size(); out[2] = st_out_total_; out[3] = st_in_total_;
    out[4] = 4096 * (st_out_total_ + st_in_total_); out[5] = (uint64_t)std::llround(st_last_us_);
  }
  void export_host_blocks(int max_blocks, int32_t *coords, uint8_t *voxels, int *n) {
    if (max_blocks < 0 || (max_blocks > 0 && (!coords || !voxels))) fail(DR_ERR_ARG, "drf_export_host_blocks: bad argument");
    settle();
    int i = 0;
    store_.for_each([&](unsigned long long k, const uint8_t *v) {
      if (i >= max_blocks) return;
      unpack_key_host(k, coords + 3 * i);
      memcpy(voxels + (size_t)i * 4096, v, 4096);
      ++i;
    });
    if (n) *n = i;
  }

 private:
  size_t host_free() const { return st_host_cap_ - std::min(st_host_cap_, store_.size()); }
  void ensure_staging() {
    if (st_cap_) return;
    st_cap_ = std::min(core_.o.num_blocks, kStageBlocks);
    sd_.ctl = core_.own.device<int>(8);
    DR_HIP(hipMemset(sd_.ctl, 0, 32));
    sd_.list = core_.own.device<int>(st_cap_);
    sd_.mv_dst = core_.own.device<int>(st_cap_);
    sd_.mv_src = core_.own.device<int>(st_cap_);
    h_ev_keys_ = core_.own.pinned<unsigned long long>(st_cap_, &sd_.h_keys);
    h_ev_vox_ = (uint8_t *)core_.own.pinned<uint4>((size_t)st_cap_ * 256, &sd_.h_vox);
    sd_.h_out = core_.own.pinned<int>(4);
    memset(sd_.h_out, 0, 16);
    h_in_keys_ = core_.own.pinned<unsigned long long>(st_cap_, &hd_in_keys_);
    h_in_vox_ = core_.own.pinned<uint8_t>((size_t)st_cap_ * 4096, &hd_in_vox_);
    for (auto &e : st_ev_) e = core_.own.event(hipEventDefault);
  }
  // Enqueue the eviction chain on core_.int_stream behind every render stream's last ray-cast (blocks move).  box = 0: blocks whose
  // centre lies beyond sqrt(r2) of p; box = 1: blocks whose origin lies in [lo, hi].  cap = 0 only counts (sd_.h_out[1]).
  void launch_eviction(F3 p, float r2, F3 lo, F3 hi, int box, int cap) {
    core_.wait_casts();
    StreamDev s = sd_;
    s.cap = cap;
    const int g = 512;
    hipLaunchKernelGGL(k_ev_select, dim3(g), dim3(256), 0, core_.int_stream, core_.d, s, p, r2, lo, hi, box);
    if (cap > 0) {
      hipLaunchKernelGGL(k_ev_gather, dim3(g), dim3(256), 0, core_.int_stream, core_.d, s);
      hipLaunchKernelGGL(k_ev_pair, dim3(cdiv(cap, 256)), dim3(256), 0, core_.int_stream, core_.d, s);
      hipLaunchKernelGGL(k_ev_move, dim3(g), dim3(256), 0, core_.int_stream, core_.d, s);
      hipLaunchKernelGGL(k_ev_zero_tail, dim3(g), dim3(256), 0, core_.int_stream, core_.d, s);
      hipLaunchKernelGGL(k_ev_clear, dim3(1024), dim3(256), 0, core_.int_stream, core_.d, s, core_.d.cmask + 1u);
      hipLaunchKernelGGL(k_ev_reindex, dim3(g), dim3(256), 0, core_.int_stream, core_.d, s);
    }
    hipLaunchKernelGGL(k_ev_finish, dim3(1), dim3(64), 0, core_.int_stream, core_.d, s);
    DR_HIP(hipGetLastError());
    ev_pending_ = cap > 0;
  }
  // the blocks the last eviction chain gathered -> host store (core_.int_stream must be idle)
  void fold_evicted() {
    if (st_scan_done_) {  // device time of the last scan's stream-in and eviction launches (0 if it had none)
      float a = 0.f, b = 0.f;
      if (st_timed_ & 1) DR_HIP(hipEventElapsedTime(&a, st_ev_[0], st_ev_[1]));
      if (st_timed_ & 2) DR_HIP(hipEventElapsedTime(&b, st_ev_[2], st_ev_[3]));
      st_last_us_ = 1000.0 * (a + b);
      st_timed_ = 0;
      st_scan_done_ = false;
    }
    if (!ev_pending_) return;
    ev_pending_ = false;
    const int m = sd_.h_out[0];
    for (int i = 0; i < m; ++i) store_.put(h_ev_keys_[i], h_ev_vox_ + (size_t)i * 4096);
    st_out_total_ += (uint64_t)m;
    // the automatic pass took every block beyond radius + hysteresis: what is resident now lies within the largest distance it
    // saw among the blocks that stayed (plus a voxel for the fp32 distance) of its centre
    if (ev_auto_ && sd_.h_out[1] == m) {
      float kept2;
      memcpy(&kept2, &sd_.h_out[3], 4);
      const double r = std::min((double)st_radius_ + hysteresis(), std::sqrt((double)kept2) + core_.o.voxel_size);
      reach_.reset();
      reach_.push(ev_p_, r);
    }
    ev_auto_ = false;
  }
  // stored blocks -> the end of the pool (behind every render stream's last ray-cast).  DR_ERR_CAPACITY before anything moves
  // if they do not fit.
  void upload(const std::vector<unsigned long long> &keys) {
    ensure_staging();
    const int na = core_.pool_blocks();
    if ((size_t)na + keys.size() > (size_t)core_.o.num_blocks)
      fail(DR_ERR_CAPACITY, "stream-in of %zu blocks does not fit in the pool (%d of num_blocks=%d in use)", keys.size(), na, core_.o.num_blocks);
    core_.wait_casts();
    for (size_t b = 0; b < keys.size(); b += st_cap_) {
      if (b) DR_HIP(hipStreamSynchronize(core_.int_stream));  // the pinned upload is reused
      const int n = (int)std::min(keys.size() - b, (size_t)st_cap_);
      pack_stored(keys.data() + b, (size_t)n, h_in_keys_, h_in_vox_);
      for (int i = 0; i < n; ++i) store_.erase(keys[b + i]);
      hipLaunchKernelGGL(k_in_place, dim3(std::min(cdiv(n, 4), 1024)), dim3(256), 0, core_.int_stream, core_.d, hd_in_keys_, (const uint4 *)hd_in_vox_, n);
      hipLaunchKernelGGL(k_in_finish, dim3(1), dim3(64), 0, core_.int_stream, core_.d.n_alloc, n);
      DR_HIP(hipGetLastError());
    }
    st_in_total_ += keys.size();
  }
  double hysteresis() const { return (double)kBS * core_.o.voxel_size; }  // one block edge
  FusionCore &core_;
  // streaming state (staging allocated with the first drf_set_streaming / region call)
  float st_radius_ = 0.0f;                  // 0 = off
  size_t st_host_cap_ = (size_t)-1;         // host store capacity in blocks
  HostBlockStore store_;
  int st_cap_ = 0;                          // staging capacity in blocks (0 = not allocated)
  StreamDev sd_{};
  unsigned long long *h_ev_keys_ = nullptr, *h_in_keys_ = nullptr, *hd_in_keys_ = nullptr;
  uint8_t *h_ev_vox_ = nullptr, *h_in_vox_ = nullptr, *hd_in_vox_ = nullptr;
  hipEvent_t st_ev_[4] = {nullptr, nullptr, nullptr, nullptr};  // [0..1] stream-in, [2..3] eviction of the last scan
  int st_timed_ = 0;
  bool st_scan_done_ = false;
  double st_last_us_ = 0.0;
  bool ev_pending_ = false, ev_auto_ = false;  // an eviction chain awaits folding; it was the automatic one (centre ev_p_)
  double ev_p_[3] = {0.0, 0.0, 0.0};
  ReachBalls reach_;  // balls that hold every block centre of the map
  uint64_t st_out_total_ = 0, st_in_total_ = 0;
};

}  // namespace dr
