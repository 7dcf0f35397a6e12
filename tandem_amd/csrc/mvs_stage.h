// mvs_stage.h -- staging one window of the DrMvsnet engine (included by dr_mvsnet.hip): WindowStager takes the caller's images to the device, in
// model order [ref, others] (dr_mvsnet.cpp:190-197), and derives every per-call kernel parameter (WindowArgs) from the window's geometry.
#pragma once
#include "mvs_cache.h"

namespace dr {

class WindowStager {
 public:
  WindowStager(const MvsCore &c, HostCopier &copier) : c_(c), copier_(copier) {}

  // The window whose images the calls below move.  Images that already live in page-locked memory (drm_host_alloc, hipHostMalloc,
  // hipHostRegister) go to the device straight from where they are -- no gather into the pinned block, which is the 0.3-0.4 ms memcpy on the
  // operator boundary's critical path; the call still returns only when the copies have completed ("inputs are copied before return": the
  // caller may reuse its buffers).  An image that starts inside a hipHostRegister'ed range and runs past its end takes the staging path (span_holds).
  void begin(int H, int W, int V, const uint8_t *const *bgrs, const int *order) {
    bgrs_ = bgrs; V_ = V;
    memcpy(order_, order, sizeof order_);
    img_bytes_ = (size_t)H * W * 3;
    pinned_ = true;
    for (int v = 0; v < V && pinned_; ++v) {
      hipPointerAttribute_t at;
      hipDeviceptr_t base = nullptr;
      size_t span = 0;
      if (hipPointerGetAttributes(&at, bgrs[v]) != hipSuccess || at.type != hipMemoryTypeHost || !at.devicePointer ||
          hipMemGetAddressRange(&base, &span, (hipDeviceptr_t)at.devicePointer) != hipSuccess) {
        (void)hipGetLastError();
        pinned_ = false;
      } else pinned_ = span_holds((uintptr_t)base, span, (uintptr_t)at.devicePointer, img_bytes_);
    }
  }

  // every per-call kernel parameter of the three stages, from the cameras and plane ranges (mvs_host.h plan_geometry) and the plan's tensors
  void fill_args(int H, int W, int V, const WindowGeometry &geo, const Blob &blob) {
    MvsPlan &plan = *c_.plan;
    for (int s = 1; s <= 3; ++s) {
      const StageGeometry &g = geo.stage[s - 1];
      const int sc = 1 << (3 - s), h = H / sc, w = W / sc, D = g.D, C = 32 >> (s - 1);
      const std::string S = std::to_string(s);
      const DevTensor &feat = plan.T("feat" + S), &vol = plan.T("volume" + S);
      CostVolArgs &a = c_.win.cv[s - 1];
      memset(&a, 0, sizeof a);
      a.feat = feat.d; a.fpad = feat.pad;
      a.vol = vol.d; a.split = vol.split;
      a.V = V; a.h = h; a.w = w;
      a.view_aggregation = blob.view_aggregation;
      a.dchunk = costvol_dchunk(s, D, a.view_aggregation, a.fpad, c_.sw);
      a.nsrc_f = g.nsrc_f;
      memcpy(a.M, g.M, sizeof a.M);
      PlaneArgs &p = a.planes;
      p.D = D; p.dmin = g.dmin; p.interval = g.interval;
      p.half_range = g.half_range; p.full_range = g.full_range;
      if (s > 1) { p.prev = plan.T("depth" + std::to_string(s - 1)).d; p.hp = h / 2; p.wp = w / 2; }
      if (blob.view_aggregation) {
        const GateFold gf = fold_gate(blob, s, C);
        memcpy(a.gw, gf.gw, sizeof a.gw);
        a.gA1 = gf.gA1; a.gB1 = gf.gB1; a.gA2 = gf.gA2; a.gB2 = gf.gB2;
      }
      RegressArgs &r = c_.win.rg[s - 1];
      r.logits = plan.T("logits" + S).d;
      r.depth = plan.T("depth" + S).d;
      r.conf = plan.T("conf" + S).d;
      r.planes = p; r.h = h; r.w = w;
    }
  }

  // view by view: the copy engine moves view v to the device while the host gathers view v + 1 into the pinned block (one 6.45 MB
  // transfer behind seven memcpys cost their sum: 0.3 + 0.2 ms at 640 x 480 x 7 on the operator boundary's critical path)
  void upload_all() {
    if (!pinned_) {
      copier_.run([&] { upload_views(1); });  // the helper thread takes every other view
      try { upload_views(0); } catch (...) { copier_.wait_quiet(); throw; }  // (the job refers to this call's window)
      copier_.wait();
    } else {
      upload_views(1);
      upload_views(0);
      record_h2d();
      wait_h2d();
    }
  }

  // PRELAUNCH (CallAsync with the feature cache answering the window): the device needs ONE image -- the new one -- to start; the other six are only compared
  // with their cache entries, which can happen last.  So the new image goes up first, the helper thread stages and uploads the rest on a second stream, and
  // THIS thread enqueues the whole forward meanwhile; the comparison (k_cache_io) is enqueued behind it once the uploads are in flight.  The device starts
  // ~0.3 ms earlier in TandemBackend's loop (it idles while a window is staged); the call still returns only when every image has been copied.
  // Returns the window's ticket: it counts as in flight from its forward's enqueue on, and the worker that publishes it takes the count over.
  template <class Forward>
  WindowTicket prelaunch(FeatureCacheDev &cache, Forward forward) {
    const int miss = cache.miss();
    if (miss >= 0) {
      upload_view(miss, c_.stream);
      if (pinned_) record_h2d();  // (read in place from the caller's page-locked image: waited for before the call returns)
    }
    copier_.run([&, miss] {
      DR_HIP(hipSetDevice(c_.device));
      for (int v = 0; v < V_; ++v) if (v != miss) upload_view(v, cache.up_stream());
      DR_HIP(hipEventRecord(cache.ev_hits(), cache.up_stream()));
    });
    WindowTicket ticket(c_.device);
    try {
      FlagScope deferred(cache.defer_io());
      forward();
    } catch (...) { copier_.wait_quiet(); throw; }
    copier_.wait();
    DR_HIP(hipStreamWaitEvent(c_.stream, cache.ev_hits(), 0));
    cache.enqueue_io();
    if (pinned_) {  // uploaded in place from the caller's page-locked images: they must have been read before the call returns
      DR_HIP(hipEventSynchronize(cache.ev_hits()));
      if (miss >= 0) wait_h2d();
    }
    return ticket;
  }

 private:
  // view v (model order): gathered into the staging block (unless page-locked already), then the copy engine
  void upload_view(int v, hipStream_t st) {
    const uint8_t *src = bgrs_[order_[v]];
    uint8_t *h_in = c_.plan->h_in + v * img_bytes_;
    if (!pinned_) { memcpy(h_in, src, img_bytes_); src = h_in; }
    DR_HIP(hipMemcpyAsync(c_.plan->d_bgr + v * img_bytes_, src, img_bytes_, hipMemcpyHostToDevice, st));
  }
  void upload_views(int v0) {  // views v0, v0 + 2, ...
    DR_HIP(hipSetDevice(c_.device));
    for (int v = v0; v < V_; v += 2) upload_view(v, c_.stream);
  }
  // completion of what was uploaded on the engine's stream straight from the caller's page-locked images
  void record_h2d() {
    if (!ev_h2d_) ev_h2d_ = c_.own.event();
    DR_HIP(hipEventRecord(ev_h2d_, c_.stream));
  }
  void wait_h2d() { DR_HIP(hipEventSynchronize(ev_h2d_)); }

  const MvsCore c_;
  HostCopier &copier_;
  hipEvent_t ev_h2d_ = nullptr;
  // the window of the call in progress (begin)
  const uint8_t *const *bgrs_ = nullptr;
  int order_[kMaxSrc + 1] = {};
  int V_ = 0;
  size_t img_bytes_ = 0;
  bool pinned_ = false;
};

}  // namespace dr
