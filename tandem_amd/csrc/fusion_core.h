// fusion_core.h -- what the DrFusion engine lends its components (stream_ops.h BlockStreamer, mesh_ops.h MeshExtractor, render_ops.h
// MapStage and MapRenderer, pose_ops.h FramePose, FrameLocator and FrameTracker, search_ops.h PoseScorer and PoseSearch), the way
// MapIo is lent the HipOwner: the owner of everything taken from the runtime, the device, the options, the volume as the kernels
// see it, the integration stream, the call order (engine_host.h CallOrder: the engine and the renderer advance it, the pose
// components only ask), the scan's pinned input pair with the upload through it, the device's error flags, and of the render
// slots the events behind their last ray-casts (MapRenderer fills them in).  The engine (dr_fusion.hip) holds it as its first
// member and fills it in its constructor.  Included by dr_fusion.hip after map_ops.h.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "fusion_host.h"
#include "hip_owner.h"

namespace dr {

constexpr int kStageBlocks = 8192;  // blocks per eviction chain / per stream-in launch (32 MiB of pinned staging each way)

struct FusionCore {
  FusionCore(const drf_options_t &o_, int device_) : device(device_), o(o_) {}
  HipOwner own;  // first: released after every other member, of the core and of the engine that holds the core first
  const int device;
  const drf_options_t o;
  FusionDev d{};
  size_t npix = 0;
  hipStream_t int_stream = nullptr;
  hipEvent_t int_done = nullptr;  // behind the last scan and the streaming around it
  std::vector<hipEvent_t> casts;  // per render slot: its ray-cast kernels finished (the volume may be written again)
  CallOrder order;
  // the scan's input pair: pinned on the host, and where IntegrateScanAsync puts it on the device
  unsigned char *d_bgr_in = nullptr, *h_bgr_in = nullptr;
  float *d_depth_in = nullptr, *h_depth_in = nullptr;

  int pool_blocks() const {  // blocks in the pool; the count lives on the device
    int na = 0;
    DR_HIP(hipMemcpy(&na, d.n_alloc, 4, hipMemcpyDeviceToHost));
    return std::min(na, o.num_blocks);
  }
  // the integration stream goes on behind every render stream's last ray-cast (blocks move, are added or change)
  void wait_casts() const { for (hipEvent_t e : casts) DR_HIP(hipStreamWaitEvent(int_stream, e, 0)); }
  // A host image pair, or a depth image alone (d_bgr null), through the scan's pinned input buffers to the device.  again: the
  // buffers carry this call's frame, which must have left them first.
  void upload_frame(const uint8_t *h_bgr, const float *h_depth, unsigned char *d_bgr, float *d_depth, bool again = false) const {
    if (again) DR_HIP(hipStreamSynchronize(int_stream));
    if (d_bgr) memcpy(h_bgr_in, h_bgr, npix * 3);
    memcpy(h_depth_in, h_depth, npix * 4);
    if (d_bgr) DR_HIP(hipMemcpyAsync(d_bgr, h_bgr_in, npix * 3, hipMemcpyHostToDevice, int_stream));
    DR_HIP(hipMemcpyAsync(d_depth, h_depth_in, npix * 4, hipMemcpyHostToDevice, int_stream));
  }
  void check_device_flags() const {  // what the kernels left beside n_alloc
    int f[4];
    DR_HIP(hipMemcpy(f, d.n_alloc, 16, hipMemcpyDeviceToHost));
    if (f[1] || f[2]) fail(DR_ERR_CAPACITY, "DrFusion: block pool exhausted (num_blocks=%d) or block coordinate out of range", o.num_blocks);
  }
};

}  // namespace dr
