// fusion_core.h -- what the DrFusion engine lends its components (stream_ops.h BlockStreamer, mesh_ops.h MeshExtractor), the way
// MapIo is lent the HipOwner: the owner of everything taken from the runtime, the device, the options, the volume as the kernels
// see it, the integration stream, and the render slots as far as a component needs them -- the events behind their last ray-casts.
// The engine (dr_fusion.hip) holds it as its first member, fills it in its constructor and keeps the render slots themselves.
// Included by dr_fusion.hip after map_ops.h.
#pragma once
#include <algorithm>
#include <vector>

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

  int pool_blocks() const {  // blocks in the pool; the count lives on the device
    int na = 0;
    DR_HIP(hipMemcpy(&na, d.n_alloc, 4, hipMemcpyDeviceToHost));
    return std::min(na, o.num_blocks);
  }
  // the integration stream goes on behind every render stream's last ray-cast (blocks move, are added or change)
  void wait_casts() const { for (hipEvent_t e : casts) DR_HIP(hipStreamWaitEvent(int_stream, e, 0)); }
};

}  // namespace dr
