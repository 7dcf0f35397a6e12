// mvs_shard.h -- the view shard of the DrMvsnet engine (included by dr_mvsnet.hip; SURVEY 8e / BASELINE configs[2], no reference counterpart): the
// RCCL binding and ViewShard -- the source-view total of a sharded window, the communicator and its collectives, the phase mode of the host-driven form.
#pragma once
#include <mutex>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is bound with dlopen when a communicator is asked for

#include "mvs_engine_host.h"
#include "mvs_plan.h"

namespace dr {

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

// The view-shard collective inside the engine: with a communicator set, every cost-volume launch of a sharded window
// is followed -- on the engine's stream, no host round trip -- by an in-place RCCL sum of that volume over the ranks, so
// drm_forward / CallAsync run the whole sharded depth map as one stream of work; FeatureNet's stage-2/3 heads on the side
// stream and the reduce of stage 1 overlap.  (The host-driven protocol of forward_phase stays as the test double: RCCL
// refuses two ranks on one device, gloo can emulate them.)
// Collective form of a sharded forward (MvsSwitches::shard_allreduce).  Default: the partial volumes are REDUCED to rank 0, which
// alone regularises and regresses the stage, and the stage's depth map (what the next stage's hypotheses hang on: 77 / 307 /
// 1229 KB) is BROADCAST back -- (n-1)/n x 354 MB over xGMI per depth map instead of the all-reduce's 2(n-1)/n, and no redundant
// CostRegNet on the other ranks.  DR_SHARD_ALLREDUCE=1: round 2's form (sum all-reduce, every rank
// regularises redundantly; no broadcast).
class ViewShard {
 public:
  ViewShard() = default;
  ViewShard(const ViewShard &) = delete;
  void operator=(const ViewShard &) = delete;

  int nsrc() const { return nsrc_; }  // > 0: view-shard rank, cost-volume divisor = source views of the whole window
  void set_nsrc(int nsrc_total) {
    if (nsrc_total < 0 || nsrc_total > kMaxSrc) fail(DR_ERR_ARG, "set_view_shard: %d source views unsupported (0..%d)", nsrc_total, kMaxSrc);
    nsrc_ = nsrc_total;
  }
  int rank() const { return rank_; }
  bool collective() const { return comm_ && nsrc_; }                        // forwards enqueue collectives (outside phase mode)
  bool excludes_cache() const { return nsrc_ || comm_ || phase_mode_; }     // a view-shard rank computes its own views every time
  bool phase_mode() const { return phase_mode_; }
  bool &phase_flag() { return phase_mode_; }  // up (FlagScope) for one forward_phase: the caller reduces between phases
  ForwardCursor::Collective form(const MvsSwitches &sw) const {
    return !collective() ? ForwardCursor::kNone : (sw.shard_allreduce ? ForwardCursor::kAllReduce : ForwardCursor::kRooted);
  }

  void comm_init(int device, int rank, int world, const void *unique_id) {
    if (comm_) fail(DR_ERR_PROTOCOL, "comm_init: a communicator is already set");
    if (!unique_id || rank < 0 || rank >= world) fail(DR_ERR_ARG, "comm_init: bad rank %d of %d", rank, world);
    Rccl &r = Rccl::get();
    DR_HIP(hipSetDevice(device));
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof id);
    r.check(r.CommInitRank(&comm_, world, id, rank), "ncclCommInitRank");
    rank_ = rank;
  }
  // ranks RCCL itself reports for the engine's communicator (ncclCommCount): what bench.py prints next to the sharded figure, so that a
  // driver record shows how many GPUs the collective really spanned.  0: no communicator; -1: the bound library has no ncclCommCount.
  int comm_count() {
    if (!comm_) return 0;
    Rccl &r = Rccl::get();
    if (!r.CommCount) return -1;
    int n = 0;
    r.check(r.CommCount(comm_, &n), "ncclCommCount");
    return n;
  }
  bool has_comm() const { return comm_ != nullptr; }
  // the caller has waited for the stream the collectives were enqueued on
  void comm_destroy() {
    if (comm_) { Rccl::get().CommDestroy(comm_); comm_ = nullptr; }
  }

  // in place, in stream order
  void reduce(const DevTensor &t, hipStream_t st) {
    Rccl &r = Rccl::get();
    r.check(r.Reduce(t.d, t.d, t.n(), ncclFloat, ncclSum, 0, comm_, st), "ncclReduce");
  }
  void all_reduce(const DevTensor &t, hipStream_t st) {
    Rccl &r = Rccl::get();
    r.check(r.AllReduce(t.d, t.d, t.n(), ncclFloat, ncclSum, comm_, st), "ncclAllReduce");
  }
  void broadcast(const DevTensor &t, hipStream_t st) {
    Rccl &r = Rccl::get();
    r.check(r.Broadcast(t.d, t.d, t.n(), ncclFloat, 0, comm_, st), "ncclBroadcast");
  }

 private:
  int nsrc_ = 0;
  ncclComm_t comm_ = nullptr;  // view-shard communicator (drm_comm_init); the volumes are reduced in stream order when set
  int rank_ = 0;
  bool phase_mode_ = false;
};

}  // namespace dr
