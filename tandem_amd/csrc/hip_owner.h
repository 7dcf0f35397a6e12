// What the engines take from the HIP runtime (included by dr_fusion.hip, map_ops.h, mvs_plan.h, dr_mvsnet.hip and dr_tracker.hip): HipOwner for what lives
// as long as its holder (an engine, a DrMvsnet window plan, one measurement), and for DrFusion DeviceBuf / PinnedBuf for scratch that grows with its
// use, BlockStaging for the double-buffered transport of stored voxel blocks to the device, PinnedPair for the two chunk buffers of the map file.
#pragma once
#include <vector>

#include "dr_common.h"

namespace dr {

// Owner of what its holder takes from the runtime for its lifetime: device and pinned buffers, events, streams.  All of it is
// released with the owner -- buffers first, then the events and streams that work on them used -- also when the holder's
// constructor throws half way; the current device at that moment is the one it was taken on (the holder sees to it).  The raw
// pointers and handles go where they are used (FusionDev, StreamDev, McArgs: by value).
class HipOwner {
 public:
  HipOwner() = default;
  HipOwner(const HipOwner &) = delete;
  void operator=(const HipOwner &) = delete;
  ~HipOwner() {
    // (nothing to wait for where nothing was taken, or events only: those of one measurement, in a function-local owner)
    if (!dev_.empty() || !pin_.empty() || !st_.empty()) (void)hipDeviceSynchronize();
    for (void *p : dev_) dfree(p);
    for (void *p : pin_) (void)hipHostFree(p);
    for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
    for (hipStream_t s : st_) (void)hipStreamDestroy(s);
  }
  // device memory, cleared on stream `zero_on` if one is given.  The guarded allocator of the parity build names the buffer `label`, or the caller's file and line.
  template <class T> T *device(size_t n, hipStream_t zero_on = nullptr, const char *label = nullptr, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    T *p = (T *)take(dev_, [&](void **q) { *q = dalloc<T>(n, label, file, line); });
    if (zero_on) DR_HIP(hipMemsetAsync(p, 0, n * sizeof(T), zero_on));
    return p;
  }
  // page-locked host memory; as_device: the address the kernels use for it
  template <class T> T *pinned(size_t n, T **as_device = nullptr) {
    T *p = (T *)take(pin_, [&](void **q) { DR_HIP(hipHostMalloc(q, n * sizeof(T), hipHostMallocDefault)); });
    if (as_device) DR_HIP(hipHostGetDevicePointer((void **)as_device, p, 0));
    return p;
  }
  hipEvent_t event(unsigned flags = hipEventDisableTiming) {
    return take(ev_, [&](hipEvent_t *e) { DR_HIP(hipEventCreateWithFlags(e, flags)); });
  }
  hipStream_t stream(int priority = 0) {
    return take(st_, [&](hipStream_t *q) { DR_HIP(hipStreamCreateWithPriority(q, hipStreamNonBlocking, priority)); });
  }
  // the same from the call that names no priority (DrMvsnet: the runtime maps streams to hardware queues as they are created; its speed was measured with this call)
  hipStream_t stream_plain() {
    return take(st_, [&](hipStream_t *q) { DR_HIP(hipStreamCreateWithFlags(q, hipStreamNonBlocking)); });
  }

 private:
  // the slot first, then what goes into it: nothing is taken that could not be recorded
  template <class H, class Make> H take(std::vector<H> &v, Make make) {
    v.push_back(H());
    make(&v.back());
    return v.back();
  }
  std::vector<void *> dev_, pin_;
  std::vector<hipEvent_t> ev_;
  std::vector<hipStream_t> st_;
};
// Device scratch that grows with its use; contents are not kept.  `st`: the stream whose work may still read the old allocation.
template <class T>
class DeviceBuf {
 public:
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf &) = delete;
  void operator=(const DeviceBuf &) = delete;
  ~DeviceBuf() { dfree(p_); }
  void reserve(size_t n, hipStream_t st) {
    if (n <= cap_) return;
    DR_HIP(hipStreamSynchronize(st));
    if (p_) DR_HIP(device_free(p_));
    p_ = nullptr; cap_ = 0;
    p_ = dalloc<T>(n);
    cap_ = n;
  }
  T *get() const { return p_; }
  size_t capacity() const { return cap_; }

 private:
  T *p_ = nullptr;
  size_t cap_ = 0;
};

// Page-locked host scratch that grows with its use; contents are not kept.  The caller makes sure no copy still reads the old allocation.
template <class T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  void operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { (void)hipHostFree(p_); }
  void reserve(size_t n) {
    if (n <= cap_) return;
    if (p_) DR_HIP(hipHostFree(p_));
    p_ = nullptr; cap_ = 0;
    DR_HIP(hipHostMalloc((void **)&p_, n * sizeof(T), hipHostMallocDefault));
    cap_ = n;
  }
  T *get() const { return p_; }

 private:
  T *p_ = nullptr;
  size_t cap_ = 0;
};

// Carries packed blocks to the device for kernels that read them there.  Two slots, each a pinned buffer and its device twin, are
// filled in turn, so that packing and copying one overlaps the kernels that read the other.  The copies run on a side stream of the
// staging's own (open(): with the first use).  Per slot, `ready` orders the consumers behind what the side stream did for it, and
// `used` -- recorded by a consumer that has one event for all its readers -- the slot's next copy behind the kernels.
class BlockStaging {
 public:
  void open(HipOwner &own) {
    stream_ = own.stream();
    for (auto &s : slot_)
      for (hipEvent_t *e : {&s.ready, &s.used}) { *e = own.event(); DR_HIP(hipEventRecord(*e, stream_)); }
  }
  // both slots hold `bytes`; contents are not kept.  The caller makes sure that nothing reads the old allocations any more.
  void reserve(size_t bytes) { for (auto &s : slot_) { s.dev.reserve(bytes, stream_); s.host.reserve(bytes); } }
  // the other slot becomes the current one: its pinned buffer, once its last copy has left it
  unsigned char *next() { cur_ ^= 1; DR_HIP(hipEventSynchronize(slot_[cur_].ready)); return slot_[cur_].host.get(); }
  // the first `bytes` of the pinned buffer to its device twin, on the side stream
  void copy(size_t bytes) { DR_HIP(hipMemcpyAsync(dev(), slot_[cur_].host.get(), bytes, hipMemcpyHostToDevice, stream_)); }
  // `ready` = everything the side stream was given so far; a consumer stream waits for it
  void record_ready() { DR_HIP(hipEventRecord(slot_[cur_].ready, stream_)); }
  void wait_ready(hipStream_t consumer) { DR_HIP(hipStreamWaitEvent(consumer, slot_[cur_].ready, 0)); }
  // the side stream goes on behind event e of a consumer
  void wait_for(hipEvent_t e) { DR_HIP(hipStreamWaitEvent(stream_, e, 0)); }
  hipStream_t stream() const { return stream_; }  // null before open()
  unsigned char *dev() const { return slot_[cur_].dev.get(); }
  hipEvent_t used() const { return slot_[cur_].used; }
  int slot() const { return cur_; }

 private:
  struct Slot {
    PinnedBuf<unsigned char> host;
    DeviceBuf<unsigned char> dev;
    hipEvent_t ready = nullptr, used = nullptr;
  } slot_[2];
  int cur_ = 0;
  hipStream_t stream_ = nullptr;
};

// Two page-locked buffers that kernels address directly, used in turn: the host fills or drains one while a kernel reads or
// writes the other (the map file's chunks: map_ops.h MapIo owns the pair and its two pumps use it).  No device twin and no stream of its own, which
// is what sets it apart from BlockStaging: the kernels run on the caller's stream, and per slot ONE event says that the kernel
// given that slot has finished with it.
class PinnedPair {
 public:
  void open(HipOwner &own) { for (auto &s : slot_) s.done = own.event(); }
  bool opened() const { return slot_[0].done != nullptr; }
  // both slots hold `bytes`; contents are not kept.  The caller makes sure that no kernel still uses the old allocations.
  void reserve(size_t bytes) {
    for (auto &s : slot_) {
      s.host.reserve(bytes);
      DR_HIP(hipHostGetDevicePointer((void **)&s.dev, s.host.get(), 0));
    }
  }
  // the other slot becomes the current one
  void flip() { cur_ ^= 1; }
  unsigned char *host() const { return slot_[cur_].host.get(); }
  unsigned char *dev() const { return slot_[cur_].dev; }  // the same bytes as the kernels address them
  // the current slot's kernel is the last thing enqueued on st / the host waits for it (at once if the slot never had one)
  void record(hipStream_t st) { DR_HIP(hipEventRecord(slot_[cur_].done, st)); slot_[cur_].busy = true; }
  void wait() {
    if (!slot_[cur_].busy) return;
    DR_HIP(hipEventSynchronize(slot_[cur_].done));
    slot_[cur_].busy = false;
  }

 private:
  struct Slot {
    PinnedBuf<unsigned char> host;
    unsigned char *dev = nullptr;
    hipEvent_t done = nullptr;
    bool busy = false;
  } slot_[2];
  int cur_ = 0;
};

}  // namespace dr
