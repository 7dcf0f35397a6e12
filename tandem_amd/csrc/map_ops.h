// map_ops.h -- the map-file layer of the DrFusion engine (included by dr_fusion.hip after the kernel headers, before fusion_core.h and the components).  One rule: what every
// map-file operation does the same way is written here once -- MapIo: the pinned chunk pair and the device index buffers, the reader
// opening, the read pump, the write pump, the evaluator tail of align, locate and track; CallMemory: device memory of a single call;
// Carver: the layout of a scratch buffer as typed spans in order (drf_locate_*, drf_track_*, drf_track_colour_*) -- and
// the operations that touch no live map (drf_transform_map, drf_align_system, drf_align_map) live here whole, as functions over
// MapIo.  save / load / merge / locate read or change the engine's map and stay members of FusionEngine, written over the same pumps.
// DESIGN.md "Where the map-file operations live" says who waits, who records and who verifies.
#pragma once
#include <climits>
#include <initializer_list>
#include <string>

#include "fusion_host.h"
#include "hip_owner.h"
#include "map_file.h"

namespace dr {

// What the map-file operations share.  Lent by the engine: its HipOwner (the pair's events), device, integration stream, voxel_size
// and the default chunk.  Owned: the pinned pair, the sorted (key, slot) pairs and index lists of save / load / merge, and the
// statistics of the operations that live in this file.
struct MapIo {
  MapIo(HipOwner &own_, int device_, float voxel_size_, size_t default_chunk_) : own(own_), device(device_), voxel_size(voxel_size_), default_chunk(default_chunk_) {}
  HipOwner &own;
  const int device;
  const float voxel_size;
  const size_t default_chunk;    // blocks per chunk when the caller names none: min(num_blocks, 8192)
  hipStream_t stream = nullptr;  // the engine's integration stream (set once it exists)
  PinnedPair pair;               // allocated with the first use (ensure)
  DeviceBuf<unsigned long long> keys;
  DeviceBuf<int> slot_in, slot, dst;
  DeviceBuf<unsigned char> tmp;
  uint64_t xf_stats[6] = {0, 0, 0, 0, 0, 0};  // drf_transform_stats
  uint64_t al_stats[6] = {0, 0, 0, 0, 0, 0};  // drf_align_stats

  // blocks per chunk of a map file of n blocks: the caller's, or the default; never more than the file has or 2^20
  size_t chunk(size_t chunk_blocks, size_t n) const {
    const size_t want = chunk_blocks ? chunk_blocks : default_chunk;
    return std::max<size_t>(1, std::min({want, n, (size_t)1 << 20}));
  }
  void ensure(size_t chunk_blocks) {  // the stream idle: no kernel uses the old buffers
    if (!pair.opened()) pair.open(own);
    pair.reserve(chunk_blocks * 4096);
  }
  // every file validated as a whole (DR_ERR_IO), then one written for another lattice refused (DR_ERR_ARG), in the order given
  struct File { const char *path; MapReader *rd; };
  void open_readers(const char *who, std::initializer_list<File> files) const {
    std::string err;
    for (const File &f : files)
      if (!f.rd->open(f.path, err)) fail(DR_ERR_IO, "%s: %s", who, err.c_str());
    for (const File &f : files) {
      const float vs = f.rd->voxel_size();
      if (memcmp(&vs, &voxel_size, 4) != 0) fail(DR_ERR_ARG, "%s: %s has voxel_size %.9g, the engine %.9g", who, f.path, vs, voxel_size);
    }
  }
  void open_reader(const char *who, const char *path, MapReader &rd) const { open_readers(who, {{path, &rd}}); }
  // The read pump: every block of rd, `chunk_blocks` at a time, through the pair.  Per chunk it waits until the slot's work of two
  // chunks ago has finished, reads the file into the slot, calls each(first_block, count, host_ptr, dev_ptr) -- which enqueues on
  // `stream` what consumes the slot, or nothing -- records the slot's event and flips.  A chunk that cannot be read is not handed
  // to each; after the last chunk the reader verifies that this pass met the bytes open() validated.  false: err says why, and
  // what each did for the earlier chunks is done.  Nothing is synchronised here: the caller does that before it judges the result.
  template <class Each>
  bool read_chunks(MapReader &rd, size_t chunk_blocks, std::string &err, Each &&each) {
    const size_t n = (size_t)rd.blocks();
    for (size_t b = 0; b < n; b += chunk_blocks) {
      const size_t m = std::min(chunk_blocks, n - b);
      pair.wait();
      if (!rd.read(pair.host(), m, err)) return false;
      each(b, m, pair.host(), pair.dev());
      pair.record(stream);
      pair.flip();
    }
    return rd.verify(err);
  }
  // The write pump: n blocks, `chunk_blocks` at a time, through the pair into w.  fill(c) enqueues on `stream` the kernel that writes
  // chunk c into the current slot (pair.dev()); the pump records the slot's event behind it.  Chunk c + 1 is enqueued into the other
  // slot before the host touches chunk c, so it runs while the host does its part -- host_part(c, host_ptr): what the host itself puts
  // into the slot -- waits for the slot's kernel and appends the slot to the file.  Then the writer is closed and the stream drained
  // (a failed write leaves the next chunk's kernel in flight); a failure of append or close is DR_ERR_IO in who's name.
  struct NoHostPart { void operator()(size_t, unsigned char *) const {} };
  template <class Fill, class HostPart = NoHostPart>
  void write_chunks(const char *who, MapWriter &w, size_t n, size_t chunk_blocks, Fill &&fill, HostPart &&host_part = HostPart()) {
    const size_t nc = (n + chunk_blocks - 1) / chunk_blocks;
    auto launch = [&](size_t c) { fill(c); pair.record(stream); };
    std::string err;
    bool ok = true;
    if (nc > 0) launch(0);
    for (size_t c = 0; c < nc && ok; ++c) {
      if (c + 1 < nc) { pair.flip(); launch(c + 1); pair.flip(); }
      host_part(c, pair.host());
      pair.wait();
      ok = w.append(pair.host(), std::min(chunk_blocks, n - c * chunk_blocks), err);
      pair.flip();
    }
    ok = ok && w.close(err);
    DR_HIP(hipStreamSynchronize(stream));
    if (!ok) fail(DR_ERR_IO, "%s: %s", who, err.c_str());
  }
  // One evaluation of align or locate: the counters cleared, launch() -- the kernel that leaves `groups` rows of 28 partial sums and
  // the counters -- then k_align_fold into the pair's current slot, the stream drained, 28 sums and ncnt counters (3 or 4) copied out.
  template <class Launch>
  void evaluate(const double *partial, int groups, unsigned long long *counts, int ncnt, double sums[28], uint64_t *cnt, Launch &&launch) {
    DR_HIP(hipMemsetAsync(counts, 0, 32, stream));
    launch();
    hipLaunchKernelGGL(k_align_fold, dim3(28), dim3(64), 0, stream, partial, groups, counts, (double *)pair.dev());
    DR_HIP(hipGetLastError());
    DR_HIP(hipStreamSynchronize(stream));
    memcpy(sums, pair.host(), 224);
    memcpy(cnt, pair.host() + 224, (size_t)ncnt * 8);
  }
  // The same for drf_track_exposure_*: rows of 45 partial sums, k_exposure_fold, 45 sums and five counters copied out -- 400 bytes of
  // the pair's slot, which ensure() never makes smaller than one block's 4096.
  template <class Launch>
  void evaluate_exposure(const double *partial, int groups, unsigned long long *counts, double sums[45], uint64_t cnt[5], Launch &&launch) {
    static_assert(45 * sizeof(double) + 5 * sizeof(uint64_t) <= 4096, "the pinned pair's smallest slot holds the exposure system");
    DR_HIP(hipMemsetAsync(counts, 0, 40, stream));
    launch();
    hipLaunchKernelGGL(k_exposure_fold, dim3(45), dim3(64), 0, stream, partial, groups, counts, (double *)pair.dev());
    DR_HIP(hipGetLastError());
    DR_HIP(hipStreamSynchronize(stream));
    memcpy(sums, pair.host(), 360);
    memcpy(cnt, pair.host() + 360, 40);
  }
};

// Device memory of one call, freed on every way out.  It goes through device_alloc, so the parity build's guarded allocator sees it.
class CallMemory {
 public:
  CallMemory() = default;
  CallMemory(const CallMemory &) = delete;
  void operator=(const CallMemory &) = delete;
  ~CallMemory() { dfree(p_); }
  // what the device has free beside what is there (the parity build can lower it: the tests' way to the does-not-fit refusals)
  static size_t available() {
    size_t free_b = 0, total_b = 0;
    DR_HIP(hipMemGetInfo(&free_b, &total_b));
    if (const char *e = hook_env("DR_TRANSFORM_MAX_BYTES")) free_b = std::min(free_b, (size_t)strtoull(e, nullptr, 10));
    return free_b;
  }
  bool take(size_t bytes) {  // false: the runtime refused (its error is cleared; the caller says what did not fit)
    if (device_alloc(&p_, bytes) == hipSuccess) return true;
    p_ = nullptr; (void)hipGetLastError();
    return false;
  }
  unsigned char *get() const { return (unsigned char *)p_; }

 private:
  void *p_ = nullptr;
};

// Typed spans taken in order from one scratch buffer: the order of the take() calls is the layout, each span at its type's alignment
// or the one stated.  carve() runs a layout twice -- over no buffer for the size, then, the buffer grown to it (DeviceBuf: never
// shrunk, 256-byte aligned), over its bytes -- so a layout is written once and its size cannot disagree with it.
class Carver {
 public:
  explicit Carver(unsigned char *base = nullptr) : base_((uintptr_t)base) {}
  template <class T>
  T *take(size_t n, size_t align = alignof(T)) {
    at_ = (at_ + align - 1) / align * align;
    T *p = (T *)(base_ + at_);
    at_ += n * sizeof(T);
    return p;
  }
  size_t bytes() const { return at_; }

 private:
  uintptr_t base_;
  size_t at_ = 0;
};
template <class Layout>
void carve(DeviceBuf<unsigned char> &buf, hipStream_t stream, Layout &&layout) {
  Carver size;
  layout(size);
  buf.reserve(size.bytes(), stream);
  Carver spans(buf.get());
  layout(spans);
}

// What dr_last_error() says after a registration or refinement that ran but found no pose: `what` (who and which search), how far it
// got, `rest` (the caller's own figures); empty for every other status.  No fixed buffer: paths of any length must not cut it off.
inline std::string no_pose_note(const std::string &what, const drf_align_result_t &r, const std::string &rest) {
  if (r.status != DRF_ALIGN_DEGENERATE && r.status != DRF_ALIGN_LOST) return std::string();
  return what + " " + align_status_name(r.status) + " after " + std::to_string(r.iterations) + " evaluations (" + std::to_string((unsigned long long)r.valid) + " of " +
         std::to_string((unsigned long long)r.samples) + " samples valid" + rest;
}

// A map file resampled on the engine's lattice in another world frame and written as a map file (the rule: fusion_host.h
// transform_voxel; DESIGN.md §7c "Moving a map into another frame").  No live map is read or changed.  protocol() is the engine's
// check of its call order, made where it always was: after the null arguments, before the paths and the motion.  The source goes to
// the device whole (voxels, then the key table: 4104 n bytes), plan_transform lists the candidate destination blocks, a count pass of
// k_map_transform tells which of them hold a weighted voxel -- MapWriter wants the key table first -- and a write pass over those
// fills the pinned buffers chunk by chunk while the host appends the other buffer to <dst>.part.
template <class Protocol>
void map_transform(MapIo &io, const char *src, const float *T16, const char *dst, size_t chunk_blocks, Protocol &&protocol) {
  const char *who = "drf_transform_map";
  if (!src || !T16 || !dst) fail(DR_ERR_ARG, "%s: null argument", who);
  protocol();
  if (!strcmp(src, dst)) fail(DR_ERR_ARG, "%s: source and destination are the same path (%s)", who, src);
  if (const char *why = transform_pose_fault(T16)) fail(DR_ERR_ARG, "%s: the motion %s", who, why);
  MapReader rd;
  io.open_reader(who, src, rd);
  const size_t n = (size_t)rd.blocks();
  const MapMotion m = map_motion(T16, io.voxel_size);
  bool in_range = true;
  const std::vector<unsigned long long> cand = plan_transform(rd.keys(), m, &in_range);
  if (!in_range) fail(DR_ERR_ARG, "%s: the motion takes blocks of %s outside the key range (2^20 blocks per axis)", who, src);
  const size_t nc = cand.size();
  if (n > (size_t)INT_MAX || nc > (size_t)INT_MAX) fail(DR_ERR_CAPACITY, "%s: %zu source and %zu candidate blocks exceed the index range", who, n, nc);
  DR_HIP(hipSetDevice(io.device));
  const size_t src_bytes = n * 4104, side_bytes = nc * 20 + 16;  // candidate keys, flags, kept keys; two counters
  if (n > 0) {
    const size_t room = CallMemory::available();
    if (src_bytes + side_bytes > room)
      fail(DR_ERR_CAPACITY, "%s: %s needs %zu bytes of device memory (%zu blocks), %zu are available", who, src, src_bytes + side_bytes, n, room);
  }
  CallMemory source, side;
  uint64_t *stats = io.xf_stats;
  for (int i = 0; i < 6; ++i) stats[i] = 0;
  stats[0] = n; stats[1] = nc;
  std::vector<unsigned long long> kept;
  const size_t chunk = io.chunk(chunk_blocks, std::max(n, nc));
  DR_HIP(hipStreamSynchronize(io.stream));  // the pinned pair is idle: every user of it ends with this
  std::string err;
  unsigned char *d_vox = nullptr;
  unsigned long long *d_keys = nullptr, *d_kept = nullptr;
  if (n > 0 && nc > 0) {
    if (!source.take(src_bytes) || !side.take(side_bytes)) fail(DR_ERR_CAPACITY, "%s: %s needs %zu bytes of device memory (%zu blocks)", who, src, src_bytes + side_bytes, n);
    stats[5] = src_bytes;
    io.ensure(chunk);
    d_vox = source.get();
    d_keys = (unsigned long long *)(d_vox + n * 4096);
    unsigned long long *d_counts = (unsigned long long *)side.get(), *d_cand = d_counts + 2;
    d_kept = d_cand + nc;
    int *d_flags = (int *)(d_kept + nc);
    DR_HIP(hipMemcpyAsync(d_keys, rd.keys().data(), n * 8, hipMemcpyHostToDevice, io.stream));
    DR_HIP(hipMemcpyAsync(d_cand, cand.data(), nc * 8, hipMemcpyHostToDevice, io.stream));
    DR_HIP(hipMemsetAsync(d_counts, 0, 16, io.stream));
    const bool ok = io.read_chunks(rd, chunk, err, [&](size_t b, size_t cnt, const unsigned char *h, const unsigned char *) {
      DR_HIP(hipMemcpyAsync(d_vox + b * 4096, h, cnt * 4096, hipMemcpyHostToDevice, io.stream));
    });
    if (!ok) {
      DR_HIP(hipStreamSynchronize(io.stream));
      fail(DR_ERR_IO, "%s: %s", who, err.c_str());
    }
    hipLaunchKernelGGL(k_map_transform<false>, dim3(cdiv((int)nc, 4)), dim3(256), 0, io.stream, d_keys, (const uint2 *)d_vox, (int)n, d_cand, (int)nc, m, (uint4 *)nullptr,
                       d_flags, d_counts);
    DR_HIP(hipGetLastError());
    std::vector<int> flags(nc);
    unsigned long long counts[2] = {0, 0};
    DR_HIP(hipMemcpyAsync(flags.data(), d_flags, nc * 4, hipMemcpyDeviceToHost, io.stream));
    DR_HIP(hipMemcpyAsync(counts, d_counts, 16, hipMemcpyDeviceToHost, io.stream));
    DR_HIP(hipStreamSynchronize(io.stream));
    for (size_t i = 0; i < nc; ++i)
      if (flags[i]) kept.push_back(cand[i]);
    stats[3] = counts[0]; stats[4] = counts[1];
    if (!kept.empty()) DR_HIP(hipMemcpyAsync(d_kept, kept.data(), kept.size() * 8, hipMemcpyHostToDevice, io.stream));
  }
  const size_t nk = kept.size();
  MapWriter w;
  if (!w.open(dst, io.voxel_size, kept.data(), nk, err)) fail(DR_ERR_IO, "%s: %s", who, err.c_str());
  io.write_chunks(who, w, nk, chunk, [&](size_t c) {  // chunk c of the kept blocks into the current buffer
    const int cnt = (int)std::min(chunk, nk - c * chunk);
    hipLaunchKernelGGL(k_map_transform<true>, dim3(cdiv(cnt, 4)), dim3(256), 0, io.stream, d_keys, (const uint2 *)d_vox, (int)n, d_kept + c * chunk, cnt, m,
                       (uint4 *)io.pair.dev(), (int *)nullptr, (unsigned long long *)nullptr);
    DR_HIP(hipGetLastError());
  });
  stats[2] = nk;
}

// Two map files registered to each other (the rule: fusion_host.h align_voxel / align_step; DESIGN.md §7c "Registering two maps").
// No live map is read or changed.  with_align_maps does what both calls share -- the refusals in their order, with protocol(who), the
// engine's check of its call order, between the options and the motion; both files to the device whole (one allocation: reference
// voxels and keys, source voxels and keys, partial sums, counters) -- and hands body an evaluator: k_map_align + k_align_fold on the
// stream, 28 doubles and 3 counters back through the pinned pair.
template <class Protocol, class Body>
void with_align_maps(MapIo &io, const char *who, const char *src, const char *ref, const float *T16, const drf_align_options_t *opt, Protocol &&protocol, Body &&body) {
  uint64_t *stats = io.al_stats;
  for (int i = 0; i < 6; ++i) stats[i] = 0;
  AlignOpt ao;
  if (const char *bad = align_options(opt, io.voxel_size, ao)) fail(DR_ERR_ARG, "%s: option %s is negative or not finite", who, bad);
  protocol(who);
  if (const char *why = transform_pose_fault(T16)) fail(DR_ERR_ARG, "%s: the motion %s", who, why);
  MapReader rs, rr;
  io.open_readers(who, {{src, &rs}, {ref, &rr}});  // both files validated before either voxel_size is judged
  const size_t ns = (size_t)rs.blocks(), nr = (size_t)rr.blocks();
  if (ns > (size_t)INT_MAX || nr > (size_t)INT_MAX) fail(DR_ERR_CAPACITY, "%s: %zu source and %zu reference blocks exceed the index range", who, ns, nr);
  DR_HIP(hipSetDevice(io.device));
  const size_t bytes = (ns + nr) * 4104 + ns * 224 + 32;
  const size_t room = CallMemory::available();
  if (bytes > room) fail(DR_ERR_CAPACITY, "%s: %zu bytes of device memory are needed (%zu + %zu blocks), %zu are available: %s and %s", who, bytes, ns, nr, room, src, ref);
  CallMemory held;
  DR_HIP(hipStreamSynchronize(io.stream));  // the pinned pair is idle: every user of it ends with this
  if (!held.take(bytes)) fail(DR_ERR_CAPACITY, "%s: %zu bytes of device memory are needed (%zu + %zu blocks): %s and %s", who, bytes, ns, nr, src, ref);
  stats[0] = ns; stats[1] = nr; stats[5] = bytes;
  // layout, every part a multiple of 8 bytes: ref voxels, src voxels, ref keys, src keys, partial sums, 3 counters (+ 1 unused)
  unsigned char *r_vox = held.get(), *s_vox = r_vox + nr * 4096;
  unsigned long long *r_keys = (unsigned long long *)(s_vox + ns * 4096), *s_keys = r_keys + nr;
  double *partial = (double *)(s_keys + ns);
  unsigned long long *counts = (unsigned long long *)(partial + ns * 28);
  const size_t chunk = io.chunk(0, std::max(ns, nr));
  io.ensure(chunk);
  std::string err;
  auto upload = [&](MapReader &rd, unsigned char *d_vox, unsigned long long *d_keys) {  // the file through the pinned pair to the device
    if (rd.blocks()) DR_HIP(hipMemcpyAsync(d_keys, rd.keys().data(), (size_t)rd.blocks() * 8, hipMemcpyHostToDevice, io.stream));
    return io.read_chunks(rd, chunk, err, [&](size_t b, size_t cnt, const unsigned char *h, const unsigned char *) {
      DR_HIP(hipMemcpyAsync(d_vox + b * 4096, h, cnt * 4096, hipMemcpyHostToDevice, io.stream));
    });
  };
  const bool ok = upload(rs, s_vox, s_keys) && upload(rr, r_vox, r_keys);
  DR_HIP(hipStreamSynchronize(io.stream));  // (also: the key tables' host memory may go now, and both slots are idle)
  if (!ok) { stats[5] = 0; fail(DR_ERR_IO, "%s: %s", who, err.c_str()); }
  double c_src[3];
  align_centre_src(rs.keys(), c_src);
  auto eval = [&](const AlignEval &e, double sums[28], uint64_t cnt[3]) {
    io.evaluate(partial, (int)ns, counts, 3, sums, cnt, [&] {
      if (!ns) return;
      hipLaunchKernelGGL(k_map_align, dim3(cdiv((int)ns, 4)), dim3(256), 0, io.stream, s_keys, (const uint4 *)s_vox, (int)ns, r_keys, (const uint2 *)r_vox, (int)nr, e,
                         partial, counts);
      DR_HIP(hipGetLastError());
    });
    stats[2] = cnt[0]; stats[3] = cnt[1]; ++stats[4];
  };
  body(ao, c_src, eval);
}
template <class Protocol>
void map_align_system(MapIo &io, const char *src, const char *ref, const float *T16, const drf_align_options_t *opt, double *sums, uint64_t *counts, Protocol &&protocol) {
  if (!src || !ref || !T16 || !sums || !counts) fail(DR_ERR_ARG, "drf_align_system: null argument");
  with_align_maps(io, "drf_align_system", src, ref, T16, opt, protocol, [&](const AlignOpt &ao, const double c_src[3], auto &eval) {
    eval(align_eval(map_motion(T16, io.voxel_size), c_src, ao, io.voxel_size), sums, counts);
  });
}
// returns what dr_last_error() says after a registration that ran but found no pose (empty otherwise)
template <class Protocol>
std::string map_align(MapIo &io, const char *src, const char *ref, const float *T16, const drf_align_options_t *opt, float *T16_out, drf_align_result_t *res,
                      Protocol &&protocol) {
  if (!src || !ref || !T16 || !T16_out) fail(DR_ERR_ARG, "drf_align_map: null argument");
  drf_align_result_t r;
  with_align_maps(io, "drf_align_map", src, ref, T16, opt, protocol,
                  [&](const AlignOpt &ao, const double c_src[3], auto &eval) { align_loop(eval, map_motion(T16, io.voxel_size), c_src, ao, io.voxel_size, r); });
  for (int i = 0; i < 16; ++i) T16_out[i] = (float)r.T[i];
  if (res) *res = r;
  return no_pose_note("drf_align_map: the registration", r, std::string("): ") + src + " to " + ref);
}

}  // namespace dr
