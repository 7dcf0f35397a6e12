// mesh_ops.h -- MeshExtractor: marching cubes over the pool (TsdfVolume::ExtractMeshAsync / GetMeshSync), over the whole map, host
// store included (DRF_MESH_MAP), and the incremental mesh (DESIGN.md §7c "Meshing the whole map", "Incremental mesh"; the kernels:
// mesh_kernels.h, mesh_update_kernels.h; the host rules: fusion_host.h plan_mesh_chunks, MeshUpdateLedger).  It owns the extraction
// in flight, its buffers -- the two 20 M-triangle buffers exist from the first extraction with a non-empty box on -- the update's
// ledger and device scratch, and the map pass's staging.  The engine lends it FusionCore and the BlockStreamer, whose store it reads.
// Everything runs on the integration stream.  Included by dr_fusion.hip after stream_ops.h.
#pragma once
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>  // device radix sort (block keys) and exclusive scan (triangle offsets)

#include "fusion_core.h"
#include "fusion_host.h"
#include "stream_ops.h"

namespace dr {

class MeshExtractor {
 public:
  MeshExtractor(FusionCore &core, BlockStreamer &streamer) : core_(core), streamer_(streamer) {}
  // every entry point that integrates comes through the engine's enqueue_scan, which reports the scan's Ti here
  void record_scan(const Mat &Ti) { ledger_.record_scan(Ti.m); }
  // ---- the entry points, behind the engine's call-order check (and the null-argument check where that comes first) ----
  // ---- marching cubes: TsdfVolume::ExtractMeshAsync / GetMeshSync (tsdf_volume.cu:759-838) ----
  void extract_mesh_async(const float *lower, const float *upper) {
    if (mesh_pending_) fail(DR_ERR_PROTOCOL, "mesh_extractor should be NULL (fetch the previous mesh with GetMeshSync first)");
    launch_extraction(lower, upper);
    mesh_pending_ = true;
  }
  size_t mesh_num_triangles() {  // blocks until the pending extraction is done; does not consume it
    if (!mesh_pending_) fail(DR_ERR_PROTOCOL, "mesh_extractor should not be NULL (did you call ExtractMeshAsync before)?");
    if (mesh_pending_update_) fail(DR_ERR_PROTOCOL, "GetMeshSync: the pending extraction is a mesh update, fetch it with drf_get_mesh_update_sync");
    return finish_mesh();
  }
  // vert / cols hold num_max vertices (3 floats each).  The reference compares num_max with the TRIANGLE count
  // (tsdf_volume.cu:796) and would overrun for meshes above num_max / 3 triangles; here the vertex count is checked.
  void get_mesh_sync(size_t num_max, size_t *num, float *vert, float *cols) {
    if (!num || !vert || !cols) fail(DR_ERR_ARG, "GetMeshSync: null argument");
    const size_t ntri = mesh_num_triangles();
    if (num_max < 3 * ntri) fail(DR_ERR_CAPACITY, "Did not provide enough storage for mesh (%zu vertices > %zu).", 3 * ntri, num_max);
    fetch_mesh(ntri, vert, cols);
    *num = 3 * ntri;  // 1 triangle = 3 vert (tsdf_volume.cu:800)
    mesh_pending_ = false;
  }
  // DrFusion::SaveMeshToFile (dr_fusion.cpp:74-93): synchronous extraction, then Mesh::SaveToFile(filename, bgr=true)
  // (mesh.cu:24-66): one "v x y z r g b" line per vertex, one "f i i+1 i+2" line per triangle.
  void save_mesh(const char *filename, const float *lower, const float *upper) {
    if (!filename || !lower || !upper) fail(DR_ERR_ARG, "SaveMeshToFile: null argument");
    if (mesh_pending_) fail(DR_ERR_PROTOCOL, "SaveMeshToFile: an ExtractMeshAsync is pending, call GetMeshSync first");
    launch_extraction(lower, upper);
    const size_t ntri = finish_mesh();
    std::vector<float> v(ntri * 9), c(ntri * 9);
    fetch_mesh(ntri, v.data(), c.data());
    FILE *f = fopen(filename, "w");
    if (!f) fail(DR_ERR_IO, "SaveMeshToFile: cannot open %s", filename);
    for (size_t i = 0; i < ntri * 3; ++i)
      fprintf(f, "v %g %g %g %g %g %g\n", v[3 * i], v[3 * i + 1], v[3 * i + 2], c[3 * i], c[3 * i + 1], c[3 * i + 2]);
    for (size_t i = 1; i <= ntri * 3; i += 3) fprintf(f, "f %zu %zu %zu\n", i, i + 1, i + 2);
    if (fclose(f) != 0) fail(DR_ERR_IO, "SaveMeshToFile: write to %s failed", filename);
  }
  // DRF_MESH_RESIDENT: the pool only (the default); DRF_MESH_MAP: the pool and the host store together
  void set_mesh_scope(int scope) {
    if (scope != DRF_MESH_RESIDENT && scope != DRF_MESH_MAP) fail(DR_ERR_ARG, "drf_set_mesh_scope: unknown scope %d", scope);
    if (mesh_pending_) fail(DR_ERR_PROTOCOL, "drf_set_mesh_scope: an extraction is pending, call GetMeshSync first");
    mesh_scope_ = scope;
  }
  // last extraction: blocks meshed (workgroups of each pass), host blocks uploaded (once per chunk that stages them), chunks
  void mesh_stats(uint64_t out[3]) const {
    if (!out) fail(DR_ERR_ARG, "drf_mesh_stats: null argument");
    for (int i = 0; i < 3; ++i) out[i] = mesh_stats_[i];
  }
  // ---- incremental mesh: an extraction that lists only the blocks whose triangles may have changed since the baseline
  // (the last update fetched); no reference counterpart.  DESIGN.md §7c "Incremental mesh".
  void extract_mesh_update_async(const float *lower, const float *upper) {
    if (mesh_pending_) fail(DR_ERR_PROTOCOL, "drf_extract_mesh_update_async: an extraction is pending, fetch it first");
    streamer_.settle();  // in either scope: what the host store holds decides below
    if (mesh_scope_ == DRF_MESH_RESIDENT && !streamer_.store().empty())
      fail(DR_ERR_PROTOCOL, "drf_extract_mesh_update_async: %zu blocks are in the host store; the resident view changes by eviction, which an update does not track (use DRF_MESH_MAP)", streamer_.store().size());
    // a round-trip mismatch writes a block that is not on the visible list (k_integrate)
    unsigned long long redirects = 0;
    DR_HIP(hipMemcpy(&redirects, core_.d.cnt + 2, 8, hipMemcpyDeviceToHost));
    ledger_.begin(lower, upper, redirects);  // (before the launch, which may throw: the pending update is read only while mesh_pending_update_ is set)
    if (streamer_.store().empty()) launch_mesh_update(lower, upper);
    else launch_mesh_map(lower, upper, true);
    ledger_.launched();  // the scans recorded so far belong to this update, later ones to the next
    mesh_pending_ = mesh_pending_update_ = true;
  }
  void mesh_update_size(size_t *nblk, size_t *ntri, int *full) {
    if (!nblk || !ntri || !full) fail(DR_ERR_ARG, "drf_mesh_update_size: null argument");
    if (!mesh_pending_ || !mesh_pending_update_) fail(DR_ERR_PROTOCOL, "drf_mesh_update_size: no mesh update is pending");
    *ntri = finish_mesh(); *nblk = ledger_.pending().nblk; *full = ledger_.pending().full ? 1 : 0;
  }
  void get_mesh_update_sync(size_t max_blocks, size_t num_max, size_t *nblk, int32_t *coords, uint64_t *first, size_t *num, float *vert,
                            float *cols, int *full) {
    if (!nblk || !coords || !first || !num || !vert || !cols || !full) fail(DR_ERR_ARG, "drf_get_mesh_update_sync: null argument");
    if (!mesh_pending_ || !mesh_pending_update_) fail(DR_ERR_PROTOCOL, "drf_get_mesh_update_sync: no mesh update is pending");
    const size_t ntri = finish_mesh(), nb = ledger_.pending().nblk;
    if (max_blocks < nb) fail(DR_ERR_CAPACITY, "Did not provide enough storage for the patch table (%zu blocks > %zu).", nb, max_blocks);
    if (num_max < 3 * ntri) fail(DR_ERR_CAPACITY, "Did not provide enough storage for mesh (%zu vertices > %zu).", 3 * ntri, num_max);
    first[0] = 0;
    if (nb > 0) {
      DR_HIP(hipMemcpy(coords, mu_coords_.get(), nb * 12, hipMemcpyDeviceToHost));
      DR_HIP(hipMemcpy(first, mu_first_.get(), (nb + 1) * 8, hipMemcpyDeviceToHost));
      fetch_mesh(ntri, vert, cols);
    }
    *nblk = nb; *num = 3 * ntri; *full = ledger_.pending().full ? 1 : 0;
    ledger_.fetched();  // the baseline advances: this box, the voxel state at the launch
    mesh_pending_ = mesh_pending_update_ = false;
  }
  void force_full_update() { ledger_.force_full(); }  // drf_load_map, drf_merge_map, drf_mesh_update_reset
  // last update launched: blocks in scope, blocks meshed again, scans folded in, full
  void mesh_update_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_mesh_update_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = mu_stats_[i];
  }

 private:
  // ---- the mesh pass, shared by every extraction ----
  void mesh_empty() {
    DR_HIP(hipMemsetAsync(mesh_total_, 0, 8, core_.int_stream));
    DR_HIP(hipEventRecord(mesh_done_ev(), core_.int_stream));
  }
  // Prologue of every extraction (core_.int_stream idle): the lattice into a.n, the statistics cleared; returns the pool's block count.
  // Nothing is launched yet: the caller enqueues the empty result (mesh_empty) or goes on with mesh_tables.
  int mesh_begin(const float *lower, const float *upper, McArgs &a) {
    for (int k = 0; k < 3; ++k) {  // lattice cells per axis (ExtractMeshKernel, mesh_extractor.cu:241-245)
      a.n[k] = f2i_host(fabsf(lower[k] - upper[k]) / core_.o.voxel_size);
      if (a.n[k] > (1 << 22))
        fail(DR_ERR_ARG, "ExtractMesh: %d lattice cells along axis %d (box too large for voxel_size %g)", a.n[k], k, core_.o.voxel_size);
    }
    if (!mesh_total_) mesh_total_ = core_.own.device<unsigned long long>(1);
    mesh_stats_[0] = mesh_stats_[1] = mesh_stats_[2] = 0;
    return core_.pool_blocks();
  }
  static bool box_empty(const McArgs &a) { return a.n[0] <= 0 || a.n[1] <= 0 || a.n[2] <= 0; }
  // The axis tables, the per-block arrays and the 20 M-triangle output (allocated with the first extraction), then k_mc_axes and
  // the pool's nblk keys sorted into mesh_keys_.  The box is not empty.
  void mesh_tables(const float *lower, McArgs &a, int nblk) {
    const float vs = core_.o.voxel_size;
    mesh_axis_.reserve((size_t)a.n[0] + a.n[1] + a.n[2], core_.int_stream);
    if (!mesh_keys_) {
      mesh_keys_ = core_.own.device<unsigned long long>(core_.o.num_blocks);
      mesh_counts_ = core_.own.device<unsigned>(core_.o.num_blocks);
      mesh_offsets_ = core_.own.device<unsigned>(core_.o.num_blocks);
      size_t t1 = 0, t2 = 0;
      DR_HIP(rocprim::radix_sort_keys(nullptr, t1, core_.d.blk_key, mesh_keys_, (size_t)core_.o.num_blocks, 0, 63, core_.int_stream));
      DR_HIP(rocprim::exclusive_scan(nullptr, t2, mesh_counts_, mesh_offsets_, 0u, (size_t)core_.o.num_blocks, rocprim::plus<unsigned>(), core_.int_stream));
      mesh_tmp_.reserve(std::max(t1, t2), core_.int_stream);
      // the reference's MeshExtractor::Init(20000000, ...) (tsdf_volume.cu:776): 72 B per triangle, 1.44 GB of HBM
      mesh_vert_ = core_.own.device<float>((size_t)kMeshMaxTriangles * 9);
      mesh_cols_ = core_.own.device<float>((size_t)kMeshMaxTriangles * 9);
    }
    McAxis *p = mesh_axis_.get();
    for (int k = 0; k < 3; ++k) {
      hipLaunchKernelGGL(k_mc_axes, dim3(cdiv(a.n[k], 256)), dim3(256), 0, core_.int_stream, p, a.n[k], lower[k], vs);
      a.ax[k] = p;
      p += a.n[k];
    }
    a.counts = mesh_counts_; a.offsets = mesh_offsets_;
    a.vert = mesh_vert_; a.cols = mesh_cols_; a.cap_tri = kMeshMaxTriangles;
    size_t tb = mesh_tmp_.capacity();
    if (nblk > 0) DR_HIP(rocprim::radix_sort_keys(mesh_tmp_.get(), tb, core_.d.blk_key, mesh_keys_, (size_t)nblk, 0, 63, core_.int_stream));
  }
  // Count, scan, emit for the blocks a.sorted_keys[0, a.nblk).  Resident form: the result is these triangles (k_mc_total).
  // STAGED (one chunk of the map pass): emitted at the running total a.base, which then advances.
  // table: rows [row0, row0 + a.nblk) of the mesh update's patch table.
  template <bool STAGED> void mesh_pass(const McArgs &a, bool table, size_t row0 = 0) {
    const dim3 grid((unsigned)a.nblk), block(256);
    hipLaunchKernelGGL((k_mc_cells<false, STAGED>), grid, block, 0, core_.int_stream, core_.d, a);
    size_t tb = mesh_tmp_.capacity();
    DR_HIP(rocprim::exclusive_scan(mesh_tmp_.get(), tb, mesh_counts_, mesh_offsets_, 0u, (size_t)a.nblk, rocprim::plus<unsigned>(), core_.int_stream));
    hipLaunchKernelGGL((k_mc_cells<true, STAGED>), grid, block, 0, core_.int_stream, core_.d, a);
    if (!STAGED) hipLaunchKernelGGL(k_mc_total, dim3(1), dim3(1), 0, core_.int_stream, mesh_counts_, mesh_offsets_, a.nblk, mesh_total_);
    if (table)
      hipLaunchKernelGGL(k_mu_table, dim3(cdiv(a.nblk + 1, 256)), dim3(256), 0, core_.int_stream, a.sorted_keys, a.nblk, mesh_counts_, mesh_offsets_,
                         a.base, row0, mu_coords_.get(), mu_first_.get());
    if (STAGED) hipLaunchKernelGGL(k_mc_advance, dim3(1), dim3(1), 0, core_.int_stream, mesh_counts_, mesh_offsets_, a.nblk, mesh_total_);
  }
  // the extraction is enqueued: blocks meshed, host blocks uploaded (once per chunk that stages them), chunks
  void mesh_end(size_t blocks, size_t uploads, size_t chunks) {
    DR_HIP(hipGetLastError());
    DR_HIP(hipEventRecord(mesh_done_ev(), core_.int_stream));
    mesh_stats_[0] = blocks; mesh_stats_[1] = uploads; mesh_stats_[2] = chunks;
  }
  // DRF_MESH_MAP folds pending evictions first; with an empty host store it is the resident pass
  void launch_extraction(const float *lower, const float *upper) {
    if (mesh_scope_ == DRF_MESH_MAP) {
      streamer_.settle();
      if (!streamer_.store().empty()) return launch_mesh_map(lower, upper);
    }
    launch_mesh(lower, upper);
  }
  // Enqueue the whole extraction on core_.int_stream (after the last integration, before the next one).
  void launch_mesh(const float *lower, const float *upper) {
    DR_HIP(hipSetDevice(core_.device));
    DR_HIP(hipStreamSynchronize(core_.int_stream));  // the block count lives on the device
    McArgs a{};
    const int nblk = mesh_begin(lower, upper, a);
    if (box_empty(a) || nblk <= 0) return mesh_empty();
    mesh_tables(lower, a, nblk);
    a.sorted_keys = mesh_keys_; a.nblk = nblk;
    mesh_pass<false>(a, false);
    mesh_end((size_t)nblk, 0, 1);
  }
  // ---- mesh update: selection and the resident form ----
  // Blocks of keys[0, n) (device, ascending) to mesh again after the recorded scans, compacted in order into mu_sel_; returns
  // their number (one 4-byte read back: the mesh kernels' grid).
  int mu_select(const unsigned long long *keys, int n) {
    mu_flags_.reserve((size_t)n, core_.int_stream); mu_pos_.reserve((size_t)n, core_.int_stream); mu_sel_.reserve((size_t)n, core_.int_stream);
    if (!mu_nsel_) mu_nsel_ = core_.own.device<int>(1);
    size_t tb = 0;  // scan scratch for n items (the mesh path's is sized for the pool; a map's scope may be longer)
    DR_HIP(rocprim::exclusive_scan(nullptr, tb, mesh_counts_, mesh_offsets_, 0u, (size_t)n, rocprim::plus<unsigned>(), core_.int_stream));
    mesh_tmp_.reserve(tb, core_.int_stream);
    MuArgs m{};
    m.keys = keys; m.n = n; m.nposes = (int)ledger_.poses().size(); m.reach2 = mesh_update_reach2(core_.o); m.flags = mu_flags_.get();
    memcpy(m.Ti, ledger_.poses().data(), ledger_.poses().size() * sizeof(MuPose));
    hipLaunchKernelGGL(k_mu_select, dim3(cdiv(n, 256)), dim3(256), 0, core_.int_stream, core_.o, m);
    tb = mesh_tmp_.capacity();
    DR_HIP(rocprim::exclusive_scan(mesh_tmp_.get(), tb, mu_flags_.get(), mu_pos_.get(), 0u, (size_t)n, rocprim::plus<unsigned>(), core_.int_stream));
    hipLaunchKernelGGL(k_mu_compact, dim3(cdiv(n, 256)), dim3(256), 0, core_.int_stream, keys, mu_flags_.get(), mu_pos_.get(), n, mu_sel_.get(), mu_nsel_);
    DR_HIP(hipGetLastError());
    int nsel = 0;
    DR_HIP(hipMemcpyAsync(&nsel, mu_nsel_, 4, hipMemcpyDeviceToHost, core_.int_stream));
    DR_HIP(hipStreamSynchronize(core_.int_stream));
    return std::max(0, std::min(nsel, n));
  }
  void mu_table_reserve(size_t nblk) { mu_coords_.reserve(3 * nblk, core_.int_stream); mu_first_.reserve(nblk + 1, core_.int_stream); }
  // The resident pass of launch_mesh over the selected blocks only (all of them when ledger_.pending().full), plus the patch table.
  void launch_mesh_update(const float *lower, const float *upper) {
    McArgs a{};
    const int nblk = mesh_begin(lower, upper, a);
    mu_stats_[0] = (uint64_t)std::max(nblk, 0); mu_stats_[1] = 0; mu_stats_[2] = ledger_.poses().size(); mu_stats_[3] = ledger_.pending().full;
    if (box_empty(a) || nblk <= 0 || (!ledger_.pending().full && ledger_.poses().empty())) return mesh_empty();
    mesh_tables(lower, a, nblk);
    a.sorted_keys = mesh_keys_; a.nblk = nblk;
    if (!ledger_.pending().full) { a.nblk = mu_select(mesh_keys_, nblk); a.sorted_keys = mu_sel_.get(); }
    if (a.nblk == 0) return mesh_empty();
    mu_table_reserve((size_t)a.nblk);
    mesh_pass<false>(a, true);
    mesh_end((size_t)a.nblk, 0, 1);
    mu_stats_[1] = (uint64_t)a.nblk; ledger_.set_rows((size_t)a.nblk);
  }
  // ---- the map pass (DRF_MESH_MAP with blocks in the host store; DESIGN.md §7c "Meshing the whole map") ----
  // Global order = ascending key over resident and stored blocks, as the resident pass orders the pool.  The merged list is cut
  // into chunks (plan_mesh_chunks); a chunk's keys and the stored blocks it stages are packed into pinned memory and copied to
  // one of two device buffers on a copy stream, so that packing and copying chunk k + 1 overlap the kernels of chunk k.  Per chunk:
  // mesh_pass at the running base (mesh_total_).  Neither the pool nor the host store changes.
  int ms_own_cap() const { return std::min(core_.o.num_blocks, kStageBlocks); }
  int ms_stage_cap() const { return std::max(ms_own_cap(), 27); }  // one block's 27 neighbours always fit
  // update: the mesh-update form (drf_extract_mesh_update_async) -- only the blocks the selection kernel keeps (all of the scope
  // when ledger_.pending().full) are planned into chunks, staged and meshed, and each chunk adds its rows to the patch table.
  void launch_mesh_map(const float *lower, const float *upper, bool update = false) {
    McArgs a{};
    const int nblk = mesh_begin(lower, upper, a);
    if (update) { mu_stats_[0] = mu_stats_[1] = 0; mu_stats_[2] = ledger_.poses().size(); mu_stats_[3] = ledger_.pending().full; }
    if (box_empty(a)) return mesh_empty();  // (an empty pool is no reason: the host store holds blocks)
    mesh_tables(lower, a, nblk);
    std::vector<unsigned long long> res(std::max(nblk, 0));
    if (nblk > 0) DR_HIP(hipMemcpyAsync(res.data(), mesh_keys_, (size_t)nblk * 8, hipMemcpyDeviceToHost, core_.int_stream));
    const std::vector<unsigned long long> sto = streamer_.store().sorted_keys();
    const BlockRange range = lattice_block_range(lower, a.n, core_.o.voxel_size);
    DR_HIP(hipStreamSynchronize(core_.int_stream));
    // update: the scope is the merged list within the range; the selection kernel runs over it and the survivors come back
    std::vector<unsigned long long> picked;
    if (update) {
      picked.reserve(res.size() + sto.size());
      for_each_in_range(res, sto, range, [&](unsigned long long key, bool) { picked.push_back(key); });
      mu_stats_[0] = picked.size();
      if (picked.empty() || (!ledger_.pending().full && ledger_.poses().empty())) return mesh_empty();
      if (picked.size() > (size_t)INT_MAX) fail(DR_ERR_CAPACITY, "mesh update: %zu blocks in scope", picked.size());
      if (!ledger_.pending().full) {
        mu_scope_.reserve(picked.size(), core_.int_stream);
        DR_HIP(hipMemcpyAsync(mu_scope_.get(), picked.data(), picked.size() * 8, hipMemcpyHostToDevice, core_.int_stream));
        const int nsel = mu_select(mu_scope_.get(), (int)picked.size());
        if (nsel == 0) return mesh_empty();
        picked.resize((size_t)nsel);
        DR_HIP(hipMemcpy(picked.data(), mu_sel_.get(), (size_t)nsel * 8, hipMemcpyDeviceToHost));
      }
      mu_table_reserve(picked.size());
    }
    const MeshPlan plan = plan_mesh_chunks(res, sto, streamer_.store(), range, (size_t)ms_own_cap(), (size_t)ms_stage_cap(), update ? &picked : nullptr);
    DR_HIP(hipMemsetAsync(mesh_total_, 0, 8, core_.int_stream));
    if (plan.chunks() > 0 && !ms_.stream()) {
      ms_.open(core_.own);
      ms_.reserve((size_t)ms_own_cap() * 8 + (size_t)ms_stage_cap() * (8 + 4096));
    }
    a.base = mesh_total_;
    for (size_t ch = 0; ch < plan.chunks(); ++ch) {
      const size_t no = plan.ob[ch + 1] - plan.ob[ch], ns = plan.sb[ch + 1] - plan.sb[ch];
      unsigned char *h = ms_.next();  // the copy of chunk ch - 2 has left this pinned buffer
      memcpy(h, plan.own.data() + plan.ob[ch], no * 8);
      streamer_.pack_stored(plan.stg.data() + plan.sb[ch], ns, h + no * 8, h + (no + ns) * 8);
      ms_.wait_for(ms_.used());  // the kernels of chunk ch - 2 have read this device buffer
      ms_.copy((no + ns) * 8 + ns * 4096);
      ms_.record_ready();
      ms_.wait_ready(core_.int_stream);
      const unsigned long long *dk = (const unsigned long long *)ms_.dev();
      a.sorted_keys = dk; a.nblk = (int)no;
      a.st_keys = dk + no; a.st_n = (int)ns; a.st_vox = (const Voxel *)(dk + no + ns);
      mesh_pass<true>(a, update, plan.ob[ch]);
      DR_HIP(hipEventRecord(ms_.used(), core_.int_stream));
    }
    mesh_end(plan.own.size(), plan.stg.size(), plan.chunks());
    if (update) { mu_stats_[1] = plan.own.size(); ledger_.set_rows(plan.own.size()); }
  }
  hipEvent_t mesh_done_ev() {
    if (!mesh_done_) mesh_done_ = core_.own.event();
    return mesh_done_;
  }
  void fetch_mesh(size_t ntri, float *vert, float *cols) {
    DR_HIP(hipMemcpy(vert, mesh_vert_, ntri * 36, hipMemcpyDeviceToHost));
    DR_HIP(hipMemcpy(cols, mesh_cols_, ntri * 36, hipMemcpyDeviceToHost));
  }
  size_t finish_mesh() {
    DR_HIP(hipSetDevice(core_.device));
    DR_HIP(hipEventSynchronize(mesh_done_ev()));
    unsigned long long t = 0;
    DR_HIP(hipMemcpy(&t, mesh_total_, 8, hipMemcpyDeviceToHost));
    if (t > kMeshMaxTriangles) fail(DR_ERR_CAPACITY, "Triangles limit reached! (%llu > %u)", t, kMeshMaxTriangles);
    return (size_t)t;
  }
  FusionCore &core_;
  BlockStreamer &streamer_;
  // mesh extraction state (allocated with the first ExtractMeshAsync)
  static constexpr unsigned kMeshMaxTriangles = 20000000;
  bool mesh_pending_ = false;
  hipEvent_t mesh_done_ = nullptr;
  DeviceBuf<McAxis> mesh_axis_;
  DeviceBuf<unsigned char> mesh_tmp_;  // radix sort / scan scratch
  unsigned long long *mesh_keys_ = nullptr, *mesh_total_ = nullptr;
  unsigned *mesh_counts_ = nullptr, *mesh_offsets_ = nullptr;
  float *mesh_vert_ = nullptr, *mesh_cols_ = nullptr;
  int mesh_scope_ = DRF_MESH_RESIDENT;
  uint64_t mesh_stats_[3] = {0, 0, 0};
  // mesh update (incremental mesh): the bookkeeping is the ledger's (fusion_host.h); the device scratch grows with the scope
  bool mesh_pending_update_ = false;
  MeshUpdateLedger ledger_;
  uint64_t mu_stats_[4] = {0, 0, 0, 0};
  DeviceBuf<unsigned> mu_flags_, mu_pos_;
  DeviceBuf<unsigned long long> mu_sel_, mu_scope_, mu_first_;
  DeviceBuf<int> mu_coords_;
  int *mu_nsel_ = nullptr;
  // map pass staging (opened by the first map-scope extraction that meets a non-empty host store): own keys + staged keys + staged voxels
  BlockStaging ms_;
};

}  // namespace dr
