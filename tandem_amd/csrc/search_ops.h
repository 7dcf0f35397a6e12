// search_ops.h -- the score stage of drf_score_poses / drf_search_frame as a component over FusionCore (the rule: pose_host.h
// score_point / search_candidate; the kernels: search_kernels.h; DESIGN.md §7c "Searching a pose lattice").  PoseScorer owns the
// stage's device scratch and the statistics of the search calls; the engine (dr_fusion.hip) does what needs its call order -- the
// prologue, the frame's intake -- and composes the refinement from its tracking and localisation as they stand.  Included by
// dr_fusion.hip after fusion_core.h.
#pragma once
#include <vector>

#include "fusion_core.h"
#include "map_ops.h"

namespace dr {

class PoseScorer {
 public:
  explicit PoseScorer(FusionCore &core) : core_(core) {}
  uint64_t stats[8] = {};  // drf_search_stats
  void reset() { for (auto &v : stats) v = 0; }

  // candidates per launch: 32 bytes of results each, and with a plain table 96 bytes of poses
  size_t chunk_size() const {
    size_t c = 65536;
    if (const char *e = hook_env("DR_SEARCH_CHUNK")) c = (size_t)std::min(1 << 20, std::max(1, atoi(e)));  // parity hook: chunk seams on small lattices
    return c;
  }
  // The layout for a call whose table holds table_entries poses at a time.  mine: where a host-given depth image goes.
  float *prepare(int step, size_t table_entries) {
    lg_ = locate_grid(core_.o, step);
    total_ = (int)locate_positions(lg_); groups_ = (int)locate_groups(lg_);
    chunk_ = chunk_size();
    const size_t padded = (size_t)groups_ * 512;
    float *mine = nullptr;
    carve(buf_, core_.int_stream, [&](Carver &c) {
      g_ = c.take<double>(padded * 3);
      table_ = c.take<double>(std::max<size_t>(table_entries, 1) * 12);
      out_ = c.take<SearchOut>(chunk_);
      mine = c.take<float>(core_.npix);
      flag_ = c.take<unsigned char>(padded);
    });
    stats[1] = (uint64_t)total_; stats[6] = buf_.capacity();
    return mine;
  }
  // k_search_points over the depth image (device memory), once per call
  void points(const float *depth) {
    const int padded = groups_ * 512;
    if (padded == 0) return;
    hipLaunchKernelGGL(k_search_points, dim3(cdiv(padded, 256)), dim3(256), 0, core_.int_stream, depth, lg_, (double)core_.o.voxel_size, total_, padded, g_, flag_);
    DR_HIP(hipGetLastError());
  }
  // Candidates [0, n) of the lattice L in chunks; cost, counts (4 per candidate) and score may each be null.  A plain table (one pose
  // per candidate) is uploaded chunk by chunk, a search's (n_anchors x n_rot entries) once.
  void score(const SearchLattice &L, const double *table, size_t table_entries, size_t n, const ScoreOpt &so, double *cost, uint32_t *counts, double *score) {
    std::vector<SearchOut> host(std::min(n, chunk_));
    if (!L.plain) DR_HIP(hipMemcpyAsync(table_, table, table_entries * 96, hipMemcpyHostToDevice, core_.int_stream));
    for (size_t first = 0; first < n; first += chunk_) {
      const size_t m = std::min(chunk_, n - first);
      if (L.plain) DR_HIP(hipMemcpyAsync(table_, table + 12 * first, m * 96, hipMemcpyHostToDevice, core_.int_stream));
      hipLaunchKernelGGL(k_search_score, dim3(cdiv((int)m, 4)), dim3(256), 0, core_.int_stream, core_.d, g_, flag_, groups_, table_, L, first, L.plain ? first : (size_t)0,
                         (int)m, so, (double)core_.o.voxel_size, out_);
      DR_HIP(hipGetLastError());
      DR_HIP(hipMemcpyAsync(host.data(), out_, m * sizeof(SearchOut), hipMemcpyDeviceToHost, core_.int_stream));
      DR_HIP(hipStreamSynchronize(core_.int_stream));
      for (size_t i = 0; i < m; ++i) {
        if (cost) cost[first + i] = host[i].cost;
        if (counts) memcpy(counts + 4 * (first + i), host[i].counts, 16);
        if (score) score[first + i] = host[i].score;
      }
      ++stats[3];
      if (first == 0) stats[2] = host[0].counts[0];
    }
    stats[0] = n;
  }

 private:
  FusionCore &core_;
  DeviceBuf<unsigned char> buf_;  // sized by the largest call so far
  LocateGrid lg_{};
  int total_ = 0, groups_ = 0;
  size_t chunk_ = 0;
  double *g_ = nullptr, *table_ = nullptr;
  unsigned char *flag_ = nullptr;
  SearchOut *out_ = nullptr;
};

}  // namespace dr
