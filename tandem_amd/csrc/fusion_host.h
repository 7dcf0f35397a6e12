// fusion_host.h -- the host half of DrFusion's map: block keys, streaming reach bounds, the host block store, the reach balls,
// the planner of the map-scope mesh pass, the rule and planner of a map merge, the rule and planner of a rigid resample, and the
// rule, step and host driver of a map-to-map registration and of a depth frame's localisation in the map.  No device state and no
// HIP header: plain C++17, so that all of it runs in the CPU tests (tests/cpp/fusion_host_check.cpp, tests/cpp/map_merge_check.cpp,
// tests/cpp/map_transform_check.cpp, tests/cpp/map_align_check.cpp, tests/cpp/map_locate_check.cpp).  The engine (dr_fusion.hip) keeps everything that throws or touches the GPU.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/dr_mi355x.h"

namespace dr {

constexpr int kBS = 8;  // voxel block edge (DrFusionOptions::block_size must be 8, as TANDEM sets it)
// ---- block key: 21 bits per axis, biased by 2^20, x in the high bits (ascending key = ascending (x, y, z)).  The one host
// definition; the kernels' pack_key / unpack_key (dr_fusion.hip) stay a device pair on I3 so that the device code is untouched.
constexpr int kKeyBias = 1 << 20;
inline unsigned long long pack_biased(long x, long y, long z) {
  return ((unsigned long long)(x + kKeyBias) << 42) | ((unsigned long long)(y + kKeyBias) << 21) | (unsigned long long)(z + kKeyBias);
}
inline void unpack_key_host(unsigned long long k, int c[3]) {
  c[0] = (int)((k >> 42) & 0x1fffff) - kKeyBias;
  c[1] = (int)((k >> 21) & 0x1fffff) - kKeyBias;
  c[2] = (int)(k & 0x1fffff) - kKeyBias;
}
inline bool pack_key_host(const int c[3], unsigned long long &k) {
  for (int a = 0; a < 3; ++a)
    if (c[a] < -kKeyBias || c[a] >= kKeyBias) return false;
  k = pack_biased(c[0], c[1], c[2]);
  return true;
}
// the store's spatial index: cells of 8^3 blocks, keyed like blocks
inline unsigned long long cell_key(unsigned long long key) {
  int c[3]; unpack_key_host(key, c);
  return pack_biased(c[0] >> 3, c[1] >> 3, c[2] >> 3);  // arithmetic shift = floor division by 8
}

inline float blk_origin_host(int c, float vs) { return (float)(c * kBS) * vs; }
inline double blk_centre_host(int c, float vs) { return ((double)(c * kBS) + 3.5) * vs; }
inline int f2i_host(float f) {  // make_int3(float...) on CUDA: cvt.rzi (saturating, NaN -> 0)
  if (f != f) return 0;
  if (f >= 2147483648.0f) return 2147483647;
  if (f <= -2147483648.0f) return -2147483647 - 1;
  return (int)f;
}
inline void camera_centre(const float *pose16, double p[3]) { p[0] = pose16[3]; p[1] = pose16[7]; p[2] = pose16[11]; }
inline double dist3(const double a[3], const double b[3]) {
  return std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
}

// Farthest a block centre can lie from the camera centre of a scan whose valid depths do not exceed `depth` and still be
// read or written by that scan (DESIGN.md "Streaming voxel blocks" derives each term):
//   allocation DDA  depth*rho + trunc + 4.5*sqrt(3)*vs    (points of the ray up to surf + trunc; block centre within 4.5 sqrt(3) vs)
//                   12.5*sqrt(3)*vs                       (the start block shifted one block back on negative axes)
//   voxel update    depth*rho + trunc + 3.5*sqrt(3)*vs    (updated voxels have vd < sd + trunc)
//   ray-cast        depth*rho + 4.5*sqrt(3)*vs            (samples at cur < max_sensor_depth, trilinear corners within sqrt(3) vs)
// plus one block diagonal (8 sqrt(3) vs) and one voxel of margin.  rho = the largest |((u - cx)/fx, (v - cy)/fy, 1)| over
// the image corners.  Evaluated in double.
inline double corner_rho(const drf_options_t &o) {
  double rho = 0.0;
  for (int k = 0; k < 4; ++k) {
    const double u = (k & 1) ? o.width - 1 : 0, v = (k & 2) ? o.height - 1 : 0;
    const double a = (u - o.cx) / o.fx, b = (v - o.cy) / o.fy;
    rho = std::max(rho, std::sqrt(a * a + b * b + 1.0));
  }
  return rho;
}
inline double stream_reach(const drf_options_t &o, double depth) {
  const double s3 = std::sqrt(3.0), vs = o.voxel_size;
  const double rho = corner_rho(o);
  const double scan = std::max(depth * rho + (double)o.truncation_distance + 4.5 * s3 * vs, 12.5 * s3 * vs);
  return scan + 8.0 * s3 * vs + vs;
}
inline bool stream_options_ok(const drf_options_t &o) {
  auto pos = [](double x) { return std::isfinite(x) && x > 0.0; };
  return pos(o.voxel_size) && pos(o.fx) && pos(o.fy) && std::isfinite(o.cx) && std::isfinite(o.cy) && o.width > 0 && o.height > 0 &&
         pos(o.max_sensor_depth) && std::isfinite(o.truncation_distance) && o.truncation_distance >= 0.0f;
}
inline float streaming_min_radius(const drf_options_t &o) { return (float)stream_reach(o, o.max_sensor_depth); }
// Mesh update: farthest a block ORIGIN can lie from the camera centre of a scan that writes one of its voxels (DESIGN.md
// "Incremental mesh"): the "voxel update" term above taken at the origin (voxels lie within 7 sqrt(3) vs of it) plus the same
// block diagonal and voxel of margin.  Options the bound is not defined for leave k_cull's test alone in charge.
inline float mesh_update_reach2(const drf_options_t &o) {
  if (!stream_options_ok(o)) return INFINITY;
  const double s3 = std::sqrt(3.0), vs = o.voxel_size;
  const double r = (double)o.max_sensor_depth * corner_rho(o) + (double)o.truncation_distance + 7.0 * s3 * vs + 8.0 * s3 * vs + vs;
  const float r2 = (float)(r * r * (1.0 + 1e-5));
  return std::isfinite(r2) ? r2 : INFINITY;
}
// the scan's largest valid depth bounds what it touches (stream_reach); eight branch-free running maxima so that the host
// compiler vectorises the pass over the image
inline float max_valid_depth(const float *depth, size_t npix, float lo, float hi) {
  float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, r = 0.f;
  size_t i = 0;
  for (; i + 8 <= npix; i += 8)
    for (int k = 0; k < 8; ++k) {
      const float z = depth[i + k], v = (z >= lo && z <= hi) ? z : 0.f;
      m[k] = v > m[k] ? v : m[k];
    }
  for (; i < npix; ++i) {
    const float z = depth[i];
    if (z >= lo && z <= hi && z > r) r = z;
  }
  for (int k = 0; k < 8; ++k) r = m[k] > r ? m[k] : r;
  return r;
}

// The host half of the map: block key -> 4 KB, in slabs of 1024 blocks, with a coarse spatial index (cells of 8^3 blocks)
// so that the per-scan "stored blocks within the radius" query visits cells near the camera only.
class HostBlockStore {
 public:
  size_t size() const { return slot_.size(); }
  bool empty() const { return slot_.empty(); }
  void put(unsigned long long key, const void *vox) {
    unsigned s;
    if (!free_.empty()) { s = free_.back(); free_.pop_back(); }
    else {
      s = next_++;
      if ((s >> kSlabShift) >= slabs_.size()) slabs_.emplace_back(new uint8_t[(size_t)4096 << kSlabShift]);
    }
    memcpy(at(s), vox, 4096);
    slot_[key] = s;
    cells_[cell_key(key)].push_back(key);
  }
  const uint8_t *get(unsigned long long key) const { return at(slot_.at(key)); }
  uint8_t *get_mut(unsigned long long key) { return at(slot_.at(key)); }  // the block changed in place (merge_block)
  bool contains(unsigned long long key) const { return slot_.count(key) != 0; }
  void erase(unsigned long long key) {  // the key must be there
    auto it = slot_.find(key);
    free_.push_back(it->second);
    slot_.erase(it);
    auto c = cells_.find(cell_key(key));
    auto &v = c->second;
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i] == key) { v[i] = v.back(); v.pop_back(); break; }
    if (v.empty()) cells_.erase(c);
  }
  template <class F> void for_each(F f) const { for (auto &kv : slot_) f(kv.first, at(kv.second)); }
  std::vector<unsigned long long> sorted_keys() const {
    std::vector<unsigned long long> k; k.reserve(slot_.size());
    for (auto &kv : slot_) k.push_back(kv.first);
    std::sort(k.begin(), k.end());
    return k;
  }
  // keys of the stored blocks whose streaming centre lies within r of p
  void query_sphere(const double p[3], double r, float vs, std::vector<unsigned long long> &out) const {
    if (slot_.empty()) return;
    const double cell = 64.0 * vs;  // 8 blocks
    long lo[3], hi[3];
    double span = 1.0;
    for (int a = 0; a < 3; ++a) {
      lo[a] = (long)std::floor((p[a] - r) / cell) - 1;
      hi[a] = (long)std::floor((p[a] + r) / cell) + 1;
      span *= (double)(hi[a] - lo[a] + 1);
    }
    auto test_cell = [&](const std::vector<unsigned long long> &v) {
      for (unsigned long long k : v) {
        int c[3]; unpack_key_host(k, c);
        const double dx = blk_centre_host(c[0], vs) - p[0], dy = blk_centre_host(c[1], vs) - p[1], dz = blk_centre_host(c[2], vs) - p[2];
        if (dx * dx + dy * dy + dz * dz <= r * r) out.push_back(k);
      }
    };
    if (span > (double)cells_.size()) {  // fewer occupied cells than cells in range: walk the occupied ones
      for (auto &kv : cells_) {
        int c[3]; unpack_key_host(kv.first, c);
        if (c[0] >= lo[0] && c[0] <= hi[0] && c[1] >= lo[1] && c[1] <= hi[1] && c[2] >= lo[2] && c[2] <= hi[2]) test_cell(kv.second);
      }
      return;
    }
    for (long x = lo[0]; x <= hi[0]; ++x)
      for (long y = lo[1]; y <= hi[1]; ++y)
        for (long z = lo[2]; z <= hi[2]; ++z) {
          auto it = cells_.find(pack_biased(x, y, z));
          if (it != cells_.end()) test_cell(it->second);
        }
  }

 private:
  static constexpr int kSlabShift = 10;
  uint8_t *at(unsigned s) const { return slabs_[s >> kSlabShift].get() + (size_t)(s & ((1u << kSlabShift) - 1)) * 4096; }
  std::unordered_map<unsigned long long, unsigned> slot_;
  std::unordered_map<unsigned long long, std::vector<unsigned long long>> cells_;
  std::vector<std::unique_ptr<uint8_t[]>> slabs_;
  std::vector<unsigned> free_;
  unsigned next_ = 0;
};

// Balls (centre, radius) that together hold every block centre of the map: what lets a scan tell on the host that no resident
// block can lie beyond the streaming radius.
class ReachBalls {
 public:
  void reset() { b_.clear(); }
  const std::vector<std::array<double, 4>> &balls() const { return b_; }
  void push(const double p[3], double r) { b_.push_back({p[0], p[1], p[2], r}); }  // kept as given
  // largest |p - centre| + radius: no point of any ball lies farther from p (0 for an empty list)
  double farthest(const double p[3]) const {
    double far = 0.0;
    for (auto &b : b_) far = std::max(far, dist3(p, b.data()) + b[3]);
    return far;
  }
  // a new ball drops the ones it contains, and a long list collapses into one ball around the newest centre
  void add(const double p[3], double r) {
    std::vector<std::array<double, 4>> keep;
    for (auto &b : b_)
      if (dist3(p, b.data()) + b[3] > r) keep.push_back(b);
    keep.push_back({p[0], p[1], p[2], r});
    b_.swap(keep);
    if (b_.size() > 256) b_.assign(1, {p[0], p[1], p[2], farthest(p)});
  }

 private:
  std::vector<std::array<double, 4>> b_;
};

// ---- the render scope (DRF_RENDER_MAP; DESIGN.md §7c "Rendering the whole map"): which stored blocks a ray-cast can read
// Farthest a block centre can lie from the camera centre of a ray-cast and still be read by it: the ray-cast term of
// stream_reach with the same block diagonal and voxel of margin.  Equals stream_reach(o, max_sensor_depth) minus the truncation
// distance whenever the depth term of that bound is the larger one, so at a scan pose no stored block is within it.
inline double render_margin(const drf_options_t &o) {
  const double s3 = std::sqrt(3.0), vs = o.voxel_size;
  return 4.5 * s3 * vs + 8.0 * s3 * vs + vs;
}
inline double render_reach(const drf_options_t &o) { return (double)o.max_sensor_depth * corner_rho(o) + render_margin(o); }
// A finite rigid motion, as far as the reach bounds need it: the twelve entries finite, |R R^T - I| < 1e-3 per entry.  The one
// statement of the rule: the mesh update applies it to a scan's world-to-camera matrix (record_scan_pose), the render scope to
// a render's camera-to-world matrix
inline bool pose_is_rigid(const float *pose16) {
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(pose16[i])) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      const double dot = (double)pose16[4 * i] * pose16[4 * j] + (double)pose16[4 * i + 1] * pose16[4 * j + 1] + (double)pose16[4 * i + 2] * pose16[4 * j + 2];
      if (!(std::fabs(dot - (i == j ? 1.0 : 0.0)) < 1e-3)) return false;
    }
  return true;
}
// Stored blocks a ray-cast from pose16 can read, appended to out (any order): the sphere of render_reach around the camera
// centre, cut by the six half-spaces that hold the pyramid of sample points {z (lx, ly, 1)}, z in [0, D], each widened by
// render_margin.  A superset by construction.  Returns false -- and appends the whole store -- for a pose that is not a
// finite rigid motion, or options the bound is not defined for.
// bz, if given, receives per appended block its camera-frame depth b_z (the third coordinate of R^T (centre - t)), or NaN where the
// cut was not applied: what plan_render_bands slices the selection by.
inline bool select_render_blocks(const HostBlockStore &store, const drf_options_t &o, const float *pose16, std::vector<unsigned long long> &out,
                                 std::vector<double> *bz = nullptr) {
  const double reach = stream_options_ok(o) ? render_reach(o) : HUGE_VAL;
  if (!pose_is_rigid(pose16) || !std::isfinite(reach)) {
    store.for_each([&](unsigned long long k, const uint8_t *) { out.push_back(k); });
    if (bz) bz->resize(bz->size() + store.size(), (double)NAN);
    return false;
  }
  double p[3];
  camera_centre(pose16, p);
  const size_t first = out.size();
  const double m = render_margin(o), vs = o.voxel_size, D = o.max_sensor_depth;
  // R R^T differs from I by < 1e-3 per entry (norm < 3e-3): R scales lengths by at most 1.5e-3, and b = R^T (c - t), which
  // stands in for the inverse below, is off by less than 4e-3 |c - t|.  Where the 8 s + vs of margin covers that, sphere and cut
  // stand as derived; where it does not (depth above ~10^4 voxels) the sphere grows by the error and the cut is not applied.
  if (4e-3 * reach > 8.0 * std::sqrt(3.0) * vs + vs) {
    store.query_sphere(p, reach * (1.0 + 4e-3), o.voxel_size, out);
    if (bz) bz->resize(bz->size() + (out.size() - first), (double)NAN);
    return true;
  }
  store.query_sphere(p, reach, o.voxel_size, out);
  const double lx[2] = {(0.0 - o.cx) / o.fx, ((double)o.width - 1.0 - o.cx) / o.fx};
  const double ly[2] = {(0.0 - o.cy) / o.fy, ((double)o.height - 1.0 - o.cy) / o.fy};
  // unit inward normals of the four side planes through the camera centre: x >= lx0 z, x <= lx1 z, y >= ly0 z, y <= ly1 z
  const double n[4][3] = {{1.0, 0.0, -lx[0]}, {-1.0, 0.0, lx[1]}, {0.0, 1.0, -ly[0]}, {0.0, -1.0, ly[1]}};
  size_t keep = first;
  for (size_t i = first; i < out.size(); ++i) {
    int c[3]; unpack_key_host(out[i], c);
    const double w[3] = {blk_centre_host(c[0], o.voxel_size) - p[0], blk_centre_host(c[1], o.voxel_size) - p[1], blk_centre_host(c[2], o.voxel_size) - p[2]};
    double b[3];
    for (int a = 0; a < 3; ++a) b[a] = (double)pose16[a] * w[0] + (double)pose16[4 + a] * w[1] + (double)pose16[8 + a] * w[2];
    bool in = b[2] >= -m && D - b[2] >= -m;
    for (int k = 0; k < 4 && in; ++k) {
      const double len = std::sqrt(n[k][0] * n[k][0] + n[k][1] * n[k][1] + n[k][2] * n[k][2]);
      in = (n[k][0] * b[0] + n[k][1] * b[1] + n[k][2] * b[2]) / len >= -m;
    }
    if (in) {
      out[keep++] = out[i];
      if (bz) bz->push_back(b[2]);
    }
  }
  out.resize(keep);
  return true;
}
// What one RenderAsync stages: the union over its poses, ascending and de-duplicated; whole = poses that selected the whole store
struct RenderStagePlan {
  std::vector<unsigned long long> keys;
  int whole = 0;
};
inline RenderStagePlan plan_render_stage(const HostBlockStore &store, const drf_options_t &o, const float *const *poses16, int n) {
  RenderStagePlan p;
  if (store.empty()) return p;
  for (int i = 0; i < n; ++i)
    if (!select_render_blocks(store, o, poses16[i], p.keys)) ++p.whole;
  std::sort(p.keys.begin(), p.keys.end());
  p.keys.erase(std::unique(p.keys.begin(), p.keys.end()), p.keys.end());
  return p;
}
// the capacity decision of a RenderAsync: the union is what is staged, however many poses share a block
inline bool render_stage_fits(const RenderStagePlan &p, size_t capacity_blocks) { return p.keys.size() <= capacity_blocks; }
// ---- the locate scope (DRF_LOCATE_MAP; DESIGN.md §7c "Locating in the whole map"): which stored blocks one evaluation of
// drf_locate_* at a pose can read, and how long a staging of them serves the poses that follow.
// A sample is a point R (z (lx, ly, 1)) + t of the pixel pyramid with z <= max_sensor_depth; its eight corners floor(q) + {0, 1}^3
// lie within sqrt(3) voxels of it and a block's farthest voxel 3.5 sqrt(3) voxels from the block's centre: every block read has
// its centre within 4.5 sqrt(3) vs of a sample point -- the ray-cast's own term.  select_render_blocks widens pyramid and sphere by
// render_margin = 4.5 sqrt(3) vs + 8 sqrt(3) vs + vs, so its selection at the pose is a superset with 8 sqrt(3) vs + vs to spare.
// Of that spare part, a pose that is rigid only within pose_is_rigid's 1e-3 takes up to 4e-3 render_reach (select_render_blocks
// says how), and the vs covers the pose's rounding from the loop's doubles to the floats these functions take (below).  What is
// left is the slack: how far every sample point may move while the selection still holds each block read.  It is 0 where
// select_render_blocks drops the cut (then every moved pose stages again).
inline double locate_stage_slack(const drf_options_t &o) {
  if (!stream_options_ok(o)) return 0.0;
  const double s = 8.0 * std::sqrt(3.0) * (double)o.voxel_size - 4e-3 * render_reach(o);
  return s > 0.0 && std::isfinite(s) ? s : 0.0;
}
// An upper bound on how far any sample point moves between two poses: |(RA - RB) g + tA - tB| <= |tA - tB| + ||RA - RB||_2 |g|,
// |g| <= max_sensor_depth * corner_rho, and the Frobenius norm bounds the spectral one.  Symmetric, and 0 for A = B.
inline double locate_pose_drift(const drf_options_t &o, const float *poseA16, const float *poseB16) {
  double t2 = 0.0, r2 = 0.0;
  for (int i = 0; i < 3; ++i) {
    const double dt = (double)poseA16[4 * i + 3] - (double)poseB16[4 * i + 3];
    t2 += dt * dt;
    for (int j = 0; j < 3; ++j) {
      const double dr = (double)poseA16[4 * i + j] - (double)poseB16[4 * i + j];
      r2 += dr * dr;
    }
  }
  return std::sqrt(t2) + std::sqrt(r2) * (double)o.max_sensor_depth * corner_rho(o);
}
// The staging selected at pose A serves an evaluation at pose B iff this holds (NaN: it does not).
inline bool locate_stage_serves(const drf_options_t &o, const float *poseA16, const float *poseB16, double slack) {
  return locate_pose_drift(o, poseA16, poseB16) <= slack;
}
// What one evaluation stages: the render's selection at the pose, ascending (select_render_blocks appends each block once).
inline std::vector<unsigned long long> select_locate_blocks(const HostBlockStore &store, const drf_options_t &o, const float *pose16) {
  std::vector<unsigned long long> keys;
  if (store.empty()) return keys;
  select_render_blocks(store, o, pose16, keys);
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  return keys;
}
// ---- depth bands (drf_set_render_bands; DESIGN.md §7c "Rendering beyond the staging"): a union that exceeds the staging is
// ray-cast in passes over consecutive slabs of camera-frame depth [z_j, z_j+1), common to all poses of the call.  A loop sample
// of pass j lies at depth cur in [z_j, z_j+1), its final colour sample in [cur - trunc, cur + vs), and a sample at depth z reads
// only blocks with |b_z - z| <= render_margin.  So of a pose's selection pass j needs the blocks with
//   b_z + trunc + margin >= z_j   and   b_z - margin - vs < z_j+1
// (a superset by construction; a block whose pose did not take the cut belongs to every pass).
struct RenderBandPlan {
  bool ok = false;                                     // false: no plan within capacity and max_passes
  std::vector<float> z;                                // P + 1 boundaries, 0 = z[0] < ... < z[P] = max_sensor_depth (fp32: the kernels compare cur against them)
  std::vector<std::vector<unsigned long long>> keys;   // per pass: ascending, de-duplicated
};
// Greedy sweep: each pass reaches as far as the union over the poses stays within `capacity`.  A further block enters at
// z = b_z - margin - vs, so a pass ends at the entry depth of the first block that does not fit (rounded down to fp32: still
// short of that block).  A pass that cannot advance past its start, or a plan of more than max_passes passes, fails.  A pass
// takes every block up to its capacity, so none stages nothing unless nothing is staged at all (one empty pass).
inline RenderBandPlan plan_render_bands(const HostBlockStore &store, const drf_options_t &o, const float *const *poses16, int n, size_t capacity,
                                        int max_passes) {
  struct Item { double enter, leave; unsigned long long key; };
  std::vector<Item> items;
  {
    std::vector<unsigned long long> k;
    std::vector<double> bz;
    const double m = render_margin(o), vs = o.voxel_size, tr = o.truncation_distance;
    for (int i = 0; i < n && !store.empty(); ++i) {
      k.clear(); bz.clear();
      select_render_blocks(store, o, poses16[i], k, &bz);
      for (size_t j = 0; j < k.size(); ++j)
        items.push_back(std::isnan(bz[j]) ? Item{-HUGE_VAL, HUGE_VAL, k[j]} : Item{bz[j] - m - vs, bz[j] + tr + m, k[j]});
    }
  }
  std::sort(items.begin(), items.end(), [](const Item &a, const Item &b) { return a.enter != b.enter ? a.enter < b.enter : a.key < b.key; });
  RenderBandPlan p;
  const float D = o.max_sensor_depth;
  if (!(D > 0.0f) || !std::isfinite(D)) return p;
  float zs = 0.0f;
  p.z.push_back(zs);
  for (;;) {
    if ((int)p.keys.size() >= max_passes) return RenderBandPlan();
    float ze = D;
    std::unordered_set<unsigned long long> in;
    for (const Item &it : items) {
      if (it.leave < (double)zs || in.count(it.key)) continue;
      if (in.size() < capacity) { in.insert(it.key); continue; }
      // the first block that does not fit: the pass ends where it enters
      if (!(it.enter > (double)zs)) return RenderBandPlan();
      ze = (float)it.enter;
      if ((double)ze > it.enter) ze = std::nextafterf(ze, -INFINITY);
      if (!(ze > zs)) return RenderBandPlan();
      break;
    }
    std::vector<unsigned long long> keys;
    for (const Item &it : items)
      if (it.leave >= (double)zs && it.enter < (double)ze) keys.push_back(it.key);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    p.keys.push_back(std::move(keys));
    p.z.push_back(ze);
    if (ze >= D) break;
    zs = ze;
  }
  p.ok = true;
  return p;
}
// Blocks the last scan's eviction chain gathered (not in the store until folded) lie beyond radius + 8 vs of that scan's
// camera centre p.  A render from q with |q - p| + render_reach <= radius + 8 vs cannot read one: it need not wait for the scan.
inline bool render_needs_fold(const drf_options_t &o, const float *pose16, const double scan_centre[3], double radius) {
  if (!pose_is_rigid(pose16) || !stream_options_ok(o)) return true;
  double q[3];
  camera_centre(pose16, q);
  return !(dist3(q, scan_centre) + render_reach(o) <= radius + (double)kBS * o.voxel_size);
}

// ---- the map-scope mesh pass (DESIGN.md §7c "Meshing the whole map")
// Blocks that can own cells of the lattice (lower, n cells per axis): floor(mc / 8) between those of the first and last cell
// per axis (k_mc_axes' expression restated on the host), widened by one block -- the kernel finds the exact range, this only
// skips the rest.
struct BlockRange {
  int lo[3], hi[3];
  bool holds(unsigned long long key) const {
    int c[3]; unpack_key_host(key, c);
    return c[0] >= lo[0] && c[0] <= hi[0] && c[1] >= lo[1] && c[1] <= hi[1] && c[2] >= lo[2] && c[2] <= hi[2];
  }
};
inline BlockRange lattice_block_range(const float *lower, const int n[3], float vs) {
  BlockRange r;
  for (int k = 0; k < 3; ++k) {
    int m[2];
    for (int e = 0; e < 2; ++e) {
      const float pa = (float)(e ? n[k] - 1 : 0) * vs + lower[k];
      m[e] = f2i_host(pa / vs + (float)((pa > 0) - (pa < 0)) * 0.5f);
    }
    auto fdiv = [](int v) { return v < 0 ? (v - kBS + 1) / kBS : v / kBS; };
    r.lo[k] = fdiv(std::min(m[0], m[1])) - 1;
    r.hi[k] = fdiv(std::max(m[0], m[1])) + 1;
  }
  return r;
}
// The global order of a map: ascending key over resident (res) and stored (sto) blocks, both sorted; f(key, stored) for those
// within the range.
template <class F>
inline void for_each_in_range(const std::vector<unsigned long long> &res, const std::vector<unsigned long long> &sto, const BlockRange &range, F f) {
  for (size_t i = 0, j = 0; i < res.size() || j < sto.size();) {
    const bool stored = j < sto.size() && (i >= res.size() || sto[j] < res[i]);
    const unsigned long long key = stored ? sto[j++] : res[i++];
    if (range.holds(key)) f(key, stored);
  }
}
// The merged list cut into chunks: chunk c meshes own[ob[c], ob[c+1]) (global order) and stages stg[sb[c], sb[c+1]) (ascending):
// its own stored blocks and every stored block among the 26 neighbours of its blocks.
struct MeshPlan {
  std::vector<unsigned long long> own, stg;
  std::vector<size_t> ob{0}, sb{0};
  size_t chunks() const { return ob.size() - 1; }
};
// Greedy: a chunk closes when it owns own_cap blocks or the next block would take its staged set beyond stage_cap (>= 27, so
// that one block's neighbourhood always fits).  sto = store.sorted_keys(); picked, if given, is a subsequence of the merged
// in-range list and only its blocks are planned.
inline MeshPlan plan_mesh_chunks(const std::vector<unsigned long long> &res, const std::vector<unsigned long long> &sto, const HostBlockStore &store,
                                 const BlockRange &range, size_t own_cap, size_t stage_cap, const std::vector<unsigned long long> *picked = nullptr) {
  MeshPlan p;
  std::vector<unsigned long long> cur;
  std::unordered_set<unsigned long long> in_cur;
  auto close_chunk = [&]() {
    std::sort(cur.begin(), cur.end());
    p.stg.insert(p.stg.end(), cur.begin(), cur.end());
    p.ob.push_back(p.own.size()); p.sb.push_back(p.stg.size());
    cur.clear(); in_cur.clear();
  };
  size_t pk = 0;
  unsigned long long need[27];
  for_each_in_range(res, sto, range, [&](unsigned long long key, bool stored) {
    if (picked) {
      if (pk == picked->size() || (*picked)[pk] != key) return;
      ++pk;
    }
    int c[3]; unpack_key_host(key, c);
    int nn = 0, fresh = 0;  // stored blocks this block reads / those not staged for the chunk yet
    for (int k = 0; k < 27; ++k) {
      const int q[3] = {c[0] + k / 9 - 1, c[1] + (k / 3) % 3 - 1, c[2] + k % 3 - 1};
      unsigned long long qk;
      if (k == 13 ? stored : (pack_key_host(q, qk) && store.contains(qk))) {
        need[nn++] = k == 13 ? key : qk;
        fresh += !in_cur.count(need[nn - 1]);
      }
    }
    if (p.own.size() - p.ob.back() == own_cap || cur.size() + fresh > stage_cap) close_chunk();
    p.own.push_back(key);
    for (int k = 0; k < nn; ++k)
      if (in_cur.insert(need[k]).second) cur.push_back(need[k]);
  });
  if (p.own.size() > p.ob.back()) close_chunk();
  return p;
}

// ---- merging a map file into the map (drf_merge_map; DESIGN.md §7c "Merging a map file")
// The rule, stated once for the host store and the kernel (k_map_merge compiles this very function for the device).  Blocks: the
// merged map holds the union of the two block sets; a file block whose key the map lacks is placed verbatim, one whose key it
// holds is combined with the map's block voxel by voxel, index by index.  Voxels: a = the map's, b = the file's,
// W = (unsigned char)max_sdf_weight, fp32 without contraction:
//   1  b.weight == 0:          a stays as it is, all 8 bytes
//   2  else a.weight == 0:     a.sdf = b.sdf, a.colour = b.colour, a.weight = min(b.weight, W)
//   3  else, wa = (float)a.weight, wb = (float)b.weight:
//        each colour channel  (unsigned char)(((float)a.c * wa + (float)b.c * wb) / (wa + wb))
//        a.sdf = (a.sdf * wa + b.sdf * wb) / (wa + wb)
//        a.weight = min((int)a.weight + (int)b.weight, (int)W)
// Case 3 is Voxel::Combine (tsdfvh/voxel.h) with any second weight, except that the weight sum is formed in int: two unsigned
// chars would wrap above 255, which integration (always + 1, clamped) never reaches and a merge does.  Cases 1 and 2 keep 0/0
// out of the map and make an absent block and an allocated, never updated one behave alike.
// A voxel here is its two little-endian words: [0] the sdf's bits, [1] b | g << 8 | r << 16 | weight << 24.  Returns the case.
#if defined(__HIPCC__)
#define DR_HOST_DEVICE __host__ __device__
#else
#define DR_HOST_DEVICE
#endif
DR_HOST_DEVICE inline int merge_voxel(uint32_t a[2], const uint32_t b[2], unsigned char W) {
  const unsigned wai = a[1] >> 24, wbi = b[1] >> 24;
  if (wbi == 0) return 1;
  if (wai == 0) {
    a[0] = b[0];
    a[1] = (b[1] & 0xffffffu) | ((wbi < W ? wbi : (unsigned)W) << 24);
    return 2;
  }
  const float wa = (float)wai, wb = (float)wbi, den = wa + wb;
  unsigned cw = 0;
  for (int k = 0; k < 24; k += 8) {
    const float ca = (float)((a[1] >> k) & 255u), cb = (float)((b[1] >> k) & 255u);
    // integer-valued operands below 2^24: products and sum exact, the quotient a correctly rounded value in [0, 255]
    cw |= (unsigned)(unsigned char)(int)((ca * wa + cb * wb) / den) << k;
  }
  float sa, sb;
  memcpy(&sa, &a[0], 4); memcpy(&sb, &b[0], 4);
  const float s = (sa * wa + sb * wb) / den;
  memcpy(&a[0], &s, 4);
  const unsigned ws = wai + wbi;
  a[1] = cw | ((ws < W ? ws : (unsigned)W) << 24);
  return 3;
}
// 512 voxels of src merged into dst; counts[0] += voxels of case 2 (taken verbatim), counts[1] += voxels of case 3 (averaged)
inline void merge_block(uint8_t *dst4096, const uint8_t *src4096, unsigned char W, uint64_t counts[2]) {
  for (int v = 0; v < kBS * kBS * kBS; ++v) {
    uint32_t a[2], b[2];
    memcpy(a, dst4096 + 8 * v, 8); memcpy(b, src4096 + 8 * v, 8);
    const int c = merge_voxel(a, b, W);
    if (c == 1) continue;
    memcpy(dst4096 + 8 * v, a, 8);
    ++counts[c - 2];
  }
}
// Every file block classified against the map in one walk over three ascending key lists: the resident keys with their pool
// slots (the sorted pairs drf_save_map works from), the host store's keys, the file's keys.  ADDED = the map lacks the key,
// RESIDENT = combined in its pool slot, STORED = combined in the host store.  The file is cut into chunks of `chunk` blocks (one
// pinned buffer each); per class the lists below are in file order, chunk c owning [xb[c], xb[c + 1]), and *_src is the block's
// position within its chunk's buffer -- what k_map_merge and k_in_place_at index by.
struct MergePlan {
  size_t chunk = 1;
  std::vector<int> res_src, res_slot;
  std::vector<int> add_src;
  std::vector<unsigned long long> add_key;
  std::vector<int> sto_src;
  std::vector<unsigned long long> sto_key;
  std::vector<size_t> rb{0}, ab{0}, sb{0};
  size_t chunks() const { return rb.size() - 1; }
};
inline MergePlan plan_merge(const std::vector<unsigned long long> &res, const std::vector<int> &res_slot, const std::vector<unsigned long long> &sto,
                            const std::vector<unsigned long long> &file, size_t chunk) {
  MergePlan p;
  p.chunk = std::max<size_t>(chunk, 1);
  size_t i = 0, j = 0;
  for (size_t f = 0; f < file.size(); ++f) {
    const unsigned long long key = file[f];
    const int at = (int)(f % p.chunk);
    while (i < res.size() && res[i] < key) ++i;
    while (j < sto.size() && sto[j] < key) ++j;
    if (i < res.size() && res[i] == key) { p.res_src.push_back(at); p.res_slot.push_back(res_slot[i]); }
    else if (j < sto.size() && sto[j] == key) { p.sto_src.push_back(at); p.sto_key.push_back(key); }
    else { p.add_src.push_back(at); p.add_key.push_back(key); }
    if (at + 1 == (int)p.chunk || f + 1 == file.size()) { p.rb.push_back(p.res_src.size()); p.ab.push_back(p.add_src.size()); p.sb.push_back(p.sto_src.size()); }
  }
  return p;
}

// ---- moving a map file into another world frame (drf_transform_map; DESIGN.md §7c "Moving a map into another frame")
// T16 maps file-world to engine-world, p_engine = R p_file + t; both maps live on the lattice g * voxel_size.  The motion in
// lattice units, once, in double: R[3 i + j] = (double)T16[4 i + j], tv[j] = (double)T16[4 j + 3] / (double)voxel_size.
struct MapMotion {
  double R[9];
  double tv[3];
};
inline MapMotion map_motion(const float *T16, float voxel_size) {
  MapMotion m;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) m.R[3 * i + j] = (double)T16[4 * i + j];
    m.tv[i] = (double)T16[4 * i + 3] / (double)voxel_size;
  }
  return m;
}
inline double det3(const double R[9]) {
  return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}
// What drf_transform_map accepts: sixteen finite entries, a last row that is exactly 0 0 0 1, pose_is_rigid, det R > 0.  Returns
// null, or what is wrong.
inline const char *transform_pose_fault(const float *T16) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(T16[i])) return "has a non-finite entry";
  if (T16[12] != 0.0f || T16[13] != 0.0f || T16[14] != 0.0f || T16[15] != 1.0f) return "has a last row other than 0 0 0 1";
  if (!pose_is_rigid(T16)) return "is not a rigid motion (R R^T differs from I: scale is not handled)";
  double R[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (double)T16[4 * i + j];
  if (!(det3(R) > 0.0)) return "is a reflection (det R <= 0)";
  return nullptr;
}
// The rule, stated once for the host and the kernel (k_map_transform compiles this very function for the device): the voxel of the
// destination lattice point g.  In double, without contraction: d = g - tv, u = R^T d as (R[0][k] d0 + R[1][k] d1) + R[2][k] d2,
// b = floor(u), f = (float)(u - b).  Corner c = 4 cx + 2 cy + cz has the fp32 weight w_c = (a_x(cx) * a_y(cy)) * a_z(cz) with
// a_k(0) = 1.0f - f_k, a_k(1) = f_k; it is USED iff w_c != 0 and then reads the source voxel at lattice point b + (cx, cy, cz)
// through fetch(x, y, z, v[2]) (an absent block, or one outside the key range: weight 0).  If any used corner has weight 0 the
// result is 8 zero bytes.  Otherwise sdf and each colour channel are the sums of w_c * value over the used corners in ascending c
// (fp32, the first used term initialises the sum), a colour channel stored as (unsigned char)min(sum + 0.5f, 255.0f), and the
// weight is the smallest of the used corners' weights.  A partly weighted neighbourhood is refused, not renormalised: DESIGN.md
// says why.  A voxel is its two little-endian words, as for merge_voxel.
// Returns 0: no used corner is weighted (empty), 1: written with weight > 0, 2: refused (some used corners weighted, some not).
template <class Fetch>
DR_HOST_DEVICE inline int transform_voxel(const MapMotion &m, int gx, int gy, int gz, Fetch &&fetch, uint32_t out[2]) {
  out[0] = 0; out[1] = 0;
  const double d0 = (double)gx - m.tv[0], d1 = (double)gy - m.tv[1], d2 = (double)gz - m.tv[2];
  int b[3];
  float f[3];
  for (int k = 0; k < 3; ++k) {
    const double u = (m.R[k] * d0 + m.R[3 + k] * d1) + m.R[6 + k] * d2;
    if (!(u > -1073741824.0 && u < 1073741824.0)) return 0;  // far outside the key range (2^23 voxels): every corner is absent
    const double fl = floor(u);
    b[k] = (int)fl;
    f[k] = (float)(u - fl);
  }
  const float ax[2] = {1.0f - f[0], f[0]}, ay[2] = {1.0f - f[1], f[1]}, az[2] = {1.0f - f[2], f[2]};
  bool first = true, any = false, all = true;
  float s = 0.0f, ch[3] = {0.0f, 0.0f, 0.0f};
  unsigned wmin = 255u;
  for (int c = 0; c < 8; ++c) {
    const int cx = c >> 2, cy = (c >> 1) & 1, cz = c & 1;
    const float w = (ax[cx] * ay[cy]) * az[cz];
    if (w == 0.0f) continue;
    uint32_t v[2];
    fetch(b[0] + cx, b[1] + cy, b[2] + cz, v);
    const unsigned wt = v[1] >> 24;
    if (wt == 0u) { all = false; continue; }
    any = true;
    float sc;
    memcpy(&sc, &v[0], 4);
    const float ts = w * sc, t0 = w * (float)(v[1] & 255u), t1 = w * (float)((v[1] >> 8) & 255u), t2 = w * (float)((v[1] >> 16) & 255u);
    if (first) { s = ts; ch[0] = t0; ch[1] = t1; ch[2] = t2; first = false; }
    else { s = s + ts; ch[0] = ch[0] + t0; ch[1] = ch[1] + t1; ch[2] = ch[2] + t2; }
    wmin = wt < wmin ? wt : wmin;
  }
  if (!all) return any ? 2 : 0;
  unsigned word = wmin << 24;
  for (int k = 0; k < 3; ++k) {
    const float r = ch[k] + 0.5f;
    word |= (unsigned)(unsigned char)(int)(r < 255.0f ? r : 255.0f) << (8 * k);
  }
  memcpy(&out[0], &s, 4);
  out[1] = word;
  return 1;
}
// The destination block at block coordinates blk: its 512 voxels to dst4096 (index x*64 + y*8 + z).  counts[0] += voxels
// written with weight > 0, counts[1] += voxels refused.  Returns whether the block holds a weighted voxel (= is written).
template <class Fetch>
inline bool transform_block(const MapMotion &m, const int blk[3], Fetch &&fetch, uint8_t *dst4096, uint64_t counts[2]) {
  bool keep = false;
  for (int v = 0; v < kBS * kBS * kBS; ++v) {
    uint32_t o[2];
    const int r = transform_voxel(m, blk[0] * kBS + (v >> 6), blk[1] * kBS + ((v >> 3) & 7), blk[2] * kBS + (v & 7), fetch, o);
    memcpy(dst4096 + 8 * v, o, 8);
    if (r == 1) { keep = true; ++counts[0]; }
    if (r == 2) ++counts[1];
  }
  return keep;
}
// Candidate destination blocks, ascending and unique: a superset of every block that can hold a voxel with a used corner inside a
// source block.  Such a voxel g has u(g) = R^T (g - tv) within one voxel of a lattice point of the block, so u lies in the box
// [8 b - 1, 8 b + 8]^3 and g = A u + tv in the image of that box, A the inverse of R^T (R itself for an orthogonal R; the inverse is
// taken so that the argument holds for every R that pose_is_rigid lets through).  The image is convex: it lies within the
// axis-aligned bounds of its eight corners, which are widened by one voxel for the rounding of either direction.  Blocks outside
// the key range are left out and *in_range, if given, says whether there were any.  (DESIGN.md §7c writes the argument out.)
inline std::vector<unsigned long long> plan_transform(const std::vector<unsigned long long> &src_keys, const MapMotion &m, bool *in_range = nullptr) {
  std::vector<unsigned long long> out;
  if (in_range) *in_range = true;
  const double *R = m.R;
  const double det = det3(R);
  // A = (R^T)^-1 = cofactor matrix of R over det
  const double A[9] = {(R[4] * R[8] - R[5] * R[7]) / det, (R[5] * R[6] - R[3] * R[8]) / det, (R[3] * R[7] - R[4] * R[6]) / det,
                       (R[2] * R[7] - R[1] * R[8]) / det, (R[0] * R[8] - R[2] * R[6]) / det, (R[1] * R[6] - R[0] * R[7]) / det,
                       (R[1] * R[5] - R[2] * R[4]) / det, (R[2] * R[3] - R[0] * R[5]) / det, (R[0] * R[4] - R[1] * R[3]) / det};
  auto fdiv = [](long v) { return v < 0 ? (v - kBS + 1) / kBS : v / kBS; };
  for (unsigned long long key : src_keys) {
    int c[3]; unpack_key_host(key, c);
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int e = 0; e < 8; ++e) {
      const double u[3] = {(double)(c[0] * kBS) + ((e & 4) ? 8.0 : -1.0), (double)(c[1] * kBS) + ((e & 2) ? 8.0 : -1.0), (double)(c[2] * kBS) + ((e & 1) ? 8.0 : -1.0)};
      for (int a = 0; a < 3; ++a) {
        const double g = (A[3 * a] * u[0] + A[3 * a + 1] * u[1]) + A[3 * a + 2] * u[2] + m.tv[a];
        lo[a] = std::min(lo[a], g); hi[a] = std::max(hi[a], g);
      }
    }
    long bl[3], bh[3];
    bool ok = true;
    for (int a = 0; a < 3; ++a) {
      if (!(lo[a] > -1e15 && hi[a] < 1e15)) { ok = false; break; }  // (long) of it would not be defined
      bl[a] = fdiv((long)std::floor(lo[a]) - 1); bh[a] = fdiv((long)std::ceil(hi[a]) + 1);
      if (bl[a] < -kKeyBias || bh[a] >= kKeyBias) ok = false;
    }
    if (!ok) {
      if (in_range) *in_range = false;
      continue;
    }
    for (long x = bl[0]; x <= bh[0]; ++x)
      for (long y = bl[1]; y <= bh[1]; ++y)
        for (long z = bl[2]; z <= bh[2]; ++z) out.push_back(pack_biased(x, y, z));
  }
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
  return out;
}
// The source as the host holds it for transform_voxel's fetch: key -> block index into voxels (n x 4096 bytes)
struct HostMapSource {
  std::unordered_map<unsigned long long, size_t> at;
  const uint8_t *vox = nullptr;
  HostMapSource(const std::vector<unsigned long long> &keys, const uint8_t *voxels) : vox(voxels) {
    at.reserve(keys.size());
    for (size_t i = 0; i < keys.size(); ++i) at[keys[i]] = i;
  }
  void operator()(int x, int y, int z, uint32_t v[2]) const {
    v[0] = 0; v[1] = 0;
    const int c[3] = {x >> 3, y >> 3, z >> 3};  // arithmetic shift = floor division by 8
    unsigned long long k;
    if (!pack_key_host(c, k)) return;
    auto it = at.find(k);
    if (it != at.end()) memcpy(v, vox + it->second * 4096 + (size_t)(((x & 7) << 6) | ((y & 7) << 3) | (z & 7)) * 8, 8);
  }
};

// ---- registering two map files (drf_align_system / drf_align_map; DESIGN.md §7c "Registering two maps")
// T maps src-world to ref-world, p_ref = R p_src + t, held as a MapMotion in double: q = R g + tv takes a source lattice point to
// reference lattice units.  The cost is the sum over the source's samples of rho(r), r = (phi_ref(q) - s_src) / voxel_size, phi_ref
// the trilinear interpolation of the reference's sdf, rho Huber's function; one evaluation yields the Gauss-Newton system of it:
// sums[0..20] = the upper triangle of H = sum w J J^T row-major, sums[21..26] = b = sum w J r, sums[27] = sum w r r.
// The rule is stated once, here (the header of the C ABI restates it for users): align_voxel is compiled by g++ for the CPU tests
// and by hipcc for k_map_align, both without contraction, and uses + - * / and floor only.
#if defined(__HIPCC__)
#define DR_UNROLL _Pragma("unroll")
#else
#define DR_UNROLL
#endif
struct AlignOpt {  // drf_align_options_t with its defaults resolved
  int max_iters, min_weight;
  float band, huber;
  double eps_rot, eps_trans, min_valid;
};
// null: all defaults.  Returns null, or which option is negative or not finite
inline const char *align_options(const drf_align_options_t *opt, float voxel_size, AlignOpt &o) {
  static const drf_align_options_t zero = {0, 0, 0.0f, 0.0f, 0.0, 0.0, 0.0};
  const drf_align_options_t &u = opt ? *opt : zero;
  if (u.max_iters < 0) return "max_iters";
  if (u.min_weight < 0) return "min_weight";
  if (!(u.band >= 0.0f) || !std::isfinite(u.band)) return "band";
  if (!(u.huber >= 0.0f) || !std::isfinite(u.huber)) return "huber";
  if (!(u.eps_rot >= 0.0) || !std::isfinite(u.eps_rot)) return "eps_rot";
  if (!(u.eps_trans >= 0.0) || !std::isfinite(u.eps_trans)) return "eps_trans";
  if (!(u.min_valid >= 0.0) || !std::isfinite(u.min_valid)) return "min_valid";
  o.max_iters = u.max_iters ? u.max_iters : 30;
  o.min_weight = u.min_weight ? u.min_weight : 1;
  o.band = u.band != 0.0f ? u.band : 2.0f * voxel_size;
  o.huber = u.huber != 0.0f ? u.huber : 1.0f;
  o.eps_rot = u.eps_rot != 0.0 ? u.eps_rot : 1e-7;
  o.eps_trans = u.eps_trans != 0.0 ? u.eps_trans : 1e-5;
  o.min_valid = u.min_valid != 0.0 ? u.min_valid : 0.25;
  return nullptr;
}
// what a kernel launch and a host evaluation share besides the pose
struct AlignEval {
  MapMotion m;
  double c[3];        // the centre at this pose: R c_src + tv
  double huber, vs;   // (double)huber, (double)voxel_size
  float band;
  int min_weight;
};
// c_src[k] = 4 (min_k + max_k + 1) over the source's block coordinates: the middle of its lattice box, an integer (0 if empty)
inline void align_centre_src(const std::vector<unsigned long long> &src_keys, double c_src[3]) {
  c_src[0] = c_src[1] = c_src[2] = 0.0;
  if (src_keys.empty()) return;
  int lo[3] = {kKeyBias, kKeyBias, kKeyBias}, hi[3] = {-kKeyBias - 1, -kKeyBias - 1, -kKeyBias - 1};
  for (unsigned long long k : src_keys) {
    int c[3]; unpack_key_host(k, c);
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], c[a]); hi[a] = std::max(hi[a], c[a]); }
  }
  for (int a = 0; a < 3; ++a) c_src[a] = (double)(4L * ((long)lo[a] + (long)hi[a] + 1L));
}
inline AlignEval align_eval(const MapMotion &m, const double c_src[3], const AlignOpt &o, float voxel_size) {
  AlignEval e;
  e.m = m;
  for (int k = 0; k < 3; ++k) e.c[k] = ((m.R[3 * k] * c_src[0] + m.R[3 * k + 1] * c_src[1]) + m.R[3 * k + 2] * c_src[2]) + m.tv[k];
  e.huber = (double)o.huber; e.vs = (double)voxel_size;
  e.band = o.band; e.min_weight = o.min_weight;
  return e;
}
// is the source voxel (its two words) a sample?
DR_HOST_DEVICE inline bool align_is_sample(const uint32_t v[2], const AlignEval &e) {
  float s;
  memcpy(&s, &v[0], 4);
  return (int)(v[1] >> 24) >= e.min_weight && (s < 0.0f ? -s : s) <= e.band;
}
// The terms of one valid sample at q with residual r and gradient n (both in voxels): J = ((q - c) x n, n), Huber's weight, the 28
// sums.  What align_point and track_point (below) end in: the same operations in the same order for all three callers.
DR_HOST_DEVICE inline void align_accumulate(const AlignEval &e, double r, double n0, double n1, double n2, const double q[3], double acc[28]) {
  const double x0 = q[0] - e.c[0], x1 = q[1] - e.c[1], x2 = q[2] - e.c[2];
  const double J[6] = {x1 * n2 - x2 * n1, x2 * n0 - x0 * n2, x0 * n1 - x1 * n0, n0, n1, n2};
  const double a = r < 0.0 ? -r : r;
  const double w = a <= e.huber ? 1.0 : e.huber / a;
  int idx = 0;
  DR_UNROLL
  for (int i = 0; i < 6; ++i) {
    const double wj = w * J[i];
    DR_UNROLL
    for (int j = i; j < 6; ++j) { acc[idx] = acc[idx] + wj * J[j]; ++idx; }
    acc[21 + i] = acc[21 + i] + wj * r;
  }
  acc[27] = acc[27] + (w * r) * r;
}
// One sample at the point g (lattice units of the moving frame, three doubles) with sdf s_src: the body that the registration
// (align_voxel: g a source lattice point) and the localisation (locate_group: g a depth pixel's point, s_src = 0) share.  Reads the
// eight reference voxels through fetch(x, y, z, v[2]) (an absent block: weight 0); returns 0 if one of them is not observed (or q
// lies outside the key range), and otherwise adds the sample's terms to acc[28] and returns 1.  BAND (the localisation only): a
// sample whose eight corners are observed but whose fp32 |phi| < band is false adds nothing and returns 2 -- it lies in the flat
// region in front of the surface, where the gradient is zero.  The operations and their order are the rule; the header of the C
// ABI spells them out.
template <bool BAND, class Fetch>
DR_HOST_DEVICE inline int align_point(const AlignEval &e, double g0, double g1, double g2, float s_src, Fetch &&fetch, double acc[28]) {
  double q[3];
  int b[3];
  float f[3];
  DR_UNROLL
  for (int k = 0; k < 3; ++k) {
    q[k] = ((e.m.R[3 * k] * g0 + e.m.R[3 * k + 1] * g1) + e.m.R[3 * k + 2] * g2) + e.m.tv[k];
    if (!(q[k] > -1073741824.0 && q[k] < 1073741824.0)) return 0;
    const double fl = floor(q[k]);
    b[k] = (int)fl;
    f[k] = (float)(q[k] - fl);
  }
  float s[8];  // index 4 cx + 2 cy + cz
  DR_UNROLL
  for (int c = 0; c < 8; ++c) {
    uint32_t v[2];
    fetch(b[0] + (c >> 2), b[1] + ((c >> 1) & 1), b[2] + (c & 1), v);
    if ((int)(v[1] >> 24) < e.min_weight) return 0;
    memcpy(&s[c], &v[0], 4);
  }
  float h[4], ez[4];  // index 2 cx + cy
  DR_UNROLL
  for (int c = 0; c < 4; ++c) {
    h[c] = s[2 * c + 1] - s[2 * c];
    ez[c] = s[2 * c] + f[2] * h[c];
  }
  float dy[2], d[2], hy[2];
  DR_UNROLL
  for (int c = 0; c < 2; ++c) {
    dy[c] = ez[2 * c + 1] - ez[2 * c];
    d[c] = ez[2 * c] + f[1] * dy[c];
    hy[c] = h[2 * c] + f[1] * (h[2 * c + 1] - h[2 * c]);
  }
  const float gxf = d[1] - d[0];
  const float phi = d[0] + f[0] * gxf;
  const float gyf = dy[0] + f[0] * (dy[1] - dy[0]);
  const float gzf = hy[0] + f[0] * (hy[1] - hy[0]);
  if (BAND) {
    const float ap = phi < 0.0f ? -phi : phi;
    if (!(ap < e.band)) return 2;
  }
  const double r = ((double)phi - (double)s_src) / e.vs;
  const double n0 = (double)gxf / e.vs, n1 = (double)gyf / e.vs, n2 = (double)gzf / e.vs;
  align_accumulate(e, r, n0, n1, n2, q, acc);
  return 1;
}
// One sample of the registration: the source voxel at lattice point (gx, gy, gz) with sdf s_src; true if it was valid.
template <class Fetch>
DR_HOST_DEVICE inline bool align_voxel(const AlignEval &e, int gx, int gy, int gz, float s_src, Fetch &&fetch, double acc[28]) {
  return align_point<false>(e, (double)gx, (double)gy, (double)gz, s_src, fetch, acc) == 1;
}
// x[l] = x[l] + x[l ^ off] for off = 32, 16, 8, 4, 2, 1 over 64 lanes of 28 values: afterwards every lane holds the same sum
inline void align_butterfly(double x[64][28]) {
  for (int off = 32; off > 0; off >>= 1) {
    double y[64][28];
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 28; ++i) y[l][i] = x[l][i] + x[l ^ off][i];
    memcpy(x, y, sizeof y);
  }
}
// One source block at block coordinates blk in the wave's order: lane l takes voxels 2 (l + 64 k) and the next, k = 0..3, then the
// butterfly.  out[28] = the block's sums; counts += {samples, valid, invalid}.
template <class Fetch>
inline void align_block(const AlignEval &e, const int blk[3], const uint8_t *src4096, Fetch &&ref, double out[28], uint64_t counts[3]) {
  double x[64][28];
  for (int l = 0; l < 64; ++l) {
    for (int i = 0; i < 28; ++i) x[l][i] = 0.0;
    for (int k = 0; k < 4; ++k)
      for (int t = 0; t < 2; ++t) {
        const int v = 2 * (l + 64 * k) + t;
        uint32_t w[2];
        memcpy(w, src4096 + 8 * v, 8);
        if (!align_is_sample(w, e)) continue;
        float s;
        memcpy(&s, &w[0], 4);
        ++counts[0];
        if (align_voxel(e, blk[0] * kBS + (v >> 6), blk[1] * kBS + ((v >> 3) & 7), blk[2] * kBS + (v & 7), s, ref, x[l])) ++counts[1];
        else ++counts[2];
      }
  }
  align_butterfly(x);
  for (int i = 0; i < 28; ++i) out[i] = x[0][i];
}
// k_align_fold on the host: per component lane l adds partial[l], partial[l + 64], ... from +0.0 and the butterfly folds the lanes
inline void align_fold_host(const double *partial, size_t n, double sums[28]) {
  double x[64][28];
  for (int l = 0; l < 64; ++l)
    for (int c = 0; c < 28; ++c) {
      double a = 0.0;
      for (size_t i = (size_t)l; i < n; i += 64) a = a + partial[i * 28 + c];
      x[l][c] = a;
    }
  align_butterfly(x);
  for (int c = 0; c < 28; ++c) sums[c] = x[0][c];
}
// The system at one pose over the whole source (keys ascending, n x 4096 bytes): align_block per block into partial[i], then
// per component lane l adds partial[l], partial[l + 64], ... from +0.0 and the butterfly folds the lanes.
template <class Fetch>
inline void align_system_host(const std::vector<unsigned long long> &src_keys, const uint8_t *src_vox, Fetch &&ref, const AlignEval &e, double sums[28],
                              uint64_t counts[3]) {
  counts[0] = counts[1] = counts[2] = 0;
  const size_t n = src_keys.size();
  std::vector<double> partial(n * 28);
  for (size_t i = 0; i < n; ++i) {
    int blk[3]; unpack_key_host(src_keys[i], blk);
    align_block(e, blk, src_vox + i * 4096, ref, &partial[i * 28], counts);
  }
  align_fold_host(partial.data(), n, sums);
}
// One Gauss-Newton step from the system sums at pose m (centre c = e.c of that evaluation).  Returns DRF_ALIGN_DEGENERATE (m
// unchanged), DRF_ALIGN_CONVERGED (the step is below both thresholds and is not applied) or -1 (m moved).  + - * / sqrt only.
inline int align_step(const double sums[28], const double c[3], double eps_rot, double eps_trans, MapMotion &m) {
  double H[6][6], L[6][6] = {{0.0}}, y[6] = {0.0}, d[6] = {0.0};
  int idx = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { H[i][j] = sums[idx]; H[j][i] = sums[idx]; ++idx; }
  double top = H[0][0];
  for (int j = 1; j < 6; ++j) top = H[j][j] > top ? H[j][j] : top;
  if (!(top > 0.0)) return DRF_ALIGN_DEGENERATE;
  for (int j = 0; j < 6; ++j) {
    double p = H[j][j];
    for (int k = 0; k < j; ++k) p = p - L[j][k] * L[j][k];
    if (!(p > 1e-12 * top)) return DRF_ALIGN_DEGENERATE;
    L[j][j] = std::sqrt(p);
    for (int i = j + 1; i < 6; ++i) {
      double t = H[i][j];
      for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  for (int i = 0; i < 6; ++i) {
    double t = -sums[21 + i];
    for (int k = 0; k < i; ++k) t = t - L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double t = y[i];
    for (int k = i + 1; k < 6; ++k) t = t - L[k][i] * d[k];
    d[i] = t / L[i][i];
  }
  const double oo = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], vv = (d[3] * d[3] + d[4] * d[4]) + d[5] * d[5];
  if (!(oo == oo) || !(vv == vv)) return DRF_ALIGN_DEGENERATE;  // a system that held a NaN
  if (std::sqrt(oo) < eps_rot && std::sqrt(vv) < eps_trans) return DRF_ALIGN_CONVERGED;
  const double a = 1.0 / std::sqrt(1.0 + oo / 4.0);
  const double qw = a, qx = (a * d[0]) / 2.0, qy = (a * d[1]) / 2.0, qz = (a * d[2]) / 2.0;
  const double Rq[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                        2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                        2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
  MapMotion o;
  const double e[3] = {m.tv[0] - c[0], m.tv[1] - c[1], m.tv[2] - c[2]};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o.R[3 * i + j] = (Rq[3 * i] * m.R[j] + Rq[3 * i + 1] * m.R[3 + j]) + Rq[3 * i + 2] * m.R[6 + j];
    o.tv[i] = (c[i] + ((Rq[3 * i] * e[0] + Rq[3 * i + 1] * e[1]) + Rq[3 * i + 2] * e[2])) + d[3 + i];
  }
  m = o;
  return -1;
}
// The loop of drf_align_map over any evaluator eval(const AlignEval &, double sums[28], uint64_t counts[3]): the host's
// (align_maps_host) or the engine's (the kernels).  trace, if given, receives the sums of every evaluation.
template <class Eval>
inline void align_loop(Eval &&eval, const MapMotion &m0, const double c_src[3], const AlignOpt &o, float voxel_size, drf_align_result_t &res,
                       std::vector<std::array<double, 28>> *trace = nullptr) {
  MapMotion m = m0, good = m0;
  memset(&res, 0, sizeof res);
  res.status = DRF_ALIGN_MAX_ITERS;
  for (int it = 0; it < o.max_iters; ++it) {
    const AlignEval e = align_eval(m, c_src, o, voxel_size);
    uint64_t counts[3];
    eval(e, res.sums, counts);
    if (trace) { std::array<double, 28> t; memcpy(t.data(), res.sums, sizeof res.sums); trace->push_back(t); }
    res.iterations = it + 1;
    res.samples = counts[0]; res.valid = counts[1];
    res.cost = counts[1] ? res.sums[27] / (double)counts[1] : 0.0;
    if (it == 0) { res.valid0 = res.valid; res.cost0 = res.cost; }
    if ((double)counts[1] < o.min_valid * (double)counts[0] || counts[1] < 6) { res.status = DRF_ALIGN_LOST; m = good; break; }
    good = m;
    const int s = align_step(res.sums, e.c, o.eps_rot, o.eps_trans, m);
    if (s >= 0) { res.status = s; break; }
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) res.T[4 * i + j] = m.R[3 * i + j];
    res.T[4 * i + 3] = m.tv[i] * (double)voxel_size;
  }
  res.T[15] = 1.0;
}
inline const char *align_status_name(int s) {
  static const char *names[] = {"converged", "reached max_iters", "is degenerate (the samples do not constrain all six degrees of freedom)",
                                "is lost (too few samples have an observed neighbourhood in the reference)"};
  return s >= 0 && s < 4 ? names[s] : "?";
}
// The whole registration on the CPU: the library's reference for drf_align_map, and what the sanitizer program runs.
inline void align_maps_host(const std::vector<unsigned long long> &src_keys, const uint8_t *src_vox, const HostMapSource &ref, const MapMotion &m0,
                            const AlignOpt &o, float voxel_size, drf_align_result_t &res, std::vector<std::array<double, 28>> *trace = nullptr) {
  double c_src[3];
  align_centre_src(src_keys, c_src);
  align_loop([&](const AlignEval &e, double sums[28], uint64_t counts[3]) { align_system_host(src_keys, src_vox, ref, e, sums, counts); }, m0, c_src, o,
             voxel_size, res, trace);
}

// ---- locating a depth frame in the map (drf_locate_system / drf_locate_frame; DESIGN.md §7c "Locating a depth frame in the map")
// T is the engine's pose16: camera-to-world, held as a MapMotion (Rd, tv = t / voxel_size).  The samples are the pixels of a depth
// image on a grid of stride `step`, each the camera-frame point g = ((u - cx) / fx * z, (v - cy) / fy * z, z) / voxel_size in
// double; from q = Rd g + tv on a sample is align_point's, with s_src = 0 and the band test on phi.  The lattice point g of the map
// sits at world g * voxel_size, as for k_integrate and transform_voxel: no half-voxel offset.  Stated once, here; the header of
// the C ABI restates it for users.  Compiled by g++ for the CPU tests and by hipcc for k_map_locate, both without contraction.
struct LocateOpt {  // drf_locate_options_t with its defaults resolved
  AlignOpt a;
  int step;
  float centre_depth;
};
// null: all defaults (band: the engine's truncation_distance).  Returns null, or which option is negative or not finite
inline const char *locate_options(const drf_locate_options_t *opt, float truncation_distance, LocateOpt &o) {
  static const drf_locate_options_t zero = {0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.0};
  const drf_locate_options_t &u = opt ? *opt : zero;
  if (u.step < 0) return "step";
  if (!(u.centre_depth >= 0.0f) || !std::isfinite(u.centre_depth)) return "centre_depth";
  const drf_align_options_t a = {u.max_iters, u.min_weight, u.band, u.huber, u.eps_rot, u.eps_trans, u.min_valid};
  if (const char *bad = align_options(&a, 1.0f, o.a)) return bad;
  if (u.band == 0.0f) o.a.band = truncation_distance;
  o.step = u.step ? u.step : 1;
  o.centre_depth = u.centre_depth;
  return nullptr;
}
// the sample grid and the camera: what a kernel launch and a host evaluation share besides AlignEval
struct LocateGrid {
  int W, H, step, Wg, Hg;  // Wg = ceil(W / step), Hg = ceil(H / step): Wg * Hg grid positions
  float fx, fy, cx, cy, min_depth, max_depth;
};
inline LocateGrid locate_grid(const drf_options_t &o, int step) {
  LocateGrid g;
  g.W = o.width; g.H = o.height; g.step = step;
  g.Wg = (o.width + step - 1) / step; g.Hg = (o.height + step - 1) / step;
  g.fx = o.fx; g.fy = o.fy; g.cx = o.cx; g.cy = o.cy; g.min_depth = o.min_sensor_depth; g.max_depth = o.max_sensor_depth;
  return g;
}
inline long locate_positions(const LocateGrid &g) { return (long)g.Wg * (long)g.Hg; }
inline long locate_groups(const LocateGrid &g) { return (locate_positions(g) + 511) / 512; }
inline void locate_centre_src(float centre_depth, float voxel_size, double c_src[3]) {
  c_src[0] = 0.0; c_src[1] = 0.0; c_src[2] = (double)centre_depth / (double)voxel_size;
}
// Grid position n < Wg * Hg: is its pixel a sample (the conditions under which k_integrate uses a pixel; a NaN is none), and if
// so its camera-frame point g in lattice units.
DR_HOST_DEVICE inline bool locate_is_sample(const LocateGrid &lg, float dep) { return dep > 0.0f && dep >= lg.min_depth && dep <= lg.max_depth; }
DR_HOST_DEVICE inline size_t locate_offset(const LocateGrid &lg, int n) {  // of grid position n's pixel in the depth image
  const int j = n / lg.Wg, i = n - j * lg.Wg;
  return (size_t)(lg.step * j) * (size_t)lg.W + (size_t)(lg.step * i);
}
DR_HOST_DEVICE inline bool locate_pixel(const LocateGrid &lg, double vs, int n, const float *depth, double g[3]) {
  const int j = n / lg.Wg, i = n - j * lg.Wg;
  const int u = lg.step * i, v = lg.step * j;
  const float dep = depth[locate_offset(lg, n)];
  if (!locate_is_sample(lg, dep)) return false;
  const double z = (double)dep;
  g[0] = ((((double)u - (double)lg.cx) / (double)lg.fx) * z) / vs;
  g[1] = ((((double)v - (double)lg.cy) / (double)lg.fy) * z) / vs;
  g[2] = z / vs;
  return true;
}
// The loop's pose (Rd, tv in lattice units, double) as the pose16 the two functions above and select_render_blocks take.  The
// evaluation itself runs at the double pose: an entry of R moves by at most 2^-25 and t_k by 2^-25 |t_k| plus the product's own
// rounding, so a sample point moves by less than 2^-24 (3 max_sensor_depth rho + |t|).  |t| is below 2^23 voxels wherever a block
// has a key, and the depth range far below that: less than one voxel, the vs that locate_stage_slack leaves out of the slack.
inline void locate_pose16(const MapMotion &m, float voxel_size, float pose16[16]) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pose16[4 * i + j] = (float)m.R[3 * i + j];
    pose16[4 * i + 3] = (float)(m.tv[i] * (double)voxel_size);
  }
  pose16[12] = pose16[13] = pose16[14] = 0.0f;
  pose16[15] = 1.0f;
}
// Group i in the wave's order: lane l takes grid positions 512 i + l + 64 k, k = 0..7 (those >= Wg * Hg are no samples), then the
// butterfly.  out[28] = the group's sums; counts += {samples, valid, unobserved, outside}.
template <class Fetch>
inline void locate_group(const AlignEval &e, const LocateGrid &lg, const float *depth, long i, Fetch &&fetch, double out[28], uint64_t counts[4]) {
  double x[64][28];
  const long total = locate_positions(lg);
  for (int l = 0; l < 64; ++l) {
    for (int c = 0; c < 28; ++c) x[l][c] = 0.0;
    for (int k = 0; k < 8; ++k) {
      const long n = 512 * i + l + 64 * k;
      double g[3];
      if (n >= total || !locate_pixel(lg, e.vs, (int)n, depth, g)) continue;
      ++counts[0];
      const int r = align_point<true>(e, g[0], g[1], g[2], 0.0f, fetch, x[l]);
      ++counts[r == 1 ? 1 : r == 0 ? 2 : 3];
    }
  }
  align_butterfly(x);
  for (int c = 0; c < 28; ++c) out[c] = x[0][c];
}
// The system at one pose over the whole sample grid: locate_group per group into partial[i], then k_align_fold's fold.
template <class Fetch>
inline void locate_system_host(const LocateGrid &lg, const float *depth, Fetch &&fetch, const AlignEval &e, double sums[28], uint64_t counts[4]) {
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  const size_t n = (size_t)locate_groups(lg);
  std::vector<double> partial(n * 28);
  for (size_t i = 0; i < n; ++i) locate_group(e, lg, depth, (long)i, fetch, &partial[i * 28], counts);
  align_fold_host(partial.data(), n, sums);
}
// align_loop over a localisation's evaluator eval(const AlignEval &, double sums[28], uint64_t counts[4]): the loop is given
// {samples, valid, unobserved + outside}.  last4, if given, receives the four counters of the last evaluation.
template <class Eval>
inline void locate_loop(Eval &&eval, const MapMotion &m0, const LocateOpt &o, float voxel_size, drf_align_result_t &res, uint64_t *last4 = nullptr,
                        std::vector<std::array<double, 28>> *trace = nullptr) {
  double c_src[3];
  locate_centre_src(o.centre_depth, voxel_size, c_src);
  align_loop([&](const AlignEval &e, double sums[28], uint64_t counts[3]) {
    uint64_t c4[4];
    eval(e, sums, c4);
    counts[0] = c4[0]; counts[1] = c4[1]; counts[2] = c4[2] + c4[3];
    if (last4) memcpy(last4, c4, sizeof c4);
  }, m0, c_src, o.a, voxel_size, res, trace);
}
// The whole refinement on the CPU over a HostMapSource or any fetch: the library's reference for drf_locate_frame, and what the
// sanitizer program runs.
template <class Fetch>
inline void locate_frame_host(const LocateGrid &lg, const float *depth, Fetch &&fetch, const MapMotion &m0, const LocateOpt &o, float voxel_size,
                              drf_align_result_t &res, std::vector<std::array<double, 28>> *trace = nullptr) {
  locate_loop([&](const AlignEval &e, double sums[28], uint64_t c4[4]) { locate_system_host(lg, depth, fetch, e, sums, c4); }, m0, o, voxel_size, res,
              nullptr, trace);
}

// ---- tracking a depth frame against the ray-cast model (drf_track_system / drf_track_frame; DESIGN.md §7c "Tracking a depth frame
// against the ray-cast model").  The frame's samples are drf_locate_*'s (locate_pixel, the same grid and test); each is associated
// projectively with a pixel of the MODEL MAP -- per pixel of a depth image Dm ray-cast at the pose Pm its depth and the unit normal
// of its back-projected neighbourhood -- and contributes the point-to-plane distance to that pixel's plane.  From the residual and
// the normal on a sample is align_accumulate's, the step and the loop align_step's and align_loop's.  Stated once, here; the
// header of the C ABI restates it for users.  Compiled by g++ and by hipcc (k_track_model, k_track), both without contraction;
// + - * / sqrt and floor only.
struct TrackOpt {  // drf_track_options_t with its defaults resolved; a.max_iters is inner_iters (a.band and a.min_weight are not read)
  AlignOpt a;
  int max_renders, step;
  float centre_depth, dist_max, max_jump;
};
// null: all defaults.  Returns null, or which option is negative or not finite
inline const char *track_options(const drf_track_options_t *opt, float voxel_size, TrackOpt &o) {
  static const drf_track_options_t zero = {0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.0};
  const drf_track_options_t &u = opt ? *opt : zero;
  if (u.max_renders < 0) return "max_renders";
  if (u.inner_iters < 0) return "inner_iters";
  if (u.step < 0) return "step";
  if (!(u.dist_max >= 0.0f) || !std::isfinite(u.dist_max)) return "dist_max";
  if (!(u.max_jump >= 0.0f) || !std::isfinite(u.max_jump)) return "max_jump";
  if (!(u.centre_depth >= 0.0f) || !std::isfinite(u.centre_depth)) return "centre_depth";
  const drf_align_options_t a = {u.inner_iters, 0, 0.0f, u.huber, u.eps_rot, u.eps_trans, u.min_valid};
  if (const char *bad = align_options(&a, 1.0f, o.a)) return bad;
  o.a.max_iters = u.inner_iters ? u.inner_iters : 4;
  o.max_renders = u.max_renders ? u.max_renders : 10;
  o.step = u.step ? u.step : 1;
  o.dist_max = u.dist_max != 0.0f ? u.dist_max : 25.0f * voxel_size;
  o.max_jump = u.max_jump != 0.0f ? u.max_jump : 5.0f * voxel_size;
  o.centre_depth = u.centre_depth;
  return nullptr;
}
// one pixel of the model map: the unit normal in the model camera's frame, towards the camera, and the depth; z = 0 is invalid
struct alignas(16) TrackPixel { float nx, ny, nz, z; };
// The model map's pixel (u, v) from the model depth image Dm (lg: the camera; its step is not read), all in fp32.  A MISS of the
// ray-cast is the 0.0f that k_raycast2 / k_raycast_fix write for a ray that found no surface; the test is !(z > 0), which a NaN
// and a negative depth fail too.  Invalid (all four floats 0): the centre is a miss; the pixel lies on the image border; one of its
// four neighbours (u -+ 1, v), (u, v -+ 1) is a miss; |z_neighbour - z| > max_jump for one of them.  Otherwise, with
// X(u, v, z) = ((((float)u - cx) / fx) * z, (((float)v - cy) / fy) * z, z): a = X(u + 1, v) - X(u - 1, v), b = X(u, v + 1) -
// X(u, v - 1), n = a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), l2 = (n0 n0 + n1 n1) + n2 n2; !(l2 > 0) is invalid;
// n = n / sqrt(l2); and with s = (n0 X0 + n1 X1) + n2 X2 at the centre, s > 0 negates n: the normal looks at the camera.
DR_HOST_DEVICE inline TrackPixel track_normal(const LocateGrid &lg, float max_jump, const float *Dm, int u, int v) {
  TrackPixel p = {0.0f, 0.0f, 0.0f, 0.0f};
  if (u <= 0 || v <= 0 || u >= lg.W - 1 || v >= lg.H - 1) return p;
  const size_t at = (size_t)v * (size_t)lg.W + (size_t)u;
  const float z = Dm[at], zl = Dm[at - 1], zr = Dm[at + 1], zu = Dm[at - (size_t)lg.W], zd = Dm[at + (size_t)lg.W];
  if (!(z > 0.0f) || !(zl > 0.0f) || !(zr > 0.0f) || !(zu > 0.0f) || !(zd > 0.0f)) return p;
  const float jl = zl - z, jr = zr - z, ju = zu - z, jd = zd - z;
  if ((jl < 0.0f ? -jl : jl) > max_jump || (jr < 0.0f ? -jr : jr) > max_jump || (ju < 0.0f ? -ju : ju) > max_jump || (jd < 0.0f ? -jd : jd) > max_jump) return p;
  const float rx = ((float)u - lg.cx) / lg.fx, ry = ((float)v - lg.cy) / lg.fy;
  const float rxl = ((float)(u - 1) - lg.cx) / lg.fx, rxr = ((float)(u + 1) - lg.cx) / lg.fx;
  const float ryu = ((float)(v - 1) - lg.cy) / lg.fy, ryd = ((float)(v + 1) - lg.cy) / lg.fy;
  const float a0 = rxr * zr - rxl * zl, a1 = ry * zr - ry * zl, a2 = zr - zl;
  const float b0 = rx * zd - rx * zu, b1 = ryd * zd - ryu * zu, b2 = zd - zu;
  float n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
  const float l2 = (n0 * n0 + n1 * n1) + n2 * n2;
  if (!(l2 > 0.0f)) return p;
  const float l = sqrtf(l2);
  n0 = n0 / l; n1 = n1 / l; n2 = n2 / l;
  const float s = (n0 * (rx * z) + n1 * (ry * z)) + n2 * z;
  if (s > 0.0f) { n0 = -n0; n1 = -n1; n2 = -n2; }
  p.nx = n0; p.ny = n1; p.nz = n2; p.z = z;
  return p;
}
inline void track_model_host(const LocateGrid &lg, float max_jump, const float *Dm, TrackPixel *out) {
  for (int v = 0; v < lg.H; ++v)
    for (int u = 0; u < lg.W; ++u) out[(size_t)v * lg.W + u] = track_normal(lg, max_jump, Dm, u, v);
}
// the model of one evaluation: its pose Pm (camera-to-world, lattice units), (dist_max / voxel_size)^2, and the map
struct TrackModel {
  MapMotion m;
  double lim2;
  const TrackPixel *map;
};
inline TrackModel track_model(const float *model_pose16, const TrackOpt &o, float voxel_size, const TrackPixel *map) {
  TrackModel t;
  t.m = map_motion(model_pose16, voxel_size);
  const double lim = (double)o.dist_max / (double)voxel_size;
  t.lim2 = lim * lim;
  t.map = map;
  return t;
}
// One sample at the camera-frame point g (lattice units, locate_pixel's): q = Rd g + tv at the estimate; m = Rm^T (q - tvm), the
// point in the model camera; !(m2 > 0) is UNASSOCIATED (behind the model camera, or a NaN); u' = fx (m0 / m2) + cx, v' likewise,
// the pixel (floor(u' + 0.5), floor(v' + 0.5)); outside the image or an invalid model pixel is UNASSOCIATED (returns 0).  The model
// vertex vm is that pixel's back-projection at its z, as locate_pixel computes a point; d = m - vm; a sample for which
// |d|^2 <= lim2 is false is REJECTED (returns 2).  Otherwise r = (n0 d0 + n1 d1) + n2 d2 with the pixel's normal widened to
// double, nw = Rm n, and tail(r, nw0, nw1, nw2, q, m, u', v') adds the sample's terms and returns the code (1 for track_point).
// The tail is where track_point and track_colour_point differ: one term, or two.
template <class Tail>
DR_HOST_DEVICE inline int track_sample(const AlignEval &e, const TrackModel &t, const LocateGrid &lg, double g0, double g1, double g2, Tail &&tail) {
  double q[3], m[3];
  DR_UNROLL
  for (int k = 0; k < 3; ++k) q[k] = ((e.m.R[3 * k] * g0 + e.m.R[3 * k + 1] * g1) + e.m.R[3 * k + 2] * g2) + e.m.tv[k];
  const double s0 = q[0] - t.m.tv[0], s1 = q[1] - t.m.tv[1], s2 = q[2] - t.m.tv[2];
  DR_UNROLL
  for (int k = 0; k < 3; ++k) m[k] = (t.m.R[k] * s0 + t.m.R[3 + k] * s1) + t.m.R[6 + k] * s2;
  if (!(m[2] > 0.0)) return 0;
  const double up = (double)lg.fx * (m[0] / m[2]) + (double)lg.cx, vp = (double)lg.fy * (m[1] / m[2]) + (double)lg.cy;
  const double pu = floor(up + 0.5), pv = floor(vp + 0.5);
  if (!(pu >= 0.0 && pu <= (double)(lg.W - 1) && pv >= 0.0 && pv <= (double)(lg.H - 1))) return 0;
  const TrackPixel p = t.map[(size_t)(int)pv * (size_t)lg.W + (size_t)(int)pu];
  if (!(p.z > 0.0f)) return 0;
  const double z = (double)p.z;
  const double d0 = m[0] - (((pu - (double)lg.cx) / (double)lg.fx) * z) / e.vs;
  const double d1 = m[1] - (((pv - (double)lg.cy) / (double)lg.fy) * z) / e.vs;
  const double d2 = m[2] - z / e.vs;
  const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
  if (!(dd <= t.lim2)) return 2;
  const double n0 = (double)p.nx, n1 = (double)p.ny, n2 = (double)p.nz;
  const double r = (n0 * d0 + n1 * d1) + n2 * d2;
  const double w0 = (t.m.R[0] * n0 + t.m.R[1] * n1) + t.m.R[2] * n2;
  const double w1 = (t.m.R[3] * n0 + t.m.R[4] * n1) + t.m.R[5] * n2;
  const double w2 = (t.m.R[6] * n0 + t.m.R[7] * n1) + t.m.R[8] * n2;
  return tail(r, w0, w1, w2, q, m, up, vp);
}
// The geometric term alone: align_accumulate adds the sample.
DR_HOST_DEVICE inline int track_point(const AlignEval &e, const TrackModel &t, const LocateGrid &lg, double g0, double g1, double g2, double acc[28]) {
  return track_sample(e, t, lg, g0, g1, g2, [&](double r, double w0, double w1, double w2, const double *q, const double *, double, double) {
    align_accumulate(e, r, w0, w1, w2, q, acc);
    return 1;
  });
}
// Group i in the wave's order (locate_group's); counts += {samples, valid, unassociated, rejected}.
inline void track_group(const AlignEval &e, const TrackModel &t, const LocateGrid &lg, const float *depth, long i, double out[28], uint64_t counts[4]) {
  double x[64][28];
  const long total = locate_positions(lg);
  for (int l = 0; l < 64; ++l) {
    for (int c = 0; c < 28; ++c) x[l][c] = 0.0;
    for (int k = 0; k < 8; ++k) {
      const long n = 512 * i + l + 64 * k;
      double g[3];
      if (n >= total || !locate_pixel(lg, e.vs, (int)n, depth, g)) continue;
      ++counts[0];
      const int r = track_point(e, t, lg, g[0], g[1], g[2], x[l]);
      ++counts[r == 1 ? 1 : r == 0 ? 2 : 3];
    }
  }
  align_butterfly(x);
  for (int c = 0; c < 28; ++c) out[c] = x[0][c];
}
// The system at one pose over the whole sample grid: track_group per group into partial[i], then k_align_fold's fold.
inline void track_system_host(const LocateGrid &lg, const float *depth, const TrackModel &t, const AlignEval &e, double sums[28], uint64_t counts[4]) {
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  const size_t n = (size_t)locate_groups(lg);
  std::vector<double> partial(n * 28);
  for (size_t i = 0; i < n; ++i) track_group(e, t, lg, depth, (long)i, &partial[i * 28], counts);
  align_fold_host(partial.data(), n, sums);
}
// The outer loop of drf_track_frame over render(const float pose16[16]), which ray-casts the map at that pose and builds the model
// map, and eval(const AlignEval &, const float model_pose16[16], double sums[28], uint64_t counts[4]), one evaluation against it.
// Round r renders at p16 -- pose_init16, later the float pose16 the round before ended on (res.T rounded to float, what
// drf_render_async would be given) -- and runs align_loop from that very pose, m = map_motion(p16), with max_iters = inner_iters
// and {samples, valid, unassociated + rejected}.  A round that ends LOST or DEGENERATE ends the call with that status; one that
// ends CONVERGED at its first evaluation ends it CONVERGED; any other round hands its pose on, and after max_renders rounds the
// call is MAX_ITERS.  res: T, sums, samples, valid, cost of the last round; valid0, cost0 of the first; iterations = evaluations in
// all.  stats2 = {evaluations, renders}; last4 the four counters of the last evaluation.
template <class Render, class Eval>
inline void track_loop(Render &&render, Eval &&eval, const float *pose_init16, const TrackOpt &o, float voxel_size, drf_align_result_t &res,
                       uint64_t *last4 = nullptr, uint64_t *stats2 = nullptr, std::vector<std::array<double, 28>> *trace = nullptr) {
  double c_src[3];
  locate_centre_src(o.centre_depth, voxel_size, c_src);
  float p16[16];
  memcpy(p16, pose_init16, sizeof p16);
  memset(&res, 0, sizeof res);
  int evaluations = 0;
  uint64_t valid0 = 0;
  double cost0 = 0.0;
  for (int r = 0; r < o.max_renders; ++r) {
    render(p16);
    if (stats2) ++stats2[1];
    drf_align_result_t in;
    align_loop([&](const AlignEval &e, double sums[28], uint64_t counts[3]) {
      uint64_t c4[4];
      eval(e, p16, sums, c4);
      counts[0] = c4[0]; counts[1] = c4[1]; counts[2] = c4[2] + c4[3];
      if (last4) memcpy(last4, c4, sizeof c4);
      if (stats2) ++stats2[0];
    }, map_motion(p16, voxel_size), c_src, o.a, voxel_size, in, trace);
    evaluations += in.iterations;
    if (r == 0) { valid0 = in.valid0; cost0 = in.cost0; }
    res = in;
    res.valid0 = valid0; res.cost0 = cost0; res.iterations = evaluations;
    if (in.status == DRF_ALIGN_LOST || in.status == DRF_ALIGN_DEGENERATE) return;
    if (in.status == DRF_ALIGN_CONVERGED && in.iterations == 1) return;
    res.status = DRF_ALIGN_MAX_ITERS;
    for (int i = 0; i < 16; ++i) p16[i] = (float)in.T[i];
  }
}
// The whole tracking on the CPU over any renderer render_depth(const float pose16[16], float *Dm): the library's reference for
// drf_track_frame, and what the sanitizer program runs.
template <class RenderDepth>
inline void track_frame_host(const LocateGrid &lg, const float *depth, RenderDepth &&render_depth, const float *pose_init16, const TrackOpt &o, float voxel_size,
                             drf_align_result_t &res, uint64_t *last4 = nullptr, uint64_t *stats2 = nullptr, std::vector<std::array<double, 28>> *trace = nullptr) {
  const size_t npix = (size_t)lg.W * (size_t)lg.H;
  std::vector<float> Dm(npix);
  std::vector<TrackPixel> map(npix);
  track_loop([&](const float *p16) { render_depth(p16, Dm.data()); track_model_host(lg, o.max_jump, Dm.data(), map.data()); },
             [&](const AlignEval &e, const float *p16, double sums[28], uint64_t c4[4]) {
               track_system_host(lg, depth, track_model(p16, o, voxel_size, map.data()), e, sums, c4);
             }, pose_init16, o, voxel_size, res, last4, stats2, trace);
}

// ---- tracking with colour (drf_track_colour_system / drf_track_colour_frame; DESIGN.md §7c "Tracking with colour").  The tracking
// above sees geometry only, and a map of planes leaves the motion inside the planes open.  Every voxel carries a colour and the
// ray-cast renders it, so a sample whose geometric term was added contributes a second, photometric term: the difference between
// the model's colour image, interpolated where the sample projects, and the frame's own pixel, as intensities, scaled to voxels by
// photo_weight.  Its gradient with respect to the point is a 3-vector like the plane's normal, so both terms go through the one
// align_accumulate into the same 28 sums, and step, loop and outer loop are the geometric call's, unchanged.  Stated once, here;
// the header of the C ABI restates it.  Compiled by g++ and by hipcc (k_track_model_colour, k_track_colour), both without
// contraction; + - * / sqrt and floor only.
#if defined(__HIPCC__)
#define DR_NO_UNROLL _Pragma("unroll 1")
#else
#define DR_NO_UNROLL
#endif
struct TrackColourOpt {  // drf_track_colour_options_t with its defaults resolved
  TrackOpt t;
  float photo_weight;  // voxels per intensity unit
};
// null: all defaults.  photo_weight 0 is (float)(1.0 / 27.0) * huber in fp32, huber resolved first: a colour residual of 27 units
// of the three-channel sum -- 9 grey levels of 255 -- weighs what a geometric residual at Huber's threshold weighs.
inline const char *track_colour_options(const drf_track_colour_options_t *opt, float voxel_size, TrackColourOpt &o) {
  static const drf_track_colour_options_t zero = {{0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.0}, 0.0f};
  const drf_track_colour_options_t &u = opt ? *opt : zero;
  if (const char *bad = track_options(&u.track, voxel_size, o.t)) return bad;
  if (!(u.photo_weight >= 0.0f) || !std::isfinite(u.photo_weight)) return "photo_weight";
  o.photo_weight = u.photo_weight != 0.0f ? u.photo_weight : (float)(1.0 / 27.0) * o.t.a.huber;
  return nullptr;
}
// the intensity of a BGR pixel: a whole number in 0..765
DR_HOST_DEVICE inline float track_intensity(const unsigned char *bgr) { return ((float)bgr[0] + (float)bgr[1]) + (float)bgr[2]; }
// One pixel of the model intensity map Ym: the intensity of the model colour image where the model map's pixel is valid, -1
// elsewhere -- misses, the border and depth discontinuities are excluded by the test the geometric term uses.
DR_HOST_DEVICE inline float track_model_intensity(const TrackPixel &p, const unsigned char *bgr) { return p.z > 0.0f ? track_intensity(bgr) : -1.0f; }
inline void track_model_colour_host(const LocateGrid &lg, float max_jump, const float *Dm, const unsigned char *Cm, TrackPixel *out, float *Ym) {
  for (int v = 0; v < lg.H; ++v)
    for (int u = 0; u < lg.W; ++u) {
      const size_t at = (size_t)v * lg.W + u;
      out[at] = track_normal(lg, max_jump, Dm, u, v);
      Ym[at] = track_model_intensity(out[at], Cm + 3 * at);
    }
}
// what an evaluation with colour reads besides the TrackModel: Ym and lambda = (double)photo_weight
struct TrackColour {
  const float *Ym;
  double weight;
};
inline TrackColour track_colour(const TrackColourOpt &o, const float *Ym) {
  TrackColour c;
  c.Ym = Ym; c.weight = (double)o.photo_weight;
  return c;
}
struct TrackPair { float a, b; };  // two neighbours of a row of Ym: one 8-byte read at a 4-byte aligned address
// The photometric term of a sample that track_sample accepted, from its m, u', v' and the frame's intensity yf at the sample's
// own pixel.  u0 = floor(u'), v0 = floor(v'), a = u' - u0, b = v' - v0; the term is SKIPPED (returns false) unless 0 <= u0,
// u0 + 1 <= W - 1, 0 <= v0, v0 + 1 <= H - 1 and the four corners y00 = Ym(u0, v0), y10 = Ym(u0 + 1, v0), y01 = Ym(u0, v0 + 1),
// y11 = Ym(u0 + 1, v0 + 1) are all >= 0.  In double, oa = 1 - a, ob = 1 - b:
//   I  = ob * (oa * y00 + a * y10) + b * (oa * y01 + a * y11)
//   Iu = ob * (y10 - y00) + b * (y11 - y01),  Iv = oa * (y01 - y00) + a * (y11 - y10)     the exact gradient of that interpolant
//   gm0 = (Iu * fx) / m2, gm1 = (Iv * fy) / m2, gm2 = -((gm0 * m0 + gm1 * m1) / m2)          dI/dm through u' = fx m0 / m2 + cx
//   r = lambda * (I - yf),  n_k = lambda * ((Rm[k][0] gm0 + Rm[k][1] gm1) + Rm[k][2] gm2)   dr/dq = Rm dr/dm, as for the plane
DR_HOST_DEVICE inline bool track_photo_term(const TrackModel &t, const TrackColour &tc, const LocateGrid &lg, const double m[3], double up, double vp, float yf,
                                            double &r, double n[3]) {
  const double fu = floor(up), fv = floor(vp);
  if (!(fu >= 0.0 && fu + 1.0 <= (double)(lg.W - 1) && fv >= 0.0 && fv + 1.0 <= (double)(lg.H - 1))) return false;
  const size_t at = (size_t)(int)fv * (size_t)lg.W + (size_t)(int)fu;
  TrackPair top, bot;
  memcpy(&top, tc.Ym + at, sizeof top);
  memcpy(&bot, tc.Ym + at + (size_t)lg.W, sizeof bot);
  if (!(top.a >= 0.0f && top.b >= 0.0f && bot.a >= 0.0f && bot.b >= 0.0f)) return false;
  const double y00 = (double)top.a, y10 = (double)top.b, y01 = (double)bot.a, y11 = (double)bot.b;
  const double a = up - fu, b = vp - fv, oa = 1.0 - a, ob = 1.0 - b;
  const double I = ob * (oa * y00 + a * y10) + b * (oa * y01 + a * y11);
  const double Iu = ob * (y10 - y00) + b * (y11 - y01), Iv = oa * (y01 - y00) + a * (y11 - y10);
  const double gm0 = (Iu * (double)lg.fx) / m[2], gm1 = (Iv * (double)lg.fy) / m[2];
  const double gm2 = -((gm0 * m[0] + gm1 * m[1]) / m[2]);
  r = tc.weight * (I - (double)yf);
  n[0] = tc.weight * ((t.m.R[0] * gm0 + t.m.R[1] * gm1) + t.m.R[2] * gm2);
  n[1] = tc.weight * ((t.m.R[3] * gm0 + t.m.R[4] * gm1) + t.m.R[5] * gm2);
  n[2] = tc.weight * ((t.m.R[6] * gm0 + t.m.R[7] * gm1) + t.m.R[8] * gm2);
  return true;
}
// One sample with colour: track_sample's codes 0 (unassociated) and 2 (rejected) add nothing; otherwise the geometric term is
// added first and, where track_photo_term has one, the photometric term second: returns 1 for the one, 3 for both.  The two are
// trips of one loop, so that align_accumulate stands once in the kernel's instruction stream.
DR_HOST_DEVICE inline int track_colour_point(const AlignEval &e, const TrackModel &t, const TrackColour &tc, const LocateGrid &lg, double g0, double g1, double g2,
                                             float yf, double acc[28]) {
  return track_sample(e, t, lg, g0, g1, g2, [&](double r, double w0, double w1, double w2, const double *q, const double *m, double up, double vp) {
    double pr = 0.0, pn[3] = {0.0, 0.0, 0.0};
    const bool photo = track_photo_term(t, tc, lg, m, up, vp, yf, pr, pn);
    const int terms = photo ? 2 : 1;
    DR_NO_UNROLL
    for (int k = 0; k < terms; ++k) {
      const bool second = k == 1;
      align_accumulate(e, second ? pr : r, second ? pn[0] : w0, second ? pn[1] : w1, second ? pn[2] : w2, q, acc);
    }
    return photo ? 3 : 1;
  });
}
// Group i in the wave's order (locate_group's); counts += {samples, valid, unassociated, rejected, photometric terms added}.
inline void track_colour_group(const AlignEval &e, const TrackModel &t, const TrackColour &tc, const LocateGrid &lg, const unsigned char *bgr, const float *depth,
                               long i, double out[28], uint64_t counts[5]) {
  double x[64][28];
  const long total = locate_positions(lg);
  for (int l = 0; l < 64; ++l) {
    for (int c = 0; c < 28; ++c) x[l][c] = 0.0;
    for (int k = 0; k < 8; ++k) {
      const long n = 512 * i + l + 64 * k;
      double g[3];
      if (n >= total || !locate_pixel(lg, e.vs, (int)n, depth, g)) continue;
      ++counts[0];
      const int r = track_colour_point(e, t, tc, lg, g[0], g[1], g[2], track_intensity(bgr + 3 * locate_offset(lg, (int)n)), x[l]);
      ++counts[(r & 1) ? 1 : r == 0 ? 2 : 3];
      if (r == 3) ++counts[4];
    }
  }
  align_butterfly(x);
  for (int c = 0; c < 28; ++c) out[c] = x[0][c];
}
inline void track_colour_system_host(const LocateGrid &lg, const unsigned char *bgr, const float *depth, const TrackModel &t, const TrackColour &tc,
                                     const AlignEval &e, double sums[28], uint64_t counts[5]) {
  for (int c = 0; c < 5; ++c) counts[c] = 0;
  const size_t n = (size_t)locate_groups(lg);
  std::vector<double> partial(n * 28);
  for (size_t i = 0; i < n; ++i) track_colour_group(e, t, tc, lg, bgr, depth, (long)i, &partial[i * 28], counts);
  align_fold_host(partial.data(), n, sums);
}
// track_loop over an evaluator with five counters: the loop sees the first four, last5 (if given) receives all five of the last
// evaluation.  The render callback builds the model map and Ym from the colour and the depth it rendered.
template <class Render, class Eval>
inline void track_colour_loop(Render &&render, Eval &&eval, const float *pose_init16, const TrackColourOpt &o, float voxel_size, drf_align_result_t &res,
                              uint64_t *last5 = nullptr, uint64_t *stats2 = nullptr, std::vector<std::array<double, 28>> *trace = nullptr) {
  track_loop(render, [&](const AlignEval &e, const float *p16, double sums[28], uint64_t c4[4]) {
    uint64_t c5[5];
    eval(e, p16, sums, c5);
    memcpy(c4, c5, 4 * sizeof(uint64_t));
    if (last5) memcpy(last5, c5, sizeof c5);
  }, pose_init16, o.t, voxel_size, res, nullptr, stats2, trace);
}
// The whole tracking with colour on the CPU over any renderer render(const float pose16[16], unsigned char *Cm, float *Dm): the
// library's reference for drf_track_colour_frame, and what the sanitizer program runs.
template <class RenderBoth>
inline void track_colour_frame_host(const LocateGrid &lg, const unsigned char *bgr, const float *depth, RenderBoth &&render_both, const float *pose_init16,
                                    const TrackColourOpt &o, float voxel_size, drf_align_result_t &res, uint64_t *last5 = nullptr, uint64_t *stats2 = nullptr,
                                    std::vector<std::array<double, 28>> *trace = nullptr) {
  const size_t npix = (size_t)lg.W * (size_t)lg.H;
  std::vector<float> Dm(npix), Ym(npix);
  std::vector<unsigned char> Cm(npix * 3);
  std::vector<TrackPixel> map(npix);
  track_colour_loop([&](const float *p16) { render_both(p16, Cm.data(), Dm.data()); track_model_colour_host(lg, o.t.max_jump, Dm.data(), Cm.data(), map.data(), Ym.data()); },
                    [&](const AlignEval &e, const float *p16, double sums[28], uint64_t c5[5]) {
                      track_colour_system_host(lg, bgr, depth, track_model(p16, o.t, voxel_size, map.data()), track_colour(o, Ym.data()), e, sums, c5);
                    }, pose_init16, o, voxel_size, res, last5, stats2, trace);
}

}  // namespace dr
