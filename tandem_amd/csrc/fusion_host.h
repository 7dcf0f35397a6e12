// fusion_host.h -- the host half of DrFusion's map: block keys, streaming reach bounds, the host block store, the reach balls,
// the planner of the map-scope mesh pass, the rule and planner of a map merge, the rule and planner of a rigid resample, the ledger of
// the incremental mesh (MeshUpdateLedger; tests/cpp/mesh_ledger_check.cpp).  The pose
// solvers over all this -- registration, localisation, tracking -- are pose_host.h, and the engine's call order and restaging rule
// engine_host.h (tests/cpp/engine_host_check.cpp), both included at the end.  No device state and no
// HIP header: plain C++17, so that all of it runs in the CPU tests (tests/cpp/fusion_host_check.cpp, tests/cpp/map_merge_check.cpp,
// tests/cpp/map_transform_check.cpp).  The engine (dr_fusion.hip) keeps everything that throws or touches the GPU.
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
// extra >= 0, in metres, widens the selection (the search scope, below): the sphere's reach and every half-space margin grow by it.
// With extra = 0 every sum below adds 0.0 to a positive number: the selection is the one without the argument, bit for bit.
inline bool select_render_blocks(const HostBlockStore &store, const drf_options_t &o, const float *pose16, std::vector<unsigned long long> &out,
                                 std::vector<double> *bz = nullptr, double extra = 0.0) {
  const double reach = stream_options_ok(o) ? render_reach(o) : HUGE_VAL;
  if (!pose_is_rigid(pose16) || !std::isfinite(reach) || !(extra >= 0.0) || !std::isfinite(extra)) {
    store.for_each([&](unsigned long long k, const uint8_t *) { out.push_back(k); });
    if (bz) bz->resize(bz->size() + store.size(), (double)NAN);
    return false;
  }
  double p[3];
  camera_centre(pose16, p);
  const size_t first = out.size();
  const double m = render_margin(o) + extra, vs = o.voxel_size, D = o.max_sensor_depth;
  // R R^T differs from I by < 1e-3 per entry (norm < 3e-3): R scales lengths by at most 1.5e-3, and b = R^T (c - t), which
  // stands in for the inverse below, is off by less than 4e-3 |c - t|.  Where the 8 s + vs of margin covers that, sphere and cut
  // stand as derived; where it does not (depth above ~10^4 voxels) the sphere grows by the error and the cut is not applied.
  if (4e-3 * reach > 8.0 * std::sqrt(3.0) * vs + vs) {
    store.query_sphere(p, reach * (1.0 + 4e-3) + extra, o.voxel_size, out);
    if (bz) bz->resize(bz->size() + (out.size() - first), (double)NAN);
    return true;
  }
  store.query_sphere(p, reach + extra, o.voxel_size, out);
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
// ---- the search scope (DRF_SEARCH_MAP; DESIGN.md §7c "Searching the whole map"): which stored blocks the score of a whole set of
// candidates can read.  A unit is a run of consecutive candidates with one rotation R whose translations lie in a box: centre t_c,
// half-diagonal h (metres).  The sample points of a candidate are R g + t over the frame's points g, so those of candidate t are
// those of the centre pose moved by t - t_c: by at most h, whatever R is.  A block the candidate reads has its centre within
// 4.5 sqrt(3) vs of one of its sample points (the locate scope's argument, above), so within 4.5 sqrt(3) vs + h of a sample point
// of the centre pose.  select_render_blocks keeps what lies within render_margin of an intersection of six half-spaces and a ball
// that holds those sample points; a point within h of the intersection is within h of each half-space and of the ball, so with every
// margin and the reach grown by `extra` >= h the selection at the centre pose holds every block any candidate of the unit reads.
// The same reading gives the statement the tests hold it to: a block of the plain selection at the candidate lies within margin
// of each half-space taken at t, hence within margin + |R^T (t - t_c)| of the one taken at t_c.  |R^T d| <= (1 + 1.5e-3) |d| for
// a pose that is rigid within pose_is_rigid's 1e-3, and b = R^T (c - t_c) is then off by 4e-3 of a length that is now up to
// reach + h, of which locate_stage_slack charges 4e-3 reach to the spare 8 sqrt(3) vs: extra = (1 + 4e-3) h covers both.
// Rounding: the candidates are evaluated at the double poses of the table (search_candidate) and only the centre pose is rounded
// to the floats select_render_blocks takes -- locate_pose16's bound, less than one voxel for every sample point, the vs that
// locate_stage_slack leaves out of the slack.  The box's centre and h are computed in double from exact small integers times
// dstep: their rounding is 2^-52 relative, far inside the same voxel.  A plain pose is a unit by itself with h = 0: the locate
// scope's selection.  plan_search_stage (engine_host.h) cuts a table of candidates into such units and the units into stagings.
inline double search_unit_extra(double half_diagonal) { return half_diagonal * (1.0 + 4e-3); }
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

// ---- the bookkeeping of the incremental mesh (drf_extract_mesh_update_async .. drf_get_mesh_update_sync; DESIGN.md §7c
// "Incremental mesh"): when an update must mesh every block of its box again, and which scans it folds in.  The baseline is the
// last update FETCHED: its box and the round-trip redirect count at its launch.  The pending update is decided by begin(), before
// anything is launched, and becomes the baseline at fetched().  The recorded poses are those of the scans since the last update
// was LAUNCHED: they belong to the next one.  mesh_ops.h MeshExtractor holds one and keeps the device scratch itself.
struct MuPose { float m[12]; };  // rows 0..2 of a scan's Ti (world -> camera); row 3 is 0 0 0 1
class MeshUpdateLedger {
 public:
  struct Update {
    bool valid = false, full = false;
    float box[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long redirects = 0; size_t nblk = 0;  // nblk: rows of its patch table
  };
  // A scan was integrated at Ti16 (world -> camera).  A pose that is not a finite rigid motion (the reach bound assumes one) or one
  // scan too many makes the next update full.
  void record_scan(const float *Ti16) {
    if (!pose_is_rigid(Ti16) || poses_.size() == (size_t)DRF_MESH_UPDATE_MAX_SCANS) { overflow_ = true; return; }
    MuPose p;
    memcpy(p.m, Ti16, 48);
    poses_.push_back(p);
  }
  void begin(const float *lower, const float *upper, unsigned long long redirects) {
    Update next;
    next.valid = true;
    next.redirects = redirects;
    memcpy(next.box, lower, 12); memcpy(next.box + 3, upper, 12);
    next.full = !base_.valid || force_full_ || overflow_ || memcmp(next.box, base_.box, 24) != 0 || next.redirects != base_.redirects;
    next_ = next;
  }
  void set_rows(size_t nblk) { next_.nblk = nblk; }  // of the pending update's patch table, once the launch knows them
  // the pending update is enqueued: the scans recorded so far belong to it, later ones to the next
  void launched() { force_full_ = false; overflow_ = false; poses_.clear(); }
  void fetched() { base_ = next_; }  // the baseline advances: this box, the voxel state at the launch
  void force_full() { force_full_ = true; }  // the map changed by something no scan pose describes (load, merge, the caller's reset)
  const Update &pending() const { return next_; }
  const Update &baseline() const { return base_; }
  const std::vector<MuPose> &poses() const { return poses_; }

 private:
  Update base_, next_;
  std::vector<MuPose> poses_;
  bool force_full_ = false, overflow_ = false;
};

}  // namespace dr

#include "pose_host.h"  // the pose solvers over all this: align, locate, track, colour
#include "engine_host.h"  // the engine's call order and the locate scope's restaging rule, as values (CallOrder, LocateStageCursor)
