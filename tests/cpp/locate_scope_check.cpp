// C entry points over the locate-scope part of tandem_amd/csrc/fusion_host.h for tests/test_locate_scope.py (plain g++, no HIP,
// no GPU): the slack, the drift bound, the selection one evaluation stages, and -- by brute force over every pixel, a list of
// depths and the eight corners, with align_point's own arithmetic -- the blocks an evaluation at a pose reads and how far its
// sample points lie from those of another pose.  tests/cpp/locate_scope_san.cpp includes this file and runs the same checks
// under the sanitizers.
#include <set>

#include "../../tandem_amd/csrc/fusion_host.h"

using namespace dr;
typedef unsigned long long u64;

static void fill(HostBlockStore &s, const u64 *keys, int n) {
  std::vector<uint8_t> v(4096, 0);
  for (int i = 0; i < n; ++i) s.put(keys[i], v.data());
}
// the lattice point q of pixel (u, v) at depth z under the loop's pose, as locate_pixel and align_point compute it
static void sample_q(const drf_options_t &o, const MapMotion &m, int u, int v, double z, double q[3]) {
  const double vs = (double)o.voxel_size;
  const double g0 = ((((double)u - (double)o.cx) / (double)o.fx) * z) / vs, g1 = ((((double)v - (double)o.cy) / (double)o.fy) * z) / vs, g2 = z / vs;
  for (int k = 0; k < 3; ++k) q[k] = ((m.R[3 * k] * g0 + m.R[3 * k + 1] * g1) + m.R[3 * k + 2] * g2) + m.tv[k];
}

extern "C" {

double ls_slack(const drf_options_t *o) { return locate_stage_slack(*o); }
double ls_drift(const drf_options_t *o, const float *a16, const float *b16) { return locate_pose_drift(*o, a16, b16); }
int ls_serves(const drf_options_t *o, const float *a16, const float *b16, double slack) { return locate_stage_serves(*o, a16, b16, slack) ? 1 : 0; }
// pose16 -> the loop's pose -> pose16 again: what the engine hands the two functions above
void ls_round_trip(const float *pose16, float voxel_size, float *out16) { locate_pose16(map_motion(pose16, voxel_size), voxel_size, out16); }

// what one evaluation at pose16 stages of a store holding keys[0, n): ascending; returns the count
int ls_select(const u64 *keys, int n, const drf_options_t *o, const float *pose16, u64 *out, int cap) {
  HostBlockStore store;
  fill(store, keys, n);
  const std::vector<u64> v = select_locate_blocks(store, *o, pose16);
  for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
  return (int)v.size();
}
// every block an evaluation at pose16 reads for the pixels [0, W-1] x [0, H-1] at the nd depths: ascending keys; returns the count
int ls_blocks_read(const drf_options_t *o, const float *pose16, const double *depths, int nd, u64 *out, int cap) {
  const MapMotion m = map_motion(pose16, o->voxel_size);
  std::set<u64> seen;
  for (int v = 0; v < o->height; ++v)
    for (int u = 0; u < o->width; ++u)
      for (int d = 0; d < nd; ++d) {
        double q[3];
        sample_q(*o, m, u, v, depths[d], q);
        for (int c = 0; c < 8; ++c) {
          const int b[3] = {((int)std::floor(q[0]) + (c >> 2)) >> 3, ((int)std::floor(q[1]) + ((c >> 1) & 1)) >> 3, ((int)std::floor(q[2]) + (c & 1)) >> 3};
          u64 k;
          if (pack_key_host(b, k)) seen.insert(k);
        }
      }
  int n = 0;
  for (u64 k : seen) {
    if (n < cap) out[n] = k;
    ++n;
  }
  return n;
}
// the largest distance, in metres, between the sample points of poses a16 and b16 over the same pixels and depths
double ls_max_displacement(const drf_options_t *o, const float *a16, const float *b16, const double *depths, int nd) {
  const MapMotion ma = map_motion(a16, o->voxel_size), mb = map_motion(b16, o->voxel_size);
  double far = 0.0;
  for (int v = 0; v < o->height; ++v)
    for (int u = 0; u < o->width; ++u)
      for (int d = 0; d < nd; ++d) {
        double qa[3], qb[3];
        sample_q(*o, ma, u, v, depths[d], qa);
        sample_q(*o, mb, u, v, depths[d], qb);
        far = std::max(far, std::sqrt((qa[0] - qb[0]) * (qa[0] - qb[0]) + (qa[1] - qb[1]) * (qa[1] - qb[1]) + (qa[2] - qb[2]) * (qa[2] - qb[2])));
      }
  return far * (double)o->voxel_size;
}

}  // extern "C"
