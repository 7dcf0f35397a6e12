// C entry points over the render-scope part of tandem_amd/csrc/fusion_host.h for tests/test_fusion_render_scope.py (plain g++,
// no HIP, no GPU): which stored blocks a ray-cast can read, the union one RenderAsync stages, the capacity decision and the
// "need not wait for the scan" predicate.
#include "../../tandem_amd/csrc/fusion_host.h"

using namespace dr;
typedef unsigned long long u64;

static void fill(HostBlockStore &s, const u64 *keys, int n) {
  std::vector<uint8_t> v(4096, 0);
  for (int i = 0; i < n; ++i) s.put(keys[i], v.data());
}
static int copy_out(const std::vector<u64> &v, u64 *out, int cap) {
  for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
  return (int)v.size();
}

extern "C" {

double rs_reach(const drf_options_t *o) { return render_reach(*o); }
double rs_margin(const drf_options_t *o) { return render_margin(*o); }
float rs_min_radius(const drf_options_t *o) { return streaming_min_radius(*o); }
int rs_rigid(const float *pose16) { return pose_is_rigid(pose16) ? 1 : 0; }

// the selection of one pose, in the order select_render_blocks leaves it; *rigid = its return value
int rs_select(const u64 *keys, int n, const drf_options_t *o, const float *pose16, u64 *out, int cap, int *rigid) {
  HostBlockStore store;
  fill(store, keys, n);
  std::vector<u64> v;
  *rigid = select_render_blocks(store, *o, pose16, v) ? 1 : 0;
  return copy_out(v, out, cap);
}
// the sphere query the selection starts from
int rs_sphere(const u64 *keys, int n, const drf_options_t *o, const float *pose16, u64 *out, int cap) {
  HostBlockStore store;
  fill(store, keys, n);
  double p[3];
  camera_centre(pose16, p);
  std::vector<u64> v;
  store.query_sphere(p, render_reach(*o), o->voxel_size, v);
  return copy_out(v, out, cap);
}
// what one RenderAsync over nposes poses (16 floats each) stages; *whole = poses that selected the whole store; *fits = the
// capacity decision for `capacity` blocks
int rs_plan(const u64 *keys, int n, const drf_options_t *o, const float *poses, int nposes, size_t capacity, u64 *out, int cap, int *whole, int *fits) {
  HostBlockStore store;
  fill(store, keys, n);
  std::vector<const float *> pp;
  for (int i = 0; i < nposes; ++i) pp.push_back(poses + 16 * i);
  const RenderStagePlan p = plan_render_stage(store, *o, pp.data(), nposes);
  *whole = p.whole;
  *fits = render_stage_fits(p, capacity) ? 1 : 0;
  return copy_out(p.keys, out, cap);
}
int rs_needs_fold(const drf_options_t *o, const float *pose16, const double *scan_centre, double radius) {
  return render_needs_fold(*o, pose16, scan_centre, radius) ? 1 : 0;
}

}  // extern "C"
