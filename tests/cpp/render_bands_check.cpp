// C entry points over the depth-band planner of tandem_amd/csrc/fusion_host.h (plan_render_bands) for
// tests/test_fusion_render_bands.py and, to choose a capacity, tests/test_fusion_render_bands_gpu.py (plain g++, no HIP, no GPU).
#include "../../tandem_amd/csrc/fusion_host.h"

using namespace dr;
typedef unsigned long long u64;

static void fill(HostBlockStore &s, const u64 *keys, int n) {
  std::vector<uint8_t> v(4096, 0);
  for (int i = 0; i < n; ++i) s.put(keys[i], v.data());
}

extern "C" {

double rb_margin(const drf_options_t *o) { return render_margin(*o); }

// the selection of one pose (any order); *cut = 1 if the frustum cut was applied, i.e. the blocks carry a depth
int rb_select(const u64 *keys, int n, const drf_options_t *o, const float *pose16, u64 *out, int cap, int *cut) {
  HostBlockStore store;
  fill(store, keys, n);
  std::vector<u64> v;
  std::vector<double> bz;
  select_render_blocks(store, *o, pose16, v, &bz);
  *cut = 1;
  for (double z : bz) if (std::isnan(z)) *cut = 0;
  for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
  return (int)v.size();
}
// the union one RenderAsync stages in one pass (plan_render_stage)
int rb_union(const u64 *keys, int n, const drf_options_t *o, const float *poses, int nposes, u64 *out, int cap) {
  HostBlockStore store;
  fill(store, keys, n);
  std::vector<const float *> pp;
  for (int i = 0; i < nposes; ++i) pp.push_back(poses + 16 * i);
  const RenderStagePlan p = plan_render_stage(store, *o, pp.data(), nposes);
  for (size_t i = 0; i < p.keys.size() && (int)i < cap; ++i) out[i] = p.keys[i];
  return (int)p.keys.size();
}
// plan_render_bands: returns the number of passes, or -1 if there is no plan.  z[passes + 1] boundaries (z_cap >= 65),
// count[passes] blocks per pass (count_cap >= 64), the passes' keys one after the other in out (as far as cap reaches); *total
// = their number.
int rb_plan(const u64 *keys, int n, const drf_options_t *o, const float *poses, int nposes, size_t capacity, int max_passes, float *z, int *count,
            u64 *out, int cap, int *total) {
  HostBlockStore store;
  fill(store, keys, n);
  std::vector<const float *> pp;
  for (int i = 0; i < nposes; ++i) pp.push_back(poses + 16 * i);
  const RenderBandPlan p = plan_render_bands(store, *o, pp.data(), nposes, capacity, max_passes);
  *total = 0;
  if (!p.ok) return -1;
  for (size_t j = 0; j < p.z.size() && j < 65; ++j) z[j] = p.z[j];
  for (size_t j = 0; j < p.keys.size(); ++j) {
    if (j < 64) count[j] = (int)p.keys[j].size();
    for (u64 k : p.keys[j]) {
      if (*total < cap) out[*total] = k;
      ++*total;
    }
  }
  return (int)p.keys.size();
}

}  // extern "C"
