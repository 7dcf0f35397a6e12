// plan_render_bands (tandem_amd/csrc/fusion_host.h) as a stand-alone program for a sanitizer build: seeded block clouds, one to
// three poses (rigid, and one that is not), capacities from "everything fits" down to zero.  Checks the invariants that need no
// restatement: boundaries ascending from 0 to max_sensor_depth, every pass ascending, unique and within the capacity, the union
// of the passes equal to the one-pass union.
#include <cstdio>
#include <random>

#include "../../tandem_amd/csrc/fusion_host.h"

using namespace dr;
typedef unsigned long long u64;

static int fail(const char *what, int seed, size_t cap) {
  fprintf(stderr, "render_bands_san: %s (seed %d, capacity %zu)\n", what, seed, cap);
  return 1;
}

int main() {
  drf_options_t o{};
  o.voxel_size = 0.01f; o.num_buckets = 1000; o.bucket_size = 10; o.num_blocks = 1000; o.block_size = 8; o.max_sdf_weight = 64;
  o.truncation_distance = 0.04f; o.max_sensor_depth = 3.0f; o.min_sensor_depth = 0.1f; o.num_render_streams = 1;
  o.fx = 100.0f; o.fy = 100.0f; o.cx = 63.5f; o.cy = 47.5f; o.height = 96; o.width = 128;
  size_t plans = 0, banded = 0, refused = 0;
  for (int seed = 0; seed < 6; ++seed) {
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> c(-38, 38);
    HostBlockStore store;
    std::vector<uint8_t> vox(4096, 0);
    for (int i = 0; i < 20000; ++i) {
      const int b[3] = {c(rng), c(rng), c(rng)};
      u64 k;
      if (pack_key_host(b, k) && !store.contains(k)) store.put(k, vox.data());
    }
    float poses[3][16] = {};
    const int np = 1 + seed % 3;
    for (int p = 0; p < 3; ++p) {  // rotations about y, camera centres near the origin
      const float a = 0.7f * (float)p + 0.3f * (float)seed, cs = std::cos(a), sn = std::sin(a);
      const float m[16] = {cs, 0, sn, 0.1f * (float)p, 0, 1, 0, -0.05f, -sn, 0, cs, 0.2f, 0, 0, 0, 1};
      memcpy(poses[p], m, sizeof m);
    }
    if (seed == 5) poses[0][1] += 0.05f;  // not rigid: its selection is the whole store, in every pass
    const float *pp[3] = {poses[0], poses[1], poses[2]};
    const RenderStagePlan one = plan_render_stage(store, o, pp, np);
    const size_t caps[] = {one.keys.size() + 5, one.keys.size(), one.keys.size() * 3 / 4, one.keys.size() / 2, one.keys.size() / 3, one.keys.size() / 8, 40, 1, 0};
    for (size_t cap : caps)
      for (int max_passes : {2, 5, 64}) {
        const RenderBandPlan p = plan_render_bands(store, o, pp, np, cap, max_passes);
        ++plans;
        if (!p.ok) { ++refused; if (cap >= one.keys.size()) return fail("a union that fits was refused", seed, cap); continue; }
        const size_t P = p.keys.size();
        if (P < 1 || (int)P > max_passes || p.z.size() != P + 1) return fail("number of passes", seed, cap);
        if (p.z[0] != 0.0f || !(p.z[P] >= o.max_sensor_depth)) return fail("first or last boundary", seed, cap);
        std::vector<u64> all;
        for (size_t j = 0; j < P; ++j) {
          if (!(p.z[j] < p.z[j + 1])) return fail("boundaries not ascending", seed, cap);
          if (p.keys[j].size() > cap) return fail("a pass beyond the capacity", seed, cap);
          for (size_t i = 1; i < p.keys[j].size(); ++i)
            if (!(p.keys[j][i - 1] < p.keys[j][i])) return fail("a pass not ascending", seed, cap);
          all.insert(all.end(), p.keys[j].begin(), p.keys[j].end());
        }
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
        if (all != one.keys) return fail("the passes' union is not the one-pass union", seed, cap);
        if (cap >= one.keys.size() && P != 1) return fail("a union that fits took more than one pass", seed, cap);
        banded += P > 1;
      }
  }
  HostBlockStore empty;
  float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float *pp[1] = {id};
  const RenderBandPlan e = plan_render_bands(empty, o, pp, 1, 0, 2);
  if (!e.ok || e.keys.size() != 1 || !e.keys[0].empty()) return fail("empty store", -1, 0);
  if (banded < 5 || refused < 5) return fail("the cases must both band and refuse", (int)banded, refused);
  printf("render_bands_san ok: %zu plans, %zu banded, %zu refused\n", plans, banded, refused);
  return 0;
}
