// C entry points over the search-scope part of tandem_amd/csrc/fusion_host.h and engine_host.h for tests/test_search_scope.py (plain
// g++, no HIP, no GPU): select_render_blocks with and without its widening, the selection of a unit of candidates, the float pose
// of a candidate, the pose table of a search and plan_search_stage.  tests/cpp/search_scope_san.cpp includes this file and runs
// the plan under the sanitizers.
#include "../../tandem_amd/csrc/fusion_host.h"

using namespace dr;
typedef unsigned long long u64;

static void fill(HostBlockStore &s, const u64 *keys, int n) {
  std::vector<uint8_t> v(4096, 0);
  for (int i = 0; i < n; ++i) s.put(keys[i], v.data());
}
static int hand_out(std::vector<u64> &v, u64 *out, int cap) {
  std::sort(v.begin(), v.end());
  for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
  return (int)v.size();
}
// N[3], half[3], dstep, plain as the test passes them
static SearchLattice lattice(const int *half, double dstep, int plain) {
  SearchLattice L;
  for (int k = 0; k < 3; ++k) { L.half[k] = plain ? 0 : half[k]; L.N[k] = 2 * L.half[k] + 1; }
  L.dstep = plain ? 0.0 : dstep;
  L.plain = plain;
  return L;
}

extern "C" {

// select_render_blocks at pose16 over a store of keys[0, n): with_extra = 0 calls it without the argument.  Ascending; returns the
// count, negated - 1 if the function returned false (the whole store).
int ss_select(const u64 *keys, int n, const drf_options_t *o, const float *pose16, int with_extra, double extra, u64 *out, int cap) {
  HostBlockStore store;
  fill(store, keys, n);
  std::vector<u64> v;
  const bool cut = with_extra ? select_render_blocks(store, *o, pose16, v, nullptr, extra) : select_render_blocks(store, *o, pose16, v);
  const int m = hand_out(v, out, cap);
  return cut ? m : -m - 1;
}
// search_table; returns 0, or 1 if it refuses
int ss_table(const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot, float voxel_size, double *table) {
  std::vector<double> t;
  if (!search_table(anchors16, n_anchors, rotations9, n_rot, voxel_size, t).empty()) return 1;
  memcpy(table, t.data(), t.size() * 8);
  return 0;
}
// n float poses as the plain table the engine makes of them
void ss_plain_table(const float *poses16, size_t n, float voxel_size, double *table) {
  for (size_t i = 0; i < n; ++i) {
    const MapMotion m = map_motion(poses16 + 16 * i, voxel_size);
    memcpy(table + 12 * i, m.R, 72);
    memcpy(table + 12 * i + 9, m.tv, 24);
  }
}
// the float pose of candidate c, and its double pose (12: R then tv)
void ss_candidate(const double *table, const int *half, double dstep, int plain, size_t c, float voxel_size, float *pose16, double *Rtv) {
  const MapMotion m = search_candidate(lattice(half, dstep, plain), table, 0, c);
  locate_pose16(m, voxel_size, pose16);
  memcpy(Rtv, m.R, 72);
  memcpy(Rtv + 9, m.tv, 24);
}
// the selection of the unit [x0, x1) of entry e
int ss_unit(const u64 *keys, int n, const drf_options_t *o, const double *table, const int *half, double dstep, int plain, size_t e, int x0, int x1, u64 *out,
            int cap) {
  HostBlockStore store;
  fill(store, keys, n);
  std::vector<u64> v = select_search_unit(store, *o, table, lattice(half, dstep, plain), e, x0, x1);
  for (size_t i = 1; i < v.size(); ++i)
    if (!(v[i - 1] < v[i])) return -1;
  return hand_out(v, out, cap);
}
// plan_search_stage: per pass first, count and number of keys, the keys of all passes one after the other.  Returns the number
// of passes, -1 for a failed plan (*too_many = its count), -2 if the outputs are too small.
int ss_plan(const u64 *keys, int n, const drf_options_t *o, const double *table, const int *half, double dstep, int plain, size_t ncand, size_t capacity,
            u64 *first, u64 *count, u64 *nkeys, int max_passes, u64 *all_keys, size_t max_keys, u64 *too_many) {
  HostBlockStore store;
  fill(store, keys, n);
  const SearchStagePlan p = plan_search_stage(store, *o, table, lattice(half, dstep, plain), ncand, capacity);
  *too_many = p.too_many;
  if (!p.ok) return p.passes.empty() ? -1 : -3;
  if ((int)p.passes.size() > max_passes) return -2;
  size_t at = 0;
  for (size_t i = 0; i < p.passes.size(); ++i) {
    first[i] = p.passes[i].first; count[i] = p.passes[i].count; nkeys[i] = p.passes[i].keys.size();
    if (at + p.passes[i].keys.size() > max_keys) return -2;
    for (u64 k : p.passes[i].keys) all_keys[at++] = k;
  }
  return (int)p.passes.size();
}

}  // extern "C"
