// C entry points over tandem_amd/csrc/fusion_host.h for tests/test_fusion_host.py (plain g++, no HIP, no GPU): the test drives
// them through ctypes and compares with restatements written in Python.
#include "../../tandem_amd/csrc/fusion_host.h"

using namespace dr;
typedef unsigned long long u64;

static std::vector<u64> vec(const u64 *p, int n) { return std::vector<u64>(p, p + n); }
static BlockRange range_of(const int *r6) {
  BlockRange r;
  for (int a = 0; a < 3; ++a) { r.lo[a] = r6[a]; r.hi[a] = r6[3 + a]; }
  return r;
}
// a store that holds `keys`; voxel bytes derived from the key
static void fill(HostBlockStore &s, const u64 *keys, int n) {
  std::vector<uint8_t> v(4096);
  for (int i = 0; i < n; ++i) {
    memset(v.data(), (int)(keys[i] * 2654435761u >> 24), 4096);
    s.put(keys[i], v.data());
  }
}

extern "C" {

int fh_pack(int x, int y, int z, u64 *k) { const int c[3] = {x, y, z}; return pack_key_host(c, *k) ? 1 : 0; }
void fh_unpack(u64 k, int *c) { unpack_key_host(k, c); }
u64 fh_cell_key(u64 k) { return cell_key(k); }
int fh_f2i(float f) { return f2i_host(f); }

float fh_min_radius(const drf_options_t *o) { return streaming_min_radius(*o); }
int fh_options_ok(const drf_options_t *o) { return stream_options_ok(*o) ? 1 : 0; }
float fh_update_reach2(const drf_options_t *o) { return mesh_update_reach2(*o); }
float fh_max_valid_depth(const float *d, size_t n, float lo, float hi) { return max_valid_depth(d, n, lo, hi); }

void *fh_store_new() { return new HostBlockStore(); }
void fh_store_free(void *s) { delete (HostBlockStore *)s; }
void fh_store_put(void *s, u64 k, const uint8_t *vox) { ((HostBlockStore *)s)->put(k, vox); }
void fh_store_get(void *s, u64 k, uint8_t *vox) { memcpy(vox, ((HostBlockStore *)s)->get(k), 4096); }
void fh_store_erase(void *s, u64 k) { ((HostBlockStore *)s)->erase(k); }
int fh_store_contains(void *s, u64 k) { return ((HostBlockStore *)s)->contains(k) ? 1 : 0; }
size_t fh_store_size(void *s) { return ((HostBlockStore *)s)->size(); }
int fh_store_sorted_keys(void *s, u64 *out) {
  const std::vector<u64> k = ((HostBlockStore *)s)->sorted_keys();
  std::copy(k.begin(), k.end(), out);
  return (int)k.size();
}
int fh_store_query(void *s, const double *p, double r, float vs, u64 *out, int cap) {
  std::vector<u64> v;
  ((HostBlockStore *)s)->query_sphere(p, r, vs, v);
  for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
  return (int)v.size();
}

void *fh_balls_new() { return new ReachBalls(); }
void fh_balls_free(void *b) { delete (ReachBalls *)b; }
void fh_balls_reset(void *b) { ((ReachBalls *)b)->reset(); }
void fh_balls_add(void *b, const double *p, double r) { ((ReachBalls *)b)->add(p, r); }
double fh_balls_farthest(void *b, const double *p) { return ((ReachBalls *)b)->farthest(p); }
int fh_balls_get(void *b, double *out4) {  // out4: [size][4]
  const auto &rb = ((ReachBalls *)b)->balls();
  for (size_t i = 0; i < rb.size(); ++i) memcpy(out4 + 4 * i, rb[i].data(), 32);
  return (int)rb.size();
}

void fh_block_range(const float *lower, const int *n, float vs, int *r6) {
  const BlockRange r = lattice_block_range(lower, n, vs);
  for (int a = 0; a < 3; ++a) { r6[a] = r.lo[a]; r6[3 + a] = r.hi[a]; }
}
// out: the merged in-range keys; flags: 1 = stored
int fh_merged(const u64 *res, int nres, const u64 *sto, int nsto, const int *r6, u64 *out, uint8_t *flags) {
  int m = 0;
  for_each_in_range(vec(res, nres), vec(sto, nsto), range_of(r6), [&](u64 k, bool stored) { out[m] = k; flags[m] = stored; ++m; });
  return m;
}
// npicked < 0: no selection.  sizes: own, stg, chunks
void *fh_plan(const u64 *res, int nres, const u64 *sto, int nsto, const int *r6, size_t own_cap, size_t stage_cap, const u64 *picked, int npicked, size_t *sizes) {
  HostBlockStore store;
  fill(store, sto, nsto);
  const std::vector<u64> pk = npicked < 0 ? std::vector<u64>() : vec(picked, npicked);
  MeshPlan *p = new MeshPlan(plan_mesh_chunks(vec(res, nres), store.sorted_keys(), store, range_of(r6), own_cap, stage_cap, npicked < 0 ? nullptr : &pk));
  sizes[0] = p->own.size(); sizes[1] = p->stg.size(); sizes[2] = p->chunks();
  return p;
}
void fh_plan_get(void *h, u64 *own, u64 *stg, size_t *ob, size_t *sb) {
  const MeshPlan &p = *(MeshPlan *)h;
  std::copy(p.own.begin(), p.own.end(), own);
  std::copy(p.stg.begin(), p.stg.end(), stg);
  std::copy(p.ob.begin(), p.ob.end(), ob);
  std::copy(p.sb.begin(), p.sb.end(), sb);
}
void fh_plan_free(void *h) { delete (MeshPlan *)h; }

}  // extern "C"
