// tests/cpp/mvs_host_check.cpp -- C entry points over tandem_amd/csrc/mvs_host.h for tests/test_mvs_host.py (ctypes).  Plain g++, no HIP, no device.
#include "../../tandem_amd/csrc/mvs_host.h"

namespace dr { std::string &last_error_slot() { static std::string s; return s; } }
using namespace dr;

// image id -> the key the index files it under (the index never looks inside a key)
static void id_key(uint64_t id, uint64_t key[2]) { key[0] = id * 0x9e3779b97f4a7c15ull + 1; key[1] = ~id; }

extern "C" {

const char *mh_last_error() { return last_error_slot().c_str(); }

// ---- image key
void mh_image_key(const uint8_t *p, size_t n, int H, int W, uint64_t key[2]) { image_key(p, n, H, W, key); }

// ---- cache index
void *mh_index_new(int capacity) { auto *x = new FeatureIndex(); x->resize((size_t)capacity); return x; }
void mh_index_free(void *x) { delete (FeatureIndex *)x; }
// one window of image ids; state: fast, fill, miss; counters: hits, misses, batch windows, collisions
void mh_index_plan(void *p, int V, const uint64_t *ids, int *slot, int *state, uint64_t *counters) {
  FeatureIndex &x = *(FeatureIndex *)p;
  uint64_t keys[kMaxSrc + 1][2];
  for (int v = 0; v < V; ++v) id_key(ids[v], keys[v]);
  x.plan(V, keys);
  for (int v = 0; v < V; ++v) slot[v] = x.slot[v];
  state[0] = x.fast; state[1] = x.fill; state[2] = x.miss;
  counters[0] = x.hits; counters[1] = x.misses; counters[2] = x.batch_windows; counters[3] = x.collisions;
}
// what the engine's forward does to the index behind a planned window: the entries it fills become valid
void mh_index_commit(void *p, int V) {
  FeatureIndex &x = *(FeatureIndex *)p;
  if (x.fast && x.miss >= 0) x.set_valid(x.slot[x.miss]);
  if (x.fill) for (int v = 0; v < V; ++v) x.set_valid(x.slot[v]);
}
// ... and what it does when a hit turns out to be a key collision
void mh_index_collision(void *p) {
  FeatureIndex &x = *(FeatureIndex *)p;
  ++x.collisions;
  x.invalidate_all();
  x.fast = false; x.fill = false;
}
// entry e: 1 if it is valid and holds image `id`
int mh_index_holds(void *p, int e, uint64_t id) {
  const FeatureIndex::Entry &en = ((FeatureIndex *)p)->entry(e);
  uint64_t k[2];
  id_key(id, k);
  return en.valid && en.key[0] == k[0] && en.key[1] == k[1];
}

// ---- geometry.  c2ws: V contiguous 4x4; M: 3 x kMaxSrc x 12; planes: 3 x {dmin, interval, half_range, full_range, nsrc_f}
int mh_geometry(int H, int W, int V, int ref, const float *K9, const float *c2ws, float dmin, float dmax, float disc, const int *depth_num, const float *ratio,
                int view_aggregation, int shard_nsrc, float *M, float *planes, int *D, int *order, unsigned *rank) {
  return guarded([&] {
    BlobMeta meta{};
    for (int i = 0; i < 3; ++i) { meta.depth_num[i] = depth_num[i]; meta.ratio[i] = ratio[i]; }
    meta.view_aggregation = view_aggregation; meta.base = 8;
    const float *ptr[kMaxSrc + 1];
    for (int v = 0; v < V; ++v) ptr[v] = c2ws + 16 * v;
    const WindowGeometry g = plan_geometry(H, W, V, ref, K9, ptr, dmin, dmax, disc, meta, shard_nsrc);
    memcpy(order, g.order, sizeof g.order);
    for (int s = 0; s < 3; ++s) {
      const StageGeometry &t = g.stage[s];
      memcpy(M + s * kMaxSrc * 12, t.M, sizeof t.M);
      const float pl[5] = {t.dmin, t.interval, t.half_range, t.full_range, t.nsrc_f};
      memcpy(planes + 5 * s, pl, sizeof pl);
      D[s] = t.D;
    }
    *rank = g.filter_rank;
  });
}

// ---- blob and folds
int mh_blob_load(const char *path, void **out) { return guarded([&] { *out = new Blob(load_blob(path)); }); }
void mh_blob_free(void *b) { delete (Blob *)b; }
void mh_blob_meta(void *b, int *depth_num, float *ratio, int *va_base) {
  const Blob &x = *(Blob *)b;
  for (int i = 0; i < 3; ++i) { depth_num[i] = x.depth_num[i]; ratio[i] = x.ratio[i]; }
  va_base[0] = x.view_aggregation; va_base[1] = x.base;
}
int mh_blob_count(void *b) { return (int)((Blob *)b)->t.size(); }
// tensor i in the blob's (name) order: its name and dims; returns the number of dims
int mh_blob_tensor(void *b, int i, char *name, size_t cap, int *dims, size_t *count) {
  auto it = ((Blob *)b)->t.begin();
  std::advance(it, i);
  snprintf(name, cap, "%s", it->first.c_str());
  for (size_t k = 0; k < it->second.dims.size(); ++k) dims[k] = it->second.dims[k];
  *count = it->second.data.size();
  return (int)it->second.dims.size();
}
int mh_blob_data(void *b, const char *name, float *out) {
  return guarded([&] { const HostTensor &t = ((Blob *)b)->at(name); memcpy(out, t.data.data(), t.data.size() * 4); });
}
int mh_fold_bn(void *b, const char *prefix, int C, float *scale, float *bias) {
  return guarded([&] {
    std::vector<float> sc, bi;
    fold_bn(*(Blob *)b, prefix, C, sc, bi);
    memcpy(scale, sc.data(), C * 4); memcpy(bias, bi.data(), C * 4);
  });
}
// out: gw[32], gA1, gB1, gA2, gB2
int mh_fold_gate(void *b, int stage, int C, float *out) {
  return guarded([&] { const GateFold g = fold_gate(*(Blob *)b, stage, C); memcpy(out, &g, 36 * 4); });
}
int mh_compose_out3(void *b, float *wa, float *T, float *bint) {
  return guarded([&] {
    const Blob &x = *(Blob *)b;
    const Out3Fold f = compose_out3(x.at("feature_net.out.stage3.weight").data, x.at("feature_net.skip.stage3.weight").data, x.at("feature_net.skip.stage3.bias").data);
    memcpy(wa, f.wa.data(), f.wa.size() * 4); memcpy(T, f.T.data(), f.T.size() * 4); memcpy(bint, f.bint.data(), f.bint.size() * 4);
  });
}
int mh_prob_taps(void *b, int stage, float *out) {
  return guarded([&] {
    const std::vector<float> wt = prob_taps(((Blob *)b)->at("cost_regularization_net.stage" + std::to_string(stage) + ".prob.weight").data);
    memcpy(out, wt.data(), wt.size() * 4);
  });
}
void mh_pad_cin(const float *w, int c_out, int c_in_real, int c_in, int taps, float *out) {
  const std::vector<float> p = pad_cin(std::vector<float>(w, w + (size_t)c_out * c_in_real * taps), c_out, c_in_real, c_in, taps);
  memcpy(out, p.data(), p.size() * 4);
}

// ---- kernel choice: the names drm_profile prints for the cost volume and the prob head of an H x W x V window (bordered feature maps, the product's
// switches with DR_PROB_ZCHUNK = prob_zchunk and DR_CV_DCHUNKs = cv_dchunk); regress[s] = the plane count k_regress_r is instantiated for (0: k_regress)
void mh_choice_names(int H, int W, int V, const int *depth_num, int view_aggregation, int prob_zchunk, int cv_dchunk, char *costvol, char *prob, size_t cap, int *regress,
                     int *prob_regresses) {
  MvsSwitches sw;
  sw.prob_zchunk = prob_zchunk;
  for (int &d : sw.cv_dchunk) d = cv_dchunk;
  for (int s = 1; s <= 3; ++s) {
    const int sc = 1 << (3 - s), h = H / sc, w = W / sc, D = depth_num[s - 1];
    const CostVolShape cs{V, h, w, D, costvol_dchunk(s, D, view_aggregation, 1, sw), 1, view_aggregation};
    choose_costvol(cs, sw, s).name(costvol + (s - 1) * cap, cap);
    const ProbChoice pc = choose_prob(ProbShape{D, h, w}, sw, s);
    pc.name(prob + (s - 1) * cap, cap);
    prob_regresses[s - 1] = pc.regresses();
    regress[s - 1] = choose_regress(D, sw);
  }
}

}  // extern "C"
