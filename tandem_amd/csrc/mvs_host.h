// mvs_host.h -- the host half of the DrMvsnet engine (dr_mvsnet.hip), plain C++17 with no HIP header: g++ compiles it alone and the CPU suite
// tests it (tests/test_mvs_host.py, tests/cpp/mvs_host_check.cpp, tests/cpp/mvs_host_san.cpp).
//   Blob / load_blob / fold_bn / compose_out3 / fold_gate / prob_taps / pad_cin : the TDMW weight blob and every fold of its tensors
//   inv4 / mul4 / world_to_pixel / plan_geometry : the per-call camera geometry (homographies, plane ranges, filter rank)
//   image_key / FeatureIndex : the key-frame feature cache's index (which views hit, miss or fill; the LRU; the counters)
//   HostCopier : the helper thread of the operator boundary's host copies
//   MvsSwitches / choose_costvol / choose_prob / choose_regress : the DR_* switches and the ONE rule per kernel family that turns a stage's
//                shape and the switches into a kernel instance -- the launchers (mvs_launch.h) and drm_profile's names both ask it
// Device pointers, streams and launches stay in the engine and in mvs_launch.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <thread>

#include "dr_host.h"

namespace dr {

constexpr int kMaxSrc = 7;  // view_num <= 8

// ------------------------------------------------------------------ TDMW blob (tandem_amd/weights.py)
struct HostTensor {
  std::vector<int> dims;
  std::vector<float> data;
};
struct BlobMeta {
  int depth_num[3];
  float ratio[3];
  int view_aggregation, base;
};
struct Blob : BlobMeta {
  std::map<std::string, HostTensor> t;
  const HostTensor &at(const std::string &k) const {
    auto it = t.find(k);
    if (it == t.end()) fail(DR_ERR_IO, "weight blob: missing tensor %s", k.c_str());
    return it->second;
  }
};

inline Blob load_blob(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) fail(DR_ERR_IO, "cannot open weight blob %s", path);
  Blob b;
  char magic[8];
  auto rd = [&](void *p, size_t n) {
    if (fread(p, 1, n, f) != n) { fclose(f); fail(DR_ERR_IO, "weight blob %s truncated", path); }
  };
  rd(magic, 8);
  if (memcmp(magic, "TDMW0001", 8)) { fclose(f); fail(DR_ERR_IO, "%s is not a TDMW blob", path); }
  rd(b.depth_num, 12); rd(b.ratio, 12); rd(&b.view_aggregation, 4); rd(&b.base, 4);
  uint32_t n;
  rd(&n, 4);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t ln, nd;
    rd(&ln, 4);
    std::string name(ln, '\0');
    rd(&name[0], ln);
    rd(&nd, 4);
    HostTensor t;
    size_t cnt = 1;
    for (uint32_t k = 0; k < nd; ++k) { uint32_t d; rd(&d, 4); t.dims.push_back((int)d); cnt *= d; }
    t.data.resize(cnt);
    rd(t.data.data(), cnt * 4);
    b.t[name] = std::move(t);
  }
  fclose(f);
  if (b.base != 8) fail(DR_ERR_UNSUPPORTED, "only feature_net_base_channels=8 is supported (got %d)", b.base);
  return b;
}

// ------------------------------------------------------------------ weight folds
inline void fold_bn(const Blob &blob, const std::string &p, int C, std::vector<float> &sc, std::vector<float> &bi) {
  const auto &g = blob.at(p + ".weight").data, &b = blob.at(p + ".bias").data;
  const auto &m = blob.at(p + ".running_mean").data, &v = blob.at(p + ".running_var").data;
  sc.resize(C); bi.resize(C);
  for (int c = 0; c < C; ++c) {
    const double s = (double)g[c] / std::sqrt((double)v[c] + 1e-5);
    sc[c] = (float)s;
    bi[c] = (float)((double)b[c] - (double)m[c] * s);
  }
}
// out.stage3 (3x3, 32 -> 8) composed with skip.stage3 (1x1, 8 -> 32, bias b3): the 8 x 8 x 9 weights of the composed layer, the 9 x 8 table
// T[tap][cout] = Wout[tap] . bskip that the border kernel subtracts where a tap falls outside the image, and the interior bias (the sum over taps)
struct Out3Fold { std::vector<float> wa, T, bint; };
inline Out3Fold compose_out3(const std::vector<float> &wo3, const std::vector<float> &w3, const std::vector<float> &b3) {
  Out3Fold f;
  std::vector<float> &wa = f.wa, &T = f.T, &bint = f.bint;
  wa.resize((size_t)8 * 8 * 9); T.resize(9 * 8); bint.assign(8, 0.f);
  for (int co = 0; co < 8; ++co)
    for (int t = 0; t < 9; ++t) {
      for (int c8 = 0; c8 < 8; ++c8) {
        double acc = 0;
        for (int c = 0; c < 32; ++c) acc += (double)wo3[((size_t)co * 32 + c) * 9 + t] * (double)w3[(size_t)c * 8 + c8];
        wa[((size_t)co * 8 + c8) * 9 + t] = (float)acc;
      }
      double tb = 0;
      for (int c = 0; c < 32; ++c) tb += (double)wo3[((size_t)co * 32 + c) * 9 + t] * (double)b3[c];
      T[t * 8 + co] = (float)tb;
    }
  for (int co = 0; co < 8; ++co) { double b = 0; for (int t = 0; t < 9; ++t) b += (double)T[t * 8 + co]; bint[co] = (float)b; }
  return f;
}
// the view-aggregation gate of stage s (conv 1x1 C -> 1, BN, ReLU, conv 1 -> 1, BN, ReLU): g = relu(A2 * relu(A1 * (gw . x) + B1) + B2)
struct GateFold { float gw[32]; float gA1, gB1, gA2, gB2; };
inline GateFold fold_gate(const Blob &blob, int s, int C) {
  GateFold a{};
  const std::string g = "volume_gates.stage" + std::to_string(s) + ".";
  const auto &w0 = blob.at(g + "0.weight").data;
  for (int c = 0; c < C; ++c) a.gw[c] = w0[c];
  auto bnf = [&](const std::string &bn, double &A, double &B) {
    const double ga = blob.at(bn + ".weight").data[0], be = blob.at(bn + ".bias").data[0];
    const double mu = blob.at(bn + ".running_mean").data[0], var = blob.at(bn + ".running_var").data[0];
    A = ga / std::sqrt(var + 1e-5); B = be - mu * A;
  };
  double A1, B1, A2, B2;
  bnf(g + "1", A1, B1); bnf(g + "4", A2, B2);
  const double b0 = blob.at(g + "0.bias").data[0], w3 = blob.at(g + "3.weight").data[0], b3 = blob.at(g + "3.bias").data[0];
  a.gA1 = (float)A1; a.gB1 = (float)(b0 * A1 + B1);
  a.gA2 = (float)(w3 * A2); a.gB2 = (float)(b3 * A2 + B2);
  return a;
}
// the prob head's weights (1,8,3,3,3) -> [tap][cin]
inline std::vector<float> prob_taps(const std::vector<float> &pw) {
  std::vector<float> wt(27 * 8);
  for (int ci = 0; ci < 8; ++ci) for (int t = 0; t < 27; ++t) wt[t * 8 + ci] = pw[ci * 27 + t];
  return wt;
}
// RGB -> RGB0: zero-pad the input-channel axis of (c_out, c_in_real, taps) weights to c_in
inline std::vector<float> pad_cin(const std::vector<float> &w, int c_out, int c_in_real, int c_in, int taps) {
  std::vector<float> padded((size_t)c_out * c_in * taps, 0.f);
  for (int co = 0; co < c_out; ++co) for (int ci = 0; ci < c_in_real; ++ci) for (int t = 0; t < taps; ++t)
    padded[((size_t)co * c_in + ci) * taps + t] = w[((size_t)co * c_in_real + ci) * taps + t];
  return padded;
}

// ------------------------------------------------------------------ small host math (double)
inline void inv4(const double *m, double *o) {  // Gauss-Jordan with partial pivoting
  double a[4][8];
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { a[i][j] = m[4 * i + j]; a[i][4 + j] = i == j; }
  for (int c = 0; c < 4; ++c) {
    int piv = c;
    for (int r = c + 1; r < 4; ++r) if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
    if (piv != c) for (int j = 0; j < 8; ++j) std::swap(a[c][j], a[piv][j]);
    const double d = a[c][c];
    for (int j = 0; j < 8; ++j) a[c][j] /= d;
    for (int r = 0; r < 4; ++r) if (r != c) { const double f = a[r][c]; for (int j = 0; j < 8; ++j) a[r][j] -= f * a[c][j]; }
  }
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) o[4 * i + j] = a[i][4 + j];
}
inline void mul4(const double *a, const double *b, double *o) {
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { double s = 0; for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j]; o[4 * i + j] = s; }
}
// world->pixel 4x4 = [K * W2C(3x4); 0 0 0 1]   (module.py:798-804)
inline void world_to_pixel(const float *K9, const double *w2c, double *o) {
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += (double)K9[3 * i + k] * w2c[4 * k + j]; o[4 * i + j] = s; }
  o[12] = w2c[12]; o[13] = w2c[13]; o[14] = w2c[14]; o[15] = w2c[15];
}

// ------------------------------------------------------------------ per-call geometry
// What a window's cameras and depth range decide, per stage and for the edge filter.  The engine copies a stage into CostVolArgs / RegressArgs
// and adds the device pointers.
struct StageGeometry {
  float M[kMaxSrc][12];          // per source view (model order): rows of [rot | trans] of ref-pixel -> src-pixel (module.py:795-809)
  int D;
  float dmin, interval;          // stage 1's uniform planes
  float half_range, full_range;  // stages 2 and 3 (0 at stage 1)
  float nsrc_f;                  // the cost volume's divisor
};
struct WindowGeometry {
  int order[kMaxSrc + 1];        // model order [ref, others] (dr_mvsnet.cpp:190-197)
  StageGeometry stage[3];
  unsigned filter_rank;
};
inline WindowGeometry plan_geometry(int H, int W, int V, int ref, const float *K9, const float *const *c2ws, float dmin, float dmax, float disc,
                                    const BlobMeta &meta, int shard_nsrc) {
  WindowGeometry g;
  memset(&g, 0, sizeof g);
  int n = 0;
  g.order[n++] = ref;
  for (int i = 0; i < V; ++i) if (i != ref) g.order[n++] = i;
  // view sharding: this rank's window holds a subset of the source views, the divisor stays the whole window's
  if (shard_nsrc && !meta.view_aggregation) fail(DR_ERR_UNSUPPORTED, "view sharding needs a view-aggregation model (the variance volume is not a sum over views)");
  // stage intrinsics: rows 0-1 x 0.25 / 0.5 / 1 (the C++ rule, dr_mvsnet.cpp:226-247)
  double w2c[8][16];
  for (int v = 0; v < V; ++v) {
    double c2w[16];
    for (int i = 0; i < 16; ++i) c2w[i] = c2ws[g.order[v]][i];
    inv4(c2w, w2c[v]);
  }
  const float base_interval = (dmax - dmin) / (float)(meta.depth_num[0] - 1);  // module.py:1493
  for (int s = 1; s <= 3; ++s) {
    const float f = s == 1 ? 0.25f : (s == 2 ? 0.5f : 1.f);
    float Ks[9];
    for (int i = 0; i < 9; ++i) Ks[i] = i < 6 ? (float)((double)f * (double)K9[i]) : K9[i];
    StageGeometry &p = g.stage[s - 1];
    const int D = meta.depth_num[s - 1];
    p.nsrc_f = shard_nsrc ? (float)shard_nsrc : (float)(V - 1);
    p.D = D; p.dmin = dmin; p.interval = base_interval;
    if (s > 1) {
      const float delta = meta.ratio[s - 1] * base_interval;  // cva_mvsnet.py:151
      p.half_range = ((float)D / 2.f) * delta;                // module.py:1518
      p.full_range = (float)D * delta;                        // module.py:1526
    }
    double r_w2p[16], r_p2w[16];
    world_to_pixel(Ks, w2c[0], r_w2p);
    inv4(r_w2p, r_p2w);
    for (int v = 1; v < V; ++v) {
      double s_w2p[16], M[16];
      world_to_pixel(Ks, w2c[v], s_w2p);
      mul4(s_w2p, r_p2w, M);
      for (int i = 0; i < 12; ++i) p.M[v - 1][i] = (float)M[i];
    }
  }
  // quantile rank, computed in float32 like module.py:1348-1349
  const float hw = (float)(H * W);
  float cut = hw * (100.f - disc);
  cut = cut / 100.f;
  long long ci = (long long)cut;
  if (ci < 0) ci = 0;
  if (ci > (long long)H * W - 1) ci = (long long)H * W - 1;
  g.filter_rank = (unsigned)ci;
  return g;
}

// ------------------------------------------------------------------ key-frame feature cache: the index
// a 128-bit key over a sample of the image: first / last 64 bytes + 511 evenly spaced 8-byte words (none when the image is shorter than 4 KiB)
inline void image_key(const uint8_t *p, size_t n, int H, int W, uint64_t key[2]) {
  uint64_t a = 0xcbf29ce484222325ull ^ (uint64_t)H, b = 0x9e3779b97f4a7c15ull ^ (uint64_t)W;
  auto mix = [&](uint64_t w) { a = (a ^ w) * 0x100000001b3ull; b = (b + w) * 0xff51afd7ed558ccdull; b ^= b >> 29; };
  auto word = [&](size_t off) { uint64_t w; memcpy(&w, p + off, 8); return w; };
  for (size_t o = 0; o < 64; o += 8) { mix(word(o)); mix(word(n - 64 + o)); }
  const size_t step = (n / 512) & ~(size_t)7;
  for (size_t k = 1; k < 512 && step; ++k) mix(word(k * step));
  key[0] = a; key[1] = b;
}
// Which entry answers which view of the window being staged.  Entries are indices; their device buffers live in the engine, in an array parallel
// to them.  plan() decides for one window: slot[v] = the entry that holds (or will hold) view v's features; fast = the cache answers the window
// (at most one view, `miss`, is computed); fill = the window is computed as a batch whose outputs fill the entries.  An entry that plan() hands to
// a view without a hit is invalid until the engine has enqueued its fill (set_valid).
class FeatureIndex {
 public:
  struct Entry { uint64_t key[2] = {0, 0}; uint64_t used = 0; bool valid = false; };
  void resize(size_t n) { e_.assign(n, Entry()); }
  void clear() { e_.clear(); }
  size_t size() const { return e_.size(); }
  const Entry &entry(int e) const { return e_[e]; }
  bool valid(int e) const { return e_[e].valid; }
  void set_valid(int e) { e_[e].valid = true; }
  void invalidate_all() { for (Entry &e : e_) e.valid = false; }
  void stand_down() { fast = false; fill = false; miss = -1; }  // the staged window takes the batch path and leaves the cache alone
  void plan(int V, const uint64_t (*keys)[2]) {
    stand_down();
    if ((int)e_.size() < V + 1) return;
    int nmiss = 0;
    ++clock_;
    for (int v = 0; v < V; ++v) {
      slot[v] = -1;
      for (size_t e = 0; e < e_.size(); ++e)
        if (e_[e].valid && e_[e].key[0] == keys[v][0] && e_[e].key[1] == keys[v][1]) { slot[v] = (int)e; break; }
      for (int u = 0; u < v; ++u) if (slot[v] >= 0 && slot[u] == slot[v]) slot[v] = -1;  // (two views with one key: only one may own the entry)
      if (slot[v] < 0) { ++nmiss; miss = v; } else e_[slot[v]].used = clock_;
    }
    auto evict = [&]() {  // the least recently used entry that this window does not use
      int best = -1;
      for (size_t e = 0; e < e_.size(); ++e) {
        bool in_window = false;
        for (int v = 0; v < V; ++v) in_window |= slot[v] == (int)e;
        if (!in_window && (best < 0 || !e_[e].valid || (e_[best].valid && e_[e].used < e_[best].used))) best = (int)e;
        if (best >= 0 && !e_[best].valid) break;
      }
      return best;
    };
    auto take = [&](int v) {
      const int e = evict();
      e_[e].valid = false;  // (valid again once a forward has enqueued its fill)
      e_[e].key[0] = keys[v][0]; e_[e].key[1] = keys[v][1]; e_[e].used = clock_;
      slot[v] = e;
    };
    if (nmiss <= 1) {
      fast = true;
      if (nmiss == 1) take(miss);
      hits += V - nmiss; misses += nmiss;
    } else {  // the batch path computes every view; its outputs fill the cache
      fill = true; miss = -1;
      for (int v = 0; v < V; ++v) if (slot[v] < 0) take(v);
      misses += V; ++batch_windows;
    }
  }
  int slot[kMaxSrc + 1] = {};
  int miss = -1;
  bool fast = false, fill = false;
  uint64_t hits = 0, misses = 0, batch_windows = 0, collisions = 0;

 private:
  std::vector<Entry> e_;
  uint64_t clock_ = 0;
};

// ------------------------------------------------------------------ helper thread
// One helper thread that takes half of the operator boundary's host copies (the window into the staging block, the result maps out of
// the pinned block): a single core moves them at ~25 GB/s, i.e. 0.27 + 0.2 ms per 640 x 480 x 7 call on the critical path of TANDEM's
// one-window-in-flight loop.  run() hands it a job, wait() returns when the job is done; the caller does its own half in between.
class HostCopier {
 public:
  HostCopier() : th_(&HostCopier::loop, this) {}
  ~HostCopier() {
    { std::lock_guard<std::mutex> lk(mu_); quit_ = true; }
    cv_.notify_all();
    th_.join();
  }
  void run(std::function<void()> job) {
    { std::lock_guard<std::mutex> lk(mu_); job_ = std::move(job); busy_ = true; }
    cv_.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return !busy_; });
    if (!error_.empty()) { std::string e = error_; error_.clear(); fail(DR_ERR_DEVICE, "%s", e.c_str()); }
  }
  void wait_quiet() {
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return !busy_; });
    error_.clear();
  }

 private:
  void loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [&] { return busy_ || quit_; });
      if (quit_) return;
      std::function<void()> job = std::move(job_);
      lk.unlock();
      std::string err;
      try { job(); } catch (const std::exception &e) { err = e.what(); }
      lk.lock();
      error_ = err;
      busy_ = false;
      done_.notify_all();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_, done_;
  std::function<void()> job_;
  std::string error_;
  bool busy_ = false, quit_ = false;
  std::thread th_;
};

// ------------------------------------------------------------------ switches
// Every DR_* switch of the engine, read ONCE when the engine is created (nothing on the launch path calls getenv).  The product library reads
// six of them (profiling, printing, tuning knobs: listed in INTEGRATION.md); every switch that selects a superseded kernel generation, the losing side of a
// settled A/B or a forced fallback is read through hook_env(), i.e. only in the parity build (-DDR_PARITY_HOOKS, libdr_mi355x_hooks.so: what the tests
// that compare generations load) -- in the product hook_env() returns null, so those members keep their defaults whatever the environment says.
struct MvsSwitches {
  static int num(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
  static bool on(const char *name) { return getenv(name) != nullptr; }
  static int hnum(const char *name, int dflt) { const char *e = hook_env(name); return e ? atoi(e) : dflt; }  // parity build only (dr_host.h): the product returns dflt
  static bool hon(const char *name) { return hook_env(name) != nullptr; }
  // ---- read by the product library ("Environment switches"): profiling, printing, tuning knobs
  bool side_stream = !on("DR_MVS_NO_SIDE_STREAM");       // FeatureNet's stage-2/3 heads on a second stream (off: strictly sequential kernels, for profiles)
  int conv_print = num("DR_CONV_PRINT", 0);              // autotune / debug printing
  std::string autotune_only = getenv("DR_AUTOTUNE_ONLY") ? getenv("DR_AUTOTUNE_ONLY") : "";  // tuning: restrict autotune to layers whose name contains this
  int cv_dchunk[3] = {num("DR_CV_DCHUNK1", 0), num("DR_CV_DCHUNK2", 0), num("DR_CV_DCHUNK3", 0)};  // tuning: depth planes per cost-volume workgroup (0: default)
  int prob_zchunk = num("DR_PROB_ZCHUNK", 0);            // tuning: z-march chunk of k_prob2 (0: default)
  int hist_blocks = std::max(1, num("DR_HIST_BLOCKS", 128));  // tuning: workgroups of a histogram level (each flushes its bins with atomics on a few hot addresses)
  // ---- parity build only: the other side of every settled A/B, superseded generations, forced fallbacks (constants in the product)
  int prob_rows = hnum("DR_PROB_ROWS", 0);               // logits per lane of k_prob2 (2 or 4: measured slower; default 1)
  bool costvol_v2 = hon("DR_COSTVOL_V2");                // k_costvol2 (the product's fallback for depth chunks that are not multiples of 4) everywhere
  bool regress_generic = hon("DR_REGRESS_GENERIC");      // k_regress (the product's fallback for other plane counts) everywhere
  bool shard_allreduce = hon("DR_SHARD_ALLREDUCE");      // view shard: round 2's all-reduce form instead of reduce + broadcast
  // CostRegNet's conv11 + prob as ONE launch (tail_kernels.h): both forms are correct (tests/test_tail_gpu.py) and the memory side of the fusion works
  // (the 78.6 MB tensor between the two layers is gone), but the transposed convolution x 1.8 (halo) and the prob stencil share the same issue slots -- fp32
  // MFMAs and vector work serialise on a SIMD -- and nothing overlaps the kernel's memory side: 0.128 / 0.113 ms (matrix pipe) and 0.118 / 0.109 (vector pipe)
  // at stages 2 / 3 against the two-kernel path's 0.100 / 0.096 (profiles/r05_tail.txt)
  int tail_fused = hnum("DR_TAIL_FUSED", 0);             // 0: the two-kernel path; 1: k_tail_m (transposed convolution on the matrix pipe); 2: k_tail (on the vector pipe)
  int tail_qy = hnum("DR_TAIL_QY", 0), tail_zchunk = hnum("DR_TAIL_ZCHUNK", 0);  // k_tail's tile (quad rows: 4, 8, 16, 32) and depth planes per workgroup (0: chosen by size)
  bool fn_front = hnum("DR_FN_FRONT", 1) != 0;           // 1: FeatureNet's first block (u8 -> float, conv0.0, conv0.1) in one launch (k_fn_front); 0: the three launches
  bool fn_head3 = hnum("DR_FN_HEAD3", 1) != 0;           // 1: the folded stage-3 head of FeatureNet (fn.out3a..d) in one launch (k_fn_head3); 0: the four launches
  bool filter_fused = hnum("DR_FILTER_FUSED", 1) != 0;   // 1: the radix select's scans run as the prologue of the kernels that follow them (5 launches); 0: a k_scan launch per level (8)
  bool prob_regress = hnum("DR_PROB_REGRESS", 1) != 0;   // 1: where a stage's planes are one depth chunk of k_prob2 (D = 8), the regression runs in the same launch (k_prob2_regress)
  bool vol_split = !hon("DR_VOL_NO_SPLIT");              // stage 1's 32-channel cost volume as two 16-channel halves (DevTensor::split); off: one (D,h,w,32) tensor
  bool costvol_v1 = hon("DR_COSTVOL_V1");                // round 2's k_costvol on unpadded feature maps
  bool costvol_v3 = hon("DR_COSTVOL_V3");                // k_costvol3 everywhere: also where the product runs k_costvol5 and where DR_CV4_STAGES selects the LDS-staged k_costvol4
  int costvol_cpl = hnum("DR_COSTVOL_CPL", 4) == 8 ? 8 : 4;
  bool prob_v1 = hon("DR_PROB_V1");                      // round 2's k_prob (L1 gathers)
  int prob_block = std::max(64, std::min(256, hnum("DR_PROB_BLOCK", 256) / 64 * 64)), prob_xo = hnum("DR_PROB_XO", 1);
  bool prob_launch_order = hon("DR_PROB_LAUNCH_ORDER"), prob_on_conv = hon("DR_PROB_ON_CONV");
  bool skip_on_conv = hon("DR_SKIP_ON_CONV"), no_skip_fusion = hon("DR_NO_SKIP_FUSION");
  bool out3_folded = hnum("DR_OUT3_FOLDED", 1) != 0;     // 0: FeatureNet's stage-3 head in its literal order (fused-skip kernel)
  // k_costvol5's two choices (round 6, profiles/r06_costvol_ab.txt): a sample whose footprint is the previous plane's issues no gathers (0.109 / 0.172 / 0.120 ->
  // 0.084 / 0.150 / 0.117 ms at depth chunks of 4 / 8 / 8 planes; 0.078 / 0.126 / 0.099 in the single-set form); the workgroup tile is four rows of a quarter segment
  // (0.108 -> 0.099 ms at stage 3, 0.126 -> 0.122 at stage 2, nothing at stage 1)
  int cv5_rows = hnum("DR_CV5_ROWS", 0);                 // 0: the product's rule (4 rows); 1 / 4: that tile at every stage
  bool cv5_reuse = hnum("DR_CV5_REUSE", 1) != 0;         // 0: every sample gathers its four taps
  int cv5_abl = hnum("DR_CV5_ABL", 0);                   // measuring hook: k_costvol5 without its gathers (1), stores (2), tap arithmetic (4)
  // k_costvol4 (round 4: source taps staged through LDS -- north_star's "LDS staging of per-pixel feature slices"): bit-identical to
  // k_costvol3 and measured 8-15 % SLOWER (0.121 / 0.163 / 0.105 against 0.106 / 0.150 / 0.099 ms per stage), so it is not in the product
  int cv4_stages = hnum("DR_CV4_STAGES", 0);             // bit s-1 set = stage s builds its cost volume with k_costvol4 where it applies
  int cv4_sp8 = hnum("DR_CV4_SP8", 0);                   // bit s-1 set = 8 planes per k_costvol4 step at stage s (else 4)
};

// ------------------------------------------------------------------ kernel choice
// One pure function per kernel family: a stage's shape (plain fields of the launch arguments), the switches and the stage number in; the kernel
// family and its template arguments out.  The launcher (mvs_launch.h) dispatches on the answer and drm_profile prints it: no rule is written twice.
struct CostVolShape { int V, h, w, D, dchunk, fpad, view_aggregation; };
// depth planes per cost-volume workgroup
inline int costvol_dchunk(int stage, int D, int view_aggregation, int fpad, const MvsSwitches &sw) {
  int dchunk = stage == 1 ? 4 : (D >= 16 ? 8 : D);  // enough workgroups to fill 256 CUs at every stage
  // k_costvol5 holds a chunk's planes in registers: 4 planes leave room for six waves per SIMD (0.150 -> 0.131 ms at stage 2, 0.117 -> 0.106 at stage 3)
  if (view_aggregation && fpad && D % 4 == 0 && !sw.costvol_v2 && !sw.costvol_v3 && !sw.cv4_stages) dchunk = 4;
  if (sw.cv_dchunk[stage - 1] > 0) dchunk = std::min(D, sw.cv_dchunk[stage - 1]);  // tuning hook
  return dchunk;
}
struct CostVolChoice {
  enum Family { V1, V2, V3, V4, V5 } family;
  int C;        // channels of the stage
  int a, b, c;  // k_costvol<C, a = CPL>, k_costvol4<C, a = DCH, b = SP>, k_costvol5<C, a = DCH, b = REUSE, c = ROWS>
  void name(char *kn, size_t n) const {  // rocprofv3's spelling of the instance, as far as drm_profile has always spelled it
    if (family == V4 || family == V5) snprintf(kn, n, family == V4 ? "k_costvol4<%d,%d>" : "k_costvol5<%d,%d>", C, a);
    else snprintf(kn, n, family == V1 ? "k_costvol<%d>" : (family == V2 ? "k_costvol2<%d>" : "k_costvol3<%d>"), C);
  }
};
inline CostVolChoice choose_costvol(const CostVolShape &a, const MvsSwitches &sw, int stage) {
  const int C = 32 >> (stage - 1);
  // DR_COSTVOL_V1: round 2's kernel on unpadded feature maps; channels per lane 4 (fewest L1 line accesses per byte) or 8
  if (!a.fpad) return {CostVolChoice::V1, C, C >= 16 ? sw.costvol_cpl : 4, 0, 0};
  const bool newer = !sw.costvol_v1 && !sw.costvol_v2 && !sw.costvol_v3 && a.view_aggregation && a.V > 1;
  // k_costvol4 (taps staged through LDS): view-aggregation models, bordered feature maps, whole pixel tiles, depth chunks of 8 (4 when D = 4)
  const int tw = C == 8 ? 16 : 8, th = (1024 / C) / tw, dch = a.D >= 8 ? 8 : 4;
  if (newer && ((sw.cv4_stages >> (stage - 1)) & 1) && a.w % tw == 0 && a.h % th == 0 && a.D % dch == 0) {
    // planes per step: 8 where neighbouring planes move a sample by a fraction of a pixel (the box hardly grows), else 4
    const bool sp8 = dch == 8 && C != 32 && ((sw.cv4_sp8 >> (stage - 1)) & 1);
    return {CostVolChoice::V4, C, dch, sp8 ? 8 : 4, 0};
  }
  // k_costvol5 (view-outer / plane-inner sweep): view-aggregation models, bordered feature maps, depth chunks of exactly 4 or 8 planes
  if (newer && (a.dchunk == 4 || a.dchunk == 8) && a.D % a.dchunk == 0) {
    const bool rows4 = sw.cv5_rows ? sw.cv5_rows == 4 : true;  // (four-row tiles at every stage since the single-set form: 0.126 -> 0.122 ms at stage 2, stage 1 unchanged)
    if (!sw.cv5_reuse) return {CostVolChoice::V5, C, a.dchunk, 0, 1};
    return {CostVolChoice::V5, C, a.dchunk, 1, rows4 ? 4 : 1};
  }
  // k_costvol3 (the lanes of a pixel share the per-sample set-up) needs whole batches of 4 iterations per depth chunk
  const bool v3 = !sw.costvol_v2 && a.dchunk % 4 == 0 && a.D % 4 == 0;
  return {v3 ? CostVolChoice::V3 : CostVolChoice::V2, C, 0, 0, 0};
}

struct ProbShape { int D, h, w; };
constexpr int kProbTY = 4, kProbTX = 64;  // k_prob2's tile: 4 NR rows x 64 columns
struct ProbChoice {
  enum Family { GATHER, STAGED, STAGED_REGRESS } family;  // k_prob<XO>, k_prob2<NR>, k_prob2_regress<8> (which also runs the stage's regression)
  int n;       // XO or NR (8 = the planes of k_prob2_regress)
  int zchunk;  // z-march chunk
  bool regresses() const { return family == STAGED_REGRESS; }
  void name(char *kn, size_t sz) const {
    if (family == GATHER) snprintf(kn, sz, "k_prob");
    else if (family == STAGED_REGRESS) snprintf(kn, sz, "k_prob2_regress<8>");
    else snprintf(kn, sz, "k_prob2<%d>", n);
  }
};
inline ProbChoice choose_prob(const ProbShape &o, const MvsSwitches &sw, int stage) {
  // z-march chunk: long chunks amortise the 2 halo planes, but the launch needs ~1000 waves to fill the chip
  // (round-2 sweep: 48x120x160 -> 4, 32x240x320 -> 8, 8x480x640 -> 8)
  if (sw.prob_v1) {  // round 2's L1-gather kernel: one output column per lane (r2 sweep: 4x the waves beats the 4-column variant)
    int zchunk = std::min(o.D, 8);
    while (zchunk > 2 && cdiv(o.h * (o.w / 4), 64) * cdiv(o.D, zchunk) < 800) zchunk /= 2;
    if (sw.prob_zchunk > 0) zchunk = std::min(o.D, sw.prob_zchunk);
    return {ProbChoice::GATHER, sw.prob_xo == 2 ? 2 : (sw.prob_xo == 4 ? 4 : 1), zchunk};
  }
  // LDS-staged plane tiles (k_prob2<NR>: NR rows per lane, tile 4 NR x 64)
  const int NR = sw.prob_rows == 2 || sw.prob_rows == 4 ? sw.prob_rows : 1;  // (measured: 0.028 / 0.044 / 0.084 ms at stage 2 for 1 / 2 / 4 rows per lane -- fewer, fatter workgroups lose more than the shared reads win)
  const int tyr = kProbTY * NR;
  int zc = std::min(o.D, 8);
  while (zc > 2 && cdiv(o.h, tyr) * cdiv(o.w, kProbTX) * cdiv(o.D, zc) < (NR == 1 ? 1024 : 512)) zc /= 2;  // enough workgroups for every CU's LDS
  if (sw.prob_zchunk > 0) zc = std::min(o.D, sw.prob_zchunk);
  // all planes are one depth chunk: the regression follows in the lane that produced the logits (k_prob2_regress); the REGRESS op of this stage then has nothing to launch
  if (NR == 1 && sw.prob_regress && cdiv(o.D, zc) == 1 && o.D == 8 && stage >= 1 && stage <= 3 && !sw.regress_generic) return {ProbChoice::STAGED_REGRESS, 8, zc};
  return {ProbChoice::STAGED, NR, zc};
}

// k_regress_r<D> for the plane counts of the shipped models, the three-pass k_regress for every other (0); DR_REGRESS_GENERIC=1: k_regress everywhere (A/B and parity hook)
inline int choose_regress(int D, const MvsSwitches &sw) {
  return !sw.regress_generic && (D == 48 || D == 32 || D == 8 || D == 4) ? D : 0;
}

}  // namespace dr
