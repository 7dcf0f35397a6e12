// Stand-alone run of tandem_amd/csrc/mvs_host.h for a sanitizer build (tests/test_mvs_host.py builds it with
// g++ -fsanitize=address,undefined and runs it): the image key on the smallest image, the cache index through the window
// sequences of the CPU test, load_blob on a good and on every truncation of a small blob, the folds and the geometry.
//   mvs_host_san DIR      exits 0 when every check holds
#include <random>

#include "../../tandem_amd/csrc/mvs_host.h"

namespace dr { std::string &last_error_slot() { static std::string s; return s; } }
using namespace dr;

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "mvs_host_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

// ---- image key: 32 x 32 x 3 bytes in an exact-size heap block (a read past either end is the sanitizer's to find)
static void keys() {
  std::mt19937 rng(1);
  for (int hw : {32, 64}) {
    const size_t n = (size_t)hw * hw * 3;
    std::vector<uint8_t> img(n);
    for (auto &b : img) b = (uint8_t)rng();
    uint64_t k0[2], k1[2];
    image_key(img.data(), n, hw, hw, k0);
    img[n - 1] ^= 1;
    image_key(img.data(), n, hw, hw, k1);
    CHECK(k0[0] != k1[0] || k0[1] != k1[1]);
    img[n - 1] ^= 1; img[n / 2 + 13] ^= 1;  // 32 x 32: between the ends nothing is read; 64 x 64: byte 6157 lies between the samples at 6144 and 6168
    image_key(img.data(), n, hw, hw, k1);
    CHECK(k0[0] == k1[0] && k0[1] == k1[1]);
  }
}

// ---- cache index
static void window(FeatureIndex &x, const std::vector<uint64_t> &ids) {
  const int V = (int)ids.size();
  uint64_t keys[kMaxSrc + 1][2];
  for (int v = 0; v < V; ++v) { keys[v][0] = ids[v] * 0x9e3779b97f4a7c15ull + 1; keys[v][1] = ~ids[v]; }
  x.plan(V, keys);
  if (!x.fast && !x.fill) return;
  for (int v = 0; v < V; ++v) {
    CHECK(x.slot[v] >= 0 && x.slot[v] < (int)x.size());
    for (int u = 0; u < v; ++u) CHECK(x.slot[u] != x.slot[v]);
  }
  if (x.fast && x.miss >= 0) x.set_valid(x.slot[x.miss]);
  if (x.fill) for (int v = 0; v < V; ++v) x.set_valid(x.slot[v]);
}
static std::vector<uint64_t> span(uint64_t first, int V) {
  std::vector<uint64_t> w;
  for (int v = 0; v < V; ++v) w.push_back(first + v);
  return w;
}
static void cache_index() {
  for (int V : {2, 8}) {
    FeatureIndex x;
    x.resize(V + 1);
    for (int t = 0; t < 12; ++t) { window(x, span(t, V)); CHECK(t == 0 ? x.fill : x.fast); }  // sliding by one
    CHECK(x.hits == 11u * (V - 1) && x.misses == (uint64_t)V + 11 && x.batch_windows == 1);
    for (int t = 0; t < 6; ++t) { window(x, span(100 + 2 * t, V)); CHECK(x.fill); }  // by two: batch windows
    window(x, span(500, V)); CHECK(x.fill);  // a reset
    window(x, span(501, V)); CHECK(x.fast && x.miss == V - 1);
    std::vector<uint64_t> twice = span(501, V);
    twice[V - 1] = twice[0];  // two views, one image
    window(x, twice); CHECK(x.fast && x.miss == V - 1);
    ++x.collisions; x.invalidate_all();  // a key collision drops every entry
    window(x, twice); CHECK(x.fill);
    FeatureIndex small;
    small.resize(V);  // capacity V: never answers
    for (int t = 0; t < 4; ++t) { window(small, span(t, V)); CHECK(!small.fast && !small.fill && small.miss == -1); }
    CHECK(small.hits == 0 && small.misses == 0);
    std::mt19937 rng(V);
    FeatureIndex r;
    r.resize(V + 3);
    for (int t = 0; t < 200; ++t) {
      std::vector<uint64_t> w;
      for (int v = 0; v < V; ++v) w.push_back(rng() % (V + 6));
      window(r, w);
    }
  }
}

// ---- blob: a small TDMW file written here (tandem_amd/weights.py's layout), read back; every truncation refused
static void put(std::vector<unsigned char> &o, const void *p, size_t n) { o.insert(o.end(), (const unsigned char *)p, (const unsigned char *)p + n); }
static void put_tensor(std::vector<unsigned char> &o, const std::string &name, const std::vector<uint32_t> &dims, std::mt19937 &rng) {
  const uint32_t ln = (uint32_t)name.size(), nd = (uint32_t)dims.size();
  put(o, &ln, 4); put(o, name.data(), ln); put(o, &nd, 4);
  size_t cnt = 1;
  for (uint32_t d : dims) { put(o, &d, 4); cnt *= d; }
  for (size_t i = 0; i < cnt; ++i) { const float f = 0.5f + (float)(rng() % 1000) / 1000.f; put(o, &f, 4); }
}
static bool spit(const std::string &p, const std::vector<unsigned char> &v, size_t bytes) {
  FILE *f = fopen(p.c_str(), "wb");
  if (!f) return false;
  const bool ok = !bytes || fwrite(v.data(), 1, bytes, f) == bytes;
  fclose(f);
  return ok;
}
static int load_code(const std::string &p, Blob *out = nullptr) {
  return guarded([&] { Blob b = load_blob(p.c_str()); if (out) *out = std::move(b); });
}
static void blob(const std::string &dir) {
  std::mt19937 rng(7);
  std::vector<unsigned char> o;
  const int dn[3] = {48, 32, 8}, va = 1, base = 8;
  const float ratio[3] = {1.f, 0.5f, 0.25f};
  const uint32_t count = 14;
  put(o, "TDMW0001", 8); put(o, dn, 12); put(o, ratio, 12); put(o, &va, 4); put(o, &base, 4); put(o, &count, 4);
  for (const char *s : {"weight", "bias", "running_mean", "running_var"}) put_tensor(o, std::string("x.bn.") + s, {8}, rng);
  put_tensor(o, "volume_gates.stage3.0.weight", {1, 8, 1, 1, 1}, rng);
  put_tensor(o, "volume_gates.stage3.0.bias", {1}, rng);
  for (const char *s : {"weight", "bias", "running_mean", "running_var"}) put_tensor(o, std::string("volume_gates.stage3.1.") + s, {1}, rng);
  put_tensor(o, "volume_gates.stage3.3.weight", {1, 1, 1, 1, 1}, rng);
  put_tensor(o, "volume_gates.stage3.3.bias", {1}, rng);
  put_tensor(o, "out3", {8, 32, 3, 3}, rng);
  put_tensor(o, "scalar", {}, rng);
  const std::string good = dir + "/good.tdmw", bad = dir + "/bad.tdmw";
  CHECK(spit(good, o, o.size()));
  Blob b;
  CHECK(load_code(good, &b) == DR_OK);
  CHECK(b.t.size() == count && b.depth_num[1] == 32 && b.at("out3").data.size() == 8u * 32 * 9 && b.at("scalar").data.size() == 1);
  std::vector<float> sc, bi;
  fold_bn(b, "x.bn", 8, sc, bi);
  CHECK(sc.size() == 8 && bi.size() == 8);
  CHECK(guarded([&] { fold_gate(b, 3, 8); }) == DR_ERR_IO);  // stage 3's second BatchNorm (".4") is not in the file
  CHECK(guarded([&] { b.at("nothing"); }) == DR_ERR_IO);
  const Out3Fold f = compose_out3(b.at("out3").data, std::vector<float>(32 * 8, 0.25f), std::vector<float>(32, 1.f));
  CHECK(f.wa.size() == 576 && f.T.size() == 72 && f.bint.size() == 8);
  CHECK(prob_taps(std::vector<float>(216, 1.f)).size() == 216 && pad_cin(std::vector<float>(8 * 3 * 9, 1.f), 8, 3, 4, 9).size() == 8u * 4 * 9);
  for (size_t cut = 0; cut < o.size(); cut += (cut < 200 ? 1 : 97)) {  // every byte of the header and the first tensors, then strides
    CHECK(spit(bad, o, cut));
    CHECK(load_code(bad) == DR_ERR_IO);
  }
  std::vector<unsigned char> m = o;
  m[7] = '2';
  CHECK(spit(bad, m, m.size()) && load_code(bad) == DR_ERR_IO);
  m = o;
  m[36] = 16;
  CHECK(spit(bad, m, m.size()) && load_code(bad) == DR_ERR_UNSUPPORTED);
  CHECK(load_code(dir + "/missing.tdmw") == DR_ERR_IO);
}

// ---- geometry: eight views on a circle looking at the origin's side, every reference index
static void geometry() {
  BlobMeta meta{};
  const int dn[3] = {48, 32, 8};
  const float ratio[3] = {1.f, 0.5f, 0.25f};
  for (int i = 0; i < 3; ++i) { meta.depth_num[i] = dn[i]; meta.ratio[i] = ratio[i]; }
  meta.view_aggregation = 1; meta.base = 8;
  const float K9[9] = {80.f, 0.f, 48.f, 0.f, 80.f, 32.f, 0.f, 0.f, 1.f};
  float c2w[8][16];
  const float *ptr[8];
  for (int v = 0; v < 8; ++v) {
    const float a = 0.05f * (float)v, c = std::cos(a), s = std::sin(a);
    const float m[16] = {c, 0.f, s, 0.1f * (float)v, 0.f, 1.f, 0.f, 0.02f * (float)v, -s, 0.f, c, 0.01f * (float)v, 0.f, 0.f, 0.f, 1.f};
    memcpy(c2w[v], m, sizeof m);
    ptr[v] = c2w[v];
  }
  for (int V : {1, 2, 3, 8})
    for (int ref = 0; ref < V; ++ref)
      for (float disc : {2.5f, 0.f, 100.f, -7.f}) {
        const WindowGeometry g = plan_geometry(64, 96, V, ref, K9, ptr, 0.5f, 5.f, disc, meta, V == 1 ? 6 : 0);
        CHECK(g.order[0] == ref && g.filter_rank < 64u * 96u && g.stage[2].D == 8);
        for (int s = 0; s < 3; ++s)
          for (int v = 0; v < V - 1; ++v) for (int i = 0; i < 12; ++i) CHECK(std::isfinite(g.stage[s].M[v][i]));
      }
  meta.view_aggregation = 0;
  CHECK(guarded([&] { plan_geometry(64, 96, 2, 0, K9, ptr, 0.5f, 5.f, 2.5f, meta, 6); }) == DR_ERR_UNSUPPORTED);
}

static void choices() {
  MvsSwitches sw;
  for (int s = 1; s <= 3; ++s)
    for (int D : {4, 8, 16, 32, 48}) {
      char kn[64];
      const CostVolShape cs{3, 16 << (s - 1), 24 << (s - 1), D, costvol_dchunk(s, D, 1, 1, sw), 1, 1};
      choose_costvol(cs, sw, s).name(kn, sizeof kn);
      CHECK(!strncmp(kn, "k_costvol5<", 11));
      choose_prob(ProbShape{D, cs.h, cs.w}, sw, s).name(kn, sizeof kn);
      CHECK(!strncmp(kn, "k_prob2", 7));
    }
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: mvs_host_san DIR\n"); return 2; }
  keys();
  cache_index();
  blob(argv[1]);
  geometry();
  choices();
  {  // the helper thread: a job, a job that throws, destruction with nothing pending
    HostCopier c;
    int n = 0;
    c.run([&] { n = 7; });
    c.wait();
    CHECK(n == 7);
    c.run([] { fail(DR_ERR_IO, "thrown in the job"); });
    CHECK(guarded([&] { c.wait(); }) == DR_ERR_DEVICE);
  }
  if (g_bad) { fprintf(stderr, "mvs_host_san: %d checks failed\n", g_bad); return 1; }
  printf("mvs_host_san ok\n");
  return 0;
}
