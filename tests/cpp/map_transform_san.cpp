// Stand-alone run of the rigid-resample half of tandem_amd/csrc/fusion_host.h for a sanitizer build (tests/test_map_transform.py
// builds it with g++ -fsanitize=address,undefined and runs it): seeded maps around the origin
// (and 700 000 blocks out) under seeded motions through the entry points of map_transform_check.cpp -- keys ascending, counts that match the blocks
// written, every kept block among the candidates; the identity and a lattice motion moving every weighted voxel byte for byte;
// the motions drf_transform_map refuses.
//   map_transform_san      exits 0 when every check holds
#include <cstdio>
#include <map>
#include <random>
#include <set>

#include "map_transform_check.cpp"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad < 20) fprintf(stderr, "map_transform_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

struct Map {
  std::vector<unsigned long long> keys;
  std::vector<unsigned char> vox;
};

static Map make_map(unsigned seed, long far) {
  std::mt19937 rng(seed);
  std::set<unsigned long long> s;
  for (long x = -1; x <= 0; ++x)
    for (long y = -1; y <= 0; ++y)
      for (long z = -1; z <= 0; ++z) s.insert(dr::pack_biased(x, y, z));
  s.insert(dr::pack_biased(5, -3, 2));
  s.insert(dr::pack_biased(far, 1, -far));
  Map m;
  m.keys.assign(s.begin(), s.end());
  m.vox.resize(m.keys.size() * 4096);
  for (size_t v = 0; v < m.keys.size() * 512; ++v) {
    const float sdf = ((int)(rng() % 2001) - 1000) * 1e-4f;
    memcpy(&m.vox[8 * v], &sdf, 4);
    for (int k = 4; k < 7; ++k) m.vox[8 * v + k] = (unsigned char)rng();
    const unsigned pick = rng() % 10;
    m.vox[8 * v + 7] = pick < 2 ? 0 : pick == 2 ? 1 : pick == 3 ? 255 : (unsigned char)(1 + rng() % 255);
  }
  return m;
}

static void rotation(double ax, double ay, double az, double angle, float T[16]) {
  const double len = std::sqrt(ax * ax + ay * ay + az * az), x = ax / len, y = ay / len, z = az / len, c = std::cos(angle), s = std::sin(angle), t = 1 - c;
  const double R[9] = {t * x * x + c, t * x * y - s * z, t * x * z + s * y, t * x * y + s * z, t * y * y + c, t * y * z - s * x, t * x * z - s * y, t * y * z + s * x, t * z * z + c};
  for (int i = 0; i < 16; ++i) T[i] = 0.0f;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R[3 * i + j];
  T[15] = 1.0f;
}

struct Result {
  std::vector<unsigned long long> keys, plan;
  std::vector<unsigned char> vox;
  unsigned long long counts[3];
};
static Result run(const Map &m, const float T[16], float vs) {
  Result r;
  int in_range = 0;
  const size_t np = mt_plan(m.keys.data(), m.keys.size(), T, vs, nullptr, 0, &in_range);
  CHECK(in_range == 1);
  r.plan.resize(np);
  CHECK(mt_plan(m.keys.data(), m.keys.size(), T, vs, r.plan.data(), np, &in_range) == np);
  const size_t n = mt_transform_blocks(m.keys.data(), m.vox.data(), m.keys.size(), T, vs, nullptr, nullptr, 0, r.counts);
  r.keys.resize(n); r.vox.resize(n * 4096);
  CHECK(mt_transform_blocks(m.keys.data(), m.vox.data(), m.keys.size(), T, vs, r.keys.data(), r.vox.data(), n, r.counts) == n);
  CHECK(r.counts[0] == np);
  unsigned long long weighted = 0;
  for (size_t i = 0; i < n; ++i) {
    CHECK(i == 0 || r.keys[i] > r.keys[i - 1]);
    CHECK(std::binary_search(r.plan.begin(), r.plan.end(), r.keys[i]));
    unsigned long long in_block = 0;
    for (int v = 0; v < 512; ++v) {
      const unsigned char *o = &r.vox[i * 4096 + 8 * (size_t)v];
      if (o[7]) ++in_block;
      else { static const unsigned char zero[8] = {0}; CHECK(memcmp(o, zero, 8) == 0); }
    }
    CHECK(in_block > 0);
    weighted += in_block;
  }
  for (size_t i = 1; i < np; ++i) CHECK(r.plan[i] > r.plan[i - 1]);
  CHECK(weighted == r.counts[1]);
  return r;
}

// voxel (8 bytes) by lattice point
typedef std::map<std::array<long, 3>, std::array<unsigned char, 8>> Cloud;
static Cloud cloud(const std::vector<unsigned long long> &keys, const std::vector<unsigned char> &vox, const long P[9], const long shift[3]) {
  Cloud c;
  for (size_t i = 0; i < keys.size(); ++i) {
    int b[3]; dr::unpack_key_host(keys[i], b);
    for (int v = 0; v < 512; ++v) {
      const unsigned char *o = &vox[i * 4096 + 8 * (size_t)v];
      if (!o[7]) continue;
      const long g[3] = {b[0] * 8L + (v >> 6), b[1] * 8L + ((v >> 3) & 7), b[2] * 8L + (v & 7)};
      std::array<long, 3> q;
      for (int a = 0; a < 3; ++a) q[a] = P[3 * a] * g[0] + P[3 * a + 1] * g[1] + P[3 * a + 2] * g[2] + shift[a];
      std::array<unsigned char, 8> bytes;
      memcpy(bytes.data(), o, 8);
      c[q] = bytes;
    }
  }
  return c;
}

static void lattice(const Map &m, const long P[9], const long shift[3]) {
  const float vs = 0.015625f;
  float T[16] = {0};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)P[3 * i + j];
    T[4 * i + 3] = (float)shift[i] * vs;
  }
  T[15] = 1.0f;
  CHECK(mt_pose_fault(T) == 0);
  const Result r = run(m, T, vs);
  const long I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0};
  CHECK(cloud(r.keys, r.vox, I, zero) == cloud(m.keys, m.vox, P, shift));
  CHECK(r.counts[2] == 0);
}

int main() {
  const long I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Rz[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, cyc[9] = {0, 0, 1, 1, 0, 0, 0, 1, 0};
  const long zero[3] = {0, 0, 0}, move[3] = {25, -5, 2};
  const Map near = make_map(1, 40), far = make_map(2, 700000);  // (|(far, 1, -far)| stays below 2^20 under every rotation)
  lattice(near, I, zero); lattice(near, Rz, move); lattice(near, cyc, zero);
  lattice(far, I, zero); lattice(far, Rz, move);
  std::mt19937 rng(9);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  for (int i = 0; i < 12; ++i) {
    float T[16];
    rotation(U(rng), U(rng), U(rng) + 1e-3, 3.2 * U(rng), T);
    for (int a = 0; a < 3; ++a) T[4 * a + 3] = (float)(U(rng) * 3.0);
    CHECK(mt_pose_fault(T) == 0);
    const Result r = run(i % 3 == 2 ? far : near, T, i % 2 ? 0.02f : 0.05f);
    CHECK(!r.keys.empty() && r.counts[2] > 0);
  }
  {  // an empty source, and what is no motion
    float T[16];
    rotation(1, 2, 3, 0.6, T);
    unsigned long long counts[3];
    CHECK(mt_transform_blocks(nullptr, nullptr, 0, T, 0.02f, nullptr, nullptr, 0, counts) == 0 && counts[0] == 0);
    float S[16], N[16], L[16], M[16];
    memcpy(S, T, 64); memcpy(N, T, 64); memcpy(L, T, 64); memcpy(M, T, 64);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) S[4 * i + j] *= 1.01f;
    N[7] = NAN; L[12] = 1e-30f;
    for (int i = 0; i < 3; ++i) M[4 * i] = -M[4 * i];
    CHECK(mt_pose_fault(S) == 1 && mt_pose_fault(N) == 1 && mt_pose_fault(L) == 1 && mt_pose_fault(M) == 1);
    int in_range = 1;
    const unsigned long long edge = dr::pack_biased((1 << 20) - 1, 0, 0);
    float E[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mt_plan(&edge, 1, E, 0.02f, nullptr, 0, &in_range);
    CHECK(in_range == 0);
    E[3] = 1e30f;
    mt_plan(&edge, 1, E, 0.02f, nullptr, 0, &in_range);
    CHECK(in_range == 0);
  }
  if (g_bad) { fprintf(stderr, "map_transform_san: %d checks failed\n", g_bad); return 1; }
  printf("map_transform_san ok\n");
  return 0;
}
