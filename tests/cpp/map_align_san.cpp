// Stand-alone run of the registration half of tandem_amd/csrc/fusion_host.h for a sanitizer build (tests/test_map_align.py builds
// it with g++ -fsanitize=address,undefined and runs it), through the entry points of map_align_check.cpp: a small map of the
// corner of three planes registered to itself moved by a small motion (align_maps_host: converges, the cost falls, the
// counts add up, every evaluation's sums are symmetric-positive where they must be); seeded noise maps near the origin and at
// the edge of the key range; the empty maps; the options and the motions the calls refuse.
//   map_align_san      exits 0 when every check holds
#include <cstdio>
#include <random>
#include <set>

#include "map_align_check.cpp"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad < 20) fprintf(stderr, "map_align_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

struct Map {
  std::vector<unsigned long long> keys;
  std::vector<unsigned char> vox;
};

// blocks [lo, hi]^3 (+ shift along x) holding field(p) at every lattice point, p in metres, weight 7
template <class Field>
static Map field_map(int lo, int hi, long shift, float vs, Field field) {
  Map m;
  for (long x = lo; x <= hi; ++x)
    for (long y = lo; y <= hi; ++y)
      for (long z = lo; z <= hi; ++z) m.keys.push_back(dr::pack_biased(x + shift, y, z));
  std::sort(m.keys.begin(), m.keys.end());
  m.vox.resize(m.keys.size() * 4096);
  for (size_t i = 0; i < m.keys.size(); ++i) {
    int b[3]; dr::unpack_key_host(m.keys[i], b);
    for (int v = 0; v < 512; ++v) {
      const double p[3] = {(b[0] * 8 + (v >> 6)) * (double)vs, (b[1] * 8 + ((v >> 3) & 7)) * (double)vs, (b[2] * 8 + (v & 7)) * (double)vs};
      const float s = (float)field(p);
      unsigned char *o = &m.vox[i * 4096 + 8 * (size_t)v];
      memcpy(o, &s, 4);
      o[4] = 10; o[5] = 20; o[6] = 30; o[7] = 7;
    }
  }
  return m;
}

static Map noise_map(unsigned seed, long far, float vs) {
  std::mt19937 rng(seed);
  std::set<unsigned long long> s;
  for (long x = -1; x <= 0; ++x)
    for (long y = -1; y <= 0; ++y)
      for (long z = -1; z <= 0; ++z) s.insert(dr::pack_biased(x, y, z));
  s.insert(dr::pack_biased(far, 1, -far));
  s.insert(dr::pack_biased((1 << 20) - 1, 0, 0));
  s.insert(dr::pack_biased(-(1 << 20), -(1 << 20), -(1 << 20)));
  Map m;
  m.keys.assign(s.begin(), s.end());
  m.vox.resize(m.keys.size() * 4096);
  for (size_t v = 0; v < m.keys.size() * 512; ++v) {
    const float sdf = ((int)(rng() % 2001) - 1000) * 6e-5f;
    memcpy(&m.vox[8 * v], &sdf, 4);
    for (int k = 4; k < 7; ++k) m.vox[8 * v + k] = (unsigned char)rng();
    const unsigned pick = rng() % 10;
    m.vox[8 * v + 7] = pick < 2 ? 0 : pick == 2 ? 1 : pick == 3 ? 255 : (unsigned char)(1 + rng() % 255);
  }
  return m;
}

static void small_rotation(double ax, double ay, double az, double angle, float T[16]) {
  const double len = std::sqrt(ax * ax + ay * ay + az * az), x = ax / len, y = ay / len, z = az / len, c = std::cos(angle), s = std::sin(angle), t = 1 - c;
  const double R[9] = {t * x * x + c, t * x * y - s * z, t * x * z + s * y, t * x * y + s * z, t * y * y + c, t * y * z - s * x, t * x * z - s * y, t * y * z + s * x, t * z * z + c};
  for (int i = 0; i < 16; ++i) T[i] = 0.0f;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R[3 * i + j];
  T[15] = 1.0f;
}

int main() {
  const float vs = 0.02f;
  // a surface that fixes all six degrees of freedom: the corner of three planes through (0.013, -0.021, 0.008), untruncated
  auto corner = [](const double p[3]) {
    const double d[3] = {p[0] - 0.013, p[1] + 0.021, p[2] - 0.008};
    const double a = d[0], b = 0.6 * d[0] + 0.8 * d[1], c = 0.36 * d[0] - 0.48 * d[1] + 0.8 * d[2];
    return std::max(a, std::max(b, c));
  };
  const Map ref = field_map(-3, 2, 0, vs, corner), src = field_map(-2, 1, 0, vs, corner);
  float T[16];
  small_rotation(1, -2, 0.5, 0.01, T);
  T[3] = 0.006f; T[7] = -0.004f; T[11] = 0.008f;
  CHECK(dr::transform_pose_fault(T) == nullptr);
  {
    drf_align_result_t r;
    std::vector<double> trace(30 * 28);
    CHECK(ma_align(src.keys.data(), src.vox.data(), src.keys.size(), ref.keys.data(), ref.vox.data(), ref.keys.size(), T, vs, nullptr, &r, trace.data(), 30) == 0);
    CHECK(r.status == DRF_ALIGN_CONVERGED);
    CHECK(r.iterations >= 2 && r.iterations < 30);
    CHECK(r.samples > 1000 && r.valid0 > r.samples / 2 && r.valid > r.samples / 2);
    CHECK(r.cost < 0.05 * r.cost0);
    // the same surface in both maps: the registration undoes the start, up to what the trilinear field resolves
    double off = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) off = std::max(off, std::fabs(r.T[4 * i + j] - (i == j ? 1.0 : 0.0)));
    CHECK(off < 2e-3);
    CHECK(r.T[12] == 0.0 && r.T[13] == 0.0 && r.T[14] == 0.0 && r.T[15] == 1.0);
    float T32[16];
    for (int i = 0; i < 16; ++i) T32[i] = (float)r.T[i];
    CHECK(dr::transform_pose_fault(T32) == nullptr);
    double sums[28];
    unsigned long long counts[3];
    CHECK(ma_system(src.keys.data(), src.vox.data(), src.keys.size(), ref.keys.data(), ref.vox.data(), ref.keys.size(), T, vs, nullptr, sums, counts) == 0);
    CHECK(memcmp(sums, trace.data(), 224) == 0);
    CHECK(counts[0] == r.samples && counts[1] == r.valid0 && counts[1] + counts[2] == counts[0]);
    const int diag[6] = {0, 6, 11, 15, 18, 20};
    for (int i = 0; i < 6; ++i) CHECK(sums[diag[i]] > 0.0);
    CHECK(sums[27] > 0.0);
    // one evaluation only: the pose moves, the status says so
    drf_align_options_t one = {1, 0, 0.0f, 0.0f, 0.0, 0.0, 0.0};
    CHECK(ma_align(src.keys.data(), src.vox.data(), src.keys.size(), ref.keys.data(), ref.vox.data(), ref.keys.size(), T, vs, &one, &r, trace.data(), 30) == 0);
    CHECK(r.status == DRF_ALIGN_MAX_ITERS && r.iterations == 1 && r.T[3] != (double)T[3]);
    // a reference 12 blocks away: lost at the first evaluation, the pose stays
    const Map away = field_map(-3, 2, 12, vs, corner);
    CHECK(ma_align(src.keys.data(), src.vox.data(), src.keys.size(), away.keys.data(), away.vox.data(), away.keys.size(), T, vs, nullptr, &r, trace.data(), 30) == 0);
    CHECK(r.status == DRF_ALIGN_LOST && r.iterations == 1 && r.valid == 0 && r.T[0] == (double)T[0] && r.T[3] == (double)T[3] / (double)vs * (double)vs);
    // one plane: degenerate
    auto plane = [](const double p[3]) { return 0.36 * p[0] - 0.48 * p[1] + 0.8 * p[2] - 0.01; };
    const Map pr = field_map(-2, 1, 0, vs, plane), ps = field_map(-1, 0, 0, vs, plane);
    CHECK(ma_align(ps.keys.data(), ps.vox.data(), ps.keys.size(), pr.keys.data(), pr.vox.data(), pr.keys.size(), T, vs, nullptr, &r, trace.data(), 30) == 0);
    CHECK(r.status == DRF_ALIGN_DEGENERATE && r.valid > 100);
  }
  {  // noise, blocks at the edge of the key range and 700 000 blocks out, both weights of min_weight: counts add up, nothing is read out of bounds
    std::mt19937 rng(9);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    for (int i = 0; i < 8; ++i) {
      const Map a = noise_map(1 + i, 40, vs), b = noise_map(20 + i, i % 2 ? 40 : 700000, vs);
      float M[16];
      small_rotation(U(rng), U(rng), U(rng) + 1e-3, i < 4 ? 0.02 * U(rng) : 3.0 * U(rng), M);
      for (int k = 0; k < 3; ++k) M[4 * k + 3] = (float)(U(rng) * (i < 4 ? 0.03 : 2.0));
      drf_align_options_t o = {5, i % 2 ? 3 : 0, 0.0f, i % 3 ? 0.0f : 0.5f, 0.0, 0.0, 0.0};
      double sums[28];
      unsigned long long counts[3];
      CHECK(ma_system(a.keys.data(), a.vox.data(), a.keys.size(), b.keys.data(), b.vox.data(), b.keys.size(), M, vs, &o, sums, counts) == 0);
      CHECK(counts[0] > 0 && counts[1] + counts[2] == counts[0]);
      drf_align_result_t r;
      double trace[5 * 28];
      CHECK(ma_align(a.keys.data(), a.vox.data(), a.keys.size(), b.keys.data(), b.vox.data(), b.keys.size(), M, vs, &o, &r, trace, 5) == 0);
      CHECK(r.iterations >= 1 && r.iterations <= 5 && r.status >= 0 && r.status <= 3);
      CHECK(memcmp(trace, sums, 224) == 0);
    }
  }
  {  // the empty maps, the options and the motions the calls refuse
    drf_align_result_t r;
    double sums[28], trace[28];
    unsigned long long counts[3];
    CHECK(ma_system(nullptr, nullptr, 0, ref.keys.data(), ref.vox.data(), ref.keys.size(), T, vs, nullptr, sums, counts) == 0);
    for (int i = 0; i < 28; ++i) CHECK(sums[i] == 0.0);
    CHECK(counts[0] == 0 && counts[1] == 0 && counts[2] == 0);
    CHECK(ma_system(src.keys.data(), src.vox.data(), src.keys.size(), nullptr, nullptr, 0, T, vs, nullptr, sums, counts) == 0);
    CHECK(counts[0] > 0 && counts[1] == 0 && counts[2] == counts[0] && sums[27] == 0.0);
    CHECK(ma_align(nullptr, nullptr, 0, nullptr, nullptr, 0, T, vs, nullptr, &r, trace, 1) == 0);
    CHECK(r.status == DRF_ALIGN_LOST && r.iterations == 1 && r.samples == 0);
    drf_align_options_t bad = {0, 0, -1.0f, 0.0f, 0.0, 0.0, 0.0};
    CHECK(ma_system(src.keys.data(), src.vox.data(), src.keys.size(), ref.keys.data(), ref.vox.data(), ref.keys.size(), T, vs, &bad, sums, counts) == 1);
    bad.band = 0.0f; bad.eps_rot = NAN;
    double out7[7];
    CHECK(ma_options(&bad, vs, out7) == 1);
    CHECK(ma_options(nullptr, vs, out7) == 0 && out7[0] == 30 && out7[1] == 1 && out7[2] == (double)(2.0f * vs));
    float S[16], N[16], L[16], M[16];
    memcpy(S, T, 64); memcpy(N, T, 64); memcpy(L, T, 64); memcpy(M, T, 64);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) S[4 * i + j] *= 1.01f;
    N[7] = NAN; L[12] = 1e-30f;
    for (int i = 0; i < 3; ++i) M[4 * i] = -M[4 * i];
    CHECK(dr::transform_pose_fault(S) && dr::transform_pose_fault(N) && dr::transform_pose_fault(L) && dr::transform_pose_fault(M));
  }
  if (g_bad) { fprintf(stderr, "map_align_san: %d checks failed\n", g_bad); return 1; }
  printf("map_align_san ok\n");
  return 0;
}
