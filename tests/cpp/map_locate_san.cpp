// Stand-alone run of the localisation half of tandem_amd/csrc/fusion_host.h for a sanitizer build (tests/test_map_locate.py builds
// it with g++ -fsanitize=address,undefined and runs it), through the entry points of map_locate_check.cpp.  It reads one case from
// a file -- u64 n, n keys, n x 4096 voxel bytes, a drf_options_t, a drf_locate_options_t, height x width depths, 16 pose floats --
// runs the system and the refinement on it and prints their sums as hexadecimal words, which the test compares with the
// restatement's; then, on its own, noise maps with depths that are no samples, strides, the edge of the key range, the empty map,
// and the options and poses the calls refuse.
//   map_locate_san CASE      exits 0 when every check holds
#include <cstdio>
#include <random>

#include "map_locate_check.cpp"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad < 20) fprintf(stderr, "map_locate_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

static void print_sums(const char *what, const double sums[28]) {
  printf("%s", what);
  for (int i = 0; i < 28; ++i) { unsigned long long w; memcpy(&w, &sums[i], 8); printf(" %llx", w); }
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: map_locate_san CASE\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  unsigned long long n = 0;
  drf_options_t cam;
  drf_locate_options_t opt;
  float pose[16];
  bool ok = fread(&n, 8, 1, f) == 1 && n < 100000;
  std::vector<unsigned long long> keys(ok ? n : 0);
  std::vector<unsigned char> vox(ok ? n * 4096 : 0);
  ok = ok && fread(keys.data(), 8, n, f) == n && fread(vox.data(), 4096, n, f) == n && fread(&cam, sizeof cam, 1, f) == 1 && fread(&opt, sizeof opt, 1, f) == 1;
  ok = ok && cam.width > 0 && cam.height > 0 && cam.width <= 4096 && cam.height <= 4096;
  std::vector<float> depth(ok ? (size_t)cam.width * cam.height : 0);
  ok = ok && fread(depth.data(), 4, depth.size(), f) == depth.size() && fread(pose, 4, 16, f) == 16;
  fclose(f);
  if (!ok) { fprintf(stderr, "map_locate_san: %s is not a case file\n", argv[1]); return 2; }
  {
    double sums[28];
    unsigned long long counts[4];
    CHECK(ml_system(keys.data(), vox.data(), n, &cam, depth.data(), pose, &opt, sums, counts) == 0);
    CHECK(counts[0] == counts[1] + counts[2] + counts[3]);
    print_sums("system", sums);
    printf(" %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3]);
    drf_align_result_t r;
    std::vector<double> trace(30 * 28);
    CHECK(ml_frame(keys.data(), vox.data(), n, &cam, depth.data(), pose, &opt, &r, trace.data(), 30) == 0);
    CHECK(memcmp(trace.data(), sums, 224) == 0);
    CHECK(r.samples == counts[0] && r.valid0 == counts[1]);
    CHECK(r.T[12] == 0.0 && r.T[13] == 0.0 && r.T[14] == 0.0 && r.T[15] == 1.0);
    print_sums("frame", r.sums);
    printf(" %d %d %llu %llu\n", r.status, r.iterations, (unsigned long long)r.samples, (unsigned long long)r.valid);
    // one evaluation only: the status says that the pose moved
    drf_locate_options_t one = opt;
    one.max_iters = 1;
    drf_align_result_t r1;
    CHECK(ml_frame(keys.data(), vox.data(), n, &cam, depth.data(), pose, &one, &r1, trace.data(), 30) == 0);
    CHECK(r1.iterations == 1 && (r1.status == DRF_ALIGN_MAX_ITERS || r1.status == r.status));
  }
  {  // noise around the origin, at the edge of the key range and 700 000 blocks out; depths that are no samples; strides up to the image
    std::mt19937 rng(9);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    std::vector<unsigned long long> k;
    for (long x = -1; x <= 0; ++x)
      for (long y = -1; y <= 0; ++y)
        for (long z = 2; z <= 5; ++z) k.push_back(dr::pack_biased(x, y, z));
    k.push_back(dr::pack_biased((1 << 20) - 1, 0, 0));
    k.push_back(dr::pack_biased(-(1 << 20), -(1 << 20), -(1 << 20)));
    k.push_back(dr::pack_biased(700000, 1, -700000));
    std::sort(k.begin(), k.end());
    std::vector<unsigned char> v(k.size() * 4096);
    for (size_t i = 0; i < k.size() * 512; ++i) {
      const float sdf = ((int)(rng() % 2001) - 1000) * 6e-5f;
      memcpy(&v[8 * i], &sdf, 4);
      v[8 * i + 7] = (unsigned char)(rng() % 5 == 0 ? 0 : 1 + rng() % 255);
    }
    drf_options_t c = cam;
    c.width = 37; c.height = 29; c.cx = 18.0f; c.cy = 14.0f; c.fx = c.fy = 40.0f;
    std::vector<float> d((size_t)c.width * c.height);
    const float special[6] = {0.0f, NAN, -1.0f, 0.01f, 1e9f, INFINITY};
    for (auto &x : d) x = rng() % 4 == 0 ? special[rng() % 6] : 0.3f + 0.6f * U(rng);
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float out[16] = {1, 0, 0, 167772.0f, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // 2^23 voxels along x: beyond the key range
    for (int step : {1, 2, 3, 7, 28, 29, 36, 37, 100}) {
      for (const float *T : {eye, out}) {
        drf_locate_options_t o = {3, step % 2 ? 0 : 3, step, step == 3 ? 0.02f : 0.0f, step == 2 ? 0.25f : 0.0f, step == 7 ? 0.6f : 0.0f, 0.0, 0.0, 0.01};
        double sums[28];
        unsigned long long counts[4];
        CHECK(ml_system(k.data(), v.data(), k.size(), &c, d.data(), T, &o, sums, counts) == 0);
        CHECK(counts[0] == counts[1] + counts[2] + counts[3]);
        if (T == out) CHECK(counts[1] == 0);
        if (T == eye && step <= 3) CHECK(counts[0] > 10 && counts[1] > 0);
        drf_align_result_t r;
        double trace[3 * 28];
        CHECK(ml_frame(k.data(), v.data(), k.size(), &c, d.data(), T, &o, &r, trace, 3) == 0);
        CHECK(r.iterations >= 1 && r.iterations <= 3 && r.status >= 0 && r.status <= 3);
        CHECK(memcmp(trace, sums, 224) == 0);
      }
    }
    // the empty map, an image without a sample
    double sums[28];
    unsigned long long counts[4];
    CHECK(ml_system(nullptr, nullptr, 0, &c, d.data(), eye, nullptr, sums, counts) == 0);
    CHECK(counts[0] > 0 && counts[1] == 0 && counts[2] == counts[0] && sums[27] == 0.0);
    std::vector<float> none(d.size(), 0.0f);
    CHECK(ml_system(k.data(), v.data(), k.size(), &c, none.data(), eye, nullptr, sums, counts) == 0);
    CHECK(counts[0] == 0 && counts[1] == 0 && counts[2] == 0 && counts[3] == 0);
    for (int i = 0; i < 28; ++i) CHECK(sums[i] == 0.0);
    drf_align_result_t r;
    double trace[28];
    CHECK(ml_frame(k.data(), v.data(), k.size(), &c, none.data(), eye, nullptr, &r, trace, 1) == 0);
    CHECK(r.status == DRF_ALIGN_LOST && r.iterations == 1 && r.samples == 0 && r.T[0] == 1.0 && r.T[3] == 0.0);
    // what the calls refuse
    drf_locate_options_t bad = {0, 0, -1, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.0};
    double out9[9];
    char name[32];
    CHECK(ml_options(&bad, 0.08f, out9, name) == 1 && strcmp(name, "step") == 0);
    bad.step = 0; bad.centre_depth = NAN;
    CHECK(ml_options(&bad, 0.08f, out9, name) == 1 && strcmp(name, "centre_depth") == 0);
    bad.centre_depth = 0.0f; bad.huber = -1.0f;
    CHECK(ml_system(k.data(), v.data(), k.size(), &c, d.data(), eye, &bad, sums, counts) == 1);
    CHECK(ml_options(nullptr, 0.08f, out9, name) == 0 && out9[0] == 30 && out9[2] == 1 && out9[3] == (double)0.08f);
    float S[16];
    memcpy(S, eye, 64);
    S[0] = 1.01f;
    CHECK(ml_system(k.data(), v.data(), k.size(), &c, d.data(), S, nullptr, sums, counts) == 2);
  }
  if (g_bad) { fprintf(stderr, "map_locate_san: %d checks failed\n", g_bad); return 1; }
  printf("map_locate_san ok\n");
  return 0;
}
