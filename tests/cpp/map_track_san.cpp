// Stand-alone run of the tracking half of tandem_amd/csrc/fusion_host.h for a sanitizer build (tests/test_map_track.py builds it
// with g++ -fsanitize=address,undefined and runs it), through the entry points of map_track_check.cpp.  It reads one case from a
// file -- a drf_options_t, a drf_track_options_t, height x width frame depths, height x width model depths, 16 model pose floats,
// 16 pose floats -- runs the system on it and prints the sums as hexadecimal words, which the test compares with the restatement's;
// then, on its own, the whole loop over an analytic renderer of three planes, images down to 1 x 1, model depths that no ray-cast
// writes (NaN, infinity, negative), strides up to and beyond the image, poses that look away, and what the calls refuse.
//   map_track_san CASE      exits 0 when every check holds
#include <cstdio>
#include <random>

#include "map_track_check.cpp"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad < 20) fprintf(stderr, "map_track_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

// the analytic ray-cast of three world planes n . X = c (the nearest hit in front of the camera, 0 where there is none)
struct Planes {
  drf_options_t cam;
  int renders = 0;
};
static void render_planes(const float *p16, float *out, void *user) {
  Planes *s = (Planes *)user;
  ++s->renders;
  static const double n[3][3] = {{0.6, 0.0, 0.8}, {-0.6, 0.0, 0.8}, {0.0, 0.8, 0.6}};
  static const double c[3] = {1.6, 1.5, 1.7};
  for (int v = 0; v < s->cam.height; ++v)
    for (int u = 0; u < s->cam.width; ++u) {
      const double ray[3] = {((double)u - s->cam.cx) / s->cam.fx, ((double)v - s->cam.cy) / s->cam.fy, 1.0};
      double best = 0.0;
      for (int k = 0; k < 3; ++k) {
        double nd = 0.0, nt = 0.0;
        for (int i = 0; i < 3; ++i) {
          nd += n[k][i] * (p16[4 * i] * ray[0] + p16[4 * i + 1] * ray[1] + p16[4 * i + 2] * ray[2]);
          nt += n[k][i] * p16[4 * i + 3];
        }
        const double z = (c[k] - nt) / nd;
        if (z > 0.0 && (best == 0.0 || z < best)) best = z;
      }
      out[(size_t)v * s->cam.width + u] = (float)best;
    }
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: map_track_san CASE\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  drf_options_t cam;
  drf_track_options_t opt;
  float mpose[16], pose[16];
  bool ok = fread(&cam, sizeof cam, 1, f) == 1 && fread(&opt, sizeof opt, 1, f) == 1 && cam.width > 0 && cam.height > 0 && cam.width <= 4096 && cam.height <= 4096;
  std::vector<float> depth(ok ? (size_t)cam.width * cam.height : 0), model(depth.size());
  ok = ok && fread(depth.data(), 4, depth.size(), f) == depth.size() && fread(model.data(), 4, model.size(), f) == model.size() && fread(mpose, 4, 16, f) == 16 &&
       fread(pose, 4, 16, f) == 16;
  fclose(f);
  if (!ok) { fprintf(stderr, "map_track_san: %s is not a case file\n", argv[1]); return 2; }
  {
    double sums[28];
    unsigned long long counts[4];
    CHECK(mt_system(&cam, depth.data(), model.data(), mpose, pose, &opt, sums, counts) == 0);
    CHECK(counts[0] == counts[1] + counts[2] + counts[3]);
    printf("system");
    for (int i = 0; i < 28; ++i) { unsigned long long w; memcpy(&w, &sums[i], 8); printf(" %llx", w); }
    printf(" %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3]);
  }
  const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  {  // the loop over the analytic renderer: a start a few voxels and degrees off the pose the frame was rendered at
    Planes s;
    s.cam = cam;
    s.cam.width = 40; s.cam.height = 30; s.cam.fx = s.cam.fy = 36.0f; s.cam.cx = 19.5f; s.cam.cy = 14.5f;
    std::vector<float> frame((size_t)s.cam.width * s.cam.height);
    render_planes(eye, frame.data(), &s);
    const float ca = 0.99939083f, sa = 0.0348995f;  // 2 degrees about y
    const float start[16] = {ca, 0, sa, 0.06f, 0, 1, 0, -0.04f, -sa, 0, ca, 0.05f, 0, 0, 0, 1};
    for (int step : {1, 2}) {
      drf_track_options_t o = {6, 3, step, 0.0f, 0.0f, 0.0f, 1.6f, 1e-4, 1e-3, 0.0};
      drf_align_result_t r;
      std::vector<double> trace(18 * 28);
      unsigned long long st[6];
      s.renders = 0;
      CHECK(mt_frame(&s.cam, frame.data(), render_planes, &s, start, &o, &r, trace.data(), 18, st) == 0);
      CHECK(r.status >= 0 && r.status <= 3 && r.iterations >= 1 && r.iterations <= 18 && (int)st[4] == r.iterations);
      CHECK((int)st[5] == s.renders && s.renders >= 1 && s.renders <= 6);
      CHECK(st[0] == st[1] + st[2] + st[3] && r.samples == st[0] && r.valid == st[1]);
      CHECK(r.T[12] == 0.0 && r.T[13] == 0.0 && r.T[14] == 0.0 && r.T[15] == 1.0);
      CHECK(memcmp(&trace[(size_t)(r.iterations - 1) * 28], r.sums, 224) == 0);
      const double e = std::sqrt(r.T[3] * r.T[3] + r.T[7] * r.T[7] + r.T[11] * r.T[11]);
      CHECK(r.status == DRF_ALIGN_LOST || r.status == DRF_ALIGN_DEGENERATE || e < 0.03);  // it came closer than the 0.088 m it started at
      printf("loop step %d: status %d, %d evaluations, %d renders, |t| %.4f\n", step, r.status, r.iterations, s.renders, e);
    }
  }
  {  // small images, depths that no ray-cast writes, strides beyond the image, poses that look away
    std::mt19937 rng(9);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const float special[6] = {0.0f, NAN, -1.0f, 0.01f, 1e9f, INFINITY};
    const float back[16] = {-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1};
    const float side[16] = {0, 0, 1, 0, 0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 0, 1};
    const float far[16] = {1, 0, 0, 167772.0f, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int w : {1, 2, 3, 5, 37})
      for (int h : {1, 2, 3, 29}) {
        drf_options_t c = cam;
        c.width = w; c.height = h; c.cx = (w - 1) / 2.0f; c.cy = (h - 1) / 2.0f; c.fx = c.fy = 40.0f;
        std::vector<float> d((size_t)w * h), m((size_t)w * h), map4((size_t)w * h * 4);
        for (auto &x : d) x = rng() % 4 == 0 ? special[rng() % 6] : 0.8f + 0.1f * U(rng);
        for (auto &x : m) x = rng() % 6 == 0 ? special[rng() % 6] : 0.8f + 0.1f * U(rng);
        CHECK(mt_model(&c, m.data(), 0.05f, map4.data()) == 0);
        for (int v = 0; v < h; ++v)
          for (int u = 0; u < w; ++u) {
            const float *p = &map4[((size_t)v * w + u) * 4];
            if (u == 0 || v == 0 || u == w - 1 || v == h - 1) CHECK(p[0] == 0.0f && p[1] == 0.0f && p[2] == 0.0f && p[3] == 0.0f);
            if (p[3] != 0.0f) CHECK(p[3] == m[(size_t)v * w + u] && p[2] < 0.0f);
          }
        for (int step : {1, 2, 3, 28, 29, 37, 100})
          for (const float *T : {eye, back, side, far}) {
            drf_track_options_t o = {0, 0, step, step == 3 ? 0.02f : 0.0f, step == 2 ? 0.01f : 0.0f, 0.0f, step == 1 ? 0.8f : 0.0f, 0.0, 0.0, 0.0};
            double sums[28];
            unsigned long long counts[4];
            CHECK(mt_system(&c, d.data(), m.data(), eye, T, &o, sums, counts) == 0);
            CHECK(counts[0] == counts[1] + counts[2] + counts[3]);
            if (T != eye) CHECK(counts[1] == 0);
            if (w < 3 || h < 3) CHECK(counts[1] == 0 && counts[3] == 0);
            CHECK(mt_system(&c, d.data(), m.data(), T, T, &o, sums, counts) == 0);  // the model's pose is the frame's: T drops out
            CHECK(counts[0] == counts[1] + counts[2] + counts[3]);
          }
      }
  }
  {  // what the calls refuse
    drf_track_options_t bad = {0, 0, -1, 0.0f, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.0};
    double out10[10], sums[28];
    unsigned long long counts[4];
    char name[32];
    CHECK(mt_options(&bad, 0.02f, out10, name) == 1 && strcmp(name, "step") == 0);
    bad.step = 0; bad.max_jump = NAN;
    CHECK(mt_options(&bad, 0.02f, out10, name) == 1 && strcmp(name, "max_jump") == 0);
    bad.max_jump = 0.0f; bad.max_renders = -4;
    CHECK(mt_system(&cam, depth.data(), model.data(), mpose, pose, &bad, sums, counts) == 1);
    CHECK(mt_options(nullptr, 0.02f, out10, name) == 0 && out10[0] == 10 && out10[1] == 4 && out10[3] == (double)(25.0f * 0.02f));
    float S[16];
    memcpy(S, eye, 64);
    S[0] = 1.01f;
    CHECK(mt_system(&cam, depth.data(), model.data(), mpose, S, nullptr, sums, counts) == 2);
    CHECK(mt_system(&cam, depth.data(), model.data(), S, pose, nullptr, sums, counts) == 2);
  }
  if (g_bad) { fprintf(stderr, "map_track_san: %d checks failed\n", g_bad); return 1; }
  printf("map_track_san ok\n");
  return 0;
}
