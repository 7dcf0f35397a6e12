// Stand-alone run of the colour half of the tracking in tandem_amd/csrc/fusion_host.h for a sanitizer build
// (tests/test_map_track_colour.py builds it with g++ -fsanitize=address,undefined and runs it), through the entry points of
// map_track_colour_check.cpp.  It reads one case from a file -- a drf_options_t, a drf_track_colour_options_t, height x width x 3
// frame colour bytes, height x width frame depths, the model's colour and depth likewise, 16 model pose floats, 16 pose floats --
// runs the system on it and prints the sums as hexadecimal words, which the test compares with the restatement's; then, on its
// own, the whole loop over an analytic renderer of one textured plane (which geometry alone leaves degenerate), images down to
// 1 x 1, model depths that no ray-cast writes, strides up to and beyond the image, poses that look away, the term at the image's
// edges, and what the calls refuse.
//   map_track_colour_san CASE      exits 0 when every check holds
#include <cstdio>
#include <random>

#include "map_track_colour_check.cpp"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad < 20) fprintf(stderr, "map_track_colour_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

// the analytic ray-cast of the world plane z = 1.5, coloured by a texture of the hit's world (X, Y)
struct Plane {
  drf_options_t cam;
  int renders = 0;
};
static void render_plane(const float *p16, unsigned char *bgr, float *out, void *user) {
  Plane *s = (Plane *)user;
  ++s->renders;
  for (int v = 0; v < s->cam.height; ++v)
    for (int u = 0; u < s->cam.width; ++u) {
      const double ray[3] = {((double)u - s->cam.cx) / s->cam.fx, ((double)v - s->cam.cy) / s->cam.fy, 1.0};
      double d[3];
      for (int i = 0; i < 3; ++i) d[i] = p16[4 * i] * ray[0] + p16[4 * i + 1] * ray[1] + p16[4 * i + 2] * ray[2];
      const double z = (1.5 - p16[11]) / d[2];
      const size_t at = (size_t)v * s->cam.width + u;
      const bool hit = z > 0.0;
      out[at] = hit ? (float)z : 0.0f;
      const double X = p16[3] + d[0] * z, Y = p16[7] + d[1] * z;
      const int y = hit ? (int)std::floor(3.0 * (127.5 + 110.0 * (std::sin(9.0 * X + 1.0) + std::sin(7.0 * Y + 2.0) + std::sin(5.0 * X - 6.0 * Y)) / 3.0) + 0.5) : 0;
      bgr[3 * at] = (unsigned char)(y / 3); bgr[3 * at + 1] = (unsigned char)((y + 1) / 3); bgr[3 * at + 2] = (unsigned char)((y + 2) / 3);
    }
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: map_track_colour_san CASE\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  drf_options_t cam;
  drf_track_colour_options_t opt;
  float mpose[16], pose[16];
  bool ok = fread(&cam, sizeof cam, 1, f) == 1 && fread(&opt, sizeof opt, 1, f) == 1 && cam.width > 0 && cam.height > 0 && cam.width <= 4096 && cam.height <= 4096;
  const size_t npix = ok ? (size_t)cam.width * cam.height : 0;
  std::vector<float> depth(npix), model(npix);
  std::vector<unsigned char> bgr(npix * 3), mbgr(npix * 3);
  ok = ok && fread(bgr.data(), 1, bgr.size(), f) == bgr.size() && fread(depth.data(), 4, npix, f) == npix && fread(mbgr.data(), 1, mbgr.size(), f) == mbgr.size() &&
       fread(model.data(), 4, npix, f) == npix && fread(mpose, 4, 16, f) == 16 && fread(pose, 4, 16, f) == 16;
  fclose(f);
  if (!ok) { fprintf(stderr, "map_track_colour_san: %s is not a case file\n", argv[1]); return 2; }
  {
    double sums[28];
    unsigned long long counts[5];
    CHECK(mtc_system(&cam, bgr.data(), depth.data(), mbgr.data(), model.data(), mpose, pose, &opt, sums, counts) == 0);
    CHECK(counts[0] == counts[1] + counts[2] + counts[3] && counts[4] <= counts[1]);
    printf("system");
    for (int i = 0; i < 28; ++i) { unsigned long long w; memcpy(&w, &sums[i], 8); printf(" %llx", w); }
    printf(" %llu %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3], counts[4]);
  }
  const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  {  // the loop over the textured plane: geometry alone is degenerate, with colour the start comes home
    Plane s;
    s.cam = cam;
    s.cam.width = 40; s.cam.height = 30; s.cam.fx = s.cam.fy = 36.0f; s.cam.cx = 19.5f; s.cam.cy = 14.5f;
    const size_t n = (size_t)s.cam.width * s.cam.height;
    std::vector<float> fd(n);
    std::vector<unsigned char> fc(n * 3);
    render_plane(eye, fc.data(), fd.data(), &s);
    const float ca = 0.99984770f, sa = 0.01745241f;  // 1 degree about z
    const float start[16] = {ca, -sa, 0, 0.032f, sa, ca, 0, -0.024f, 0, 0, 1, 0.01f, 0, 0, 0, 1};
    for (int step : {1, 2}) {
      drf_track_colour_options_t o = {{6, 3, step, 0.0f, 0.0f, 0.0f, 1.5f, 1e-4, 1e-3, 0.0}, 0.0f};
      drf_align_result_t r;
      std::vector<double> trace(18 * 28);
      unsigned long long st[7];
      s.renders = 0;
      CHECK(mtc_frame(&s.cam, fc.data(), fd.data(), render_plane, &s, start, &o, 0, &r, trace.data(), 18, st) == 0);
      CHECK(r.status == DRF_ALIGN_DEGENERATE && r.iterations == 1 && s.renders == 1);
      s.renders = 0;
      CHECK(mtc_frame(&s.cam, fc.data(), fd.data(), render_plane, &s, start, &o, 1, &r, trace.data(), 18, st) == 0);
      CHECK(r.status >= 0 && r.status <= 3 && r.status != DRF_ALIGN_DEGENERATE && r.iterations >= 1 && r.iterations <= 18 && (int)st[5] == r.iterations);
      CHECK((int)st[6] == s.renders && s.renders >= 1 && s.renders <= 6);
      CHECK(st[0] == st[1] + st[2] + st[3] && st[4] <= st[1] && st[4] > 0 && r.samples == st[0] && r.valid == st[1]);
      CHECK(memcmp(&trace[(size_t)(r.iterations - 1) * 28], r.sums, 224) == 0);
      const double e = std::sqrt(r.T[3] * r.T[3] + r.T[7] * r.T[7] + r.T[11] * r.T[11]);
      CHECK(r.status == DRF_ALIGN_LOST || e < 0.02);  // it came closer than the 0.041 m it started at
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
        const size_t n = (size_t)w * h;
        std::vector<float> d(n), m(n), map4(n * 4), Ym(n);
        std::vector<unsigned char> dc(n * 3), mc(n * 3);
        for (auto &x : d) x = rng() % 4 == 0 ? special[rng() % 6] : 0.8f + 0.1f * U(rng);
        for (auto &x : m) x = rng() % 6 == 0 ? special[rng() % 6] : 0.8f + 0.1f * U(rng);
        for (auto &x : dc) x = (unsigned char)(rng() % 256);
        for (auto &x : mc) x = (unsigned char)(rng() % 256);
        CHECK(mtc_model(&c, mc.data(), m.data(), 0.05f, map4.data(), Ym.data()) == 0);
        for (size_t i = 0; i < n; ++i) CHECK(map4[4 * i + 3] > 0.0f ? Ym[i] == (float)(mc[3 * i] + mc[3 * i + 1] + mc[3 * i + 2]) : Ym[i] == -1.0f);
        for (int step : {1, 2, 3, 28, 29, 37, 100})
          for (const float *T : {eye, back, side, far}) {
            drf_track_colour_options_t o = {{0, 0, step, step == 3 ? 0.02f : 0.0f, step == 2 ? 0.01f : 0.0f, 0.0f, step == 1 ? 0.8f : 0.0f, 0.0, 0.0, 0.0},
                                            step == 2 ? 0.2f : 0.0f};
            double sums[28];
            unsigned long long counts[5];
            CHECK(mtc_system(&c, dc.data(), d.data(), mc.data(), m.data(), eye, T, &o, sums, counts) == 0);
            CHECK(counts[0] == counts[1] + counts[2] + counts[3] && counts[4] <= counts[1]);
            if (T != eye) CHECK(counts[1] == 0);
            if (w < 3 || h < 3) CHECK(counts[1] == 0 && counts[3] == 0 && counts[4] == 0);
            CHECK(mtc_system(&c, dc.data(), d.data(), mc.data(), m.data(), T, T, &o, sums, counts) == 0);  // the model's pose is the frame's
            CHECK(counts[0] == counts[1] + counts[2] + counts[3] && counts[4] <= counts[1]);
          }
        // the term at and beyond every edge of an intensity map whose border carries colour
        std::vector<float> Y(n);
        for (auto &x : Y) x = rng() % 7 == 0 ? -1.0f : (float)(rng() % 766);
        for (double up : {-0.5, -1e-9, 0.0, 0.5, w - 2.0, w - 1.5, w - 1.0 - 1e-9, w - 1.0, w - 0.51})
          for (double vp : {-0.5, 0.0, h - 2.0, h - 1.0 - 1e-9, h - 1.0, h - 0.51}) {
            const double mm[3] = {1.0, -2.0, 45.0};
            double out4[4];
            const int added = mtc_term(&c, Y.data(), eye, mm, up, vp, 100.0f, 0.037f, out4);
            if (up < 0.0 || vp < 0.0 || std::floor(up) + 1.0 > w - 1.0 || std::floor(vp) + 1.0 > h - 1.0) CHECK(added == 0);
            if (added) CHECK(std::isfinite(out4[0]) && std::isfinite(out4[3]));
          }
      }
  }
  {  // what the calls refuse
    drf_track_colour_options_t bad = {{0, 0, -1, 0.0f, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.0}, 0.0f};
    double out11[11], sums[28];
    unsigned long long counts[5];
    unsigned wb;
    char name[32];
    CHECK(mtc_options(&bad, 0.02f, out11, &wb, name) == 1 && strcmp(name, "step") == 0);
    bad.track.step = 0; bad.photo_weight = NAN;
    CHECK(mtc_options(&bad, 0.02f, out11, &wb, name) == 1 && strcmp(name, "photo_weight") == 0);
    bad.photo_weight = -0.5f;
    CHECK(mtc_system(&cam, bgr.data(), depth.data(), mbgr.data(), model.data(), mpose, pose, &bad, sums, counts) == 1);
    CHECK(mtc_options(nullptr, 0.02f, out11, &wb, name) == 0 && out11[0] == 10 && out11[1] == 4 && out11[10] == (double)(float)(1.0 / 27.0));
    float S[16];
    memcpy(S, eye, 64);
    S[0] = 1.01f;
    CHECK(mtc_system(&cam, bgr.data(), depth.data(), mbgr.data(), model.data(), mpose, S, nullptr, sums, counts) == 2);
    CHECK(mtc_system(&cam, bgr.data(), depth.data(), mbgr.data(), model.data(), S, pose, nullptr, sums, counts) == 2);
  }
  if (g_bad) { fprintf(stderr, "map_track_colour_san: %d checks failed\n", g_bad); return 1; }
  printf("map_track_colour_san ok\n");
  return 0;
}
