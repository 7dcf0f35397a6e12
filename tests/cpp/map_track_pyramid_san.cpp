// Stand-alone run of the coarse-to-fine half of the tracking in tandem_amd/csrc/pose_host.h for a sanitizer build
// (tests/test_map_track_pyramid.py builds it with g++ -fsanitize=address,undefined and runs it), through the entry points of
// map_track_pyramid_check.cpp.  It reads one case from a file -- a drf_options_t, a drf_track_pyramid_options_t, height x width x 3
// frame colour bytes, height x width frame depths, the model's colour and depth likewise, 16 model pose floats, 16 pose floats --
// runs the level-1 system on it and prints the sums as hexadecimal words, which the test compares with the restatement's; then,
// on its own: the reduction of images of every small size at every level, with depths that no sensor writes, into buffers of
// exactly the level's size; systems on cameras at and one pixel below the smallest level; the whole schedule over an analytic
// renderer of one textured plane, with and without colour; and what the calls refuse.
//   map_track_pyramid_san CASE      exits 0 when every check holds
#include <cstdio>
#include <random>

#include "map_track_pyramid_check.cpp"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad < 20) fprintf(stderr, "map_track_pyramid_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

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
  if (argc != 2) { fprintf(stderr, "usage: map_track_pyramid_san CASE\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  drf_options_t cam;
  drf_track_pyramid_options_t opt;
  float mpose[16], pose[16];
  bool ok = fread(&cam, sizeof cam, 1, f) == 1 && fread(&opt, sizeof opt, 1, f) == 1 && cam.width > 0 && cam.height > 0 && cam.width <= 4096 && cam.height <= 4096;
  const size_t npix = ok ? (size_t)cam.width * cam.height : 0;
  std::vector<float> depth(npix), model(npix);
  std::vector<unsigned char> bgr(npix * 3), mbgr(npix * 3);
  ok = ok && fread(bgr.data(), 1, bgr.size(), f) == bgr.size() && fread(depth.data(), 4, npix, f) == npix && fread(mbgr.data(), 1, mbgr.size(), f) == mbgr.size() &&
       fread(model.data(), 4, npix, f) == npix && fread(mpose, 4, 16, f) == 16 && fread(pose, 4, 16, f) == 16;
  fclose(f);
  if (!ok) { fprintf(stderr, "map_track_pyramid_san: %s is not a case file\n", argv[1]); return 2; }
  {
    double sums[28];
    unsigned long long counts[5];
    CHECK(mtp_system(&cam, 1, bgr.data(), depth.data(), mbgr.data(), model.data(), mpose, pose, &opt, sums, counts) == 0);
    CHECK(counts[0] == counts[1] + counts[2] + counts[3] && counts[4] <= counts[1]);
    printf("system");
    for (int i = 0; i < 28; ++i) { unsigned long long w; memcpy(&w, &sums[i], 8); printf(" %llx", w); }
    printf(" %llu %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3], counts[4]);
  }
  const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  {  // the reduction: every small size at every level, outputs of exactly the level's size (possibly empty)
    std::mt19937 rng(9);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const float special[6] = {0.0f, NAN, -1.0f, 0.01f, 1e9f, INFINITY};
    for (int w : {1, 2, 3, 7, 8, 15, 16, 17, 33, 67})
      for (int h : {1, 2, 5, 16, 31}) {
        const size_t n = (size_t)w * h;
        std::vector<float> d(n);
        std::vector<unsigned char> c(n * 3);
        for (auto &x : d) x = rng() % 4 == 0 ? special[rng() % 6] : 0.8f + 0.3f * U(rng);
        for (auto &x : c) x = (unsigned char)(rng() % 256);
        for (int L = 0; L < 5; ++L) {
          const size_t nl = (size_t)(w >> L) * (h >> L);
          std::vector<float> dl(nl);
          std::vector<unsigned char> cl(nl * 3);
          CHECK(mtp_reduce(w, h, L, 0.05f * (float)(1 << L), c.data(), d.data(), cl.data(), dl.data()) == 0);
          for (size_t i = 0; i < nl; ++i) {
            CHECK(dl[i] == 0.0f || (dl[i] >= 0.01f && dl[i] <= 1e9f));
            if (dl[i] == 0.0f) CHECK(cl[3 * i] == 0 && cl[3 * i + 1] == 0 && cl[3 * i + 2] == 0);
          }
          std::vector<float> alone(nl);
          CHECK(mtp_reduce(w, h, L, 0.05f * (float)(1 << L), nullptr, d.data(), nullptr, alone.data()) == 0);
          CHECK(nl == 0 || memcmp(alone.data(), dl.data(), nl * 4) == 0);
        }
        CHECK(mtp_reduce(w, h, 5, 0.1f, c.data(), d.data(), nullptr, nullptr) == 1 && mtp_reduce(w, h, -1, 0.1f, c.data(), d.data(), nullptr, nullptr) == 1);
      }
  }
  {  // a camera whose level 1 has exactly 8 pixels on a side, and one whose level 1 is one pixel too small
    for (int w : {16, 17, 15})
      for (int h : {16, 15}) {
        drf_options_t c = cam;
        c.width = w; c.height = h; c.cx = (w - 1) / 2.0f; c.cy = (h - 1) / 2.0f; c.fx = c.fy = 20.0f;
        const size_t n = (size_t)w * h;
        std::vector<float> d(n, 1.0f), m(n, 1.0f);
        std::vector<unsigned char> dc(n * 3, 90), mc(n * 3, 90);
        double sums[28];
        unsigned long long counts[5];
        drf_track_pyramid_options_t two = {{{0, 0, 0, 0.0f, 0.0f, 0.0f, 1.0f, 0.0, 0.0, 0.0}, 0.0f}, 2, 0}, one = two;
        one.levels = 1;
        const bool fits = w >= 16 && h >= 16;
        CHECK(mtp_system(&c, 1, dc.data(), d.data(), mc.data(), m.data(), eye, eye, &one, sums, counts) == (fits ? 0 : 1));
        CHECK(mtp_system(&c, 1, dc.data(), d.data(), mc.data(), m.data(), eye, eye, &two, sums, counts) == (fits ? 0 : 1));
        if (fits) CHECK(counts[0] == 64 && counts[1] == 36 && counts[4] > 0);  // the level's border has no model pixel
        CHECK(mtp_system(&c, 0, nullptr, d.data(), nullptr, m.data(), eye, eye, &one, sums, counts) == 0 && counts[0] == n && counts[4] == 0);
        drf_align_result_t r;
        unsigned long long st[33];
        Plane s;
        s.cam = c;
        std::vector<float> fd(n);
        std::vector<unsigned char> fc(n * 3);
        render_plane(eye, fc.data(), fd.data(), &s);
        std::vector<double> trace(64 * 28);
        CHECK(mtp_frame(&c, fc.data(), fd.data(), render_plane, &s, eye, &two, &r, trace.data(), 64, st) == (fits ? 0 : 1));
      }
  }
  {  // the schedule over the textured plane at 64 x 48: three levels, the start comes home; geometry alone is abandoned twice
    Plane s;
    s.cam = cam;
    s.cam.width = 64; s.cam.height = 48; s.cam.fx = s.cam.fy = 56.0f; s.cam.cx = 31.5f; s.cam.cy = 23.5f;
    const size_t n = (size_t)s.cam.width * s.cam.height;
    std::vector<float> fd(n);
    std::vector<unsigned char> fc(n * 3);
    render_plane(eye, fc.data(), fd.data(), &s);
    const float ca = 0.99984770f, sa = 0.01745241f;  // 1 degree about z
    const float start[16] = {ca, -sa, 0, 0.032f, sa, ca, 0, -0.024f, 0, 0, 1, 0.01f, 0, 0, 0, 1};
    for (int step : {1, 2}) {
      drf_track_pyramid_options_t o = {{{4, 3, step, 0.0f, 0.0f, 0.0f, 1.5f, 1e-4, 1e-3, 0.0}, 0.0f}, 3, 2};
      drf_align_result_t r;
      std::vector<double> trace(40 * 28);
      unsigned long long st[33];
      s.renders = 0;
      CHECK(mtp_frame(&s.cam, fc.data(), fd.data(), render_plane, &s, start, &o, &r, trace.data(), 40, st) == 0);
      CHECK(r.status >= 0 && r.status <= 3 && r.status != DRF_ALIGN_DEGENERATE);
      CHECK((int)st[4] == s.renders && st[6] == 3 && st[3] <= 24 && st[3] >= 3 && (int)st[8 + 2] == r.iterations && st[8 + 1] <= 4 && st[12 + 1] <= 2 && st[16 + 1] <= 2);
      CHECK(st[3] == st[8 + 2] + st[12 + 2] + st[16 + 2] && st[20 + 2] == 0 && st[24 + 2] == 0);
      CHECK(st[28] == st[29] + st[30] + st[31] && st[32] <= st[29] && r.samples == st[28] && r.valid == st[29]);
      CHECK(memcmp(&trace[(size_t)(st[3] - 1) * 28], r.sums, 224) == 0);
      const double e = std::sqrt(r.T[3] * r.T[3] + r.T[7] * r.T[7] + r.T[11] * r.T[11]);
      CHECK(r.status == DRF_ALIGN_LOST || e < 0.02);  // it came closer than the 0.041 m it started at
      printf("schedule step %d: status %d, %llu evaluations, %d renders, %llu abandoned, |t| %.4f\n", step, r.status, st[3], s.renders, st[7], e);
      s.renders = 0;
      CHECK(mtp_frame(&s.cam, nullptr, fd.data(), render_plane, &s, start, &o, &r, trace.data(), 40, st) == 0);
      CHECK(r.status == DRF_ALIGN_DEGENERATE && st[6] == 3 && st[7] == 2 && s.renders == 3 && st[3] == 3 && st[32] == 0);
      for (int i = 0; i < 16; ++i) CHECK((float)r.T[i] == start[i]);
    }
  }
  {  // what the calls refuse
    drf_track_pyramid_options_t bad = {{{0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.0}, 0.0f}, -1, 0};
    double out4[4], sums[28];
    unsigned long long counts[5];
    char name[32];
    CHECK(mtp_options(&bad, 0.02f, 128, 96, out4, name) == 1 && strcmp(name, "levels") == 0);
    bad.levels = 6;
    CHECK(mtp_options(&bad, 0.02f, 4096, 4096, out4, name) == 1 && strcmp(name, "levels") == 0);
    bad.levels = 2; bad.coarse_renders = -3;
    CHECK(mtp_options(&bad, 0.02f, 128, 96, out4, name) == 1 && strcmp(name, "coarse_renders") == 0);
    bad.colour.photo_weight = NAN;
    CHECK(mtp_options(&bad, 0.02f, 128, 96, out4, name) == 1 && strcmp(name, "photo_weight") == 0);
    CHECK(mtp_system(&cam, 1, bgr.data(), depth.data(), mbgr.data(), model.data(), mpose, pose, &bad, sums, counts) == 1);
    CHECK(mtp_options(nullptr, 0.02f, 128, 96, out4, name) == 0 && out4[0] == 3 && out4[1] == 3 && out4[2] == 10);
    float S[16];
    memcpy(S, eye, 64);
    S[0] = 1.01f;
    CHECK(mtp_system(&cam, 1, bgr.data(), depth.data(), mbgr.data(), model.data(), mpose, S, &opt, sums, counts) == 2);
    CHECK(mtp_system(&cam, 1, bgr.data(), depth.data(), mbgr.data(), model.data(), S, pose, &opt, sums, counts) == 2);
  }
  if (g_bad) { fprintf(stderr, "map_track_pyramid_san: %d checks failed\n", g_bad); return 1; }
  printf("map_track_pyramid_san ok\n");
  return 0;
}
