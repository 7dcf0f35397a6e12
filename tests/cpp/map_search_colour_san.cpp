// Stand-alone run of the colour half of the search in tandem_amd/csrc/pose_host.h for a sanitizer build
// (tests/test_map_search_colour.py builds it with g++ -fsanitize=address,undefined and runs it), through the entry points of
// map_search_colour_check.cpp.  It reads one case from a file -- u64 n, n keys, n x 4096 voxel bytes, a drf_options_t, height x
// width x 3 colour bytes, height x width depths, u64 n_poses and their 16 floats each, u64 n_anchors and theirs, u64 n_rot and 9
// doubles each -- scores the poses (step 3, weight 0.01, cap 3) and a lattice (half 1 2 0, 0.08 m, the same options) and prints
// cost, photo and the lattice's scores as hexadecimal words, which the test compares with the restatement's; then, on its own, a
// whole search over a renderer that sees nothing and one that returns the frame, a lattice of one candidate, the empty map, an
// image without a sample, strides up to the image, and what the calls refuse.
//   map_search_colour_san CASE      exits 0 when every check holds
#include <cstdio>
#include <random>

#include "map_search_colour_check.cpp"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad < 20) fprintf(stderr, "map_search_colour_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

static void print_words(const char *what, const std::vector<double> &v) {
  printf("%s", what);
  for (double x : v) { unsigned long long w; memcpy(&w, &x, 8); printf(" %llx", w); }
  printf("\n");
}
struct Frame { const unsigned char *bgr; const float *depth; size_t n; };
static void render_none(const float *, unsigned char *cout, float *dout, void *user) {
  memset(cout, 0, ((Frame *)user)->n * 3);
  memset(dout, 0, ((Frame *)user)->n * 4);
}
static void render_frame(const float *, unsigned char *cout, float *dout, void *user) {
  memcpy(cout, ((Frame *)user)->bgr, ((Frame *)user)->n * 3);
  memcpy(dout, ((Frame *)user)->depth, ((Frame *)user)->n * 4);
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: map_search_colour_san CASE\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  unsigned long long n = 0, np = 0, na = 0, nr = 0;
  drf_options_t cam;
  bool ok = fread(&n, 8, 1, f) == 1 && n < 100000;
  std::vector<unsigned long long> keys(ok ? n : 0);
  std::vector<unsigned char> vox(ok ? n * 4096 : 0);
  ok = ok && fread(keys.data(), 8, n, f) == n && fread(vox.data(), 4096, n, f) == n && fread(&cam, sizeof cam, 1, f) == 1;
  ok = ok && cam.width > 0 && cam.height > 0 && cam.width <= 4096 && cam.height <= 4096;
  std::vector<unsigned char> bgr(ok ? (size_t)cam.width * cam.height * 3 : 0);
  std::vector<float> depth(ok ? (size_t)cam.width * cam.height : 0);
  ok = ok && fread(bgr.data(), 1, bgr.size(), f) == bgr.size() && fread(depth.data(), 4, depth.size(), f) == depth.size() && fread(&np, 8, 1, f) == 1 && np > 0 && np < 10000;
  std::vector<float> poses(ok ? np * 16 : 0);
  ok = ok && fread(poses.data(), 4, poses.size(), f) == poses.size() && fread(&na, 8, 1, f) == 1 && na > 0 && na < 100;
  std::vector<float> anchors(ok ? na * 16 : 0);
  ok = ok && fread(anchors.data(), 4, anchors.size(), f) == anchors.size() && fread(&nr, 8, 1, f) == 1 && nr > 0 && nr < 100;
  std::vector<double> rot(ok ? nr * 9 : 0);
  ok = ok && fread(rot.data(), 8, rot.size(), f) == rot.size();
  fclose(f);
  if (!ok) { fprintf(stderr, "map_search_colour_san: %s is not a case file\n", argv[1]); return 2; }
  Frame frame = {bgr.data(), depth.data(), depth.size()};
  float out[16];
  char name[32];
  drf_search_colour_result_t res;
  {
    drf_score_colour_options_t so = {{3, 0, 0.0f, 0.0f, 0.0f, 0.0f}, 0.01f, 3.0f};
    std::vector<double> cost(np), photo(np), score(np), geo(np);
    std::vector<uint32_t> counts(4 * np);
    CHECK(msc_score(keys.data(), vox.data(), n, &cam, bgr.data(), depth.data(), poses.data(), np, &so, cost.data(), photo.data(), counts.data(), score.data(), geo.data()) == 0);
    for (size_t i = 0; i < np; ++i) {
      CHECK(counts[4 * i] == counts[4 * i + 1] + counts[4 * i + 2] + counts[4 * i + 3]);
      CHECK(photo[i] >= 0.0 && photo[i] <= 3.0 * counts[4 * i + 1] && !(score[i] < geo[i]));
    }
    print_words("cost", cost);
    print_words("photo", photo);
    drf_search_colour_options_t lo = {{so.score, 0.08f, {1, 2, 0}, 5, 1, 0.0}, 0.01f, 3.0f};
    const size_t nc = na * nr * 15;
    std::vector<double> all(nc), allp(nc);
    CHECK(msc_search(keys.data(), vox.data(), n, &cam, bgr.data(), depth.data(), render_none, &frame, anchors.data(), na, rot.data(), nr, &lo, nullptr, nullptr, out, &res,
                     all.data(), allp.data(), name) == 0);
    CHECK(res.status == DRF_ALIGN_MAX_ITERS && res.winner == 0 && res.refined == 0 && res.n_candidates == nc && res.n_entries == 5);
    for (int k = 1; k < res.n_entries; ++k) CHECK(!(res.entries[k].score < res.entries[k - 1].score));
    for (int k = 0; k < res.n_entries; ++k) CHECK(res.entries[k].photo == allp[res.entries[k].index] && res.entries[k].final_score == 0.0);
    print_words("lattice", all);
    // the whole search: a renderer that sees nothing loses every entry at its tracking; one that returns the frame itself tracks
    lo.search.score_only = 0; lo.search.top_k = 3;
    CHECK(msc_search(keys.data(), vox.data(), n, &cam, bgr.data(), depth.data(), render_none, &frame, anchors.data(), na, rot.data(), nr, &lo, nullptr, nullptr, out, &res,
                     nullptr, nullptr, name) == 0);
    CHECK(res.status == DRF_ALIGN_LOST && res.winner == -1 && res.refined == 3);
    for (int k = 0; k < 3; ++k) CHECK(res.entries[k].track_status == DRF_ALIGN_LOST && res.entries[k].locate_status == -1 && res.entries[k].final_score == 0.0);
    for (int i = 0; i < 16; ++i) CHECK(out[i] == (float)res.entries[0].T[i]);
    drf_track_pyramid_options_t to;
    memset(&to, 0, sizeof to);
    to.colour.track.max_renders = 2; to.colour.track.inner_iters = 2; to.colour.track.step = 3; to.colour.track.min_valid = 0.01;
    to.levels = 2; to.coarse_renders = 1;
    drf_locate_options_t lc = {3, 0, 3, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.01};
    for (double accept : {0.0, 0.01}) {
      lo.search.accept_valid = accept;
      CHECK(msc_search(keys.data(), vox.data(), n, &cam, bgr.data(), depth.data(), render_frame, &frame, anchors.data(), na, rot.data(), nr, &lo, &to, &lc, out, &res,
                       nullptr, nullptr, name) == 0);
      CHECK(res.refined >= 1 && res.refined <= 3 && res.status >= 0 && res.status <= 3 && res.winner >= -1 && res.winner < 3);
      if (res.winner >= 0) CHECK(res.entries[res.winner].locate_status <= DRF_ALIGN_MAX_ITERS && res.status == res.entries[res.winner].locate_status);
    }
    // one candidate; top_k above the count
    drf_search_colour_options_t one = {{so.score, 0.0f, {0, 0, 0}, 32, 1, 0.0}, 0.0f, 0.0f};
    double s1 = 0.0;
    CHECK(msc_search(keys.data(), vox.data(), n, &cam, bgr.data(), depth.data(), render_none, &frame, anchors.data(), 1, rot.data(), 1, &one, nullptr, nullptr, out, &res,
                     &s1, nullptr, name) == 0);
    CHECK(res.n_entries == 1 && res.n_candidates == 1 && res.entries[0].score == s1);
  }
  {  // strides up to the image, the empty map, an image without a sample
    drf_options_t c = cam;
    c.width = 37; c.height = 29; c.cx = 18.0f; c.cy = 14.0f; c.fx = c.fy = 40.0f;
    std::mt19937 rng(9);
    std::vector<float> d((size_t)c.width * c.height);
    std::vector<unsigned char> col(d.size() * 3);
    const float special[6] = {0.0f, NAN, -1.0f, 0.01f, 1e9f, INFINITY};
    for (auto &x : d) x = rng() % 4 == 0 ? special[rng() % 6] : 0.4f + 1.2f * (float)(rng() % 1000) / 1000.0f;
    for (auto &x : col) x = (unsigned char)(rng() & 255);
    for (int step : {1, 2, 3, 7, 28, 29, 36, 37, 100}) {
      drf_score_colour_options_t so = {{step, step % 2 ? 0 : 3, step == 3 ? 0.02f : 0.0f, step == 2 ? 0.25f : 0.0f, step == 7 ? 0.5f : 0.0f, 0.0f}, step == 1 ? 0.5f : 0.0f,
                                       step == 2 ? 0.01f : 0.0f};
      std::vector<double> cost(np), photo(np), score(np), geo(np);
      std::vector<uint32_t> counts(4 * np);
      CHECK(msc_score(keys.data(), vox.data(), n, &c, col.data(), d.data(), poses.data(), np, &so, cost.data(), photo.data(), counts.data(), score.data(), geo.data()) == 0);
      for (size_t i = 0; i < np; ++i) CHECK(counts[4 * i] == counts[0] && counts[4 * i] == counts[4 * i + 1] + counts[4 * i + 2] + counts[4 * i + 3]);
    }
    double cost, photo, score;
    uint32_t counts[4];
    CHECK(msc_score(nullptr, nullptr, 0, &c, col.data(), d.data(), poses.data(), 1, nullptr, &cost, &photo, counts, &score, nullptr) == 0);
    CHECK(counts[0] > 0 && counts[1] == 0 && counts[2] == counts[0] && cost == 0.0 && photo == 0.0 && score == 8.0);
    std::vector<float> none(d.size(), 0.0f);
    CHECK(msc_score(keys.data(), vox.data(), n, &c, col.data(), none.data(), poses.data(), 1, nullptr, &cost, &photo, counts, &score, nullptr) == 0);
    CHECK(counts[0] == 0 && counts[1] == 0 && counts[2] == 0 && counts[3] == 0 && cost == 0.0 && photo == 0.0 && score == 8.0);
  }
  {  // what the calls refuse
    drf_search_colour_options_t bad;
    memset(&bad, 0, sizeof bad);
    double out16[16];
    bad.photo_cap = -1.0f;
    CHECK(msc_options(&bad, 0, 0.08f, 0.02f, out16, name) == 1 && strcmp(name, "photo_cap") == 0);
    bad.photo_weight = NAN;
    CHECK(msc_options(&bad, 0, 0.08f, 0.02f, out16, name) == 1 && strcmp(name, "photo_weight") == 0);
    bad.search.top_k = DRF_SEARCH_MAX_TOP + 1;
    CHECK(msc_options(&bad, 0, 0.08f, 0.02f, out16, name) == 1 && strcmp(name, "top_k") == 0);
    CHECK(msc_options(nullptr, 0, 0.08f, 0.02f, out16, name) == 0 && out16[0] == 4 && out16[10] == 8 && out16[15] == 4.0);
    drf_search_colour_options_t big;
    memset(&big, 0, sizeof big);
    big.search.half[0] = big.search.half[1] = big.search.half[2] = 200;
    CHECK(msc_search(keys.data(), vox.data(), n, &cam, bgr.data(), depth.data(), render_none, &frame, anchors.data(), na, rot.data(), nr, &big, nullptr, nullptr, out, &res,
                     nullptr, nullptr, name) == 3);
    std::vector<float> scaled(anchors.begin(), anchors.begin() + 16);
    scaled[0] *= 1.01f;
    CHECK(msc_search(keys.data(), vox.data(), n, &cam, bgr.data(), depth.data(), render_none, &frame, scaled.data(), 1, rot.data(), nr, nullptr, nullptr, nullptr, out, &res,
                     nullptr, nullptr, name) == 2);
    double cost;
    CHECK(msc_score(keys.data(), vox.data(), n, &cam, bgr.data(), depth.data(), scaled.data(), 1, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == 2);
  }
  if (g_bad) { fprintf(stderr, "map_search_colour_san: %d checks failed\n", g_bad); return 1; }
  printf("map_search_colour_san ok\n");
  return 0;
}
