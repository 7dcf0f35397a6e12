// Stand-alone run of the search half of tandem_amd/csrc/pose_host.h for a sanitizer build (tests/test_map_search.py builds it with
// g++ -fsanitize=address,undefined and runs it), through the entry points of map_search_check.cpp.  It reads one case from a file
// -- u64 n, n keys, n x 4096 voxel bytes, a drf_options_t, height x width depths, u64 n_poses and their 16 floats each, u64
// n_anchors and theirs, u64 n_rot and 9 doubles each -- scores the poses (step 3) and a lattice (half 1 2 0, 0.08 m, step 3) and
// prints the costs and the lattice's scores as hexadecimal words, which the test compares with the restatement's; then, on its own,
// a whole search over a renderer that sees nothing and one that returns the frame, lattices of one candidate, the empty map, an
// image without a sample, strides up to the image, and what the calls refuse.
//   map_search_san CASE      exits 0 when every check holds
#include <cstdio>
#include <random>

#include "map_search_check.cpp"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad < 20) fprintf(stderr, "map_search_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

static void print_words(const char *what, const std::vector<double> &v) {
  printf("%s", what);
  for (double x : v) { unsigned long long w; memcpy(&w, &x, 8); printf(" %llx", w); }
  printf("\n");
}
struct Frame { const float *depth; size_t n; };
static void render_none(const float *, float *out, void *user) { memset(out, 0, ((Frame *)user)->n * 4); }
static void render_frame(const float *, float *out, void *user) { memcpy(out, ((Frame *)user)->depth, ((Frame *)user)->n * 4); }

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: map_search_san CASE\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  unsigned long long n = 0, np = 0, na = 0, nr = 0;
  drf_options_t cam;
  bool ok = fread(&n, 8, 1, f) == 1 && n < 100000;
  std::vector<unsigned long long> keys(ok ? n : 0);
  std::vector<unsigned char> vox(ok ? n * 4096 : 0);
  ok = ok && fread(keys.data(), 8, n, f) == n && fread(vox.data(), 4096, n, f) == n && fread(&cam, sizeof cam, 1, f) == 1;
  ok = ok && cam.width > 0 && cam.height > 0 && cam.width <= 4096 && cam.height <= 4096;
  std::vector<float> depth(ok ? (size_t)cam.width * cam.height : 0);
  ok = ok && fread(depth.data(), 4, depth.size(), f) == depth.size() && fread(&np, 8, 1, f) == 1 && np > 0 && np < 10000;
  std::vector<float> poses(ok ? np * 16 : 0);
  ok = ok && fread(poses.data(), 4, poses.size(), f) == poses.size() && fread(&na, 8, 1, f) == 1 && na > 0 && na < 100;
  std::vector<float> anchors(ok ? na * 16 : 0);
  ok = ok && fread(anchors.data(), 4, anchors.size(), f) == anchors.size() && fread(&nr, 8, 1, f) == 1 && nr > 0 && nr < 100;
  std::vector<double> rot(ok ? nr * 9 : 0);
  ok = ok && fread(rot.data(), 8, rot.size(), f) == rot.size();
  fclose(f);
  if (!ok) { fprintf(stderr, "map_search_san: %s is not a case file\n", argv[1]); return 2; }
  Frame frame = {depth.data(), depth.size()};
  float out[16];
  char name[32];
  drf_search_result_t res;
  {
    drf_score_options_t so = {3, 0, 0.0f, 0.0f, 0.0f, 0.0f};
    std::vector<double> cost(np), score(np);
    std::vector<uint32_t> counts(4 * np);
    CHECK(ms_score(keys.data(), vox.data(), n, &cam, depth.data(), poses.data(), np, &so, cost.data(), counts.data(), score.data()) == 0);
    for (size_t i = 0; i < np; ++i) CHECK(counts[4 * i] == counts[4 * i + 1] + counts[4 * i + 2] + counts[4 * i + 3]);
    print_words("score", cost);
    unsigned long long seen[4];
    CHECK(ms_point(keys.data(), vox.data(), n, &cam, depth.data(), poses.data(), &so, seen) == 0 && seen[3] == counts[0]);
    drf_search_options_t lo = {so, 0.08f, {1, 2, 0}, 5, 1, 0.0};
    const size_t nc = na * nr * 15;
    std::vector<double> all(nc);
    CHECK(ms_search(keys.data(), vox.data(), n, &cam, depth.data(), render_none, &frame, anchors.data(), na, rot.data(), nr, &lo, nullptr, nullptr, out, &res, all.data(),
                    name) == 0);
    CHECK(res.status == DRF_ALIGN_MAX_ITERS && res.winner == 0 && res.refined == 0 && res.n_candidates == nc && res.n_entries == 5);
    for (int k = 1; k < res.n_entries; ++k) CHECK(!(res.entries[k].score < res.entries[k - 1].score));
    print_words("lattice", all);
    // the whole search: a renderer that sees nothing loses every entry at its tracking; one that returns the frame itself tracks
    lo.score_only = 0; lo.top_k = 3;
    CHECK(ms_search(keys.data(), vox.data(), n, &cam, depth.data(), render_none, &frame, anchors.data(), na, rot.data(), nr, &lo, nullptr, nullptr, out, &res, nullptr,
                    name) == 0);
    CHECK(res.status == DRF_ALIGN_LOST && res.winner == -1 && res.refined == 3);
    for (int k = 0; k < 3; ++k) CHECK(res.entries[k].track_status == DRF_ALIGN_LOST && res.entries[k].locate_status == -1);
    for (int i = 0; i < 16; ++i) CHECK(out[i] == (float)res.entries[0].T[i]);
    drf_track_options_t to = {2, 2, 3, 0.0f, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.01};
    drf_locate_options_t lc = {3, 0, 3, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.01};
    lo.accept_valid = 0.01;
    CHECK(ms_search(keys.data(), vox.data(), n, &cam, depth.data(), render_frame, &frame, anchors.data(), na, rot.data(), nr, &lo, &to, &lc, out, &res, nullptr, name) == 0);
    CHECK(res.refined >= 1 && res.refined <= 3 && res.status >= 0 && res.status <= 3 && res.winner >= -1 && res.winner < 3);
    // one candidate; top_k above the count
    drf_search_options_t one = {so, 0.0f, {0, 0, 0}, 32, 1, 0.0};
    double s1 = 0.0;
    CHECK(ms_search(keys.data(), vox.data(), n, &cam, depth.data(), render_none, &frame, anchors.data(), 1, rot.data(), 1, &one, nullptr, nullptr, out, &res, &s1, name) == 0);
    CHECK(res.n_entries == 1 && res.n_candidates == 1 && res.entries[0].score == s1);
  }
  {  // strides up to the image, the empty map, an image without a sample
    drf_options_t c = cam;
    c.width = 37; c.height = 29; c.cx = 18.0f; c.cy = 14.0f; c.fx = c.fy = 40.0f;
    std::mt19937 rng(9);
    std::vector<float> d((size_t)c.width * c.height);
    const float special[6] = {0.0f, NAN, -1.0f, 0.01f, 1e9f, INFINITY};
    for (auto &x : d) x = rng() % 4 == 0 ? special[rng() % 6] : 0.4f + 1.2f * (float)(rng() % 1000) / 1000.0f;
    for (int step : {1, 2, 3, 7, 28, 29, 36, 37, 100}) {
      drf_score_options_t so = {step, step % 2 ? 0 : 3, step == 3 ? 0.02f : 0.0f, step == 2 ? 0.25f : 0.0f, step == 7 ? 0.5f : 0.0f, 0.0f};
      std::vector<double> cost(np), score(np);
      std::vector<uint32_t> counts(4 * np);
      CHECK(ms_score(keys.data(), vox.data(), n, &c, d.data(), poses.data(), np, &so, cost.data(), counts.data(), score.data()) == 0);
      for (size_t i = 0; i < np; ++i) CHECK(counts[4 * i] == counts[0] && counts[4 * i] == counts[4 * i + 1] + counts[4 * i + 2] + counts[4 * i + 3]);
    }
    double cost, score;
    uint32_t counts[4];
    CHECK(ms_score(nullptr, nullptr, 0, &c, d.data(), poses.data(), 1, nullptr, &cost, counts, &score) == 0);
    CHECK(counts[0] > 0 && counts[1] == 0 && counts[2] == counts[0] && cost == 0.0 && score == 8.0);
    std::vector<float> none(d.size(), 0.0f);
    CHECK(ms_score(keys.data(), vox.data(), n, &c, none.data(), poses.data(), 1, nullptr, &cost, counts, &score) == 0);
    CHECK(counts[0] == 0 && counts[1] == 0 && counts[2] == 0 && counts[3] == 0 && cost == 0.0 && score == 8.0);
  }
  {  // what the calls refuse
    drf_search_options_t bad;
    memset(&bad, 0, sizeof bad);
    double out13[13];
    bad.top_k = DRF_SEARCH_MAX_TOP + 1;
    CHECK(ms_options(&bad, 0.08f, 0.02f, out13, name) == 1 && strcmp(name, "top_k") == 0);
    bad.top_k = 0; bad.half[1] = -1;
    CHECK(ms_options(&bad, 0.08f, 0.02f, out13, name) == 1 && strcmp(name, "half") == 0);
    bad.half[1] = 0; bad.score.unobserved_cost = NAN;
    CHECK(ms_options(&bad, 0.08f, 0.02f, out13, name) == 1 && strcmp(name, "unobserved_cost") == 0);
    CHECK(ms_options(nullptr, 0.08f, 0.02f, out13, name) == 0 && out13[0] == 4 && out13[10] == 8);
    drf_search_options_t big;
    memset(&big, 0, sizeof big);
    big.half[0] = big.half[1] = big.half[2] = 200;
    CHECK(ms_search(keys.data(), vox.data(), n, &cam, depth.data(), render_none, &frame, anchors.data(), na, rot.data(), nr, &big, nullptr, nullptr, out, &res, nullptr,
                    name) == 3);
    CHECK(ms_search(keys.data(), vox.data(), n, &cam, depth.data(), render_none, &frame, anchors.data(), 0, rot.data(), nr, nullptr, nullptr, nullptr, out, &res, nullptr,
                    name) == 3);
    std::vector<double> mirror(rot.begin(), rot.begin() + 9);
    mirror[4] = -mirror[4];
    CHECK(ms_search(keys.data(), vox.data(), n, &cam, depth.data(), render_none, &frame, anchors.data(), na, mirror.data(), 1, nullptr, nullptr, nullptr, out, &res, nullptr,
                    name) == 2);
    std::vector<float> scaled(anchors.begin(), anchors.begin() + 16);
    scaled[0] *= 1.01f;
    CHECK(ms_search(keys.data(), vox.data(), n, &cam, depth.data(), render_none, &frame, scaled.data(), 1, rot.data(), nr, nullptr, nullptr, nullptr, out, &res, nullptr,
                    name) == 2);
    double cost;
    CHECK(ms_score(keys.data(), vox.data(), n, &cam, depth.data(), scaled.data(), 1, nullptr, &cost, nullptr, nullptr) == 2);
  }
  if (g_bad) { fprintf(stderr, "map_search_san: %d checks failed\n", g_bad); return 1; }
  printf("map_search_san ok\n");
  return 0;
}
