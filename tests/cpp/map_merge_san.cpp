// Stand-alone run of the merge half of tandem_amd/csrc/fusion_host.h for a sanitizer build (tests/test_map_merge.py builds it
// with g++ -fsanitize=address,undefined and runs it): merge_voxel over every weight pair with seeded sdf and colours, merge_block
// on blocks that are all case 1, plan_merge on seeded key lists against std::set, through the entry points of
// map_merge_check.cpp.
//   map_merge_san      exits 0 when every check holds
#include <cstdio>
#include <random>
#include <set>

#include "map_merge_check.cpp"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad < 20) fprintf(stderr, "map_merge_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

static void voxels(int W, unsigned seed) {
  std::mt19937 rng(seed);
  const size_t n = 256 * 256 * 4;
  std::vector<unsigned char> a(8 * n), b(8 * n), cases(n);
  for (size_t i = 0; i < n; ++i) {
    const float sa = ((int)(rng() % 2001) - 1000) * 1e-4f, sb = ((int)(rng() % 2001) - 1000) * 1e-4f;
    memcpy(&a[8 * i], &sa, 4); memcpy(&b[8 * i], &sb, 4);
    for (int k = 4; k < 7; ++k) { a[8 * i + k] = (unsigned char)rng(); b[8 * i + k] = (unsigned char)rng(); }
    a[8 * i + 7] = (unsigned char)((i / 4) & 255); b[8 * i + 7] = (unsigned char)((i / 4) >> 8);
  }
  const std::vector<unsigned char> a0 = a;
  mm_merge_voxels(a.data(), b.data(), n, W, cases.data());
  for (size_t i = 0; i < n; ++i) {
    const unsigned char *o = &a[8 * i], *x = &a0[8 * i], *y = &b[8 * i];
    const int wa = x[7], wb = y[7];
    if (wb == 0) { CHECK(cases[i] == 1 && memcmp(o, x, 8) == 0); continue; }
    if (wa == 0) { CHECK(cases[i] == 2 && memcmp(o, y, 7) == 0 && o[7] == std::min(wb, W)); continue; }
    CHECK(cases[i] == 3 && o[7] == std::min(wa + wb, W));
    for (int k = 4; k < 7; ++k) CHECK(o[k] >= std::min(x[k], y[k]) && o[k] <= std::max(x[k], y[k]));
    float s, sa, sb;
    memcpy(&s, o, 4); memcpy(&sa, x, 4); memcpy(&sb, y, 4);
    CHECK(s >= std::min(sa, sb) - 1e-6f && s <= std::max(sa, sb) + 1e-6f);
  }
}

static void blocks_of_case_one() {
  std::mt19937 rng(5);
  std::vector<unsigned char> dst(3 * 4096), src(3 * 4096);
  for (auto &v : dst) v = (unsigned char)rng();
  for (auto &v : src) v = (unsigned char)rng();
  for (size_t v = 0; v < 3 * 512; ++v) src[8 * v + 7] = 0;
  const std::vector<unsigned char> before = dst;
  unsigned long long counts[2] = {0, 0};
  mm_merge_blocks(dst.data(), src.data(), 3, 64, counts);
  CHECK(dst == before && counts[0] == 0 && counts[1] == 0);
}

static void plan(size_t nres, size_t nsto, size_t nfile, size_t chunk, unsigned seed) {
  std::mt19937_64 rng(seed);
  auto draw = [&](size_t n, std::set<unsigned long long> &s, const std::set<unsigned long long> *avoid) {
    while (s.size() < n) {
      const unsigned long long k = dr::pack_biased((long)(rng() % 9) - 4, (long)(rng() % 9) - 4, (long)(rng() % 9) - 4);
      if (!avoid || !avoid->count(k)) s.insert(k);
    }
  };
  std::set<unsigned long long> sr, ss, sf;
  draw(nres, sr, nullptr); draw(nsto, ss, &sr); draw(nfile, sf, nullptr);
  const std::vector<unsigned long long> res(sr.begin(), sr.end()), sto(ss.begin(), ss.end()), file(sf.begin(), sf.end());
  std::vector<int> slot(nres);
  for (size_t i = 0; i < nres; ++i) slot[i] = (int)((i * 7 + 3) % std::max<size_t>(nres, 1));
  std::vector<int> r_src(nfile + 2), r_slot(nfile + 2), a_src(nfile + 2), s_src(nfile + 2);
  std::vector<unsigned long long> a_key(nfile + 2), s_key(nfile + 2), rb(nfile + 2), ab(nfile + 2), sb(nfile + 2);
  unsigned long long counts[3];
  const size_t nc = mm_plan(res.data(), slot.data(), nres, sto.data(), nsto, file.data(), nfile, chunk, r_src.data(), r_slot.data(), a_src.data(), a_key.data(),
                            s_src.data(), s_key.data(), rb.data(), ab.data(), sb.data(), counts);
  CHECK(nc == (nfile + chunk - 1) / chunk);
  CHECK(counts[0] + counts[1] + counts[2] == nfile);
  size_t r = 0, a = 0, s = 0;
  for (size_t f = 0; f < nfile; ++f) {
    const size_t c = f / chunk;
    const int at = (int)(f % chunk);
    if (sr.count(file[f])) {
      const size_t i = (size_t)std::distance(sr.begin(), sr.find(file[f]));
      CHECK(r >= rb[c] && r < rb[c + 1] && r_src[r] == at && r_slot[r] == slot[i]);
      ++r;
    } else if (ss.count(file[f])) {
      CHECK(s >= sb[c] && s < sb[c + 1] && s_src[s] == at && s_key[s] == file[f]);
      ++s;
    } else {
      CHECK(a >= ab[c] && a < ab[c + 1] && a_src[a] == at && a_key[a] == file[f]);
      ++a;
    }
  }
  CHECK(r == counts[0] && a == counts[1] && s == counts[2]);
}

int main() {
  for (int W : {1, 64, 255}) voxels(W, 100 + (unsigned)W);
  blocks_of_case_one();
  unsigned seed = 1;
  for (size_t chunk : {(size_t)1, (size_t)5, (size_t)1000})
    for (size_t nfile : {(size_t)0, (size_t)1, (size_t)37})
      for (size_t nres : {(size_t)0, (size_t)40})
        for (size_t nsto : {(size_t)0, (size_t)25}) plan(nres, nsto, nfile, chunk, seed++);
  if (g_bad) { fprintf(stderr, "map_merge_san: %d checks failed\n", g_bad); return 1; }
  printf("map_merge_san ok\n");
  return 0;
}
