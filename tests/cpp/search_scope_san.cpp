// The search-scope rule of tandem_amd/csrc/fusion_host.h and engine_host.h under AddressSanitizer and UBSan: a plain executable,
// nothing preloaded, nothing loaded into Python (tests/test_search_scope.py builds and runs it).  It reads the inputs of that test's
// plans from a file -- the keys of the store, the options, a lattice with its capacity, a plain table with its capacity -- runs
// plan_search_stage over both, checks the shape of each plan and that every pass holds the plain selection of each of its
// candidates, and prints per plan its passes as first:count:keys, which the test holds to the plans it made itself.
//   search_scope_san CASE
#include <cstdio>

#include "search_scope_check.cpp"

template <class T>
static bool get(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

static int run(const char *name, const HostBlockStore &store, const drf_options_t &o, const std::vector<double> &table, const SearchLattice &L, size_t n,
               size_t capacity) {
  const SearchStagePlan p = plan_search_stage(store, o, table.data(), L, n, capacity);
  if (!p.ok) { printf("%s: the plan failed with %zu\n", name, p.too_many); return 1; }
  printf("%s", name);
  size_t at = 0;
  for (const SearchStagePass &pass : p.passes) {
    if (pass.first != at || pass.count == 0 || pass.keys.size() > capacity) { printf("\n%s: a pass out of place or above the capacity\n", name); return 1; }
    for (size_t i = 1; i < pass.keys.size(); ++i)
      if (!(pass.keys[i - 1] < pass.keys[i])) { printf("\n%s: keys not ascending\n", name); return 1; }
    for (size_t c = pass.first; c < pass.first + pass.count; ++c) {
      float p16[16];
      locate_pose16(search_candidate(L, table.data(), 0, c), o.voxel_size, p16);
      const std::vector<u64> mine = select_locate_blocks(store, o, p16);
      if (!std::includes(pass.keys.begin(), pass.keys.end(), mine.begin(), mine.end())) { printf("\n%s: candidate %zu selects a block its pass lacks\n", name, c); return 1; }
    }
    at += pass.count;
    printf(" %zu:%zu:%zu", pass.first, pass.count, pass.keys.size());
  }
  printf("\n");
  if (at != n) { printf("%s: the passes do not tile the candidates\n", name); return 1; }
  const SearchStagePlan none = plan_search_stage(HostBlockStore(), o, table.data(), L, n, capacity);
  if (!none.ok || none.passes.size() != 1 || none.passes[0].first != 0 || none.passes[0].count != n || !none.passes[0].keys.empty()) {
    printf("%s: an empty store is not one pass without keys\n", name);
    return 1;
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: search_scope_san CASE\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "search_scope_san: cannot open %s\n", argv[1]); return 2; }
  uint64_t nk = 0, na = 0, nr = 0, np = 0, cap_lattice = 0, cap_plain = 0;
  drf_options_t o;
  int half[3];
  float trans_step = 0.0f;
  bool ok = get(f, &nk, 1) && nk < (1u << 20);
  std::vector<u64> keys(ok ? nk : 0);
  ok = ok && get(f, keys.data(), keys.size()) && get(f, &o, 1) && get(f, &na, 1) && na > 0 && na < 100;
  std::vector<float> anchors(ok ? na * 16 : 0);
  ok = ok && get(f, anchors.data(), anchors.size()) && get(f, &nr, 1) && nr > 0 && nr < 100;
  std::vector<double> rot(ok ? nr * 9 : 0);
  ok = ok && get(f, rot.data(), rot.size()) && get(f, half, 3) && get(f, &trans_step, 1) && get(f, &cap_lattice, 1) && get(f, &np, 1) && np > 0 && np < 100000;
  std::vector<float> poses(ok ? np * 16 : 0);
  ok = ok && get(f, poses.data(), poses.size()) && get(f, &cap_plain, 1);
  fclose(f);
  if (!ok) { fprintf(stderr, "search_scope_san: cannot read %s\n", argv[1]); return 2; }
  HostBlockStore store;
  fill(store, keys.data(), (int)keys.size());
  std::vector<double> table;
  if (!search_table(anchors.data(), na, rot.data(), nr, o.voxel_size, table).empty()) { printf("the table is refused\n"); return 1; }
  const SearchLattice L = lattice(half, (double)trans_step / (double)o.voxel_size, 0);
  if (run("lattice", store, o, table, L, search_count(na, nr, L), cap_lattice)) return 1;
  std::vector<double> plain(np * 12);
  ss_plain_table(poses.data(), np, o.voxel_size, plain.data());
  if (run("plain", store, o, plain, lattice(half, 0.0, 1), np, cap_plain)) return 1;
  printf("search_scope_san ok\n");
  return 0;
}
