// conv_plan_check.cpp -- walk over tandem_amd/csrc/conv_plan.h for tests/test_conv_plan_host.py: a g++ program (no HIP header, no device) that builds
// every rank of the planner's ranking for the small cases of tests/cpp/conv_emul.hip, one fused-skip, one split-input and two up2 calls, with and
// without the tuned swap, and holds every plan to what the kernels assume of it.  The same source is the sanitizer run: compiled with
// -fsanitize=address,undefined it is a stand-alone program with its own main (nothing is loaded into Python).
//   conv_plan_check [rows-rank0]     prints one line per case and "conv_plan_check ok"; exits 1 when a check fails
#include <cstdio>
#include <random>
#include <set>
#include <tuple>

#include "../../tandem_amd/csrc/conv_plan.h"

namespace dr { std::string &last_error_slot() { static std::string s; return s; } }
using namespace dr;

static int g_bad = 0;
static const char *g_case = "";
static int g_rank = 0;
#define CHECK(c) do { if (!(c)) { if (g_bad++ < 40) fprintf(stderr, "conv_plan_check: %s rank %d, line %d: %s\n", g_case, g_rank, __LINE__, #c); } } while (0)

struct Call {
  const char *name;
  int D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw;
  bool transposed;
  int up2;
  ConvMode mode;
  int add_mode;  // 0: no residual operand
  bool fz;
  int in_split;
};
typedef std::tuple<int, int, int, int, int, int, int> PlanKey;  // family, ci, ct, pt, tile

// what the kernels assume of one plan; returns its key
static PlanKey check_plan(const ConvPlanOut &P, const HostArena &ar, const ConvCand &cand) {
  const ConvLaunch &c = P.launches.at(0);
  const ConvArgs &a = c.args;
  const ConvFamily fam = conv_family(c);
  CHECK(fam == cand.family && c.ci == cand.ci && c.ct == cand.ct && c.pt == cand.pt && a.TZ == cand.tz && a.TY == cand.ty && a.TXT == cand.txt);
  CHECK(c.lds_bytes <= kConvMaxLds);
  const unsigned NP = (unsigned)a.TZI * a.TYI * a.TXI;
  CHECK(NP < 65536u);
  CHECK(c.grid.x % 8 == 0 && c.grid.x > 0 && c.grid.y > 0 && c.grid.z > 0);
  CHECK(conv_launch_instance_exists(c));
  bool exact = true;  // magicX and magicY divide every position of the halo tile exactly
  for (unsigned pos = 0; pos < NP && exact; ++pos) {
    const unsigned t = a.magicX ? (unsigned)(((uint64_t)pos * a.magicX) >> 32) : pos, z = a.magicY ? (unsigned)(((uint64_t)t * a.magicY) >> 32) : t;
    exact = t == pos / a.TXI && z == t / a.TYI;
  }
  CHECK(exact);
  // uploads, in order: packed weights, scale, bias, tap table, classes (then zero16 / the marching tap table)
  CHECK(ar.ptrs.size() >= 5 && ar.ptrs[0] == (const void *)a.wpk && ar.ptrs[3] == (const void *)a.tapoff && ar.ptrs[4] == (const void *)a.cls);
  const size_t n_w4 = ar.bytes[0] / 16, n_tap = ar.bytes[3] / 4, n_cls = ar.bytes[4] / sizeof(ConvClass);
  CHECK(n_cls == (a.class_loop > 0 ? (size_t)a.class_loop : (size_t)c.grid.y));
  CHECK(ar.bytes[1] == (size_t)a.ctTot * 16 * 4 && ar.bytes[2] == ar.bytes[1]);
  const int TPC = (c.bf3 ? 32 : 16) / c.ci, sub = fam == CONV_FAM_WINO ? 4 : (fam == CONV_FAM_WINOMARCH ? 3 : 1);
  // the last staged position any lane of the workgroup starts from (conv_tile_body's base[], k_conv_a's bpos[])
  const int base_max = (((a.TZ - 1) * a.sz) * a.TYI + (a.TY - 1) * a.sy) * a.TXI + (a.TXT * 16 - 1) * a.sx;
  const bool tiles = fam == CONV_FAM_TILE || fam == CONV_FAM_ASYNC || fam == CONV_FAM_WINO;
  int tap_end = 0, w_end = 0;
  for (size_t i = 0; i < n_cls; ++i) {
    const ConvClass &k = a.cls[i];
    CHECK(k.NU > 0 && k.NU <= a.nuMax && k.NU % sub == 0);
    CHECK(k.tap_base >= tap_end && k.w_base >= w_end && (i == 0 ? (k.tap_base == 0 && k.w_base == 0) : (k.tap_base > 0 && k.w_base > 0)));
    const int ntap = k.NU / sub * TPC;
    tap_end = k.tap_base + ntap;
    w_end = k.w_base + a.npass * k.NU * a.ctTot * 64 * (c.bf3 ? 2 : 1);
    CHECK((size_t)tap_end <= n_tap && (size_t)w_end <= n_w4);
    for (int t = 0; t < ntap && (size_t)tap_end <= n_tap; ++t) {
      const int off = a.tapoff[k.tap_base + t];
      CHECK(off >= 0 && (unsigned)off < NP);
      if (tiles) CHECK((unsigned)(base_max + off + (fam == CONV_FAM_WINO ? 3 * a.TXI : 0)) < NP);  // (k_conv_w adds rows 1..3 of the pair's window itself)
    }
  }
  if (c.async == 2) {  // k_conv_m: the in-plane tap table against the staged plane
    const MarchArgs &m = c.march;
    CHECK(ar.ptrs.size() == 7 && ar.ptrs[6] == (const void *)m.tap2d && ar.bytes[6] == (size_t)c.nup * TPC * 4);
    CHECK(m.NP < 65536 && m.NP == a.TYI * a.TXI && m.nit <= kMarchMaxIt && m.PS * 16 >= m.NP * c.ci * 4);
    CHECK((size_t)m.R * m.PS * 16 + (size_t)m.geo.KZ * m.geo.NPI * c.nup * c.ct * 1024 + kMarchFlagInts * 4 == c.lds_bytes);
    const int tau = c.ncw * c.pt - 1, bpos_max = (tau / a.TXT) * a.sy * a.TXI + ((tau % a.TXT) * 16 + 15) * a.sx;
    for (int t = 0; t < c.nup * TPC && ar.ptrs.size() == 7; ++t)
      CHECK(m.tap2d[t] >= 0 && bpos_max + m.tap2d[t] + (m.wino ? 3 * a.TXI : 0) < m.NP);
  }
  return PlanKey((int)fam, c.ci, c.ct, c.pt, a.TZ, a.TY, a.TXT);
}

// every rank of one call: the plans are pairwise different (the ranking is a permutation of the candidates) and each holds check_plan
static int walk(const Call &q, bool checks) {
  std::mt19937 rng(4321);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  std::vector<float> w((size_t)q.Cin * q.Cout * q.kd * q.kh * q.kw);
  for (auto &v : w) v = U(rng) * 0.2f;
  ConvLayer L;
  L.Cin = q.Cin; L.Cout = q.Cout; L.kd = q.kd; L.kh = q.kh; L.kw = q.kw; L.sd = q.sd; L.sh = q.sh; L.sw = q.sw;
  L.transposed = q.transposed; L.up2 = q.up2; L.weight = w.data(); L.relu = true;
  float in = 0.f, out = 0.f, add = 0.f, fzv = 0.f;  // plan_conv only reads the tensors' addresses
  const ConvFuse fuse{&fzv, &fzv, &fzv, &fzv, 8};
  // the ranking itself, by the planner's own steps
  ConvPlanner R(L, q.mode, &in, q.D, q.H, q.W, q.Cin, &out, q.add_mode ? &add : nullptr, q.add_mode, q.fz ? &fuse : nullptr, q.in_split);
  R.geometry();
  R.candidates();
  R.choose(0);
  std::set<PlanKey> seen;
  g_case = q.name;
  for (int rank = 0; rank < (int)R.cands.size(); ++rank) {
    g_rank = rank;
    HostArena ar;
    const ConvPlanOut P = plan_conv(L, q.mode, &in, q.D, q.H, q.W, q.Cin, &out, q.add_mode ? &add : nullptr, q.add_mode, ar, rank, q.fz ? &fuse : nullptr, q.in_split);
    CHECK(P.ncand == (int)R.cands.size());
    const ConvLaunch &c = P.launches.at(0);
    if (checks) seen.insert(check_plan(P, ar, R.cands[rank]));
    else {
      CHECK(conv_family(c) == R.cands[rank].family);
      seen.insert(PlanKey((int)conv_family(c), c.ci, c.ct, c.pt, c.args.TZ, c.args.TY, c.args.TXT));
    }
  }
  CHECK(seen.size() == R.cands.size());
  return (int)R.cands.size();
}

int main(int argc, char **argv) {
  const bool rows_rank0_only = argc > 1 && !strcmp(argv[1], "rows-rank0");  // (the sanitizer run: the tuned rows' layers at rank 0 only)
  const ConvMode N = CONV_NORMAL, XP = CONV_XPAIR, X8 = CONV_X8;
  const Call calls[] = {
      // the cases of tests/cpp/conv_emul.hip
      {"conv2d_5x5_s2_8_16", 2, 13, 22, 8, 16, 1, 5, 5, 1, 2, 2, false, 0, N, 0, false, 0},
      {"conv2d_1x1_16_32_up2add", 2, 8, 20, 16, 32, 1, 1, 1, 1, 1, 1, false, 0, N, 2, false, 0},
      {"xpair2d_4_8", 2, 9, 36, 4, 8, 1, 3, 3, 1, 1, 1, false, 0, XP, 0, false, 0},
      {"conv3d_s2_8_16", 6, 10, 20, 8, 16, 3, 3, 3, 2, 2, 2, false, 0, N, 0, false, 0},
      {"conv3d_s122_32_64", 1, 6, 12, 32, 64, 3, 3, 3, 1, 2, 2, false, 0, N, 0, false, 0},
      {"conv3d_64_64", 3, 4, 6, 64, 64, 3, 3, 3, 1, 1, 1, false, 0, N, 0, false, 0},
      {"x8_prob_8_1", 5, 6, 24, 8, 1, 3, 3, 3, 1, 1, 1, false, 0, X8, 0, false, 0},
      {"deconv_16_8_skip", 3, 5, 9, 16, 8, 3, 3, 3, 2, 2, 2, true, 0, N, 1, false, 0},
      {"deconv_32_16_skip", 3, 4, 10, 32, 16, 3, 3, 3, 2, 2, 2, true, 0, N, 1, false, 0},
      {"deconv_64_32_s122", 1, 4, 6, 64, 32, 3, 3, 3, 1, 2, 2, true, 0, N, 1, false, 0},
      {"up2_32_8_inplace_add.py0", 2, 7, 19, 32, 8, 1, 3, 3, 1, 1, 1, false, 1, N, 1, false, 0},
      {"up2_32_8_inplace_add.py1", 2, 7, 19, 32, 8, 1, 3, 3, 1, 1, 1, false, 2, N, 1, false, 0},
      {"up2_16_16.py0", 1, 5, 33, 16, 16, 1, 3, 3, 1, 1, 1, false, 1, N, 0, false, 0},
      {"conv2d_3x3_16_16", 2, 24, 48, 16, 16, 1, 3, 3, 1, 1, 1, false, 0, N, 0, false, 0},
      {"conv2d_3x3_32_16", 2, 16, 40, 32, 16, 1, 3, 3, 1, 1, 1, false, 0, N, 0, false, 0},
      {"conv3d_16_16_skip", 6, 12, 32, 16, 16, 3, 3, 3, 1, 1, 1, false, 0, N, 1, false, 0},
      {"xpair3d_16_8", 5, 10, 70, 16, 8, 3, 3, 3, 1, 1, 1, false, 0, XP, 0, false, 0},
      {"xpair2d_8_8", 2, 12, 36, 8, 8, 1, 3, 3, 1, 1, 1, false, 0, XP, 0, false, 0},
      {"conv2d_3x3_32_32_up2add", 2, 8, 24, 32, 32, 1, 3, 3, 1, 1, 1, false, 0, N, 2, false, 0},
      {"conv3d_32_32", 4, 6, 20, 32, 32, 3, 3, 3, 1, 1, 1, false, 0, N, 0, false, 0},
      {"xpair3d_32_8", 4, 8, 40, 32, 8, 3, 3, 3, 1, 1, 1, false, 0, XP, 0, false, 0},
      {"conv3d_64_64_D1", 1, 6, 10, 64, 64, 3, 3, 3, 1, 1, 1, false, 0, N, 0, false, 0},
      {"conv3d_s2_32_64_D2", 2, 8, 12, 32, 64, 3, 3, 3, 2, 2, 2, false, 0, N, 0, false, 0},
      {"conv3d_32_32_D2", 2, 6, 20, 32, 32, 3, 3, 3, 1, 1, 1, false, 0, N, 0, false, 0},
      {"deconv_64_32_D1", 1, 4, 6, 64, 32, 3, 3, 3, 2, 2, 2, true, 0, N, 1, false, 0},
      // the fused skip (the 32 -> 8 XPAIR head), a split input, and one more up2 call
      {"fz_head_32_8", 3, 16, 64, 32, 8, 1, 3, 3, 1, 1, 1, false, 0, XP, 0, true, 0},
      {"split16_xpair3d_32_8", 6, 12, 40, 32, 8, 3, 3, 3, 1, 1, 1, false, 0, XP, 0, false, 16},
      {"up2_16_8.py1", 2, 12, 40, 16, 8, 1, 3, 3, 1, 1, 1, false, 2, N, 0, false, 0},
  };
  int plans = 0;
  for (int tuned = 1; tuned >= 0; --tuned) {
    if (tuned) unsetenv("DR_CONV_NO_TUNED"); else setenv("DR_CONV_NO_TUNED", "1", 1);
    for (const Call &q : calls) {
      const int n = walk(q, true);
      plans += n;
      if (tuned) printf("%-28s %3d ranks\n", q.name, n);
    }
  }
  // every row of the tuned table: rank 0 is the row's plan, and with the swap (and without) the ranks stay a permutation
  int rows = 0;
  for (const ConvTuned &t : kConvTuned) {
    if (t.Cin == 0) continue;  // sentinel
    ++rows;
    char name[64];
    snprintf(name, sizeof name, "tuned row %d", rows);
    const Call q{name, t.inD, t.inH, t.inW, t.Cin, t.Cout, t.kd, t.kh, t.kw, t.sd, t.sh, t.sw, t.transposed == 1, t.transposed >= 2 ? t.transposed - 1 : 0, (ConvMode)(t.mode & 7), 0,
                 (t.mode & 8) != 0, (t.mode & 16) ? 16 : 0};
    for (int tuned = 1; tuned >= 0 && !rows_rank0_only; --tuned) {
      if (tuned) unsetenv("DR_CONV_NO_TUNED"); else setenv("DR_CONV_NO_TUNED", "1", 1);
      plans += walk(q, false);
    }
    unsetenv("DR_CONV_NO_TUNED");
    g_case = name; g_rank = 0;
    std::vector<float> w((size_t)t.Cin * t.Cout * t.kd * t.kh * t.kw, 0.01f);
    ConvLayer L;
    L.Cin = t.Cin; L.Cout = t.Cout; L.kd = t.kd; L.kh = t.kh; L.kw = t.kw; L.sd = t.sd; L.sh = t.sh; L.sw = t.sw; L.transposed = q.transposed; L.up2 = q.up2; L.weight = w.data();
    float in = 0.f, out = 0.f, fzv = 0.f;
    const ConvFuse fuse{&fzv, &fzv, &fzv, &fzv, 8};
    HostArena ar;
    const ConvLaunch c = plan_conv(L, q.mode, &in, q.D, q.H, q.W, q.Cin, &out, nullptr, 0, ar, 0, q.fz ? &fuse : nullptr, q.in_split).launches.at(0);
    CHECK((int)conv_family(c) == t.async_ && c.ci == t.ci && c.ct == t.ct && c.pt == t.pt && c.args.TZ == t.tz && c.args.TY == t.ty && c.args.TXT == t.txt);
  }
  printf("%d tuned rows, %d plans\n", rows, plans);
  if (g_bad) { fprintf(stderr, "conv_plan_check: %d checks failed\n", g_bad); return 1; }
  printf("conv_plan_check ok\n");
  return 0;
}
