// tools/conv_plan_digest.cpp -- host tool: a digest of everything plan_conv produces, for comparing two versions of the planner bit for bit
// (profiles/conv_plan_refactor_ab.json was made with it).  For each case one line per rank 0 .. ncand (one past the end: the clamp), hashing every
// non-pointer field of the ConvLaunch (args, march, grid, lds_bytes, flops), outD/H/W, ncand, and the bytes of every uploaded array in upload
// order; an argument plan_conv refuses prints the error text instead.  Cases: every row of kConvTuned, the cases of tests/cpp/conv_emul.hip, the
// layers of tools/dump_plans.cpp, and one call each of the fused skip, a split input, both add modes, a bordered output and both up2 parities.
//   g++ -O2 -std=c++17 [-DDR_PARITY_HOOKS] tools/conv_plan_digest.cpp -o digest && ./digest > lines.txt     (the DR_* switches come from the environment)
//   ./digest time    plans every case at rank 0 twenty times and prints the milliseconds
// -DDIGEST_KERNEL_HEADER=\"path/conv_mfma.h\" (hipcc) builds it against a tree whose planner still lives in the kernel header; its arena then has to
// record upload sizes in a member `bytes` (and takes `host_only = true` where it has that flag: -DDIGEST_HOST_ONLY_FLAG).
#include <chrono>
#include <cstdio>
#include <random>

#ifdef DIGEST_KERNEL_HEADER
#include DIGEST_KERNEL_HEADER
#else
#include "../tandem_amd/csrc/conv_plan.h"
#endif
namespace dr { std::string &last_error_slot() { static std::string s; return s; } }
using namespace dr;

#ifdef DIGEST_HOST_ONLY_FLAG
struct Arena : DeviceArena { Arena() { host_only = true; } };
#else
typedef HostArena Arena;
#endif

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void *p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char *)p)[i]; h *= 1099511628211ull; } }
  template <class T> void v(const T &x) { bytes(&x, sizeof x); }
};

static uint64_t digest(const ConvPlanOut &P, const Arena &ar) {
  Fnv f;
  const ConvLaunch &c = P.launches.at(0);
  const ConvArgs &a = c.args;
  const int ai[] = {a.inD, a.inH, a.inW, a.inC, a.outD, a.outH, a.outW, a.outC, a.nPD, a.nPH, a.nPW, a.sz, a.sy, a.sx, a.pz, a.py, a.px, a.omz, a.omy, a.omx,
                    a.TZ, a.TY, a.TXT, a.TZI, a.TYI, a.TXI, a.npass, a.ctTot, a.rows_valid, a.relu, a.add_mode, a.addH, a.addW, a.par_rows, a.par_map,
                    (int)a.magicX, (int)a.magicY, a.nuMax, a.tilesD, a.tilesH, a.tilesW, a.pass_stride, a.a_slots, a.a_wbufs, a.class_loop,
                    a.fz_x != nullptr, a.zero16 != nullptr, a.add != nullptr};
  f.v(ai);
  const MarchArgs &m = c.march;
  const int mi[] = {m.geo.Dc, m.geo.KZ, m.geo.NPI, m.NPO, m.ncols, m.colsH, m.colsW, m.R, m.PS, m.NP, m.nit, m.wsec, m.NU, m.steps, m.ncw,
                    m.i_sv, m.i_sz, m.i_sy, m.o_sv, m.o_sz, m.o_sy, m.depth, m.inHp, m.rm, m.wino, m.tap2d != nullptr, m.err != nullptr};
  f.v(mi);
  const int li[] = {c.ci, c.ct, c.pt, c.fz, c.async, c.nup, c.ncw, c.bf3, (int)c.grid.x, (int)c.grid.y, (int)c.grid.z, P.outD, P.outH, P.outW, P.ncand, (int)P.launches.size()};
  f.v(li);
  f.v(c.lds_bytes);
  f.v(c.flops);
  for (size_t i = 0; i < ar.ptrs.size(); ++i) { f.v(ar.bytes[i]); f.bytes(ar.ptrs[i], ar.bytes[i]); }
  return f.h;
}

struct Call {
  std::string name;
  ConvLayer L;
  ConvMode mode = CONV_NORMAL;
  int D = 1, H = 1, W = 1, inC = 0;
  bool add = false;
  int add_mode = 1;
  bool fz = false;
  int fz_cin = 8, in_split = 0;
};
static std::vector<Call> g_calls;
static bool g_time = false;

static void run(const Call &q) {
  std::mt19937 rng(99);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  ConvLayer L = q.L;
  std::vector<float> w((size_t)std::max(1, L.Cin) * std::max(1, L.Cout) * L.kd * L.kh * L.kw);
  for (auto &v : w) v = U(rng);
  L.weight = w.data();
  L.scale.resize(std::max(1, L.Cout)); L.bias.resize(std::max(1, L.Cout));
  for (auto &v : L.scale) v = 0.5f + 0.5f * std::fabs(U(rng));
  for (auto &v : L.bias) v = 0.3f * U(rng);
  float in = 0.f, out = 0.f, addv = 0.f, fzv[4] = {0.f, 0.f, 0.f, 0.f};  // plan_conv only reads the tensors' addresses
  int err_flag = 0;
  const ConvFuse fuse{&fzv[0], &fzv[1], &fzv[2], &fzv[3], q.fz_cin};
  for (int rank = 0, ncand = 0; rank <= ncand; ++rank) {
    try {
      Arena ar;
      ar.err_flag = &err_flag;
      const ConvPlanOut P = plan_conv(L, q.mode, &in, q.D, q.H, q.W, q.inC ? q.inC : L.Cin, &out, q.add ? &addv : nullptr, q.add_mode, ar, rank, q.fz ? &fuse : nullptr, q.in_split);
      ncand = P.ncand;
      if (g_time) return;
      const ConvLaunch &c = P.launches.at(0);
      printf("%s rank %d/%d: ci=%d ct=%d pt=%d tile %dx%dx%d async=%d rm=%d wino=%d grid %ux%ux%u lds %zu uploads %zu  %016llx\n", q.name.c_str(), rank, ncand, c.ci, c.ct, c.pt,
             c.args.TZ, c.args.TY, c.args.TXT, c.async, c.march.rm, c.march.wino, c.grid.x, c.grid.y, c.grid.z, c.lds_bytes, ar.ptrs.size(), (unsigned long long)digest(P, ar));
    } catch (const Error &e) {
      if (!g_time) printf("%s rank %d: refused (%d): %s\n", q.name.c_str(), rank, e.code, e.what());
      return;
    }
  }
}

static Call &call(const std::string &name, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, bool tr, ConvMode mode) {
  Call q;
  q.name = name; q.D = D; q.H = H; q.W = W; q.mode = mode;
  q.L.Cin = Cin; q.L.Cout = Cout; q.L.kd = kd; q.L.kh = kh; q.L.kw = kw; q.L.sd = sd; q.L.sh = sh; q.L.sw = sw; q.L.transposed = tr;
  g_calls.push_back(q);
  return g_calls.back();
}

int main(int argc, char **argv) {
  g_time = argc > 1 && !strcmp(argv[1], "time");
  // ---- every row of the tuned table ----
  int row = 0;
  for (const ConvTuned &t : kConvTuned) {
    if (t.Cin == 0) continue;
    char n[64];
    snprintf(n, sizeof n, "tuned%02d", row++);
    Call &q = call(n, t.inD, t.inH, t.inW, t.Cin, t.Cout, t.kd, t.kh, t.kw, t.sd, t.sh, t.sw, t.transposed == 1, (ConvMode)(t.mode & 7));
    q.L.up2 = t.transposed >= 2 ? t.transposed - 1 : 0;
    q.fz = (t.mode & 8) != 0;
    q.in_split = (t.mode & 16) ? 16 : 0;
  }
  // ---- the cases of tests/cpp/conv_emul.hip ----
  struct Emul { const char *name; int kind, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw; bool relu; int add; };
  const Emul emul[] = {
      {"conv2d_5x5_s2_8_16", 0, 2, 13, 22, 8, 16, 1, 5, 5, 1, 2, 2, true, 0},   {"conv2d_1x1_16_32_up2add", 0, 2, 8, 20, 16, 32, 1, 1, 1, 1, 1, 1, false, 2},
      {"xpair2d_4_8", 0, 2, 9, 36, 4, 8, 1, 3, 3, 1, 1, 1, true, 0},            {"conv3d_s2_8_16", 0, 6, 10, 20, 8, 16, 3, 3, 3, 2, 2, 2, true, 0},
      {"conv3d_s122_32_64", 0, 1, 6, 12, 32, 64, 3, 3, 3, 1, 2, 2, true, 0},    {"conv3d_64_64", 0, 3, 4, 6, 64, 64, 3, 3, 3, 1, 1, 1, true, 0},
      {"x8_prob_8_1", 0, 5, 6, 24, 8, 1, 3, 3, 3, 1, 1, 1, false, 0},           {"deconv_16_8_skip", 1, 3, 5, 9, 16, 8, 3, 3, 3, 2, 2, 2, true, 1},
      {"deconv_32_16_skip", 1, 3, 4, 10, 32, 16, 3, 3, 3, 2, 2, 2, true, 1},    {"deconv_64_32_s122", 1, 1, 4, 6, 64, 32, 3, 3, 3, 1, 2, 2, true, 1},
      {"up2_32_8_inplace_add", 2, 2, 7, 19, 32, 8, 1, 3, 3, 1, 1, 1, false, 1}, {"up2_16_16", 2, 1, 5, 33, 16, 16, 1, 3, 3, 1, 1, 1, true, 0},
      {"conv2d_3x3_16_16", 0, 2, 24, 48, 16, 16, 1, 3, 3, 1, 1, 1, true, 0},    {"conv2d_3x3_32_16", 0, 2, 16, 40, 32, 16, 1, 3, 3, 1, 1, 1, false, 0},
      {"conv3d_16_16_skip", 0, 6, 12, 32, 16, 16, 3, 3, 3, 1, 1, 1, true, 1},   {"xpair3d_16_8", 0, 5, 10, 70, 16, 8, 3, 3, 3, 1, 1, 1, true, 0},
      {"xpair2d_8_8", 0, 2, 12, 36, 8, 8, 1, 3, 3, 1, 1, 1, true, 0},           {"conv2d_3x3_32_32_up2add", 0, 2, 8, 24, 32, 32, 1, 3, 3, 1, 1, 1, false, 2},
      {"conv3d_32_32", 0, 4, 6, 20, 32, 32, 3, 3, 3, 1, 1, 1, true, 0},         {"xpair3d_32_8", 0, 4, 8, 40, 32, 8, 3, 3, 3, 1, 1, 1, true, 0},
      {"conv3d_64_64_D1", 0, 1, 6, 10, 64, 64, 3, 3, 3, 1, 1, 1, true, 0},      {"conv3d_s2_32_64_D2", 0, 2, 8, 12, 32, 64, 3, 3, 3, 2, 2, 2, true, 0},
      {"conv3d_32_32_D2", 0, 2, 6, 20, 32, 32, 3, 3, 3, 1, 1, 1, true, 0},      {"deconv_64_32_D1", 1, 1, 4, 6, 64, 32, 3, 3, 3, 2, 2, 2, true, 1},
  };
  for (const Emul &e : emul)
    for (int py = 0; py < (e.kind == 2 ? 2 : 1); ++py) {
      const ConvMode mode = (e.kind == 0 && e.sw == 1 && e.Cout == 8) ? CONV_XPAIR : ((e.kind == 0 && e.sw == 1 && e.Cout == 1) ? CONV_X8 : CONV_NORMAL);
      Call &q = call(std::string("emul.") + e.name + (e.kind == 2 ? (py ? ".py1" : ".py0") : ""), e.D, e.H, e.W, e.Cin, e.Cout, e.kd, e.kh, e.kw, e.sd, e.sh, e.sw, e.kind == 1, mode);
      q.L.up2 = e.kind == 2 ? 1 + py : 0; q.L.relu = e.relu; q.add = e.add != 0; q.add_mode = e.add == 2 ? 2 : 1;
    }
  // ---- the layers of tools/dump_plans.cpp ----
  const int Ds[3] = {48, 32, 8}, hs[3] = {120, 240, 480}, ws[3] = {160, 320, 640}, Cs[3] = {32, 16, 8};
  for (int s = 0; s < 3; ++s) {
    const int D = Ds[s], h = hs[s], w = ws[s];
    const std::string p = "dump.s" + std::to_string(s + 1) + ".";
    call(p + "conv0", D, h, w, Cs[s], 8, 3, 3, 3, 1, 1, 1, false, CONV_XPAIR);
    call(p + "conv1", D, h, w, 8, 16, 3, 3, 3, 2, 2, 2, false, CONV_NORMAL);
    call(p + "conv2", D / 2, h / 2, w / 2, 16, 16, 3, 3, 3, 1, 1, 1, false, CONV_NORMAL);
    call(p + "conv3", D / 2, h / 2, w / 2, 16, 32, 3, 3, 3, 2, 2, 2, false, CONV_NORMAL);
    call(p + "conv4", D / 4, h / 4, w / 4, 32, 32, 3, 3, 3, 1, 1, 1, false, CONV_NORMAL);
    call(p + "conv5", D / 4, h / 4, w / 4, 32, 64, 3, 3, 3, 2, 2, 2, false, CONV_NORMAL);
    call(p + "conv6", D / 8, h / 8, w / 8, 64, 64, 3, 3, 3, 1, 1, 1, false, CONV_NORMAL);
    call(p + "conv7", D / 8, h / 8, w / 8, 64, 32, 3, 3, 3, 2, 2, 2, true, CONV_NORMAL);
    call(p + "conv9", D / 4, h / 4, w / 4, 32, 16, 3, 3, 3, 2, 2, 2, true, CONV_NORMAL);
    call(p + "conv11", D / 2, h / 2, w / 2, 16, 8, 3, 3, 3, 2, 2, 2, true, CONV_NORMAL);
  }
  // ---- one call each of what the above leave out ----
  call("x.fz_head_32_8", 3, 64, 96, 32, 8, 1, 3, 3, 1, 1, 1, false, CONV_XPAIR).fz = true;
  call("x.split16_32_8", 12, 30, 64, 32, 8, 3, 3, 3, 1, 1, 1, false, CONV_XPAIR).in_split = 16;
  call("x.split16_32_32", 6, 16, 40, 32, 32, 3, 3, 3, 1, 1, 1, false, CONV_NORMAL).in_split = 16;
  call("x.add1_16_16", 4, 16, 48, 16, 16, 3, 3, 3, 1, 1, 1, false, CONV_NORMAL).add = true;
  { Call &q = call("x.add2_16_32", 3, 16, 40, 16, 32, 1, 1, 1, 1, 1, 1, false, CONV_NORMAL); q.add = true; q.add_mode = 2; }
  call("x.outpad1_xpair_8_8", 3, 32, 64, 8, 8, 1, 3, 3, 1, 1, 1, false, CONV_XPAIR).L.out_pad = 1;
  call("x.outpad2_16_16", 3, 32, 64, 16, 16, 1, 3, 3, 1, 1, 1, false, CONV_NORMAL).L.out_pad = 2;
  call("x.up2_py0_32_8", 3, 30, 40, 32, 8, 1, 3, 3, 1, 1, 1, false, CONV_NORMAL).L.up2 = 1;
  call("x.up2_py1_32_8", 3, 30, 40, 32, 8, 1, 3, 3, 1, 1, 1, false, CONV_NORMAL).L.up2 = 2;
  call("x.inC_wider_16_16", 2, 20, 40, 16, 16, 1, 3, 3, 1, 1, 1, false, CONV_NORMAL).inC = 32;
  // ---- arguments plan_conv refuses ----
  call("no.cin6", 2, 8, 16, 6, 16, 1, 3, 3, 1, 1, 1, false, CONV_NORMAL);
  call("no.inC_narrow", 2, 8, 16, 16, 16, 1, 3, 3, 1, 1, 1, false, CONV_NORMAL).inC = 8;
  call("no.cout6", 2, 8, 16, 8, 6, 1, 3, 3, 1, 1, 1, false, CONV_NORMAL);
  call("no.up2_3", 2, 8, 16, 8, 8, 1, 3, 3, 1, 1, 1, false, CONV_NORMAL).L.up2 = 3;
  call("no.up2_3d", 2, 8, 16, 8, 8, 3, 3, 3, 1, 1, 1, false, CONV_NORMAL).L.up2 = 1;
  call("no.up2_xpair", 2, 8, 16, 8, 8, 1, 3, 3, 1, 1, 1, false, CONV_XPAIR).L.up2 = 1;
  call("no.xpair_cout16", 2, 8, 16, 8, 16, 1, 3, 3, 1, 1, 1, false, CONV_XPAIR);
  call("no.xpair_oddW", 2, 8, 15, 8, 8, 1, 3, 3, 1, 1, 1, false, CONV_XPAIR);
  call("no.xpair_strided", 2, 8, 16, 8, 8, 1, 3, 3, 1, 1, 2, false, CONV_XPAIR);
  call("no.x8_cout8", 2, 8, 16, 8, 8, 1, 3, 3, 1, 1, 1, false, CONV_X8);
  call("no.x8_W12", 2, 8, 12, 8, 1, 3, 3, 3, 1, 1, 1, false, CONV_X8);
  call("no.transposed_xpair", 2, 8, 16, 16, 8, 3, 3, 3, 2, 2, 2, true, CONV_XPAIR);
  call("no.transposed_x8", 2, 8, 16, 16, 1, 3, 3, 3, 2, 2, 2, true, CONV_X8);
  call("no.border_x8", 4, 8, 16, 8, 1, 3, 3, 3, 1, 1, 1, false, CONV_X8).L.out_pad = 1;
  call("no.split8", 4, 8, 16, 32, 8, 3, 3, 3, 1, 1, 1, false, CONV_XPAIR).in_split = 8;
  call("no.split16_cin8", 4, 8, 16, 8, 8, 3, 3, 3, 1, 1, 1, false, CONV_XPAIR).in_split = 16;
  { Call &q = call("no.split16_fz", 3, 16, 32, 32, 8, 1, 3, 3, 1, 1, 1, false, CONV_XPAIR); q.in_split = 16; q.fz = true; }
  call("no.fz_strided", 3, 16, 32, 32, 16, 1, 3, 3, 1, 2, 2, false, CONV_NORMAL).fz = true;
  { Call &q = call("no.fz_cin4", 3, 16, 32, 32, 8, 1, 3, 3, 1, 1, 1, false, CONV_XPAIR); q.fz = true; q.fz_cin = 4; }
  call("no.fz_transposed", 2, 8, 16, 32, 16, 3, 3, 3, 2, 2, 2, true, CONV_NORMAL).fz = true;

  const auto t0 = std::chrono::steady_clock::now();
  for (int rep = 0; rep < (g_time ? 20 : 1); ++rep)
    for (const Call &q : g_calls) run(q);
  if (g_time) printf("%.2f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return 0;
}
