// march_scatter_emul.hip -- host emulation of the SCATTER (plane-major) order of k_conv_m's Winograd consumer (march_consumer_ws,
// tandem_amd/csrc/conv_march.h), run by tests/test_march_scatter.py on the CPU.  The companion of march_emul.hip, which covers the
// gather order: plan_conv builds the real launch (host-only arena), the producer's DMA pieces fill a ring image through the kernel's
// own index helpers, and the consumer's walk is replayed EVENT BY EVENT in the kernel's program order -- operand fetches one group
// ahead into the two alternating operand sets, the release, the three accumulator sets that move up by one plane after every
// plane, the epilogues -- with the kernel's own formulas for which set is which.
// Checked for every case, for rings of R = 2, 3 and 4 slots and for the planned grid as well as a grid of eight workgroups (long
// ranges that cross columns):
//   * every product (output plane, chunk of x taps, section dz) is issued exactly once, and per output plane in the gather order
//     (dz ascending, chunk ascending), so that every accumulator sees the same fmaf chain;
//   * a ring slot is never read after its release or while it holds another load, a load never overwrites a slot still in use,
//     the consumer never waits for a load the producers could not have issued, and the weights of a channel pass are not read
//     once the pass's last load is released (the producers overwrite them then);
//   * the result equals a direct convolution.
// What this does not cover is the timing side of the protocol on real hardware: tests/test_conv_march_scatter_gpu.py.
// A stand-alone program: its host code also builds and runs clean with -Xarch_host -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <map>
#include <random>

#include "../../tandem_amd/csrc/conv_mfma.h"

namespace dr {
std::string &last_error_slot() {
  static std::string s;
  return s;
}
}  // namespace dr
using namespace dr;

struct F4 { float v[4]; };
#define EMUL_FAIL(...) do { printf("emul: " __VA_ARGS__); printf("\n"); return false; } while (0)

template <int CI>
static bool emulate(const ConvLaunch &c, int R, int grid_x, const float *in, float *out, const float *add, int &za_mid, int &two_cols) {
  const ConvArgs &a = c.args;
  const MarchArgs &m = c.march;
  const int NUP = c.nup, CT = c.ct, PT = c.pt, TPC = 16 / CI, NRP = NUP / 3, NG = 3 * NRP, WSEC = NUP * CT * 64;
  if (m.geo.KZ != 3 || m.geo.NPI != 1 || !m.wino || NUP % 3 || NRP < 2) EMUL_FAIL("not a 3-D Winograd marching plan");
  if (m.wsec != WSEC) EMUL_FAIL("m.wsec %d is not NUP * CT * 64 = %d", m.wsec, WSEC);
  const int Dc = m.geo.Dc, NW = m.ncw;
  const size_t lanes = (size_t)NW * 64;  // every consumer wave in lock step
  for (unsigned bz = 0; bz < c.grid.z; ++bz) {
    const int ct0 = (int)bz * CT;
    for (int b = 0; b < grid_x; ++b) {
      const int nwg = grid_x, id = (b & 7) * (nwg >> 3) + (b >> 3);
      int s0, s1;
      march_range(m.steps, id, nwg, s0, s1);
      if (s0 >= s1) continue;
      std::vector<F4> ring((size_t)R * m.PS), wl((size_t)3 * WSEC);
      std::vector<int> owner(R, -1);  // load held by each slot
      // operand sets and accumulator sets, indexed as the kernel indexes them
      std::vector<F4> dd[2], gg[2];
      for (int k = 0; k < 2; ++k) { dd[k].assign(lanes * 4 * PT, F4{}); gg[k].assign(lanes * 3 * CT, F4{}); }
      std::vector<float> acc[3];
      for (auto &s : acc) s.assign((size_t)4 * lanes * CT * PT * 4, 0.f);
      auto acc_at = [&](int set, int pp, int wave, int ct, int pt, int lane, int e) -> float & {
        return acc[set][((((size_t)pp * NW + wave) * CT + ct) * PT + pt) * 256 + (size_t)lane * 4 + e];
      };
      int loaded = 0, released = 0, idx = 0;
      for (int po = 0; po < m.NPO; ++po) {
        if (released != idx) EMUL_FAIL("pass %d starts with %d of %d loads released", po, released, idx);
        for (int e = 0; e < 3 * NUP * CT; ++e)
          for (int lane = 0; lane < 64; ++lane) {
            const float4 w = a.wpk[march_weight_src(a, m, po, e, NUP, CT, ct0) + lane];
            wl[(size_t)e * 64 + lane] = F4{{w.x, w.y, w.z, w.w}};
          }
        struct Load { int zc, plane, iy0, ix0; };
        std::vector<Load> loads;
        for (int s = s0; s < s1;) {
          const MarchSeg sg = march_segment(m.geo, s, s1);
          int zc, py0, px0;
          march_tile_origin(a, m, sg.col, zc, py0, px0);
          for (int l = 0; l < sg.nl; ++l) {
            int plane, pi;
            march_load_plane(m.geo, sg, l, plane, pi);
            loads.push_back({zc, plane, py0 * a.sy - a.py, px0 * a.sx - a.px});
          }
          s += sg.zb - sg.za;
        }
        const int Lpass = idx, Lend = idx + (int)loads.size();
        auto do_load = [&](int i) -> bool {
          if (i >= R && released < i - R + 1) EMUL_FAIL("load %d would overwrite a slot still in use (released %d, R %d)", i, released, R);
          const Load &ld = loads[i - Lpass];
          const long long pofs = march_plane_offset(a, m, ld.zc, ld.plane, ld.iy0, ld.ix0, po, CI);
          for (int pw = 0; pw < kMarchProducers; ++pw)
            for (int it = 0; it < m.nit; ++it)
              for (int lane = 0; lane < 64; ++lane) {
                int rel; unsigned yx;
                march_piece_entry<CI>(a, m, pw, it, lane, rel, yx);
                F4 v{{0.f, 0.f, 0.f, 0.f}};
                if (march_piece_inside(a, m, yx, ld.iy0, ld.ix0)) for (int k = 0; k < 4; ++k) v.v[k] = in[pofs + rel + k];
                if ((it * kMarchProducers + pw) * 64 + lane >= m.PS) EMUL_FAIL("DMA piece outside its ring slot");
                ring[(size_t)(i % R) * m.PS + (size_t)(it * kMarchProducers + pw) * 64 + lane] = v;
              }
          owner[i % R] = i;
          return true;
        };
        // march_wait_ready: the producers issue in order and only into slots every reader has released
        auto wait_ready = [&](int i) -> bool {
          if (i >= Lend) EMUL_FAIL("the consumer waits for load %d beyond the producers' list of this pass", i);
          while (loaded <= i) { if (!do_load(loaded)) return false; ++loaded; }
          return true;
        };
        auto load_g = [&](int sec, int r, std::vector<F4> &o) -> bool {
          if (released >= Lend) EMUL_FAIL("weights read after the last load of the pass was released");
          for (int wave = 0; wave < NW; ++wave)
            for (int lane = 0; lane < 64; ++lane)
              for (int k = 0; k < 3; ++k)
                for (int ct = 0; ct < CT; ++ct) o[(((size_t)wave * 64 + lane) * 3 + k) * CT + ct] = wl[(size_t)sec * WSEC + (size_t)((r * 3 + k) * CT + ct) * 64 + lane];
          return true;
        };
        auto load_d = [&](int li, int r, std::vector<F4> &o) -> bool {
          if (li < released) EMUL_FAIL("load %d is read after its release", li);
          if (li >= loaded || owner[li % R] != li) EMUL_FAIL("load %d is read out of a slot that holds load %d", li, owner[li % R]);
          for (int wave = 0; wave < NW; ++wave)
            for (int lane = 0; lane < 64; ++lane) {
              const int j = lane & 15, g = lane >> 4, sub = (4 * g) / CI, c4 = ((4 * g) % CI) / 4;
              for (int pt = 0; pt < PT; ++pt)
                for (int q = 0; q < 4; ++q) {
                  const int slot = conv_a_unit<CI>(march_bpos(a, wave, pt, PT, j) + m.tap2d[r * TPC + sub] + q * a.TXI, c4);
                  if (slot < 0 || slot >= m.PS) EMUL_FAIL("operand slot %d outside the plane (%d slots)", slot, m.PS);
                  o[(((size_t)wave * 64 + lane) * 4 + q) * PT + pt] = ring[(size_t)(li % R) * m.PS + slot];
                }
            }
          return true;
        };
        const int raw = m.NPO == 1 ? 0 : (po == 0 ? 1 : 2);
        for (int s = s0; s < s1;) {
          const MarchSeg sg = march_segment(m.geo, s, s1);
          if (sg.za > 0) ++za_mid;
          if (s > s0) ++two_cols;
          int zc, py0, px0;
          march_tile_origin(a, m, sg.col, zc, py0, px0);
          std::map<int, int> last_key, count;  // per output plane of the segment: last product issued (dz * NRP + r), products issued
          for (int i = 0; i < sg.nl; ++i, ++idx) {
            const int p = sg.p0 + i;
            if (loads[idx - Lpass].plane != p) EMUL_FAIL("walk and producer disagree on load %d", idx);
            const bool more = i + 1 < sg.nl || s + (sg.zb - sg.za) < s1;
            if (more != (idx + 1 < Lend)) EMUL_FAIL("`more` disagrees with the load list at load %d", idx);
            const bool on[3] = {march_plane_feeds(sg, p, 0), march_plane_feeds(sg, p, 1), march_plane_feeds(sg, p, 2)};
            if (!wait_ready(idx) || !load_g(0, 0, gg[0]) || !load_d(idx, 0, dd[0])) return false;
            for (int r = 0; r < NRP; ++r)
              for (int dz = 0; dz < 3; ++dz) {
                const int t = r * 3 + dz;
                std::vector<F4> &gn = gg[(t + 1) & 1], &dn = dd[(r + 1) & 1], &gc = gg[t & 1], &dc = dd[r & 1];
                if (t + 1 < NG) {
                  if (!load_g((dz + 1) % 3, dz == 2 ? r + 1 : r, gn)) return false;
                  if (dz == 2 && !load_d(idx, r + 1, dn)) return false;
                }
                if (dz == 0)  // input transform, in place, once per chunk
                  for (size_t wl_ = 0; wl_ < lanes; ++wl_)
                    for (int pt = 0; pt < PT; ++pt) {
                      F4 *d[4];
                      for (int q = 0; q < 4; ++q) d[q] = &dc[(wl_ * 4 + q) * PT + pt];
                      for (int e = 0; e < 4; ++e) {
                        const float d0 = d[0]->v[e], d1 = d[1]->v[e], d2 = d[2]->v[e], d3 = d[3]->v[e];
                        d[0]->v[e] = d0 - d2; d[3]->v[e] = d1 - d3; d[1]->v[e] = d1 + d2; d[2]->v[e] = d2 - d1;
                      }
                    }
                if (on[dz]) {
                  const int zo = p + 1 - dz, key = dz * NRP + r, set = 2 - dz;
                  if (zo - 1 + dz != p || march_section_load(m.geo, sg, zo, dz) != i) EMUL_FAIL("plane %d section %d is not what step %d reads", p, dz, zo);
                  if (last_key.count(zo) && last_key[zo] >= key) EMUL_FAIL("output plane %d: product (dz %d, chunk %d) out of the gather order", zo, dz, r);
                  last_key[zo] = key; ++count[zo];
                  for (int wave = 0; wave < NW; ++wave)
                    for (int ct = 0; ct < CT; ++ct)
                      for (int pt = 0; pt < PT; ++pt) {
                        F4 u[4][64], v[4][64];
                        for (int lane = 0; lane < 64; ++lane) {
                          const size_t wl_ = (size_t)wave * 64 + lane;
                          const F4 &g0 = gc[(wl_ * 3 + 0) * CT + ct], &gh = gc[(wl_ * 3 + 1) * CT + ct], &g2 = gc[(wl_ * 3 + 2) * CT + ct];
                          for (int e = 0; e < 4; ++e) {
                            u[0][lane].v[e] = g0.v[e]; u[3][lane].v[e] = g2.v[e];
                            u[1][lane].v[e] = march_w_u1(g0.v[e], gh.v[e], g2.v[e]);
                            u[2][lane].v[e] = march_w_u2(g0.v[e], gh.v[e], g2.v[e]);
                          }
                          for (int q = 0; q < 4; ++q) v[q][lane] = dc[(wl_ * 4 + q) * PT + pt];
                        }
                        for (int pp = 0; pp < 4; ++pp)
                          for (int col = 0; col < 16; ++col)
                            for (int row = 0; row < 16; ++row) {
                              float &dst = acc_at(set, pp, wave, ct, pt, (row >> 2) * 16 + col, row & 3);
                              for (int sidx = 0; sidx < 4; ++sidx)
                                for (int g = 0; g < 4; ++g) dst = std::fmaf(u[pp][g * 16 + row].v[sidx], v[pp][g * 16 + col].v[sidx], dst);
                            }
                      }
                }
                if (more ? (r == NRP - 2 && dz == 2) : t == NG - 2) {
                  if (idx + 1 <= released) EMUL_FAIL("release counter would not advance at load %d", idx);
                  released = idx + 1;
                }
              }
            if (released != idx + 1) EMUL_FAIL("load %d was not released by the end of its plane", idx);
            int lo, hi;
            march_plane_completes(m.geo, sg, p, lo, hi);
            if ((on[2] ? 1 : 0) + ((on[1] && p == Dc - 1) ? 1 : 0) != hi - lo) EMUL_FAIL("epilogues after plane %d disagree with march_plane_completes", p);
            for (int zo = lo; zo < hi; ++zo) {
              const int set = zo == p - 1 ? 0 : 1;
              const int nsec = (zo > 0 ? 1 : 0) + 1 + (zo < Dc - 1 ? 1 : 0);
              if (count[zo] != nsec * NRP) EMUL_FAIL("output plane %d finished with %d of %d products", zo, count[zo], nsec * NRP);
              count[zo] = -1000000;  // finished: anything more is caught
              for (int wave = 0; wave < NW; ++wave)
                for (int pt = 0; pt < PT; ++pt)
                  for (int lane = 0; lane < 64; ++lane) {
                    const int j = lane & 15, g = lane >> 4;
                    const int tau = wave * PT + pt, xt = tau % a.TXT, yt = tau / a.TXT;
                    const int qy = py0 + yt, qx = px0 + xt * 16 + j;
                    if (qy >= a.nPH || qx >= a.nPW) continue;
                    for (int ct = 0; ct < CT; ++ct) {
                      const int c0 = (ct0 + ct) * 16 + 4 * g;
                      if (c0 >= a.rows_valid) continue;
                      for (int ro = 0; ro < 2; ++ro) {
                        const size_t ob = march_out_index(a, m, zc, zo, 2 * qy + ro, qx, c0);
                        for (int e = 0; e < 4; ++e) {
                          const float m0 = acc_at(set, 0, wave, ct, pt, lane, e), m1 = acc_at(set, 1, wave, ct, pt, lane, e), m2 = acc_at(set, 2, wave, ct, pt, lane, e),
                                      m3 = acc_at(set, 3, wave, ct, pt, lane, e);
                          float v = ro == 0 ? (m0 + m1) + m2 : (m1 - m2) - m3;
                          if (raw == 2) v += out[ob + e];
                          if (raw != 1) {
                            v = v * a.scale[c0 + e] + a.bias[c0 + e];
                            if (a.relu) v = std::max(v, 0.f);
                            if (a.add_mode == 1) v += add[ob + e];
                          }
                          out[ob + e] = v;
                        }
                      }
                    }
                  }
              std::fill(acc[set].begin(), acc[set].end(), 0.f);
            }
            acc[0].swap(acc[1]);  // the sets move up by one plane: 0 <- 1 <- 2 <- zeros
            acc[1].swap(acc[2]);
            std::fill(acc[2].begin(), acc[2].end(), 0.f);
          }
          for (int z = sg.za; z < sg.zb; ++z)
            if (count[z] >= 0) EMUL_FAIL("output plane %d of column %d never got its epilogue", z, sg.col);
          s += sg.zb - sg.za;
        }
        for (auto &sacc : acc)
          for (float v : sacc) if (v != 0.f) EMUL_FAIL("an accumulator set is not clear at the end of a pass");
        if (loaded != idx || released != idx || idx != Lend) EMUL_FAIL("pass %d ends with %d loaded / %d released of %d", po, loaded, released, Lend);
      }
    }
  }
  return true;
}

struct Case { const char *name; int D, H, W, Cin, Cout; bool relu, add; bool planned_only = false; };  // planned_only: the planner's ring and grid only (large cases)

static int run_case(const Case &cs, int max_plans, int &za_mid, int &two_cols) {
  std::mt19937 rng(4321);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  std::vector<float> in((size_t)cs.D * cs.H * cs.W * cs.Cin), w((size_t)cs.Cout * cs.Cin * 27), sc(cs.Cout), bi(cs.Cout);
  for (auto &v : in) v = U(rng);
  for (auto &v : w) v = U(rng) * 0.2f;
  for (auto &v : sc) v = 0.5f + 0.5f * std::fabs(U(rng));
  for (auto &v : bi) v = 0.3f * U(rng);
  const size_t on = (size_t)cs.D * cs.H * cs.W * cs.Cout;
  std::vector<float> add(on);
  for (auto &v : add) v = U(rng);
  std::vector<float> ref(on);  // direct convolution (torch Conv3d semantics, zero padding 1), channels-last
  for (int z = 0; z < cs.D; ++z) for (int y = 0; y < cs.H; ++y) for (int x = 0; x < cs.W; ++x) for (int co = 0; co < cs.Cout; ++co) {
    double s = 0;
    for (int tz = 0; tz < 3; ++tz) for (int ty = 0; ty < 3; ++ty) for (int tx = 0; tx < 3; ++tx) {
      const int iz = z + tz - 1, iy = y + ty - 1, ix = x + tx - 1;
      if (iz < 0 || iz >= cs.D || iy < 0 || iy >= cs.H || ix < 0 || ix >= cs.W) continue;
      for (int ci = 0; ci < cs.Cin; ++ci)
        s += (double)w[((((size_t)co * cs.Cin + ci) * 3 + tz) * 3 + ty) * 3 + tx] * in[(((size_t)iz * cs.H + iy) * cs.W + ix) * cs.Cin + ci];
    }
    double v = s * sc[co] + bi[co];
    if (cs.relu) v = std::max(v, 0.0);
    if (cs.add) v += add[(((size_t)z * cs.H + y) * cs.W + x) * cs.Cout + co];
    ref[(((size_t)z * cs.H + y) * cs.W + x) * cs.Cout + co] = (float)v;
  }
  ConvLayer L;
  L.Cin = cs.Cin; L.Cout = cs.Cout; L.kd = 3; L.kh = 3; L.kw = 3; L.weight = w.data(); L.scale = sc; L.bias = bi; L.relu = cs.relu;
  const ConvMode mode = cs.Cout == 8 ? CONV_XPAIR : CONV_NORMAL;
  int done = 0, fails = 0;
  for (int rank = 0; rank < 400 && done < max_plans; ++rank) {
    HostArena arena;
    std::vector<float> out(on);
    ConvPlanOut P = plan_conv(L, mode, in.data(), cs.D, cs.H, cs.W, cs.Cin, out.data(), cs.add ? add.data() : nullptr, 1, arena, rank);
    if (rank >= P.ncand) break;
    const ConvLaunch &c = P.launches.at(0);
    if (c.async != 2 || !c.march.wino) continue;
    ++done;
    int za_planned = 0, cross_planned = 0;
    for (int R = 2; R <= 4; ++R)
      for (int gi = 0; gi < 2; ++gi) {
        const int grid_x = gi ? 8 : (int)c.grid.x;
        if (gi && c.grid.x == 8) continue;
        if (cs.planned_only && (gi || R != c.march.R)) continue;
        const int za0 = za_mid, cr0 = two_cols;
        std::fill(out.begin(), out.end(), -777.f);
        const bool ok = c.ci == 8 ? emulate<8>(c, R, grid_x, in.data(), out.data(), add.data(), za_mid, two_cols)
                                  : emulate<16>(c, R, grid_x, in.data(), out.data(), add.data(), za_mid, two_cols);
        double worst = 0;
        for (size_t i = 0; i < on; ++i) worst = std::max(worst, (double)std::fabs(out[i] - ref[i]) / (1.0 + std::fabs(ref[i])));
        const bool pass = ok && worst < 2e-5;
        printf("%-16s plan scatter order %d ci=%d nup=%d ct=%d pt=%d tile %dx%d R=%d (planned %d) NPO=%d grid %dx%u steps %d Dc=%d: %s (max rel err %.2e)\n", cs.name, c.march.wino, c.ci,
               c.nup, c.ct, c.pt, c.args.TY, c.args.TXT * 16, R, c.march.R, c.march.NPO, grid_x, c.grid.z, c.march.steps, c.march.geo.Dc, pass ? "ok" : "FAIL", worst);
        if (!pass) ++fails;
        if (!gi && R == c.march.R) { za_planned = za_mid - za0; cross_planned = two_cols - cr0; }
      }
    printf("%-16s planned grid: %d segments start inside a column, %d ranges cross a column\n", cs.name, za_planned, cross_planned);
  }
  if (!done) { printf("%-16s no Winograd marching plan was produced\n", cs.name); return 1; }
  return fails;
}

int main(int argc, char **argv) {
  setenv("DR_CONV_MARCH", "2", 1);
  setenv("DR_CONV_WINO", "2", 1);  // the Winograd form of the 3-D march first in the planner's ranking
  // (this program is compiled with -DDR_PARITY_HOOKS, as the library the GPU test loads: layers smaller than half a tile get a marching plan, a depth of one keeps its three z taps)
  setenv("DR_MARCH_ANY_TILE", "1", 1);
  setenv("DR_CONV_NO_TAP_PRUNE", "1", 1);
  const int max_plans = argc > 1 ? atoi(argv[1]) : 2;
  const Case cases[] = {
      // (Cin, Cout, D, H, W) of tests/test_conv_march_scatter_gpu.py
      {"d1_c16", 1, 4, 16, 16, 8, true, false},        // D = 1: only dz = 1 exists
      {"d2_c16", 2, 4, 16, 16, 8, true, false},        // D = 2
      {"d3_c16_ragged", 3, 6, 40, 16, 8, true, false}, // partial x tile; three live sets exactly once
      {"c8", 8, 8, 32, 8, 8, true, false},             // the stage-3 instance (two chunks per plane)
      {"c32_two_passes", 5, 8, 32, 32, 8, true, false},// two channel passes through raw partial sums
      {"conv2_16_16", 4, 8, 32, 16, 16, true, false},  // the conv2 instance: three chunks per plane (six phases), no XPAIR
      {"conv2_add", 7, 12, 24, 16, 16, true, true},    // residual add, odd depth
      {"cols_c16", 5, 36, 70, 16, 8, true, false},     // several columns: ranges start inside a column and cross columns
      {"cols_c8", 3, 34, 66, 8, 8, false, false},
      {"cols_c32", 4, 18, 36, 32, 8, true, false},     // the same with two channel passes
      // the two grid cases of the GPU test: more steps than workgroups / fewer
      {"gpu_cross", 3, 96, 480, 16, 8, true, false, true},
      {"gpu_mid_column", 6, 16, 64, 16, 8, true, false, true},
  };
  int fails = 0, za_mid = 0, two_cols = 0;
  for (const Case &cs : cases) fails += run_case(cs, max_plans, za_mid, two_cols);
  printf("segments starting inside a column: %d, ranges crossing a column: %d\n", za_mid, two_cols);
  if (!za_mid || !two_cols) { printf("the cases never split a column / crossed one\n"); ++fails; }
  printf(fails ? "SCATTER MARCH EMULATION: %d FAILED\n" : "SCATTER MARCH EMULATION: all ok\n", fails);
  return fails ? 1 : 0;
}
