// pose_host.h -- the pose solvers of DrFusion: the rule, step and host driver of a map-to-map registration (align), of a depth
// frame's localisation in the map (locate), of its tracking against the ray-cast model, without and with colour (track), and of the
// search that finds their start on a lattice of poses (search: the locate rule's cost without its Jacobian, at the file's end).  One
// Gauss-Newton system (align_accumulate), one step (align_step), one loop (align_loop), one walk over a frame's sample grid
// (frame_group) for all of them.  The DR_HOST_DEVICE functions are the text the kernels compile.  Plain C++17 over fusion_host.h,
// which includes this file at its end: whoever includes either has both (tests/cpp/map_align_check.cpp, map_locate_check.cpp,
// map_track_check.cpp, map_track_colour_check.cpp, map_track_exposure_check.cpp, map_search_check.cpp run it on the CPU).
#pragma once
#include <string>
#include <type_traits>

#include "fusion_host.h"

namespace dr {

// ---- registering two map files (drf_align_system / drf_align_map; DESIGN.md §7c "Registering two maps")
// T maps src-world to ref-world, p_ref = R p_src + t, held as a MapMotion in double: q = R g + tv takes a source lattice point to
// reference lattice units.  The cost is the sum over the source's samples of rho(r), r = (phi_ref(q) - s_src) / voxel_size, phi_ref
// the trilinear interpolation of the reference's sdf, rho Huber's function; one evaluation yields the Gauss-Newton system of it:
// sums[0..20] = the upper triangle of H = sum w J J^T row-major, sums[21..26] = b = sum w J r, sums[27] = sum w r r.
// The rule is stated once, here (the header of the C ABI restates it for users): align_voxel is compiled by g++ for the CPU tests
// and by hipcc for k_map_align, both without contraction, and uses + - * / and floor only.
#if defined(__HIPCC__)
#define DR_UNROLL _Pragma("unroll")
#else
#define DR_UNROLL
#endif
struct AlignOpt {  // drf_align_options_t with its defaults resolved
  int max_iters, min_weight;
  float band, huber;
  double eps_rot, eps_trans, min_valid;
};
// null: all defaults.  Returns null, or which option is negative or not finite
inline const char *align_options(const drf_align_options_t *opt, float voxel_size, AlignOpt &o) {
  static const drf_align_options_t zero = {0, 0, 0.0f, 0.0f, 0.0, 0.0, 0.0};
  const drf_align_options_t &u = opt ? *opt : zero;
  if (u.max_iters < 0) return "max_iters";
  if (u.min_weight < 0) return "min_weight";
  if (!(u.band >= 0.0f) || !std::isfinite(u.band)) return "band";
  if (!(u.huber >= 0.0f) || !std::isfinite(u.huber)) return "huber";
  if (!(u.eps_rot >= 0.0) || !std::isfinite(u.eps_rot)) return "eps_rot";
  if (!(u.eps_trans >= 0.0) || !std::isfinite(u.eps_trans)) return "eps_trans";
  if (!(u.min_valid >= 0.0) || !std::isfinite(u.min_valid)) return "min_valid";
  o.max_iters = u.max_iters ? u.max_iters : 30;
  o.min_weight = u.min_weight ? u.min_weight : 1;
  o.band = u.band != 0.0f ? u.band : 2.0f * voxel_size;
  o.huber = u.huber != 0.0f ? u.huber : 1.0f;
  o.eps_rot = u.eps_rot != 0.0 ? u.eps_rot : 1e-7;
  o.eps_trans = u.eps_trans != 0.0 ? u.eps_trans : 1e-5;
  o.min_valid = u.min_valid != 0.0 ? u.min_valid : 0.25;
  return nullptr;
}
// what a kernel launch and a host evaluation share besides the pose
struct AlignEval {
  MapMotion m;
  double c[3];        // the centre at this pose: R c_src + tv
  double huber, vs;   // (double)huber, (double)voxel_size
  float band;
  int min_weight;
};
// c_src[k] = 4 (min_k + max_k + 1) over the source's block coordinates: the middle of its lattice box, an integer (0 if empty)
inline void align_centre_src(const std::vector<unsigned long long> &src_keys, double c_src[3]) {
  c_src[0] = c_src[1] = c_src[2] = 0.0;
  if (src_keys.empty()) return;
  int lo[3] = {kKeyBias, kKeyBias, kKeyBias}, hi[3] = {-kKeyBias - 1, -kKeyBias - 1, -kKeyBias - 1};
  for (unsigned long long k : src_keys) {
    int c[3]; unpack_key_host(k, c);
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], c[a]); hi[a] = std::max(hi[a], c[a]); }
  }
  for (int a = 0; a < 3; ++a) c_src[a] = (double)(4L * ((long)lo[a] + (long)hi[a] + 1L));
}
inline AlignEval align_eval(const MapMotion &m, const double c_src[3], const AlignOpt &o, float voxel_size) {
  AlignEval e;
  e.m = m;
  for (int k = 0; k < 3; ++k) e.c[k] = ((m.R[3 * k] * c_src[0] + m.R[3 * k + 1] * c_src[1]) + m.R[3 * k + 2] * c_src[2]) + m.tv[k];
  e.huber = (double)o.huber; e.vs = (double)voxel_size;
  e.band = o.band; e.min_weight = o.min_weight;
  return e;
}
// is the source voxel (its two words) a sample?
DR_HOST_DEVICE inline bool align_is_sample(const uint32_t v[2], const AlignEval &e) {
  float s;
  memcpy(&s, &v[0], 4);
  return (int)(v[1] >> 24) >= e.min_weight && (s < 0.0f ? -s : s) <= e.band;
}
// The terms of one valid sample at q with residual r and gradient n (both in voxels): J = ((q - c) x n, n), Huber's weight, the 28
// sums.  What align_point and track_point (below) end in: the same operations in the same order for all three callers.
DR_HOST_DEVICE inline void align_accumulate(const AlignEval &e, double r, double n0, double n1, double n2, const double q[3], double acc[28]) {
  const double x0 = q[0] - e.c[0], x1 = q[1] - e.c[1], x2 = q[2] - e.c[2];
  const double J[6] = {x1 * n2 - x2 * n1, x2 * n0 - x0 * n2, x0 * n1 - x1 * n0, n0, n1, n2};
  const double a = r < 0.0 ? -r : r;
  const double w = a <= e.huber ? 1.0 : e.huber / a;
  int idx = 0;
  DR_UNROLL
  for (int i = 0; i < 6; ++i) {
    const double wj = w * J[i];
    DR_UNROLL
    for (int j = i; j < 6; ++j) { acc[idx] = acc[idx] + wj * J[j]; ++idx; }
    acc[21 + i] = acc[21 + i] + wj * r;
  }
  acc[27] = acc[27] + (w * r) * r;
}
// One sample at the point g (lattice units of the moving frame, three doubles) with sdf s_src: the body that the registration
// (align_voxel: g a source lattice point) and the localisation (frame_group: g a depth pixel's point, s_src = 0) share.  Reads the
// eight reference voxels through fetch(x, y, z, v[2]) (an absent block: weight 0); returns 0 if one of them is not observed (or q
// lies outside the key range), and otherwise adds the sample's terms to acc[28] and returns 1.  BAND (the localisation only): a
// sample whose eight corners are observed but whose fp32 |phi| < band is false adds nothing and returns 2 -- it lies in the flat
// region in front of the surface, where the gradient is zero.  The operations and their order are the rule; the header of the C
// ABI spells them out.
template <bool BAND, class Fetch>
DR_HOST_DEVICE inline int align_point(const AlignEval &e, double g0, double g1, double g2, float s_src, Fetch &&fetch, double acc[28]) {
  double q[3];
  int b[3];
  float f[3];
  DR_UNROLL
  for (int k = 0; k < 3; ++k) {
    q[k] = ((e.m.R[3 * k] * g0 + e.m.R[3 * k + 1] * g1) + e.m.R[3 * k + 2] * g2) + e.m.tv[k];
    if (!(q[k] > -1073741824.0 && q[k] < 1073741824.0)) return 0;
    const double fl = floor(q[k]);
    b[k] = (int)fl;
    f[k] = (float)(q[k] - fl);
  }
  float s[8];  // index 4 cx + 2 cy + cz
  DR_UNROLL
  for (int c = 0; c < 8; ++c) {
    uint32_t v[2];
    fetch(b[0] + (c >> 2), b[1] + ((c >> 1) & 1), b[2] + (c & 1), v);
    if ((int)(v[1] >> 24) < e.min_weight) return 0;
    memcpy(&s[c], &v[0], 4);
  }
  float h[4], ez[4];  // index 2 cx + cy
  DR_UNROLL
  for (int c = 0; c < 4; ++c) {
    h[c] = s[2 * c + 1] - s[2 * c];
    ez[c] = s[2 * c] + f[2] * h[c];
  }
  float dy[2], d[2], hy[2];
  DR_UNROLL
  for (int c = 0; c < 2; ++c) {
    dy[c] = ez[2 * c + 1] - ez[2 * c];
    d[c] = ez[2 * c] + f[1] * dy[c];
    hy[c] = h[2 * c] + f[1] * (h[2 * c + 1] - h[2 * c]);
  }
  const float gxf = d[1] - d[0];
  const float phi = d[0] + f[0] * gxf;
  const float gyf = dy[0] + f[0] * (dy[1] - dy[0]);
  const float gzf = hy[0] + f[0] * (hy[1] - hy[0]);
  if (BAND) {
    const float ap = phi < 0.0f ? -phi : phi;
    if (!(ap < e.band)) return 2;
  }
  const double r = ((double)phi - (double)s_src) / e.vs;
  const double n0 = (double)gxf / e.vs, n1 = (double)gyf / e.vs, n2 = (double)gzf / e.vs;
  align_accumulate(e, r, n0, n1, n2, q, acc);
  return 1;
}
// One sample of the registration: the source voxel at lattice point (gx, gy, gz) with sdf s_src; true if it was valid.
template <class Fetch>
DR_HOST_DEVICE inline bool align_voxel(const AlignEval &e, int gx, int gy, int gz, float s_src, Fetch &&fetch, double acc[28]) {
  return align_point<false>(e, (double)gx, (double)gy, (double)gz, s_src, fetch, acc) == 1;
}
// x[l] = x[l] + x[l ^ off] for off = 32, 16, 8, 4, 2, 1 over 64 lanes of S values (28; 45 with the exposure): afterwards every lane
// holds the same sum
template <int S>
inline void align_butterfly(double x[64][S]) {
  for (int off = 32; off > 0; off >>= 1) {
    double y[64][S];
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < S; ++i) y[l][i] = x[l][i] + x[l ^ off][i];
    memcpy(x, y, sizeof y);
  }
}
// One source block at block coordinates blk in the wave's order: lane l takes voxels 2 (l + 64 k) and the next, k = 0..3, then the
// butterfly.  out[28] = the block's sums; counts += {samples, valid, invalid}.
template <class Fetch>
inline void align_block(const AlignEval &e, const int blk[3], const uint8_t *src4096, Fetch &&ref, double out[28], uint64_t counts[3]) {
  double x[64][28];
  for (int l = 0; l < 64; ++l) {
    for (int i = 0; i < 28; ++i) x[l][i] = 0.0;
    for (int k = 0; k < 4; ++k)
      for (int t = 0; t < 2; ++t) {
        const int v = 2 * (l + 64 * k) + t;
        uint32_t w[2];
        memcpy(w, src4096 + 8 * v, 8);
        if (!align_is_sample(w, e)) continue;
        float s;
        memcpy(&s, &w[0], 4);
        ++counts[0];
        if (align_voxel(e, blk[0] * kBS + (v >> 6), blk[1] * kBS + ((v >> 3) & 7), blk[2] * kBS + (v & 7), s, ref, x[l])) ++counts[1];
        else ++counts[2];
      }
  }
  align_butterfly(x);
  for (int i = 0; i < 28; ++i) out[i] = x[0][i];
}
// k_align_fold (S = 45: k_exposure_fold) on the host: per component lane l adds partial[l], partial[l + 64], ... from +0.0 and the
// butterfly folds the lanes
template <int S = 28>
inline void align_fold_host(const double *partial, size_t n, double sums[S]) {
  double x[64][S];
  for (int l = 0; l < 64; ++l)
    for (int c = 0; c < S; ++c) {
      double a = 0.0;
      for (size_t i = (size_t)l; i < n; i += 64) a = a + partial[i * S + c];
      x[l][c] = a;
    }
  align_butterfly(x);
  for (int c = 0; c < S; ++c) sums[c] = x[0][c];
}
// The system at one pose over the whole source (keys ascending, n x 4096 bytes): align_block per block into partial[i], then
// per component lane l adds partial[l], partial[l + 64], ... from +0.0 and the butterfly folds the lanes.
template <class Fetch>
inline void align_system_host(const std::vector<unsigned long long> &src_keys, const uint8_t *src_vox, Fetch &&ref, const AlignEval &e, double sums[28],
                              uint64_t counts[3]) {
  counts[0] = counts[1] = counts[2] = 0;
  const size_t n = src_keys.size();
  std::vector<double> partial(n * 28);
  for (size_t i = 0; i < n; ++i) {
    int blk[3]; unpack_key_host(src_keys[i], blk);
    align_block(e, blk, src_vox + i * 4096, ref, &partial[i * 28], counts);
  }
  align_fold_host(partial.data(), n, sums);
}
// The Cholesky solve that every step shares, H d = -b for a symmetric N x N H (6; 8 with the exposure): the pivot test is
// p > 1e-12 top, top the largest diagonal entry.  Returns the index of the first pivot that fails it, or -1 with d solved.
template <int N>
inline int align_solve(const double H[N][N], const double b[N], double top, double d[N]) {
  double L[N][N] = {{0.0}}, y[N] = {0.0};
  for (int i = 0; i < N; ++i) d[i] = 0.0;
  for (int j = 0; j < N; ++j) {
    double p = H[j][j];
    for (int k = 0; k < j; ++k) p = p - L[j][k] * L[j][k];
    if (!(p > 1e-12 * top)) return j;
    L[j][j] = std::sqrt(p);
    for (int i = j + 1; i < N; ++i) {
      double t = H[i][j];
      for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  for (int i = 0; i < N; ++i) {
    double t = -b[i];
    for (int k = 0; k < i; ++k) t = t - L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
  for (int i = N - 1; i >= 0; --i) {
    double t = y[i];
    for (int k = i + 1; k < N; ++k) t = t - L[k][i] * d[k];
    d[i] = t / L[i][i];
  }
  return -1;
}
// the pose moved by the step d[0..5] (rotation vector about c, translation), oo = |d[0..2]|^2
inline void align_move(const double d[6], double oo, const double c[3], MapMotion &m) {
  const double a = 1.0 / std::sqrt(1.0 + oo / 4.0);
  const double qw = a, qx = (a * d[0]) / 2.0, qy = (a * d[1]) / 2.0, qz = (a * d[2]) / 2.0;
  const double Rq[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                        2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                        2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
  MapMotion o;
  const double e[3] = {m.tv[0] - c[0], m.tv[1] - c[1], m.tv[2] - c[2]};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o.R[3 * i + j] = (Rq[3 * i] * m.R[j] + Rq[3 * i + 1] * m.R[3 + j]) + Rq[3 * i + 2] * m.R[6 + j];
    o.tv[i] = (c[i] + ((Rq[3 * i] * e[0] + Rq[3 * i + 1] * e[1]) + Rq[3 * i + 2] * e[2])) + d[3 + i];
  }
  m = o;
}
// One Gauss-Newton step from the system sums at pose m (centre c = e.c of that evaluation).  Returns DRF_ALIGN_DEGENERATE (m
// unchanged), DRF_ALIGN_CONVERGED (the step is below both thresholds and is not applied) or -1 (m moved).  + - * / sqrt only.
inline int align_step(const double sums[28], const double c[3], double eps_rot, double eps_trans, MapMotion &m) {
  double H[6][6], d[6];
  int idx = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { H[i][j] = sums[idx]; H[j][i] = sums[idx]; ++idx; }
  double top = H[0][0];
  for (int j = 1; j < 6; ++j) top = H[j][j] > top ? H[j][j] : top;
  if (!(top > 0.0)) return DRF_ALIGN_DEGENERATE;
  if (align_solve<6>(H, sums + 21, top, d) >= 0) return DRF_ALIGN_DEGENERATE;
  const double oo = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], vv = (d[3] * d[3] + d[4] * d[4]) + d[5] * d[5];
  if (!(oo == oo) || !(vv == vv)) return DRF_ALIGN_DEGENERATE;  // a system that held a NaN
  if (std::sqrt(oo) < eps_rot && std::sqrt(vv) < eps_trans) return DRF_ALIGN_CONVERGED;
  align_move(d, oo, c, m);
  return -1;
}
// What a solver's state holds beside the pose: nothing, for every call but drf_track_exposure_* (ExposureState, below).  The loops
// ask it to keep() the state an evaluation passed with, to go back() to it when a later one is LOST, and for the step.
struct PoseState {
  void keep() {}
  void back() {}
  void level_begin() {}
  void level_abandoned() {}
  int step(const double sums[28], const double c[3], double eps_rot, double eps_trans, MapMotion &m) { return align_step(sums, c, eps_rot, eps_trans, m); }
};
// The loop of every solver over any evaluator eval(const AlignEval &, double sums[28], uint64_t counts[N]): the host's or the
// engine's (the kernels).  The loop reads counts[0] = samples and counts[1] = valid; what else an evaluator counts (N = 3 for the
// registration, 4 for a frame, 5 with colour) passes through: last, if given, receives the N counters of the last evaluation, and
// trace the sums of every evaluation.  state: what the solver holds beside the pose (an evaluator that reads it is given it by its
// own means); LOST restores the last good pose and state.
template <int N = 3, class Eval, class State = PoseState>
inline void align_loop(Eval &&eval, const MapMotion &m0, const double c_src[3], const AlignOpt &o, float voxel_size, drf_align_result_t &res,
                       uint64_t *last = nullptr, std::vector<std::array<double, 28>> *trace = nullptr, State *state = nullptr) {
  MapMotion m = m0, good = m0;
  State none{};
  State &x = state ? *state : none;
  x.keep();
  memset(&res, 0, sizeof res);
  res.status = DRF_ALIGN_MAX_ITERS;
  for (int it = 0; it < o.max_iters; ++it) {
    const AlignEval e = align_eval(m, c_src, o, voxel_size);
    uint64_t counts[N];
    eval(e, res.sums, counts);
    if (last) memcpy(last, counts, sizeof counts);
    if (trace) { std::array<double, 28> t; memcpy(t.data(), res.sums, sizeof res.sums); trace->push_back(t); }
    res.iterations = it + 1;
    res.samples = counts[0]; res.valid = counts[1];
    res.cost = counts[1] ? res.sums[27] / (double)counts[1] : 0.0;
    if (it == 0) { res.valid0 = res.valid; res.cost0 = res.cost; }
    if ((double)counts[1] < o.min_valid * (double)counts[0] || counts[1] < 6) { res.status = DRF_ALIGN_LOST; m = good; x.back(); break; }
    good = m;
    x.keep();
    const int s = x.step(res.sums, e.c, o.eps_rot, o.eps_trans, m);
    if (s >= 0) { res.status = s; break; }
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) res.T[4 * i + j] = m.R[3 * i + j];
    res.T[4 * i + 3] = m.tv[i] * (double)voxel_size;
  }
  res.T[15] = 1.0;
}
inline const char *align_status_name(int s) {
  static const char *names[] = {"converged", "reached max_iters", "is degenerate (the samples do not constrain all six degrees of freedom)",
                                "is lost (too few samples have an observed neighbourhood in the reference)"};
  return s >= 0 && s < 4 ? names[s] : "?";
}
// The whole registration on the CPU: the library's reference for drf_align_map, and what the sanitizer program runs.
inline void align_maps_host(const std::vector<unsigned long long> &src_keys, const uint8_t *src_vox, const HostMapSource &ref, const MapMotion &m0,
                            const AlignOpt &o, float voxel_size, drf_align_result_t &res, std::vector<std::array<double, 28>> *trace = nullptr) {
  double c_src[3];
  align_centre_src(src_keys, c_src);
  align_loop([&](const AlignEval &e, double sums[28], uint64_t counts[3]) { align_system_host(src_keys, src_vox, ref, e, sums, counts); }, m0, c_src, o,
             voxel_size, res, nullptr, trace);
}

// ---- locating a depth frame in the map (drf_locate_system / drf_locate_frame; DESIGN.md §7c "Locating a depth frame in the map")
// T is the engine's pose16: camera-to-world, held as a MapMotion (Rd, tv = t / voxel_size).  The samples are the pixels of a depth
// image on a grid of stride `step`, each the camera-frame point g = ((u - cx) / fx * z, (v - cy) / fy * z, z) / voxel_size in
// double; from q = Rd g + tv on a sample is align_point's, with s_src = 0 and the band test on phi.  The lattice point g of the map
// sits at world g * voxel_size, as for k_integrate and transform_voxel: no half-voxel offset.  Stated once, here; the header of
// the C ABI restates it for users.  Compiled by g++ for the CPU tests and by hipcc for k_map_locate, both without contraction.
struct LocateOpt {  // drf_locate_options_t with its defaults resolved
  AlignOpt a;
  int step;
  float centre_depth;
};
// null: all defaults (band: the engine's truncation_distance).  Returns null, or which option is negative or not finite
inline const char *locate_options(const drf_locate_options_t *opt, float truncation_distance, LocateOpt &o) {
  static const drf_locate_options_t zero = {0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.0};
  const drf_locate_options_t &u = opt ? *opt : zero;
  if (u.step < 0) return "step";
  if (!(u.centre_depth >= 0.0f) || !std::isfinite(u.centre_depth)) return "centre_depth";
  const drf_align_options_t a = {u.max_iters, u.min_weight, u.band, u.huber, u.eps_rot, u.eps_trans, u.min_valid};
  if (const char *bad = align_options(&a, 1.0f, o.a)) return bad;
  if (u.band == 0.0f) o.a.band = truncation_distance;
  o.step = u.step ? u.step : 1;
  o.centre_depth = u.centre_depth;
  return nullptr;
}
// the sample grid and the camera: what a kernel launch and a host evaluation share besides AlignEval
struct LocateGrid {
  int W, H, step, Wg, Hg;  // Wg = ceil(W / step), Hg = ceil(H / step): Wg * Hg grid positions
  float fx, fy, cx, cy, min_depth, max_depth;
};
inline LocateGrid locate_grid(const drf_options_t &o, int step) {
  LocateGrid g;
  g.W = o.width; g.H = o.height; g.step = step;
  g.Wg = (o.width + step - 1) / step; g.Hg = (o.height + step - 1) / step;
  g.fx = o.fx; g.fy = o.fy; g.cx = o.cx; g.cy = o.cy; g.min_depth = o.min_sensor_depth; g.max_depth = o.max_sensor_depth;
  return g;
}
inline long locate_positions(const LocateGrid &g) { return (long)g.Wg * (long)g.Hg; }
inline long locate_groups(const LocateGrid &g) { return (locate_positions(g) + 511) / 512; }
inline void locate_centre_src(float centre_depth, float voxel_size, double c_src[3]) {
  c_src[0] = 0.0; c_src[1] = 0.0; c_src[2] = (double)centre_depth / (double)voxel_size;
}
// Grid position n < Wg * Hg: is its pixel a sample (the conditions under which k_integrate uses a pixel; a NaN is none), and if
// so its camera-frame point g in lattice units.
DR_HOST_DEVICE inline bool locate_is_sample(const LocateGrid &lg, float dep) { return dep > 0.0f && dep >= lg.min_depth && dep <= lg.max_depth; }
DR_HOST_DEVICE inline size_t locate_offset(const LocateGrid &lg, int n) {  // of grid position n's pixel in the depth image
  const int j = n / lg.Wg, i = n - j * lg.Wg;
  return (size_t)(lg.step * j) * (size_t)lg.W + (size_t)(lg.step * i);
}
DR_HOST_DEVICE inline bool locate_pixel(const LocateGrid &lg, double vs, int n, const float *depth, double g[3]) {
  const int j = n / lg.Wg, i = n - j * lg.Wg;
  const int u = lg.step * i, v = lg.step * j;
  const float dep = depth[locate_offset(lg, n)];
  if (!locate_is_sample(lg, dep)) return false;
  const double z = (double)dep;
  g[0] = ((((double)u - (double)lg.cx) / (double)lg.fx) * z) / vs;
  g[1] = ((((double)v - (double)lg.cy) / (double)lg.fy) * z) / vs;
  g[2] = z / vs;
  return true;
}
// The loop's pose (Rd, tv in lattice units, double) as the pose16 the two functions above and select_render_blocks take.  The
// evaluation itself runs at the double pose: an entry of R moves by at most 2^-25 and t_k by 2^-25 |t_k| plus the product's own
// rounding, so a sample point moves by less than 2^-24 (3 max_sensor_depth rho + |t|).  |t| is below 2^23 voxels wherever a block
// has a key, and the depth range far below that: less than one voxel, the vs that locate_stage_slack leaves out of the slack.
inline void locate_pose16(const MapMotion &m, float voxel_size, float pose16[16]) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pose16[4 * i + j] = (float)m.R[3 * i + j];
    pose16[4 * i + 3] = (float)(m.tv[i] * (double)voxel_size);
  }
  pose16[12] = pose16[13] = pose16[14] = 0.0f;
  pose16[15] = 1.0f;
}
// The walk every evaluation over a frame shares, group i in the wave's order: lane l takes grid positions 512 i + l + 64 k,
// k = 0..7 (those >= Wg * Hg are no samples), then the butterfly.  sample(n, g, acc) adds the sample at grid position n, camera-frame
// point g, to acc[28] and returns its code; count(code) names the counter the code adds to besides counts[0], the samples.
// out[S] = the group's sums (S = 28; 45 with the exposure).
template <int S = 28, class Sample, class Count>
inline void frame_group(const AlignEval &e, const LocateGrid &lg, const float *depth, long i, Sample &&sample, Count &&count, double out[S], uint64_t *counts) {
  double x[64][S];
  const long total = locate_positions(lg);
  for (int l = 0; l < 64; ++l) {
    for (int c = 0; c < S; ++c) x[l][c] = 0.0;
    for (int k = 0; k < 8; ++k) {
      const long n = 512 * i + l + 64 * k;
      double g[3];
      if (n >= total || !locate_pixel(lg, e.vs, (int)n, depth, g)) continue;
      ++counts[0];
      count(sample((int)n, g, x[l]), counts);
    }
  }
  align_butterfly(x);
  for (int c = 0; c < S; ++c) out[c] = x[0][c];
}
// The system at one pose over the whole sample grid: N counters from zero, frame_group per group into partial[i], then
// k_align_fold's fold.
template <int N, int S = 28, class Sample, class Count>
inline void frame_system_host(const LocateGrid &lg, const float *depth, const AlignEval &e, Sample &&sample, Count &&count, double sums[S], uint64_t counts[N]) {
  for (int c = 0; c < N; ++c) counts[c] = 0;
  const size_t n = (size_t)locate_groups(lg);
  std::vector<double> partial(n * S);
  for (size_t i = 0; i < n; ++i) frame_group<S>(e, lg, depth, (long)i, sample, count, &partial[i * S], counts);
  align_fold_host<S>(partial.data(), n, sums);
}
// the codes of align_point<true> and track_point: 1 valid, 0 counts[2] (unobserved / unassociated), 2 counts[3] (outside / rejected)
inline void frame_count(int r, uint64_t *counts) { ++counts[r == 1 ? 1 : r == 0 ? 2 : 3]; }
// counts = {samples, valid, unobserved, outside}
template <class Fetch>
inline void locate_system_host(const LocateGrid &lg, const float *depth, Fetch &&fetch, const AlignEval &e, double sums[28], uint64_t counts[4]) {
  frame_system_host<4>(lg, depth, e, [&](int, const double *g, double *acc) { return align_point<true>(e, g[0], g[1], g[2], 0.0f, fetch, acc); }, frame_count,
                       sums, counts);
}
// align_loop over a localisation's evaluator eval(const AlignEval &, double sums[28], uint64_t counts[4]); last4, if given, receives
// the four counters of the last evaluation.
template <class Eval>
inline void locate_loop(Eval &&eval, const MapMotion &m0, const LocateOpt &o, float voxel_size, drf_align_result_t &res, uint64_t *last4 = nullptr,
                        std::vector<std::array<double, 28>> *trace = nullptr) {
  double c_src[3];
  locate_centre_src(o.centre_depth, voxel_size, c_src);
  align_loop<4>(eval, m0, c_src, o.a, voxel_size, res, last4, trace);
}
// The whole refinement on the CPU over a HostMapSource or any fetch: the library's reference for drf_locate_frame, and what the
// sanitizer program runs.
template <class Fetch>
inline void locate_frame_host(const LocateGrid &lg, const float *depth, Fetch &&fetch, const MapMotion &m0, const LocateOpt &o, float voxel_size,
                              drf_align_result_t &res, std::vector<std::array<double, 28>> *trace = nullptr) {
  locate_loop([&](const AlignEval &e, double sums[28], uint64_t c4[4]) { locate_system_host(lg, depth, fetch, e, sums, c4); }, m0, o, voxel_size, res,
              nullptr, trace);
}

// ---- tracking a depth frame against the ray-cast model (drf_track_system / drf_track_frame; DESIGN.md §7c "Tracking a depth frame
// against the ray-cast model").  The frame's samples are drf_locate_*'s (locate_pixel, the same grid and test); each is associated
// projectively with a pixel of the MODEL MAP -- per pixel of a depth image Dm ray-cast at the pose Pm its depth and the unit normal
// of its back-projected neighbourhood -- and contributes the point-to-plane distance to that pixel's plane.  From the residual and
// the normal on a sample is align_accumulate's, the step and the loop align_step's and align_loop's.  Stated once, here; the
// header of the C ABI restates it for users.  Compiled by g++ and by hipcc (k_track_model, k_track), both without contraction;
// + - * / sqrt and floor only.
struct TrackOpt {  // drf_track_options_t with its defaults resolved; a.max_iters is inner_iters (a.band and a.min_weight are not read)
  AlignOpt a;
  int max_renders, step;
  float centre_depth, dist_max, max_jump;
};
// null: all defaults.  Returns null, or which option is negative or not finite
inline const char *track_options(const drf_track_options_t *opt, float voxel_size, TrackOpt &o) {
  static const drf_track_options_t zero = {0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.0};
  const drf_track_options_t &u = opt ? *opt : zero;
  if (u.max_renders < 0) return "max_renders";
  if (u.inner_iters < 0) return "inner_iters";
  if (u.step < 0) return "step";
  if (!(u.dist_max >= 0.0f) || !std::isfinite(u.dist_max)) return "dist_max";
  if (!(u.max_jump >= 0.0f) || !std::isfinite(u.max_jump)) return "max_jump";
  if (!(u.centre_depth >= 0.0f) || !std::isfinite(u.centre_depth)) return "centre_depth";
  const drf_align_options_t a = {u.inner_iters, 0, 0.0f, u.huber, u.eps_rot, u.eps_trans, u.min_valid};
  if (const char *bad = align_options(&a, 1.0f, o.a)) return bad;
  o.a.max_iters = u.inner_iters ? u.inner_iters : 4;
  o.max_renders = u.max_renders ? u.max_renders : 10;
  o.step = u.step ? u.step : 1;
  o.dist_max = u.dist_max != 0.0f ? u.dist_max : 25.0f * voxel_size;
  o.max_jump = u.max_jump != 0.0f ? u.max_jump : 5.0f * voxel_size;
  o.centre_depth = u.centre_depth;
  return nullptr;
}
// one pixel of the model map: the unit normal in the model camera's frame, towards the camera, and the depth; z = 0 is invalid
struct alignas(16) TrackPixel { float nx, ny, nz, z; };
// The model map's pixel (u, v) from the model depth image Dm (lg: the camera; its step is not read), all in fp32.  A MISS of the
// ray-cast is the 0.0f that k_raycast2 / k_raycast_fix write for a ray that found no surface; the test is !(z > 0), which a NaN
// and a negative depth fail too.  Invalid (all four floats 0): the centre is a miss; the pixel lies on the image border; one of its
// four neighbours (u -+ 1, v), (u, v -+ 1) is a miss; |z_neighbour - z| > max_jump for one of them.  Otherwise, with
// X(u, v, z) = ((((float)u - cx) / fx) * z, (((float)v - cy) / fy) * z, z): a = X(u + 1, v) - X(u - 1, v), b = X(u, v + 1) -
// X(u, v - 1), n = a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), l2 = (n0 n0 + n1 n1) + n2 n2; !(l2 > 0) is invalid;
// n = n / sqrt(l2); and with s = (n0 X0 + n1 X1) + n2 X2 at the centre, s > 0 negates n: the normal looks at the camera.
DR_HOST_DEVICE inline TrackPixel track_normal(const LocateGrid &lg, float max_jump, const float *Dm, int u, int v) {
  TrackPixel p = {0.0f, 0.0f, 0.0f, 0.0f};
  if (u <= 0 || v <= 0 || u >= lg.W - 1 || v >= lg.H - 1) return p;
  const size_t at = (size_t)v * (size_t)lg.W + (size_t)u;
  const float z = Dm[at], zl = Dm[at - 1], zr = Dm[at + 1], zu = Dm[at - (size_t)lg.W], zd = Dm[at + (size_t)lg.W];
  if (!(z > 0.0f) || !(zl > 0.0f) || !(zr > 0.0f) || !(zu > 0.0f) || !(zd > 0.0f)) return p;
  const float jl = zl - z, jr = zr - z, ju = zu - z, jd = zd - z;
  if ((jl < 0.0f ? -jl : jl) > max_jump || (jr < 0.0f ? -jr : jr) > max_jump || (ju < 0.0f ? -ju : ju) > max_jump || (jd < 0.0f ? -jd : jd) > max_jump) return p;
  const float rx = ((float)u - lg.cx) / lg.fx, ry = ((float)v - lg.cy) / lg.fy;
  const float rxl = ((float)(u - 1) - lg.cx) / lg.fx, rxr = ((float)(u + 1) - lg.cx) / lg.fx;
  const float ryu = ((float)(v - 1) - lg.cy) / lg.fy, ryd = ((float)(v + 1) - lg.cy) / lg.fy;
  const float a0 = rxr * zr - rxl * zl, a1 = ry * zr - ry * zl, a2 = zr - zl;
  const float b0 = rx * zd - rx * zu, b1 = ryd * zd - ryu * zu, b2 = zd - zu;
  float n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
  const float l2 = (n0 * n0 + n1 * n1) + n2 * n2;
  if (!(l2 > 0.0f)) return p;
  const float l = sqrtf(l2);
  n0 = n0 / l; n1 = n1 / l; n2 = n2 / l;
  const float s = (n0 * (rx * z) + n1 * (ry * z)) + n2 * z;
  if (s > 0.0f) { n0 = -n0; n1 = -n1; n2 = -n2; }
  p.nx = n0; p.ny = n1; p.nz = n2; p.z = z;
  return p;
}
inline void track_model_host(const LocateGrid &lg, float max_jump, const float *Dm, TrackPixel *out) {
  for (int v = 0; v < lg.H; ++v)
    for (int u = 0; u < lg.W; ++u) out[(size_t)v * lg.W + u] = track_normal(lg, max_jump, Dm, u, v);
}
// the model of one evaluation: its pose Pm (camera-to-world, lattice units), (dist_max / voxel_size)^2, and the map
struct TrackModel {
  MapMotion m;
  double lim2;
  const TrackPixel *map;
};
inline TrackModel track_model(const float *model_pose16, const TrackOpt &o, float voxel_size, const TrackPixel *map) {
  TrackModel t;
  t.m = map_motion(model_pose16, voxel_size);
  const double lim = (double)o.dist_max / (double)voxel_size;
  t.lim2 = lim * lim;
  t.map = map;
  return t;
}
// One sample at the camera-frame point g (lattice units, locate_pixel's): q = Rd g + tv at the estimate; m = Rm^T (q - tvm), the
// point in the model camera; !(m2 > 0) is UNASSOCIATED (behind the model camera, or a NaN); u' = fx (m0 / m2) + cx, v' likewise,
// the pixel (floor(u' + 0.5), floor(v' + 0.5)); outside the image or an invalid model pixel is UNASSOCIATED (returns 0).  The model
// vertex vm is that pixel's back-projection at its z, as locate_pixel computes a point; d = m - vm; a sample for which
// |d|^2 <= lim2 is false is REJECTED (returns 2).  Otherwise r = (n0 d0 + n1 d1) + n2 d2 with the pixel's normal widened to
// double, nw = Rm n, and tail(r, nw0, nw1, nw2, q, m, u', v') adds the sample's terms and returns the code (1 for track_point).
// The tail is where track_point and track_colour_point differ: one term, or two.
template <class Tail>
DR_HOST_DEVICE inline int track_sample(const AlignEval &e, const TrackModel &t, const LocateGrid &lg, double g0, double g1, double g2, Tail &&tail) {
  double q[3], m[3];
  DR_UNROLL
  for (int k = 0; k < 3; ++k) q[k] = ((e.m.R[3 * k] * g0 + e.m.R[3 * k + 1] * g1) + e.m.R[3 * k + 2] * g2) + e.m.tv[k];
  const double s0 = q[0] - t.m.tv[0], s1 = q[1] - t.m.tv[1], s2 = q[2] - t.m.tv[2];
  DR_UNROLL
  for (int k = 0; k < 3; ++k) m[k] = (t.m.R[k] * s0 + t.m.R[3 + k] * s1) + t.m.R[6 + k] * s2;
  if (!(m[2] > 0.0)) return 0;
  const double up = (double)lg.fx * (m[0] / m[2]) + (double)lg.cx, vp = (double)lg.fy * (m[1] / m[2]) + (double)lg.cy;
  const double pu = floor(up + 0.5), pv = floor(vp + 0.5);
  if (!(pu >= 0.0 && pu <= (double)(lg.W - 1) && pv >= 0.0 && pv <= (double)(lg.H - 1))) return 0;
  const TrackPixel p = t.map[(size_t)(int)pv * (size_t)lg.W + (size_t)(int)pu];
  if (!(p.z > 0.0f)) return 0;
  const double z = (double)p.z;
  const double d0 = m[0] - (((pu - (double)lg.cx) / (double)lg.fx) * z) / e.vs;
  const double d1 = m[1] - (((pv - (double)lg.cy) / (double)lg.fy) * z) / e.vs;
  const double d2 = m[2] - z / e.vs;
  const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
  if (!(dd <= t.lim2)) return 2;
  const double n0 = (double)p.nx, n1 = (double)p.ny, n2 = (double)p.nz;
  const double r = (n0 * d0 + n1 * d1) + n2 * d2;
  const double w0 = (t.m.R[0] * n0 + t.m.R[1] * n1) + t.m.R[2] * n2;
  const double w1 = (t.m.R[3] * n0 + t.m.R[4] * n1) + t.m.R[5] * n2;
  const double w2 = (t.m.R[6] * n0 + t.m.R[7] * n1) + t.m.R[8] * n2;
  return tail(r, w0, w1, w2, q, m, up, vp);
}
// The geometric term alone: align_accumulate adds the sample.
DR_HOST_DEVICE inline int track_point(const AlignEval &e, const TrackModel &t, const LocateGrid &lg, double g0, double g1, double g2, double acc[28]) {
  return track_sample(e, t, lg, g0, g1, g2, [&](double r, double w0, double w1, double w2, const double *q, const double *, double, double) {
    align_accumulate(e, r, w0, w1, w2, q, acc);
    return 1;
  });
}
// The system at one pose over the whole sample grid (frame_system_host); counts = {samples, valid, unassociated, rejected}.
inline void track_system_host(const LocateGrid &lg, const float *depth, const TrackModel &t, const AlignEval &e, double sums[28], uint64_t counts[4]) {
  frame_system_host<4>(lg, depth, e, [&](int, const double *g, double *acc) { return track_point(e, t, lg, g[0], g[1], g[2], acc); }, frame_count, sums, counts);
}
// The outer loop of drf_track_frame and drf_track_colour_frame over render(const float pose16[16]), which ray-casts the map at that
// pose and builds the model map (with colour: and Ym), and eval(const AlignEval &, const float model_pose16[16], double sums[28],
// uint64_t counts[N]), one evaluation against it (N = 4, or 5 with colour).
// Round r renders at p16 -- pose_init16, later the float pose16 the round before ended on (res.T rounded to float, what
// drf_render_async would be given) -- and runs align_loop from that very pose, m = map_motion(p16), with max_iters = inner_iters.
// A round that ends LOST or DEGENERATE ends the call with that status; one that
// ends CONVERGED at its first evaluation ends it CONVERGED; any other round hands its pose on, and after max_renders rounds the
// call is MAX_ITERS.  res: T, sums, samples, valid, cost of the last round; valid0, cost0 of the first; iterations = evaluations in
// all.  stats2 = {evaluations, renders}; last the N counters of the last evaluation.
// state (align_loop's) carries from round to round.
template <int N = 4, class Render, class Eval, class State = PoseState>
inline void track_loop(Render &&render, Eval &&eval, const float *pose_init16, const TrackOpt &o, float voxel_size, drf_align_result_t &res,
                       uint64_t *last = nullptr, uint64_t *stats2 = nullptr, std::vector<std::array<double, 28>> *trace = nullptr, State *state = nullptr) {
  double c_src[3];
  locate_centre_src(o.centre_depth, voxel_size, c_src);
  float p16[16];
  memcpy(p16, pose_init16, sizeof p16);
  memset(&res, 0, sizeof res);
  int evaluations = 0;
  uint64_t valid0 = 0;
  double cost0 = 0.0;
  for (int r = 0; r < o.max_renders; ++r) {
    render(p16);
    if (stats2) ++stats2[1];
    drf_align_result_t in;
    align_loop<N>([&](const AlignEval &e, double sums[28], uint64_t *counts) {
      eval(e, p16, sums, counts);
      if (stats2) ++stats2[0];
    }, map_motion(p16, voxel_size), c_src, o.a, voxel_size, in, last, trace, state);
    evaluations += in.iterations;
    if (r == 0) { valid0 = in.valid0; cost0 = in.cost0; }
    res = in;
    res.valid0 = valid0; res.cost0 = cost0; res.iterations = evaluations;
    if (in.status == DRF_ALIGN_LOST || in.status == DRF_ALIGN_DEGENERATE) return;
    if (in.status == DRF_ALIGN_CONVERGED && in.iterations == 1) return;
    res.status = DRF_ALIGN_MAX_ITERS;
    for (int i = 0; i < 16; ++i) p16[i] = (float)in.T[i];
  }
}
// (track_frame_host, the whole tracking on the CPU, is track_colour_frame_host<4> below)

// ---- tracking with colour (drf_track_colour_system / drf_track_colour_frame; DESIGN.md §7c "Tracking with colour").  The tracking
// above sees geometry only, and a map of planes leaves the motion inside the planes open.  Every voxel carries a colour and the
// ray-cast renders it, so a sample whose geometric term was added contributes a second, photometric term: the difference between
// the model's colour image, interpolated where the sample projects, and the frame's own pixel, as intensities, scaled to voxels by
// photo_weight.  Its gradient with respect to the point is a 3-vector like the plane's normal, so both terms go through the one
// align_accumulate into the same 28 sums, and step, loop and outer loop are the geometric call's, unchanged.  Stated once, here;
// the header of the C ABI restates it.  Compiled by g++ and by hipcc (k_track_model_colour, k_track_colour), both without
// contraction; + - * / sqrt and floor only.
#if defined(__HIPCC__)
#define DR_NO_UNROLL _Pragma("unroll 1")
#else
#define DR_NO_UNROLL
#endif
struct TrackColourOpt {  // drf_track_colour_options_t with its defaults resolved
  TrackOpt t;
  float photo_weight;  // voxels per intensity unit
};
// null: all defaults.  photo_weight 0 is (float)(1.0 / 27.0) * huber in fp32, huber resolved first: a colour residual of 27 units
// of the three-channel sum -- 9 grey levels of 255 -- weighs what a geometric residual at Huber's threshold weighs.
inline const char *track_colour_options(const drf_track_colour_options_t *opt, float voxel_size, TrackColourOpt &o) {
  static const drf_track_colour_options_t zero = {{0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0, 0.0, 0.0}, 0.0f};
  const drf_track_colour_options_t &u = opt ? *opt : zero;
  if (const char *bad = track_options(&u.track, voxel_size, o.t)) return bad;
  if (!(u.photo_weight >= 0.0f) || !std::isfinite(u.photo_weight)) return "photo_weight";
  o.photo_weight = u.photo_weight != 0.0f ? u.photo_weight : (float)(1.0 / 27.0) * o.t.a.huber;
  return nullptr;
}
// the intensity of a BGR pixel: a whole number in 0..765
DR_HOST_DEVICE inline float track_intensity(const unsigned char *bgr) { return ((float)bgr[0] + (float)bgr[1]) + (float)bgr[2]; }
// One pixel of the model intensity map Ym: the intensity of the model colour image where the model map's pixel is valid, -1
// elsewhere -- misses, the border and depth discontinuities are excluded by the test the geometric term uses.
DR_HOST_DEVICE inline float track_model_intensity(const TrackPixel &p, const unsigned char *bgr) { return p.z > 0.0f ? track_intensity(bgr) : -1.0f; }
inline void track_model_colour_host(const LocateGrid &lg, float max_jump, const float *Dm, const unsigned char *Cm, TrackPixel *out, float *Ym) {
  for (int v = 0; v < lg.H; ++v)
    for (int u = 0; u < lg.W; ++u) {
      const size_t at = (size_t)v * lg.W + u;
      out[at] = track_normal(lg, max_jump, Dm, u, v);
      Ym[at] = track_model_intensity(out[at], Cm + 3 * at);
    }
}
// what an evaluation with colour reads besides the TrackModel: Ym and lambda = (double)photo_weight
struct TrackColour {
  const float *Ym;
  double weight;
};
inline TrackColour track_colour(const TrackColourOpt &o, const float *Ym) {
  TrackColour c;
  c.Ym = Ym; c.weight = (double)o.photo_weight;
  return c;
}
struct TrackPair { float a, b; };  // two neighbours of a row of Ym: one 8-byte read at a 4-byte aligned address
// The photometric term of a sample that track_sample accepted, from its m, u', v' and the frame's intensity yf at the sample's
// own pixel.  u0 = floor(u'), v0 = floor(v'), a = u' - u0, b = v' - v0; the term is SKIPPED (returns false) unless 0 <= u0,
// u0 + 1 <= W - 1, 0 <= v0, v0 + 1 <= H - 1 and the four corners y00 = Ym(u0, v0), y10 = Ym(u0 + 1, v0), y01 = Ym(u0, v0 + 1),
// y11 = Ym(u0 + 1, v0 + 1) are all >= 0.  In double, oa = 1 - a, ob = 1 - b:
//   I  = ob * (oa * y00 + a * y10) + b * (oa * y01 + a * y11)
//   Iu = ob * (y10 - y00) + b * (y11 - y01),  Iv = oa * (y01 - y00) + a * (y11 - y10)     the exact gradient of that interpolant
//   gm0 = (Iu * fx) / m2, gm1 = (Iv * fy) / m2, gm2 = -((gm0 * m0 + gm1 * m1) / m2)          dI/dm through u' = fx m0 / m2 + cx
//   r = lambda * (I - yf),  n_k = lambda * ((Rm[k][0] gm0 + Rm[k][1] gm1) + Rm[k][2] gm2)   dr/dq = Rm dr/dm, as for the plane
DR_HOST_DEVICE inline bool track_photo_term(const TrackModel &t, const TrackColour &tc, const LocateGrid &lg, const double m[3], double up, double vp, float yf,
                                            double &r, double n[3]) {
  const double fu = floor(up), fv = floor(vp);
  if (!(fu >= 0.0 && fu + 1.0 <= (double)(lg.W - 1) && fv >= 0.0 && fv + 1.0 <= (double)(lg.H - 1))) return false;
  const size_t at = (size_t)(int)fv * (size_t)lg.W + (size_t)(int)fu;
  TrackPair top, bot;
  memcpy(&top, tc.Ym + at, sizeof top);
  memcpy(&bot, tc.Ym + at + (size_t)lg.W, sizeof bot);
  if (!(top.a >= 0.0f && top.b >= 0.0f && bot.a >= 0.0f && bot.b >= 0.0f)) return false;
  const double y00 = (double)top.a, y10 = (double)top.b, y01 = (double)bot.a, y11 = (double)bot.b;
  const double a = up - fu, b = vp - fv, oa = 1.0 - a, ob = 1.0 - b;
  const double I = ob * (oa * y00 + a * y10) + b * (oa * y01 + a * y11);
  const double Iu = ob * (y10 - y00) + b * (y11 - y01), Iv = oa * (y01 - y00) + a * (y11 - y10);
  const double gm0 = (Iu * (double)lg.fx) / m[2], gm1 = (Iv * (double)lg.fy) / m[2];
  const double gm2 = -((gm0 * m[0] + gm1 * m[1]) / m[2]);
  r = tc.weight * (I - (double)yf);
  n[0] = tc.weight * ((t.m.R[0] * gm0 + t.m.R[1] * gm1) + t.m.R[2] * gm2);
  n[1] = tc.weight * ((t.m.R[3] * gm0 + t.m.R[4] * gm1) + t.m.R[5] * gm2);
  n[2] = tc.weight * ((t.m.R[6] * gm0 + t.m.R[7] * gm1) + t.m.R[8] * gm2);
  return true;
}
// One sample with colour: track_sample's codes 0 (unassociated) and 2 (rejected) add nothing; otherwise the geometric term is
// added first and, where track_photo_term has one, the photometric term second: returns 1 for the one, 3 for both.  The two are
// trips of one loop, so that align_accumulate stands once in the kernel's instruction stream.
DR_HOST_DEVICE inline int track_colour_point(const AlignEval &e, const TrackModel &t, const TrackColour &tc, const LocateGrid &lg, double g0, double g1, double g2,
                                             float yf, double acc[28]) {
  return track_sample(e, t, lg, g0, g1, g2, [&](double r, double w0, double w1, double w2, const double *q, const double *m, double up, double vp) {
    double pr = 0.0, pn[3] = {0.0, 0.0, 0.0};
    const bool photo = track_photo_term(t, tc, lg, m, up, vp, yf, pr, pn);
    const int terms = photo ? 2 : 1;
    DR_NO_UNROLL
    for (int k = 0; k < terms; ++k) {
      const bool second = k == 1;
      align_accumulate(e, second ? pr : r, second ? pn[0] : w0, second ? pn[1] : w1, second ? pn[2] : w2, q, acc);
    }
    return photo ? 3 : 1;
  });
}
// the codes of track_colour_point: 3 is valid and adds to the fifth counter
inline void track_colour_count(int r, uint64_t *c) { ++c[(r & 1) ? 1 : r == 0 ? 2 : 3]; if (r == 3) ++c[4]; }
// The system at one pose over the whole sample grid (frame_system_host); counts = {samples, valid, unassociated, rejected,
// photometric terms added}.
inline void track_colour_system_host(const LocateGrid &lg, const unsigned char *bgr, const float *depth, const TrackModel &t, const TrackColour &tc,
                                     const AlignEval &e, double sums[28], uint64_t counts[5]) {
  frame_system_host<5>(lg, depth, e, [&](int n, const double *g, double *acc) {
    return track_colour_point(e, t, tc, lg, g[0], g[1], g[2], track_intensity(bgr + 3 * locate_offset(lg, n)), acc);
  }, track_colour_count, sums, counts);
}
// The whole tracking on the CPU over any renderer render(const float pose16[16], unsigned char *Cm, float *Dm): the library's
// reference for drf_track_colour_frame (N = 5: track_loop's render builds the model map and Ym from the colour and the depth it
// rendered) and, without the colour images, for drf_track_frame (N = 4: bgr is not read, Cm is empty, o.photo_weight is not read);
// what the sanitizer programs run.  last, if given, receives the N counters of the last evaluation.
// state: null, or the ExposureState of drf_track_exposure_frame (below), whose evaluation then takes the colour one's place.
template <int N = 5, class RenderBoth, class State = PoseState>
inline void track_colour_frame_host(const LocateGrid &lg, const unsigned char *bgr, const float *depth, RenderBoth &&render_both, const float *pose_init16,
                                    const TrackColourOpt &o, float voxel_size, drf_align_result_t &res, uint64_t *last = nullptr, uint64_t *stats2 = nullptr,
                                    std::vector<std::array<double, 28>> *trace = nullptr, State *state = nullptr) {
  constexpr bool colour = N == 5;
  const size_t npix = (size_t)lg.W * (size_t)lg.H;
  std::vector<float> Dm(npix), Ym(colour ? npix : 0);
  std::vector<unsigned char> Cm(colour ? npix * 3 : 0);
  std::vector<TrackPixel> map(npix);
  track_loop<N>([&](const float *p16) {
    render_both(p16, Cm.data(), Dm.data());
    if (colour) track_model_colour_host(lg, o.t.max_jump, Dm.data(), Cm.data(), map.data(), Ym.data());
    else track_model_host(lg, o.t.max_jump, Dm.data(), map.data());
  }, [&](const AlignEval &e, const float *p16, double sums[28], uint64_t *c) {
    const TrackModel tm = track_model(p16, o.t, voxel_size, map.data());
    if constexpr (!std::is_same<State, PoseState>::value) state->evaluate_host(lg, bgr, depth, tm, track_colour(o, Ym.data()), e, sums, c);
    else if (colour) track_colour_system_host(lg, bgr, depth, tm, track_colour(o, Ym.data()), e, sums, c);
    else track_system_host(lg, depth, tm, e, sums, c);
  }, pose_init16, o.t, voxel_size, res, last, stats2, trace, state);
}
template <class RenderDepth>
inline void track_frame_host(const LocateGrid &lg, const float *depth, RenderDepth &&render_depth, const float *pose_init16, const TrackOpt &o, float voxel_size,
                             drf_align_result_t &res, uint64_t *last4 = nullptr, uint64_t *stats2 = nullptr, std::vector<std::array<double, 28>> *trace = nullptr) {
  track_colour_frame_host<4>(lg, nullptr, depth, [&](const float *p16, unsigned char *, float *Dm) { render_depth(p16, Dm); }, pose_init16, TrackColourOpt{o, 0.0f},
                             voxel_size, res, last4, stats2, trace);
}

// ---- tracking coarse to fine (drf_track_reduce / drf_track_pyramid_system / drf_track_pyramid_frame; DESIGN.md §7c "Tracking coarse
// to fine").  Both calls above run at the camera's resolution, where a render aliases a texture finer than a pixel and the cost has
// minima at the texture's scale.  Level L = 0 .. levels - 1 halves the images L times, s = 2^L: frame and model are REDUCED by one
// rule, the camera is scaled, and the level's evaluation is the rule above on the reduced images -- track_normal,
// track_model_intensity, track_point and track_colour_point as they stand, given the level's LocateGrid.  The levels run from the
// coarsest down, each track_loop from the pose the one above ended on; level 0 is the call above, bit for bit.  Stated once,
// here; the header of the C ABI restates it.  Compiled by g++ and by hipcc (k_track_reduce), both without contraction; + - * / sqrt
// floor and integer arithmetic only.
constexpr int kTrackMaxLevels = 5, kTrackMinLevelSide = 8;
// The camera of level L from the camera lg0 of level 0 (its step is kept): W_L = W / s, H_L = H / s by integer division -- the
// remainder columns and rows are dropped -- fx_L = fx / s, cx_L = (cx + 0.5f) / s - 0.5f in fp32 (a pixel's centre is at its index:
// a block's centre in level units), fy_L and cy_L likewise; the depth limits are unchanged.  Level 0 is lg0 itself.
inline LocateGrid track_level_grid(const LocateGrid &lg0, int L) {
  if (L == 0) return lg0;
  LocateGrid g = lg0;
  const int s = 1 << L;
  const float sf = (float)s;
  g.W = lg0.W / s; g.H = lg0.H / s;
  g.Wg = (g.W + g.step - 1) / g.step; g.Hg = (g.H + g.step - 1) / g.step;
  g.fx = lg0.fx / sf; g.fy = lg0.fy / sf;
  g.cx = (lg0.cx + 0.5f) / sf - 0.5f; g.cy = (lg0.cy + 0.5f) / sf - 0.5f;
  return g;
}
inline bool track_level_fits(int W, int H, int L) { return L >= 0 && L < kTrackMaxLevels && (W >> L) >= kTrackMinLevelSide && (H >> L) >= kTrackMinLevelSide; }
struct TrackPyramidOpt {  // drf_track_pyramid_options_t with its defaults resolved
  TrackColourOpt c;
  int levels, coarse_renders;
};
// null: all defaults.  Returns null, or which option is refused: the colour options' own first, then levels (negative, above 5, or
// its coarsest level below 8 pixels on a side of the W x H camera), then coarse_renders (negative).
inline const char *track_pyramid_options(const drf_track_pyramid_options_t *opt, float voxel_size, int W, int H, TrackPyramidOpt &o) {
  if (const char *bad = track_colour_options(opt ? &opt->colour : nullptr, voxel_size, o.c)) return bad;
  const int levels = opt ? opt->levels : 0, coarse = opt ? opt->coarse_renders : 0;
  if (levels < 0 || levels > kTrackMaxLevels) return "levels";
  o.levels = levels ? levels : 3;
  if (!track_level_fits(W, H, o.levels - 1)) return "levels";
  if (coarse < 0) return "coarse_renders";
  o.coarse_renders = coarse ? coarse : 3;
  return nullptr;
}
// the options of level L: max_jump_L = (float)s * max_jump (max_jump resolved first), and above level 0 max_renders = coarse_renders
inline TrackColourOpt track_level_options(const TrackPyramidOpt &o, int L) {
  TrackColourOpt c = o.c;
  c.t.max_jump = (float)(1 << L) * o.c.t.max_jump;
  if (L > 0) c.t.max_renders = o.coarse_renders;
  return c;
}
// The pieces of the reduction that the host and k_track_reduce share.  A pixel is VALID iff z > 0 (a NaN is not); it is ACCEPTED
// iff it is valid and z - z0 <= max_jump in fp32, z0 the smallest valid depth of its block (an infinite z is never accepted:
// inf - z0 is inf or NaN).  A channel's output from its integer sum c over the n accepted pixels: (2 c + n) / (2 n), half up.
DR_HOST_DEVICE inline bool track_reduce_valid(float z) { return z > 0.0f; }
DR_HOST_DEVICE inline bool track_reduce_accepted(float z, float z0, float max_jump) { return z > 0.0f && z - z0 <= max_jump; }
DR_HOST_DEVICE inline unsigned char track_reduce_colour(int c, int n) { return (unsigned char)((2 * c + n) / (2 * n)); }
// A (bgr, depth) pair of W x H reduced to level L (bgr null: the depth alone): level pixel (u, v) covers the block
// [u s, u s + s) x [v s, v s + s).  z0 = the smallest valid depth of the block; none valid: depth 0.0f, colour 0, 0, 0.  n = the
// accepted pixels; 2 n < s s: the same zeros.  Otherwise depth = S / (float)n, where a pixel that is not accepted contributes
// +0.0f, each row of the block is summed by the butterfly t[i] = t[i] + t[i ^ off], off = s / 2 .. 1, its sum t[0], and the rows
// are added in ascending order from the first row's sum; and each channel is track_reduce_colour of its sum over the accepted.
// The butterfly is what a wave does across the s lanes that hold a row of the block.  max_jump is the level's own.
inline void track_reduce_host(int W, int H, int L, float max_jump, const unsigned char *bgr, const float *depth, unsigned char *bgr_out, float *depth_out) {
  const int s = 1 << L, WL = W / s, HL = H / s;
  for (int v = 0; v < HL; ++v)
    for (int u = 0; u < WL; ++u) {
      const size_t at = (size_t)(v * s) * (size_t)W + (size_t)(u * s), to = (size_t)v * (size_t)WL + (size_t)u;
      bool any = false;
      float z0 = 0.0f;
      for (int r = 0; r < s; ++r)
        for (int i = 0; i < s; ++i) {
          const float z = depth[at + (size_t)r * W + i];
          if (track_reduce_valid(z) && (!any || z < z0)) { z0 = z; any = true; }
        }
      int n = 0, c[3] = {0, 0, 0};
      float S = 0.0f;
      for (int r = 0; r < s && any; ++r) {
        float t[16];
        for (int i = 0; i < s; ++i) {
          const size_t px = at + (size_t)r * W + i;
          const bool acc = track_reduce_accepted(depth[px], z0, max_jump);
          t[i] = acc ? depth[px] : 0.0f;
          if (!acc) continue;
          ++n;
          if (bgr) { c[0] += bgr[3 * px]; c[1] += bgr[3 * px + 1]; c[2] += bgr[3 * px + 2]; }
        }
        for (int off = s >> 1; off > 0; off >>= 1) {
          float y[16];
          for (int i = 0; i < s; ++i) y[i] = t[i] + t[i ^ off];
          memcpy(t, y, sizeof(float) * (size_t)s);
        }
        S = r == 0 ? t[0] : S + t[0];
      }
      const bool keep = any && 2 * n >= s * s;
      depth_out[to] = keep ? S / (float)n : 0.0f;
      if (bgr)
        for (int k = 0; k < 3; ++k) bgr_out[3 * to + k] = keep ? track_reduce_colour(c[k], n) : (unsigned char)0;
    }
}
// The schedule of drf_track_pyramid_frame over run(L, p16, level options, res, last[5], stats2[2]), one track_loop at level L from
// p16 (the engine's, over its kernels, or track_pyramid_frame_host's).  L = levels - 1 down to 1: a level that ends LOST or
// DEGENERATE is ABANDONED, the pose it started from goes to the next finer level; any other level hands on its T rounded to
// float.  Level 0 then runs with max_renders as given and res is its result, exactly.  stats8 = {[0] grid positions, [1] samples and
// [2] valid samples at the last evaluation, each summed over the levels; [3] evaluations and [4] renders in all; [5] left to the
// caller; [6] levels run; [7] levels abandoned}; level4[L] = {status, renders, evaluations, valid at the last evaluation}.
template <class Run>
inline void track_pyramid_schedule(Run &&run, const LocateGrid &lg0, const float *pose_init16, const TrackPyramidOpt &o, drf_align_result_t &res, uint64_t stats8[8],
                                   uint64_t level4[kTrackMaxLevels][4], uint64_t *last5 = nullptr) {
  float p16[16];
  memcpy(p16, pose_init16, sizeof p16);
  for (int i = 0; i < 8; ++i) stats8[i] = i == 5 ? stats8[5] : 0;
  memset(level4, 0, sizeof(uint64_t) * kTrackMaxLevels * 4);
  for (int L = o.levels - 1; L >= 0; --L) {
    const TrackColourOpt lo = track_level_options(o, L);
    drf_align_result_t r;
    uint64_t last[5] = {0, 0, 0, 0, 0}, st2[2] = {0, 0};
    run(L, p16, lo, r, last, st2);
    level4[L][0] = (uint64_t)r.status; level4[L][1] = st2[1]; level4[L][2] = st2[0]; level4[L][3] = last[1];
    stats8[0] += (uint64_t)locate_positions(track_level_grid(lg0, L));
    stats8[1] += last[0]; stats8[2] += last[1]; stats8[3] += st2[0]; stats8[4] += st2[1];
    ++stats8[6];
    if (L == 0) {
      res = r;
      if (last5) memcpy(last5, last, sizeof last);
      break;
    }
    if (r.status == DRF_ALIGN_LOST || r.status == DRF_ALIGN_DEGENERATE) { ++stats8[7]; continue; }
    for (int i = 0; i < 16; ++i) p16[i] = (float)r.T[i];
  }
}
// One evaluation at level L on the CPU: both full-resolution pairs reduced (max_jump_L), the level's model map (and Ym), then the
// system of the rule above with the level's camera.  bgr null: the geometric system, counts[4] = 0.
inline void track_pyramid_system_host(const LocateGrid &lg0, int L, const unsigned char *bgr, const float *depth, const unsigned char *model_bgr, const float *model_depth,
                                      const float *model_pose16, const float *pose16, const TrackPyramidOpt &o, float voxel_size, double sums[28], uint64_t counts[5]) {
  const bool colour = bgr != nullptr;
  const TrackColourOpt lo = track_level_options(o, L);
  const LocateGrid lg = track_level_grid(lg0, L);
  const size_t npix = (size_t)lg.W * (size_t)lg.H;
  std::vector<float> fd(npix), md(npix), Ym(colour ? npix : 0);
  std::vector<unsigned char> fc(colour ? 3 * npix : 0), mc(colour ? 3 * npix : 0);
  track_reduce_host(lg0.W, lg0.H, L, lo.t.max_jump, bgr, depth, fc.data(), fd.data());
  track_reduce_host(lg0.W, lg0.H, L, lo.t.max_jump, colour ? model_bgr : nullptr, model_depth, mc.data(), md.data());
  std::vector<TrackPixel> map(npix);
  if (colour) track_model_colour_host(lg, lo.t.max_jump, md.data(), mc.data(), map.data(), Ym.data());
  else track_model_host(lg, lo.t.max_jump, md.data(), map.data());
  double c_src[3];
  locate_centre_src(lo.t.centre_depth, voxel_size, c_src);
  const AlignEval e = align_eval(map_motion(pose16, voxel_size), c_src, lo.t.a, voxel_size);
  const TrackModel tm = track_model(model_pose16, lo.t, voxel_size, map.data());
  counts[4] = 0;
  if (colour) track_colour_system_host(lg, fc.data(), fd.data(), tm, track_colour(lo, Ym.data()), e, sums, counts);
  else track_system_host(lg, fd.data(), tm, e, sums, counts);
}
// The whole coarse-to-fine tracking on the CPU over a renderer of the FULL-resolution images, render_both(pose16, Cm, Dm): the
// library's reference for drf_track_pyramid_frame (bgr null: geometry only, Cm is not read), and what the sanitizer program runs.
// A round of a level above 0 renders at full resolution, reduces to the level, and from there is track_colour_frame_host's.
// state: null, or the ExposureState of drf_track_exposure_frame (below; bgr is then given): it carries from level to level, and an
// abandoned level hands on the state it started from.
template <class RenderBoth, class State = PoseState>
inline void track_pyramid_frame_host(const LocateGrid &lg0, const unsigned char *bgr, const float *depth, RenderBoth &&render_both, const float *pose_init16,
                                     const TrackPyramidOpt &o, float voxel_size, drf_align_result_t &res, uint64_t stats8[8], uint64_t level4[kTrackMaxLevels][4],
                                     uint64_t *last5 = nullptr, std::vector<std::array<double, 28>> *trace = nullptr, State *state = nullptr) {
  const bool colour = bgr != nullptr;
  const size_t npix0 = (size_t)lg0.W * (size_t)lg0.H;
  std::vector<float> Dm(npix0);
  std::vector<unsigned char> Cm(npix0 * 3);
  std::vector<std::vector<float>> fd((size_t)o.levels);
  std::vector<std::vector<unsigned char>> fc((size_t)o.levels);
  for (int L = 1; L < o.levels; ++L) {  // the frame, reduced once per call
    const LocateGrid lg = track_level_grid(lg0, L);
    fd[L].resize((size_t)lg.W * lg.H);
    fc[L].resize(colour ? (size_t)lg.W * lg.H * 3 : 0);
    track_reduce_host(lg0.W, lg0.H, L, track_level_options(o, L).t.max_jump, bgr, depth, fc[L].data(), fd[L].data());
  }
  track_pyramid_schedule([&](int L, const float *p16, const TrackColourOpt &lo, drf_align_result_t &r, uint64_t *last, uint64_t *st2) {
    const LocateGrid lg = track_level_grid(lg0, L);
    auto render_level = [&](const float *p, unsigned char *Cl, float *Dl) {
      if (L == 0) { render_both(p, colour ? Cl : Cm.data(), Dl); return; }  // the renderer always has a colour image to write
      render_both(p, Cm.data(), Dm.data());
      track_reduce_host(lg0.W, lg0.H, L, lo.t.max_jump, colour ? Cm.data() : nullptr, Dm.data(), Cl, Dl);
    };
    const unsigned char *fbgr = L == 0 ? bgr : fc[L].data();
    const float *fdepth = L == 0 ? depth : fd[L].data();
    if (state) state->level_begin();
    if (colour) track_colour_frame_host<5>(lg, fbgr, fdepth, render_level, p16, lo, voxel_size, r, last, st2, trace, state);
    else track_colour_frame_host<4>(lg, nullptr, fdepth, render_level, p16, lo, voxel_size, r, last, st2, trace);
    if (state && L > 0 && (r.status == DRF_ALIGN_LOST || r.status == DRF_ALIGN_DEGENERATE)) state->level_abandoned();
  }, lg0, pose_init16, o, res, stats8, level4, last5);
}

// ---- tracking under a change of exposure (drf_track_exposure_system / drf_track_exposure_frame; DESIGN.md §7c "Tracking under a
// change of exposure").  Every colour call above takes frame and map to share their exposure; a camera that changes it between
// frames puts the photometric term, and with it the pose, in the wrong place.  These calls solve for two more unknowns beside the
// six of the pose, as the reference's dense tracker does: frame intensity ~ G * (model intensity) + B, gain G and offset B in
// double, B in units of the intensity (the three-channel sum 0..765).  The sample, the association and the geometric term are
// track_sample's, unchanged; the photometric term reads track_photo_model's I and gm and the state; the 8 x 8 system is 45 sums.
// G = 1, B = 0 gives track_photo_term's bits.  Stated once, here; the header of the C ABI restates it.  Compiled by g++ and by
// hipcc (k_track_exposure), both without contraction; + - * / sqrt and floor only -- no exp: G is the gain itself, not its logarithm.
struct TrackExposure { double gain, offset; };  // what an evaluation reads of the state
// track_photo_term's conditions and interpolation up to I and gm, which the term under an exposure is made of: the same operations
// in the same order.  (track_photo_term itself is not written over this function: k_track_colour keeps its instructions and its
// registers only while its text stays as it is -- sharing the lines cost it 12 bytes of scratch.)
DR_HOST_DEVICE inline bool track_photo_model(const TrackColour &tc, const LocateGrid &lg, const double m[3], double up, double vp, double &I, double gm[3]) {
  const double fu = floor(up), fv = floor(vp);
  if (!(fu >= 0.0 && fu + 1.0 <= (double)(lg.W - 1) && fv >= 0.0 && fv + 1.0 <= (double)(lg.H - 1))) return false;
  const size_t at = (size_t)(int)fv * (size_t)lg.W + (size_t)(int)fu;
  TrackPair top, bot;
  memcpy(&top, tc.Ym + at, sizeof top);
  memcpy(&bot, tc.Ym + at + (size_t)lg.W, sizeof bot);
  if (!(top.a >= 0.0f && top.b >= 0.0f && bot.a >= 0.0f && bot.b >= 0.0f)) return false;
  const double y00 = (double)top.a, y10 = (double)top.b, y01 = (double)bot.a, y11 = (double)bot.b;
  const double a = up - fu, b = vp - fv, oa = 1.0 - a, ob = 1.0 - b;
  I = ob * (oa * y00 + a * y10) + b * (oa * y01 + a * y11);
  const double Iu = ob * (y10 - y00) + b * (y11 - y01), Iv = oa * (y01 - y00) + a * (y11 - y10);
  gm[0] = (Iu * (double)lg.fx) / m[2]; gm[1] = (Iv * (double)lg.fy) / m[2];
  gm[2] = -((gm[0] * m[0] + gm[1] * m[1]) / m[2]);
  return true;
}
// The 17 sums of a photometric term beside align_accumulate's 28, from the same J (recomputed by the same operations) and Huber's
// weight: ext[i] += (w J_i) J6 and ext[6 + i] += (w J_i) J7 for the pose's i = 0..5, then H66, H67, H77, b6, b7.  J6 = lambda I is
// dr/dG, J7 = lambda is dr/dB.
DR_HOST_DEVICE inline void exposure_accumulate(const AlignEval &e, double J6, double J7, double r, double n0, double n1, double n2, const double q[3], double ext[17]) {
  const double x0 = q[0] - e.c[0], x1 = q[1] - e.c[1], x2 = q[2] - e.c[2];
  const double J[6] = {x1 * n2 - x2 * n1, x2 * n0 - x0 * n2, x0 * n1 - x1 * n0, n0, n1, n2};
  const double a = r < 0.0 ? -r : r;
  const double w = a <= e.huber ? 1.0 : e.huber / a;
  DR_UNROLL
  for (int i = 0; i < 6; ++i) {
    const double wj = w * J[i];
    ext[i] = ext[i] + wj * J6;
    ext[6 + i] = ext[6 + i] + wj * J7;
  }
  const double w6 = w * J6, w7 = w * J7;
  ext[12] = ext[12] + w6 * J6;
  ext[13] = ext[13] + w6 * J7;
  ext[14] = ext[14] + w7 * J7;
  ext[15] = ext[15] + w6 * r;
  ext[16] = ext[16] + w7 * r;
}
// One sample with colour under the exposure x: track_colour_point's codes and order -- the geometric term first, into acc[0..27]
// alone; then, where track_photo_model has one, the photometric term r = lambda ((G I + B) - yf), n_k = (lambda (Rm gm)_k) G
// through align_accumulate into acc[0..27] and exposure_accumulate into acc[28..44].
DR_HOST_DEVICE inline int track_exposure_point(const AlignEval &e, const TrackModel &t, const TrackColour &tc, const TrackExposure &x, const LocateGrid &lg, double g0,
                                               double g1, double g2, float yf, double acc[45]) {
  return track_sample(e, t, lg, g0, g1, g2, [&](double r, double w0, double w1, double w2, const double *q, const double *m, double up, double vp) {
    double I = 0.0, gm[3] = {0.0, 0.0, 0.0};
    const bool photo = track_photo_model(tc, lg, m, up, vp, I, gm);
    const double pr = tc.weight * ((x.gain * I + x.offset) - (double)yf);
    const double pn[3] = {(tc.weight * ((t.m.R[0] * gm[0] + t.m.R[1] * gm[1]) + t.m.R[2] * gm[2])) * x.gain,
                          (tc.weight * ((t.m.R[3] * gm[0] + t.m.R[4] * gm[1]) + t.m.R[5] * gm[2])) * x.gain,
                          (tc.weight * ((t.m.R[6] * gm[0] + t.m.R[7] * gm[1]) + t.m.R[8] * gm[2])) * x.gain};
    const int terms = photo ? 2 : 1;
    DR_NO_UNROLL
    for (int k = 0; k < terms; ++k) {
      const bool second = k == 1;
      align_accumulate(e, second ? pr : r, second ? pn[0] : w0, second ? pn[1] : w1, second ? pn[2] : w2, q, acc);
    }
    if (photo) exposure_accumulate(e, tc.weight * I, tc.weight, pr, pn[0], pn[1], pn[2], q, acc + 28);
    return photo ? 3 : 1;
  });
}
// The system at one pose and exposure over the whole sample grid: sums[45] = the pose system in drf_track_colour_system's layout
// ([27] the cost of both terms), then the 17 sums; counts[5] are drf_track_colour_system's.
inline void track_exposure_system_host(const LocateGrid &lg, const unsigned char *bgr, const float *depth, const TrackModel &t, const TrackColour &tc,
                                       const TrackExposure &x, const AlignEval &e, double sums[45], uint64_t counts[5]) {
  frame_system_host<5, 45>(lg, depth, e, [&](int n, const double *g, double *acc) {
    return track_exposure_point(e, t, tc, x, lg, g[0], g[1], g[2], track_intensity(bgr + 3 * locate_offset(lg, n)), acc);
  }, track_colour_count, sums, counts);
}
struct TrackExposureOpt {  // drf_track_exposure_options_t with its defaults resolved
  TrackPyramidOpt p;
  double gain_init, offset_init, gain_min, gain_max, eps_gain, eps_offset;
};
constexpr double kExposureOffsetMax = 765.0;
// null: all defaults.  Returns null, or which option is refused: the pyramid options' own first (levels = 1 on any camera); then gain_init, offset_init,
// gain_min, gain_max, eps_gain, eps_offset where one is negative (not offset_init) or not finite; then gain_min (above gain_max),
// gain_init (outside the bounds), offset_init (beyond +-765).
// Level 0 is the camera itself and fits a camera of any size, as for drf_track_colour_*: with levels = 1 the rule of 8 pixels on
// a side, which binds the levels above 0, refuses nothing (track_exposure_level_fits is the same for a system's level).
inline bool track_exposure_level_fits(int W, int H, int L) { return L == 0 || track_level_fits(W, H, L); }
inline const char *track_exposure_options(const drf_track_exposure_options_t *opt, float voxel_size, int W, int H, TrackExposureOpt &o) {
  const bool single = opt && opt->pyramid.levels == 1;
  if (const char *bad = track_pyramid_options(opt ? &opt->pyramid : nullptr, voxel_size, single ? std::max(W, kTrackMinLevelSide) : W,
                                              single ? std::max(H, kTrackMinLevelSide) : H, o.p))
    return bad;
  static const drf_track_exposure_options_t zero = {};
  const drf_track_exposure_options_t &u = opt ? *opt : zero;
  if (!(u.gain_init >= 0.0f) || !std::isfinite(u.gain_init)) return "gain_init";
  if (!std::isfinite(u.offset_init)) return "offset_init";
  if (!(u.gain_min >= 0.0f) || !std::isfinite(u.gain_min)) return "gain_min";
  if (!(u.gain_max >= 0.0f) || !std::isfinite(u.gain_max)) return "gain_max";
  if (!(u.eps_gain >= 0.0) || !std::isfinite(u.eps_gain)) return "eps_gain";
  if (!(u.eps_offset >= 0.0) || !std::isfinite(u.eps_offset)) return "eps_offset";
  o.gain_init = u.gain_init != 0.0f ? (double)u.gain_init : 1.0;
  o.offset_init = (double)u.offset_init;
  o.gain_min = u.gain_min != 0.0f ? (double)u.gain_min : 0.25;
  o.gain_max = u.gain_max != 0.0f ? (double)u.gain_max : 4.0;
  o.eps_gain = u.eps_gain != 0.0 ? u.eps_gain : 1e-4;
  o.eps_offset = u.eps_offset != 0.0 ? u.eps_offset : 1e-2;
  if (o.gain_min > o.gain_max) return "gain_min";
  if (o.gain_init < o.gain_min || o.gain_init > o.gain_max) return "gain_init";
  if (o.offset_init < -kExposureOffsetMax || o.offset_init > kExposureOffsetMax) return "offset_init";
  return nullptr;
}
// What the loops hold beside the pose (PoseState's interface): G and B, the 17 sums of the last evaluation -- an evaluator leaves
// them in ext next to the 28 it hands the loop -- the bounds and thresholds, and how many evaluations held the exposure.
struct ExposureState {
  double gain = 1.0, offset = 0.0, ext[17] = {};
  double gain_min = 0.25, gain_max = 4.0, eps_gain = 1e-4, eps_offset = 1e-2;
  uint64_t held = 0;
  double good[2] = {1.0, 0.0}, level[2] = {1.0, 0.0};
  ExposureState() = default;
  explicit ExposureState(const TrackExposureOpt &o)
      : gain(o.gain_init), offset(o.offset_init), gain_min(o.gain_min), gain_max(o.gain_max), eps_gain(o.eps_gain), eps_offset(o.eps_offset) {}
  TrackExposure at() const { return {gain, offset}; }
  void keep() { good[0] = gain; good[1] = offset; }
  void back() { gain = good[0]; offset = good[1]; }
  void level_begin() { level[0] = gain; level[1] = offset; }
  void level_abandoned() { gain = level[0]; offset = level[1]; }
  inline int step(const double sums[28], const double c[3], double eps_rot, double eps_trans, MapMotion &m);
  void evaluate_host(const LocateGrid &lg, const unsigned char *bgr, const float *depth, const TrackModel &t, const TrackColour &tc, const AlignEval &e, double sums[28],
                     uint64_t counts[5]) {
    double s45[45];
    track_exposure_system_host(lg, bgr, depth, t, tc, at(), e, s45, counts);
    memcpy(sums, s45, 28 * sizeof(double));
    memcpy(ext, s45 + 28, sizeof ext);
  }
};
// One Gauss-Newton step of the 8 x 8 system from sums[45] at pose m and exposure (G, B).  H is the pose block of sums[0..20], the
// columns H(i,6) = sums[28 + i], H(i,7) = sums[34 + i], H66, H67, H77 = sums[40..42]; b = sums[21..26], sums[43], sums[44].
// align_solve's pivot test with top over the 8 diagonals: a failing pivot 0..5 is DRF_ALIGN_DEGENERATE; a failing pivot 6 or 7
// HOLDS the exposure -- a map of one colour, or no photometric term: the step is align_step on sums[0..27] as it stands, G and B
// keep their values, held goes up.  Otherwise: a NaN in d is DEGENERATE; CONVERGED (not applied) needs the rotation and the
// translation below their thresholds, |d6| < eps_gain and |d7| < eps_offset; any other step moves the pose as align_step does,
// G = min(max(G + d6, gain_min), gain_max), B = min(max(B + d7, -765), 765), and returns -1.
inline int exposure_step(const double sums[45], const double c[3], double eps_rot, double eps_trans, ExposureState &x, MapMotion &m) {
  double H[8][8], b[8], d[8];
  int idx = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { H[i][j] = sums[idx]; H[j][i] = sums[idx]; ++idx; }
  for (int i = 0; i < 6; ++i) {
    H[i][6] = H[6][i] = sums[28 + i];
    H[i][7] = H[7][i] = sums[34 + i];
    b[i] = sums[21 + i];
  }
  H[6][6] = sums[40]; H[6][7] = H[7][6] = sums[41]; H[7][7] = sums[42];
  b[6] = sums[43]; b[7] = sums[44];
  double top = H[0][0];
  for (int j = 1; j < 8; ++j) top = H[j][j] > top ? H[j][j] : top;
  if (!(top > 0.0)) return DRF_ALIGN_DEGENERATE;
  const int failed = align_solve<8>(H, b, top, d);
  if (failed >= 6) { ++x.held; return align_step(sums, c, eps_rot, eps_trans, m); }
  if (failed >= 0) return DRF_ALIGN_DEGENERATE;
  const double oo = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], vv = (d[3] * d[3] + d[4] * d[4]) + d[5] * d[5];
  if (!(oo == oo) || !(vv == vv) || !(d[6] == d[6]) || !(d[7] == d[7])) return DRF_ALIGN_DEGENERATE;
  const double a6 = d[6] < 0.0 ? -d[6] : d[6], a7 = d[7] < 0.0 ? -d[7] : d[7];
  if (std::sqrt(oo) < eps_rot && std::sqrt(vv) < eps_trans && a6 < x.eps_gain && a7 < x.eps_offset) return DRF_ALIGN_CONVERGED;
  align_move(d, oo, c, m);
  const double G = x.gain + d[6], B = x.offset + d[7];
  x.gain = std::min(std::max(G, x.gain_min), x.gain_max);
  x.offset = std::min(std::max(B, -kExposureOffsetMax), kExposureOffsetMax);
  return -1;
}
inline int ExposureState::step(const double sums[28], const double c[3], double eps_rot, double eps_trans, MapMotion &m) {
  double s45[45];
  memcpy(s45, sums, 28 * sizeof(double));
  memcpy(s45 + 28, ext, sizeof ext);
  return exposure_step(s45, c, eps_rot, eps_trans, *this, m);
}
// the call's result from level 0's and the state it ended in
inline void exposure_result(const drf_align_result_t &pose, const ExposureState &x, const uint64_t last5[5], drf_exposure_result_t &res) {
  res.pose = pose;
  res.gain = x.gain; res.offset = x.offset;
  memcpy(res.ext, x.ext, sizeof res.ext);
  res.photometric = last5[4]; res.held = x.held;
}
// One evaluation at level L on the CPU: track_pyramid_system_host's reductions and model map, then the system above.
inline void track_exposure_system_at_host(const LocateGrid &lg0, int L, const unsigned char *bgr, const float *depth, const unsigned char *model_bgr,
                                          const float *model_depth, const float *model_pose16, const float *pose16, double gain, double offset, const TrackExposureOpt &o,
                                          float voxel_size, double sums[45], uint64_t counts[5]) {
  const TrackColourOpt lo = track_level_options(o.p, L);
  const LocateGrid lg = track_level_grid(lg0, L);
  const size_t npix = (size_t)lg.W * (size_t)lg.H;
  std::vector<float> fd(npix), md(npix), Ym(npix);
  std::vector<unsigned char> fc(3 * npix), mc(3 * npix);
  track_reduce_host(lg0.W, lg0.H, L, lo.t.max_jump, bgr, depth, fc.data(), fd.data());
  track_reduce_host(lg0.W, lg0.H, L, lo.t.max_jump, model_bgr, model_depth, mc.data(), md.data());
  std::vector<TrackPixel> map(npix);
  track_model_colour_host(lg, lo.t.max_jump, md.data(), mc.data(), map.data(), Ym.data());
  double c_src[3];
  locate_centre_src(lo.t.centre_depth, voxel_size, c_src);
  const AlignEval e = align_eval(map_motion(pose16, voxel_size), c_src, lo.t.a, voxel_size);
  track_exposure_system_host(lg, fc.data(), fd.data(), track_model(model_pose16, lo.t, voxel_size, map.data()), track_colour(lo, Ym.data()), {gain, offset}, e, sums, counts);
}
// The whole tracking on the CPU over a renderer of the full-resolution images: track_pyramid_frame_host with the exposure as the
// solver's state -- the library's reference for drf_track_exposure_frame, and what the sanitizer program runs.
template <class RenderBoth>
inline void track_exposure_frame_host(const LocateGrid &lg0, const unsigned char *bgr, const float *depth, RenderBoth &&render_both, const float *pose_init16,
                                      const TrackExposureOpt &o, float voxel_size, drf_exposure_result_t &res, uint64_t stats8[8], uint64_t level4[kTrackMaxLevels][4],
                                      std::vector<std::array<double, 28>> *trace = nullptr) {
  ExposureState x(o);
  drf_align_result_t r;
  uint64_t last5[5] = {0, 0, 0, 0, 0};
  track_pyramid_frame_host(lg0, bgr, depth, render_both, pose_init16, o.p, voxel_size, r, stats8, level4, last5, trace, &x);
  exposure_result(r, x, last5, res);
}

// ---- searching a pose lattice (drf_score_poses / drf_search_frame; DESIGN.md §7c "Searching a pose lattice").  Every call above
// refines; the guess they start from is found here: one evaluation of the localisation WITHOUT its Jacobian at each of 10^4..10^6
// poses of one depth image, the best few handed to track_loop and locate_loop as they stand.  The per-sample rule is align_point<true>'s
// with s_src = 0, word for word up to phi -- grid, sample test, point, q, corners, trilinear fp32 phi, the three codes, r, Huber's w --
// and keeps acc[27] alone.  Stated once, here; the header of the C ABI restates it.  Compiled by g++ and by hipcc (k_search_points,
// k_search_score), both without contraction; + - * / and floor only.  No trigonometry: rotations are data.
// The colour family (ScoreColourOpt, SearchColourOpt, below) runs the same text: what is written once for both is a template over
// the options, which say their family (colour) and hand out the part the other family consists of (geo, search, score).
struct ScoreOpt {  // drf_score_options_t with its defaults resolved
  static constexpr bool colour = false;
  int step, min_weight;
  float band, huber;
  double oc, uc;  // voxels per OUTSIDE / UNOBSERVED sample
  DR_HOST_DEVICE const ScoreOpt &geo() const { return *this; }
};
// null: all defaults.  Returns null, or which option is negative or not finite
inline const char *score_options(const drf_score_options_t *opt, float truncation_distance, float voxel_size, ScoreOpt &o) {
  static const drf_score_options_t zero = {0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
  const drf_score_options_t &u = opt ? *opt : zero;
  if (u.step < 0) return "step";
  if (u.min_weight < 0) return "min_weight";
  if (!(u.band >= 0.0f) || !std::isfinite(u.band)) return "band";
  if (!(u.huber >= 0.0f) || !std::isfinite(u.huber)) return "huber";
  if (!(u.outside_cost >= 0.0f) || !std::isfinite(u.outside_cost)) return "outside_cost";
  if (!(u.unobserved_cost >= 0.0f) || !std::isfinite(u.unobserved_cost)) return "unobserved_cost";
  o.step = u.step ? u.step : 4;
  o.min_weight = u.min_weight ? u.min_weight : 1;
  o.band = u.band != 0.0f ? u.band : truncation_distance;
  o.huber = u.huber != 0.0f ? u.huber : 1.0f;
  o.oc = u.outside_cost != 0.0f ? (double)u.outside_cost : (double)o.huber * ((double)o.band / (double)voxel_size);  // Huber's value at the band's edge
  o.uc = u.unobserved_cost != 0.0f ? (double)u.unobserved_cost : 2.0 * o.oc;
  return nullptr;
}
// what score_sample reads of an AlignEval: the pose, huber, vs, band, min_weight (there is no centre: nothing turns)
DR_HOST_DEVICE inline AlignEval score_eval(const MapMotion &m, const ScoreOpt &o, double vs) {
  AlignEval e;
  e.m = m;
  e.c[0] = 0.0; e.c[1] = 0.0; e.c[2] = 0.0;
  e.huber = (double)o.huber; e.vs = vs;
  e.band = o.band; e.min_weight = o.min_weight;
  return e;
}
// One sample at the camera-frame point g, the one text of both families: align_point<true> with s_src = 0 up to phi, its codes
// (0 UNOBSERVED, 2 OUTSIDE, 1 valid), and of its sums the last: cost = cost + (w r) r.  With colour (Opt::colour; yf is the frame's
// intensity at the sample) the colour bytes of the eight corners are kept, and a valid sample adds the colour term behind the
// geometric one: y[c] = the intensity of corner c's three bytes (bits 0-7, 8-15, 16-23 of its second word), Ym their fp32 trilinear
// interpolant in phi's stages and order with the same f, rp = lambda (Ym - yf) in double, Huber's weight with the geometric huber,
// the term capped at pc.  Without colour o, yf and photo are not touched.
template <class Opt, class Fetch>
DR_HOST_DEVICE inline int score_sample(const AlignEval &e, const Opt &o, double g0, double g1, double g2, float yf, Fetch &&fetch, double &cost, double &photo) {
  int b[3];
  float f[3];
  DR_UNROLL
  for (int k = 0; k < 3; ++k) {
    const double q = ((e.m.R[3 * k] * g0 + e.m.R[3 * k + 1] * g1) + e.m.R[3 * k + 2] * g2) + e.m.tv[k];
    if (!(q > -1073741824.0 && q < 1073741824.0)) return 0;
    const double fl = floor(q);
    b[k] = (int)fl;
    f[k] = (float)(q - fl);
  }
  float s[8];  // index 4 cx + 2 cy + cz
  [[maybe_unused]] uint32_t col[8];
  DR_UNROLL
  for (int c = 0; c < 8; ++c) {
    uint32_t v[2];
    fetch(b[0] + (c >> 2), b[1] + ((c >> 1) & 1), b[2] + (c & 1), v);
    if ((int)(v[1] >> 24) < e.min_weight) return 0;
    memcpy(&s[c], &v[0], 4);
    if constexpr (Opt::colour) col[c] = v[1];
  }
  float ez[4];  // index 2 cx + cy
  DR_UNROLL
  for (int c = 0; c < 4; ++c) ez[c] = s[2 * c] + f[2] * (s[2 * c + 1] - s[2 * c]);
  float d[2];
  DR_UNROLL
  for (int c = 0; c < 2; ++c) d[c] = ez[2 * c] + f[1] * (ez[2 * c + 1] - ez[2 * c]);
  const float phi = d[0] + f[0] * (d[1] - d[0]);
  const float ap = phi < 0.0f ? -phi : phi;
  if (!(ap < e.band)) return 2;
  const double r = (double)phi / e.vs;  // align_point's ((double)phi - (double)s_src) / vs with s_src = 0: the same bits
  const double a = r < 0.0 ? -r : r;
  const double w = a <= e.huber ? 1.0 : e.huber / a;
  cost = cost + (w * r) * r;
  if constexpr (Opt::colour) {
    float y[8];
    DR_UNROLL
    for (int c = 0; c < 8; ++c) y[c] = ((float)(col[c] & 255u) + (float)((col[c] >> 8) & 255u)) + (float)((col[c] >> 16) & 255u);
    float yz[4];
    DR_UNROLL
    for (int c = 0; c < 4; ++c) yz[c] = y[2 * c] + f[2] * (y[2 * c + 1] - y[2 * c]);
    float yd[2];
    DR_UNROLL
    for (int c = 0; c < 2; ++c) yd[c] = yz[2 * c] + f[1] * (yz[2 * c + 1] - yz[2 * c]);
    const float Ym = yd[0] + f[0] * (yd[1] - yd[0]);
    const double rp = o.lambda * ((double)Ym - (double)yf);
    const double app = rp < 0.0 ? -rp : rp;
    const double wp = app <= e.huber ? 1.0 : e.huber / app;
    double tp = (wp * rp) * rp;
    if (tp > o.pc) tp = o.pc;
    photo = photo + tp;
  }
  return 1;
}
// the geometric sample by itself: what tests/cpp/map_search_check.cpp holds to align_point<true>
template <class Fetch>
DR_HOST_DEVICE inline int score_point(const AlignEval &e, double g0, double g1, double g2, Fetch &&fetch, double &cost) {
  double none = 0.0;
  return score_sample(e, ScoreOpt{}, g0, g1, g2, 0.0f, fetch, cost, none);
}// score = ((cost + oc outside) + uc unobserved) / samples in double, in that order; no sample: uc.  Lower is better.
DR_HOST_DEVICE inline double score_value(double cost, uint32_t samples, uint32_t unobserved, uint32_t outside, double oc, double uc) {
  if (samples == 0) return uc;
  return ((cost + oc * (double)outside) + uc * (double)unobserved) / (double)samples;
}
// The candidates of a call.  plain (drf_score_poses): candidate c is entry c of the pose table, as it stands.  Otherwise
// (drf_search_frame) c = (((a n_rot + r) Nx + ix) Ny + iy) Nz + iz, N = 2 half + 1: entry a n_rot + r of the table holds (Rd, ta) --
// 12 doubles, Rd row-major, then ta in lattice units -- and tv_k = ta_k + (double)(i_k - half_k) * dstep, dstep =
// (double)trans_step / vs.  The kernel decodes the index with this very function.
struct SearchLattice {
  int N[3], half[3];
  double dstep;
  int plain;
};
inline size_t search_cells(const SearchLattice &L) { return (size_t)L.N[0] * (size_t)L.N[1] * (size_t)L.N[2]; }
DR_HOST_DEVICE inline MapMotion search_candidate(const SearchLattice &L, const double *table, size_t table_first, size_t c) {
  MapMotion m;
  size_t ar = c;
  int off[3] = {0, 0, 0};
  if (!L.plain) {
    const size_t iz = c % (size_t)L.N[2], cy = c / (size_t)L.N[2];
    const size_t iy = cy % (size_t)L.N[1], cx = cy / (size_t)L.N[1];
    const size_t ix = cx % (size_t)L.N[0];
    ar = cx / (size_t)L.N[0];
    off[0] = (int)ix - L.half[0]; off[1] = (int)iy - L.half[1]; off[2] = (int)iz - L.half[2];
  }
  const double *t = table + 12 * (ar - table_first);
  DR_UNROLL
  for (int i = 0; i < 9; ++i) m.R[i] = t[i];
  DR_UNROLL
  for (int k = 0; k < 3; ++k) m.tv[k] = L.plain ? t[9 + k] : t[9 + k] + (double)off[k] * L.dstep;
  return m;
}
// The pose table of a search: per (anchor a, rotation r) Rd = Rr Ra, each entry (Rr[i][0] Ra[0][j] + Rr[i][1] Ra[1][j]) +
// Rr[i][2] Ra[2][j] -- a turn about the world axes through the camera centre -- and ta, the anchor's translation in lattice units,
// (Ra, ta) read from the anchor as every pose is read (map_motion).  Returns an empty string, or what is refused: an anchor, a
// rotation (as a pose with no translation) or a product (as locate_pose16 makes it a pose16) that transform_pose_fault refuses.
inline std::string search_table(const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot, float voxel_size, std::vector<double> &table) {
  table.assign(n_anchors * n_rot * 12, 0.0);
  for (size_t a = 0; a < n_anchors; ++a)
    if (const char *why = transform_pose_fault(anchors16 + 16 * a)) return "anchor " + std::to_string(a) + " " + why;
  for (size_t r = 0; r < n_rot; ++r) {
    float T[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)rotations9[9 * r + 3 * i + j];
    if (const char *why = transform_pose_fault(T)) return "rotation " + std::to_string(r) + " " + why;
  }
  for (size_t a = 0; a < n_anchors; ++a) {
    const MapMotion ma = map_motion(anchors16 + 16 * a, voxel_size);
    for (size_t r = 0; r < n_rot; ++r) {
      const double *Rr = rotations9 + 9 * r;
      MapMotion m = ma;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m.R[3 * i + j] = (Rr[3 * i] * ma.R[j] + Rr[3 * i + 1] * ma.R[3 + j]) + Rr[3 * i + 2] * ma.R[6 + j];
      float T[16];
      locate_pose16(m, voxel_size, T);
      if (const char *why = transform_pose_fault(T)) return "rotation " + std::to_string(r) + " applied to anchor " + std::to_string(a) + " " + why;
      double *t = &table[(a * n_rot + r) * 12];
      memcpy(t, m.R, 72);
      memcpy(t + 9, m.tv, 24);
    }
  }
  return std::string();
}
struct SearchOpt {  // drf_search_options_t with its defaults resolved
  static constexpr bool colour = false;
  ScoreOpt s;
  SearchLattice L;
  int top_k;
  bool score_only;
  double accept_valid;
  const SearchOpt &search() const { return *this; }
  const ScoreOpt &score() const { return s; }
};
constexpr size_t kSearchMaxCandidates = (size_t)1 << 24;
// null: all defaults (half = 0 0 0: the anchors turned, not moved).  Returns null, or which option is refused
inline const char *search_options(const drf_search_options_t *opt, float truncation_distance, float voxel_size, SearchOpt &o) {
  static const drf_search_options_t zero = {{0, 0, 0.0f, 0.0f, 0.0f, 0.0f}, 0.0f, {0, 0, 0}, 0, 0, 0.0};
  const drf_search_options_t &u = opt ? *opt : zero;
  if (const char *bad = score_options(&u.score, truncation_distance, voxel_size, o.s)) return bad;
  if (!(u.trans_step >= 0.0f) || !std::isfinite(u.trans_step)) return "trans_step";
  for (int k = 0; k < 3; ++k)
    if (u.half[k] < 0 || u.half[k] > (1 << 20)) return "half";
  if (u.top_k < 0 || u.top_k > DRF_SEARCH_MAX_TOP) return "top_k";
  if (u.score_only < 0 || u.score_only > 1) return "score_only";
  if (!(u.accept_valid >= 0.0) || !std::isfinite(u.accept_valid)) return "accept_valid";
  const float ts = u.trans_step != 0.0f ? u.trans_step : 2.0f * truncation_distance;
  for (int k = 0; k < 3; ++k) { o.L.half[k] = u.half[k]; o.L.N[k] = 2 * u.half[k] + 1; }
  o.L.dstep = (double)ts / (double)voxel_size;
  o.L.plain = 0;
  o.top_k = u.top_k ? u.top_k : 8;
  o.score_only = u.score_only != 0;
  o.accept_valid = u.accept_valid;
  return nullptr;
}
// n_anchors * n_rot * Nx * Ny * Nz, or 0 if that is no count a call takes: zero, or above 2^24
inline size_t search_count(size_t n_anchors, size_t n_rot, const SearchLattice &L) {
  size_t n = 1;
  for (size_t f : {n_anchors, n_rot, (size_t)L.N[0], (size_t)L.N[1], (size_t)L.N[2]}) {
    if (f == 0 || f > kSearchMaxCandidates) return 0;
    n *= f;
    if (n > kSearchMaxCandidates) return 0;
  }
  return n;
}
// The top_k smallest scores, ties to the lower index, a NaN score behind every number: the indices in rank order
inline std::vector<size_t> search_select(const double *score, size_t n, int top_k) {
  std::vector<size_t> idx(n);
  for (size_t i = 0; i < n; ++i) idx[i] = i;
  const size_t k = std::min(n, (size_t)top_k);
  auto key = [&](size_t i) { return score[i] == score[i] ? score[i] : HUGE_VAL; };
  std::partial_sort(idx.begin(), idx.begin() + k, idx.end(), [&](size_t a, size_t b) { return key(a) < key(b) || (key(a) == key(b) && a < b); });
  idx.resize(k);
  return idx;
}

// ---- searching with colour (drf_score_colour_poses / drf_search_colour_frame; DESIGN.md §7c "Searching with colour").  The score
// above is geometric: on one wall every in-plane offset of the lattice scores alike.  Every voxel carries a colour, and the fetch
// of a corner already returns it as the second word of its load; the colour score keeps those bytes and adds an appearance term
// per valid sample -- the trilinear model intensity against the frame's pixel -- into a second sum, photo, reduced exactly as cost
// is.  cost and counts keep drf_score_poses' bits.  Frame and map share their exposure, as for drf_track_colour_* (drf_track_exposure_* solve for it).
struct ScoreColourOpt {  // drf_score_colour_options_t with its defaults resolved
  static constexpr bool colour = true;
  ScoreOpt s;
  float photo_weight;  // voxels per intensity unit
  double lambda, pc;   // (double)photo_weight; the most one sample's colour term costs
  DR_HOST_DEVICE const ScoreOpt &geo() const { return s; }
};
// the two colour fields behind a resolved ScoreOpt.  Returns null, or which is negative or not finite
inline const char *score_photo_options(float photo_weight, float photo_cap, const ScoreOpt &s, ScoreColourOpt &o) {
  if (!(photo_weight >= 0.0f) || !std::isfinite(photo_weight)) return "photo_weight";
  if (!(photo_cap >= 0.0f) || !std::isfinite(photo_cap)) return "photo_cap";
  o.s = s;
  o.photo_weight = photo_weight != 0.0f ? photo_weight : (float)(1.0 / 27.0) * s.huber;  // track_colour_options' default, for its reason
  o.lambda = (double)o.photo_weight;
  o.pc = photo_cap != 0.0f ? (double)photo_cap : s.oc;
  return nullptr;
}
// null: all defaults.  The score options' own refusals first
inline const char *score_colour_options(const drf_score_colour_options_t *opt, float truncation_distance, float voxel_size, ScoreColourOpt &o) {
  ScoreOpt s{};
  if (const char *bad = score_options(opt ? &opt->score : nullptr, truncation_distance, voxel_size, s)) return bad;
  return score_photo_options(opt ? opt->photo_weight : 0.0f, opt ? opt->photo_cap : 0.0f, s, o);
}
struct SearchColourOpt {  // drf_search_colour_options_t with its defaults resolved
  static constexpr bool colour = true;
  SearchOpt s;
  ScoreColourOpt c;
  const SearchOpt &search() const { return s; }
  const ScoreColourOpt &score() const { return c; }
};
inline const char *search_colour_options(const drf_search_colour_options_t *opt, float truncation_distance, float voxel_size, SearchColourOpt &o) {
  if (const char *bad = search_options(opt ? &opt->search : nullptr, truncation_distance, voxel_size, o.s)) return bad;
  return score_photo_options(opt ? opt->photo_weight : 0.0f, opt ? opt->photo_cap : 0.0f, o.s.s, o.c);
}
// (((cost + photo) + oc outside) + uc unobserved) / samples in double, in that order; no sample: uc
DR_HOST_DEVICE inline double score_colour_value(double cost, double photo, uint32_t samples, uint32_t unobserved, uint32_t outside, double oc, double uc) {
  if (samples == 0) return uc;
  return (((cost + photo) + oc * (double)outside) + uc * (double)unobserved) / (double)samples;
}
// either score, by the family of the options
template <class Opt>
DR_HOST_DEVICE inline double score_of(const Opt &o, double cost, double photo, uint32_t samples, uint32_t unobserved, uint32_t outside) {
  if constexpr (Opt::colour) return score_colour_value(cost, photo, samples, unobserved, outside, o.s.oc, o.s.uc);
  else return score_value(cost, samples, unobserved, outside, o.oc, o.uc);
}

// ---- what both families run (Opt: ScoreOpt or ScoreColourOpt, SearchOpt or SearchColourOpt)
// k_search_points(_colour) on the host: per grid position of the groups (512 each, the last padded) its point g, locate_pixel's
// bits, and whether it is a sample; given bgr, per position also the frame intensity yf -- track_intensity of the sample's own
// pixel, 0 where the position is no sample.  bgr null (the geometric form): yf is empty.
struct SearchPoints {
  std::vector<double> g;  // 3 per position
  std::vector<unsigned char> flag;
  std::vector<float> yf;
};
inline void search_points_host(const LocateGrid &lg, double vs, const unsigned char *bgr, const float *depth, SearchPoints &p) {
  const long total = locate_positions(lg), padded = 512 * locate_groups(lg);
  p.g.assign((size_t)padded * 3, 0.0);
  p.flag.assign((size_t)padded, 0);
  p.yf.assign(bgr ? (size_t)padded : 0, 0.0f);
  for (long n = 0; n < total; ++n) {
    p.flag[n] = locate_pixel(lg, vs, (int)n, depth, &p.g[3 * n]) ? 1 : 0;
    if (bgr && p.flag[n]) p.yf[n] = track_intensity(bgr + 3 * locate_offset(lg, (int)n));
  }
}
// k_search_score(_colour)'s wave on the host: the groups in order, lane l on positions 512 i + l + 64 k, per sum (cost; with colour
// also photo) one double per lane, the butterfly, partial i added in ascending i by lane i % 64 from +0.0, the butterfly again:
// every sum in the one order.  sums = {cost, photo} (photo untouched without colour), counts = {samples, valid, unobserved,
// outside}.  cost and counts: bit for bit sums[27] and the counts of locate_system_host at the same pose and options.
template <class Opt, class Fetch>
inline void score_candidate_host(long groups, const SearchPoints &p, Fetch &&fetch, const AlignEval &e, const Opt &o, double sums[2], uint32_t counts[4]) {
  constexpr int NS = Opt::colour ? 2 : 1;
  auto butterfly = [](double x[64]) {
    for (int off = 32; off > 0; off >>= 1) {
      double y[64];
      for (int l = 0; l < 64; ++l) y[l] = x[l] + x[l ^ off];
      memcpy(x, y, sizeof y);
    }
  };
  double fold[NS][64];
  for (int s = 0; s < NS; ++s)
    for (int l = 0; l < 64; ++l) fold[s][l] = 0.0;
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  for (long i = 0; i < groups; ++i) {
    double x[2][64];
    for (int l = 0; l < 64; ++l) {
      x[0][l] = x[1][l] = 0.0;
      for (int k = 0; k < 8; ++k) {
        const size_t n = (size_t)(512 * i + l + 64 * k);
        if (!p.flag[n]) continue;
        ++counts[0];
        const int r = score_sample(e, o, p.g[3 * n], p.g[3 * n + 1], p.g[3 * n + 2], Opt::colour ? p.yf[n] : 0.0f, fetch, x[0][l], x[1][l]);
        ++counts[r == 1 ? 1 : r == 0 ? 2 : 3];
      }
    }
    for (int s = 0; s < NS; ++s) {
      butterfly(x[s]);
      fold[s][i & 63] = fold[s][i & 63] + x[s][0];
    }
  }
  for (int s = 0; s < NS; ++s) {
    butterfly(fold[s]);
    sums[s] = fold[s][0];
  }
}
// The score calls and the score stage of the searches on the CPU: candidates [0, n) of the lattice over the table.  Without colour
// bgr is not read and photo not written (both may be null).
template <class Opt, class Fetch>
inline void score_candidates_host(const LocateGrid &lg, const unsigned char *bgr, const float *depth, Fetch &&fetch, const SearchLattice &L, const double *table, size_t n,
                                  const Opt &o, float voxel_size, double *cost, double *photo, uint32_t *counts, double *score) {
  SearchPoints p;
  search_points_host(lg, (double)voxel_size, Opt::colour ? bgr : nullptr, depth, p);
  for (size_t c = 0; c < n; ++c) {
    const AlignEval e = score_eval(search_candidate(L, table, 0, c), o.geo(), (double)voxel_size);
    double sums[2] = {0.0, 0.0};
    score_candidate_host(locate_groups(lg), p, fetch, e, o, sums, counts + 4 * c);
    cost[c] = sums[0];
    if (Opt::colour) photo[c] = sums[1];
    score[c] = score_of(o, sums[0], sums[1], counts[4 * c], counts[4 * c + 2], counts[4 * c + 3]);
  }
}
// What follows the score stage of either search, over track(p16, res) and locate(p16, res), the *_frame calls' loops from a float
// pose (with colour the tracking is the pyramid's with the frame's bgr): the entries of the selected candidates (photo: with colour
// only), then each refined in rank order -- tracked from its float pose (locate_pose16 of its (Rd, tv)); if that ends <= MAX_ITERS,
// located from the tracked pose rounded to float.  An entry QUALIFIES if its locate status is <= MAX_ITERS.  accept_valid > 0 ends
// the refinement at the first qualifying entry whose located valid >= accept_valid * samples: it wins.  Otherwise the winner is
// winner(res, qual, nq)'s, the family's rule over the nq >= 1 qualifying entries in rank order (search_winner,
// search_colour_winner; it runs in either case).  None qualifies (or score_only): pose16_out is the best-scoring candidate's float
// pose, status LOST (score_only: MAX_ITERS, winner 0).
template <class Opt, class Result, class Track, class Locate, class Winner>
inline void search_refine(const Opt &opt, const double *table, const std::vector<size_t> &sel, const double *cost, const double *photo, const uint32_t *counts,
                          const double *score, size_t n_candidates, float voxel_size, Track &&track, Locate &&locate, Winner &&winner, float pose16_out[16], Result &res) {
  const SearchOpt &o = opt.search();
  memset(&res, 0, sizeof res);
  res.n_candidates = n_candidates;
  res.n_entries = (int)sel.size();
  res.winner = -1;
  float p16[DRF_SEARCH_MAX_TOP][16];
  for (size_t k = 0; k < sel.size(); ++k) {
    auto &en = res.entries[k];
    const size_t c = sel[k];
    en.index = c; en.score = score[c]; en.cost = cost[c];
    if constexpr (Opt::colour) en.photo = photo[c];
    for (int i = 0; i < 4; ++i) en.counts[i] = counts[4 * c + i];
    en.track_status = en.locate_status = -1;
    locate_pose16(search_candidate(o.L, table, 0, c), voxel_size, p16[k]);
    for (int i = 0; i < 16; ++i) en.T[i] = (double)p16[k][i];
  }
  memcpy(pose16_out, p16[0], sizeof p16[0]);
  if (o.score_only) { res.status = DRF_ALIGN_MAX_ITERS; res.winner = 0; return; }
  res.status = DRF_ALIGN_LOST;
  int accepted = -1, qual[DRF_SEARCH_MAX_TOP], nq = 0;
  for (size_t k = 0; k < sel.size(); ++k) {
    auto &en = res.entries[k];
    drf_align_result_t r;
    track(p16[k], r);
    ++res.refined;
    en.track_status = r.status;
    memcpy(en.T, r.T, sizeof en.T);
    if (r.status > DRF_ALIGN_MAX_ITERS) continue;
    float t16[16];
    for (int i = 0; i < 16; ++i) t16[i] = (float)r.T[i];
    locate(t16, r);
    en.locate_status = r.status;
    en.samples = r.samples; en.valid = r.valid; en.located_cost = r.cost;
    memcpy(en.T, r.T, sizeof en.T);
    if (r.status > DRF_ALIGN_MAX_ITERS) continue;
    qual[nq++] = (int)k;
    if (o.accept_valid > 0.0 && (double)en.valid >= o.accept_valid * (double)en.samples) { accepted = (int)k; break; }
  }
  if (nq == 0) return;
  res.winner = winner(res, qual, nq);
  if (accepted >= 0) res.winner = accepted;
  res.status = res.entries[res.winner].locate_status;
  for (int i = 0; i < 16; ++i) pose16_out[i] = (float)res.entries[res.winner].T[i];
}
// drf_search_frame's winner: the greatest located valid among the qualifying, ties to the lower located cost, then the better rank
inline int search_winner(const drf_search_result_t &res, const int *qual, int nq) {
  int w = qual[0];
  for (int j = 1; j < nq; ++j) {
    const drf_search_entry_t &en = res.entries[qual[j]], &best = res.entries[w];
    if (en.valid > best.valid || (en.valid == best.valid && en.located_cost < best.located_cost)) w = qual[j];
  }
  return w;
}
// drf_search_colour_frame's, over rescore(poses16, n, final_score, final_photo): the located float poses of the qualifying entries
// are scored once more by the colour score, in rank order, in one call of rescore; the smallest final_score wins, ties to the
// better rank.  An entry that does not qualify keeps final_score = final_photo = 0.
template <class Rescore>
inline int search_colour_winner(drf_search_colour_result_t &res, const int *qual, int nq, Rescore &&rescore) {
  float q16[DRF_SEARCH_MAX_TOP][16];
  double fs[DRF_SEARCH_MAX_TOP], fp[DRF_SEARCH_MAX_TOP];
  for (int j = 0; j < nq; ++j)
    for (int i = 0; i < 16; ++i) q16[j][i] = (float)res.entries[qual[j]].T[i];
  rescore(&q16[0][0], (size_t)nq, fs, fp);
  int w = qual[0];
  for (int j = 0; j < nq; ++j) {
    drf_search_colour_entry_t &en = res.entries[qual[j]];
    en.final_score = fs[j]; en.final_photo = fp[j];
    if (en.final_score < res.entries[w].final_score) w = qual[j];
  }
  return w;
}
// The two families by the names and argument lists they had before they were one text, each one call of it: what the host checks
// (tests/cpp/map_search_check.cpp, map_search_colour_check.cpp) call, so that they hold the shared text to the unchanged tests.
template <class Fetch>
inline void score_candidates_host(const LocateGrid &lg, const float *depth, Fetch &&fetch, const SearchLattice &L, const double *table, size_t n, const ScoreOpt &o,
                                  float voxel_size, double *cost, uint32_t *counts, double *score) {
  score_candidates_host(lg, nullptr, depth, fetch, L, table, n, o, voxel_size, cost, nullptr, counts, score);
}
template <class Fetch>
inline void score_colour_candidates_host(const LocateGrid &lg, const unsigned char *bgr, const float *depth, Fetch &&fetch, const SearchLattice &L, const double *table,
                                         size_t n, const ScoreColourOpt &o, float voxel_size, double *cost, double *photo, uint32_t *counts, double *score) {
  score_candidates_host(lg, bgr, depth, fetch, L, table, n, o, voxel_size, cost, photo, counts, score);
}
template <class Track, class Locate>
inline void search_refine(const SearchOpt &o, const double *table, const std::vector<size_t> &sel, const double *cost, const uint32_t *counts, const double *score,
                          size_t n_candidates, float voxel_size, Track &&track, Locate &&locate, float pose16_out[16], drf_search_result_t &res) {
  search_refine(o, table, sel, cost, nullptr, counts, score, n_candidates, voxel_size, track, locate, search_winner, pose16_out, res);
}
template <class Track, class Locate, class Rescore>
inline void search_colour_refine(const SearchColourOpt &o, const double *table, const std::vector<size_t> &sel, const double *cost, const double *photo,
                                 const uint32_t *counts, const double *score, size_t n_candidates, float voxel_size, Track &&track, Locate &&locate, Rescore &&rescore,
                                 float pose16_out[16], drf_search_colour_result_t &res) {
  search_refine(o, table, sel, cost, photo, counts, score, n_candidates, voxel_size, track, locate,
                [&](drf_search_colour_result_t &r, const int *qual, int nq) { return search_colour_winner(r, qual, nq, rescore); }, pose16_out, res);
}

}  // namespace dr
