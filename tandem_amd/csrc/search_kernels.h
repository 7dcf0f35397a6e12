// search_kernels.h -- drf_score_poses / drf_search_frame and their colour forms (drf_score_colour_poses / drf_search_colour_frame) on
// the device: the localisation's cost, without its Jacobian, at many poses of one depth image (the rule: pose_host.h score_sample /
// search_candidate; DESIGN.md §7c "Searching a pose lattice", "Searching with colour").  Each pair of kernels is two entry points
// over one device body, the colour half under if constexpr: the entry points keep their names and arguments, and what they compile
// to is what their own text compiled to (DESIGN.md §7c "Where the search code lives").  Included by dr_fusion.hip inside namespace
// dr, behind locate_kernels.h, whose LocateFetch reads the live map (the block kept across corners and samples, far blocks
// through find_block).  Launched by search_ops.h.

// Once per call: grid position n < padded = 512 groups -> its camera-frame point g (three doubles, locate_pixel's bits) and whether
// it is a sample, in grid order; COLOUR: and yf, the frame intensity of the sample's own pixel (track_intensity of its BGR bytes),
// 0 where the position is no sample.  No candidate then repeats the double divisions or reads an image.  Positions >= total (the
// last group's tail) are no samples.
template <bool COLOUR>
__device__ __forceinline__ void search_points(const float *__restrict__ depth, const unsigned char *__restrict__ bgr, const LocateGrid &lg, double vs, int total,
                                              int padded, double *__restrict__ g, unsigned char *__restrict__ flag, float *__restrict__ yf) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= padded) return;
  double p[3] = {0.0, 0.0, 0.0};
  const bool s = n < total && locate_pixel(lg, vs, n, depth, p);
  g[3 * (size_t)n] = s ? p[0] : 0.0; g[3 * (size_t)n + 1] = s ? p[1] : 0.0; g[3 * (size_t)n + 2] = s ? p[2] : 0.0;
  flag[n] = s ? 1 : 0;
  if constexpr (COLOUR) yf[n] = s ? track_intensity(bgr + 3 * locate_offset(lg, n)) : 0.0f;
}
__global__ __launch_bounds__(256) void k_search_points(const float *__restrict__ depth, const LocateGrid lg, double vs, int total, int padded,
                                                       double *__restrict__ g, unsigned char *__restrict__ flag) {
  search_points<false>(depth, nullptr, lg, vs, total, padded, g, flag, nullptr);
}
__global__ __launch_bounds__(256) void k_search_points_colour(const float *__restrict__ depth, const unsigned char *__restrict__ bgr, const LocateGrid lg, double vs,
                                                              int total, int padded, double *__restrict__ g, unsigned char *__restrict__ flag, float *__restrict__ yf) {
  search_points<true>(depth, bgr, lg, vs, total, padded, g, flag, yf);
}

struct SearchOut {  // 32 bytes per candidate of a chunk
  double cost;
  unsigned counts[4];  // samples, valid, unobserved, outside
  double score;
};
struct SearchColourOut {  // 40 bytes per candidate of a chunk
  double cost, photo;
  unsigned counts[4];  // samples, valid, unobserved, outside
  double score;
};
template <class Opt>
using SearchOutOf = std::conditional_t<Opt::colour, SearchColourOut, SearchOut>;  // the record of ScoreOpt / ScoreColourOpt

// One wave per candidate first + local, local in [0, n) (no grid stride; the four waves of a workgroup share nothing).  The pose is
// search_candidate's, from the table: wave-uniform, read once.  The wave walks the groups in order, lane l on positions
// 512 i + l + 64 k, k = 0..7, one double per lane from +0.0 (with colour two: cost and photo) and three integer counters; the
// butterfly x = x + shfl_xor(x, off), off = 32..1, leaves the group's partial in every lane, and lane i % 64 adds it to its fold
// accumulator: partial i in ascending i, k_align_fold's order, every sum in the one order.  A group no lane of which added a term
// has partial +0.0 in every sum, which changes no accumulator: its butterfly is skipped (wave-uniform).  The last butterfly folds
// the lanes and the counters; lane 0 writes the candidate's record (32 bytes, 40 with colour) with plain stores.  No atomics, no
// LDS, no second launch.  The map is only read.  yf is read with colour only.
// A template over the staging too (drf_set_search_scope; DESIGN.md §7c "Searching the whole map"): NoStage (raycast_kernels.h) is the
// resident score over LocateFetch, a RenderStage the map-scope score over LocateFetchStaged, pool and staged blocks together; what
// differs is the fetch and nothing else.  The staging is only read.
__device__ __forceinline__ LocateFetch search_fetch(const FusionDev &d, const NoStage &) { return LocateFetch(d); }
__device__ __forceinline__ LocateFetchStaged search_fetch(const FusionDev &d, const RenderStage &sg) { return LocateFetchStaged(d, sg); }
template <class Opt, class Stage>
__device__ __forceinline__ void search_score_wave(const FusionDev &d, const double *__restrict__ g, const unsigned char *__restrict__ flag, const float *__restrict__ yf,
                                                  int groups, const double *__restrict__ table, const SearchLattice &lat, size_t first, size_t table_first, int n,
                                                  const Opt &so, double vs, SearchOutOf<Opt> *__restrict__ out, const Stage &sg) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int local = blockIdx.x * 4 + wave;
  if (local >= n) return;
  const AlignEval e = score_eval(search_candidate(lat, table, table_first, first + (size_t)local), so.geo(), vs);
  double fold = 0.0, foldp = 0.0;
  unsigned ns = 0, nv = 0, nu = 0;
  auto fetch = search_fetch(d, sg);
#pragma unroll 1
  for (int i = 0; i < groups; ++i) {
    double x = 0.0, xp = 0.0;
    bool added = false;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
      const size_t p = (size_t)(512 * i + lane + 64 * k);
      if (!flag[p]) continue;
      ++ns;
      fetch.corner = 0;
      float y = 0.0f;
      if constexpr (Opt::colour) y = yf[p];
      const int r = score_sample(e, so, g[3 * p], g[3 * p + 1], g[3 * p + 2], y, fetch, x, xp);
      nv += r == 1 ? 1u : 0u;
      nu += r == 0 ? 1u : 0u;
      added = added || r == 1;
    }
    if (!__any(added)) continue;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      x = x + __shfl_xor(x, off);
      if constexpr (Opt::colour) xp = xp + __shfl_xor(xp, off);
    }
    if (lane == (i & 63)) {
      fold = fold + x;
      if constexpr (Opt::colour) foldp = foldp + xp;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    fold = fold + __shfl_xor(fold, off);
    if constexpr (Opt::colour) foldp = foldp + __shfl_xor(foldp, off);
    ns += __shfl_xor(ns, off); nv += __shfl_xor(nv, off); nu += __shfl_xor(nu, off);
  }
  if (lane == 0) {
    SearchOutOf<Opt> o;
    o.cost = fold;
    if constexpr (Opt::colour) o.photo = foldp;
    o.counts[0] = ns; o.counts[1] = nv; o.counts[2] = nu; o.counts[3] = ns - nv - nu;
    o.score = score_of(so, fold, foldp, ns, nu, ns - nv - nu);
    out[local] = o;
  }
}
__global__ __launch_bounds__(256) void k_search_score(const FusionDev d, const double *__restrict__ g, const unsigned char *__restrict__ flag, int groups,
                                                      const double *__restrict__ table, const SearchLattice lat, size_t first, size_t table_first, int n,
                                                      const ScoreOpt so, double vs, SearchOut *__restrict__ out) {
  search_score_wave(d, g, flag, nullptr, groups, table, lat, first, table_first, n, so, vs, out, NoStage{});
}
__global__ __launch_bounds__(256) void k_search_score_colour(const FusionDev d, const double *__restrict__ g, const unsigned char *__restrict__ flag,
                                                             const float *__restrict__ yf, int groups, const double *__restrict__ table, const SearchLattice lat,
                                                             size_t first, size_t table_first, int n, const ScoreColourOpt so, double vs,
                                                             SearchColourOut *__restrict__ out) {
  search_score_wave(d, g, flag, yf, groups, table, lat, first, table_first, n, so, vs, out, NoStage{});
}
// The map-scope forms: the resident kernels' arguments, then the staging (by value).
__global__ __launch_bounds__(256) void k_search_score_staged(const FusionDev d, const double *__restrict__ g, const unsigned char *__restrict__ flag, int groups,
                                                             const double *__restrict__ table, const SearchLattice lat, size_t first, size_t table_first, int n,
                                                             const ScoreOpt so, double vs, SearchOut *__restrict__ out, const RenderStage sg) {
  search_score_wave(d, g, flag, nullptr, groups, table, lat, first, table_first, n, so, vs, out, sg);
}
__global__ __launch_bounds__(256) void k_search_score_colour_staged(const FusionDev d, const double *__restrict__ g, const unsigned char *__restrict__ flag,
                                                                    const float *__restrict__ yf, int groups, const double *__restrict__ table,
                                                                    const SearchLattice lat, size_t first, size_t table_first, int n, const ScoreColourOpt so,
                                                                    double vs, SearchColourOut *__restrict__ out, const RenderStage sg) {
  search_score_wave(d, g, flag, yf, groups, table, lat, first, table_first, n, so, vs, out, sg);
}
