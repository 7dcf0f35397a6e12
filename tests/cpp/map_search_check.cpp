// C entry points over the search half of tandem_amd/csrc/pose_host.h for tests/test_map_search.py (plain g++, no HIP): ms_options,
// what the calls make of their option structs; ms_point, score_point held to align_point<true> sample by sample; ms_score, the
// score of many poses (score_candidates_host: the rule of drf_score_poses run on the host); ms_search, the whole search over a
// renderer the caller supplies as a function (search_refine over track_frame_host and locate_frame_host: the CPU reference of
// drf_search_frame).  The map is given as for map_locate_check.cpp: ascending keys and n x 4096 voxel bytes; the camera is a
// drf_options_t.
#include "../../tandem_amd/csrc/fusion_host.h"

extern "C" {

// 0 and the resolved options to out13 = {step, min_weight, band, huber, oc, uc, dstep, Nx, Ny, Nz, top_k, score_only, accept_valid};
// 1: refused, and name (if given, 32 bytes) receives the option's name
int ms_options(const drf_search_options_t *opt, float truncation_distance, float voxel_size, double out13[13], char *name) {
  dr::SearchOpt o;
  if (const char *bad = dr::search_options(opt, truncation_distance, voxel_size, o)) {
    if (name) { strncpy(name, bad, 31); name[31] = 0; }
    return 1;
  }
  const double v[13] = {(double)o.s.step, (double)o.s.min_weight, o.s.band, o.s.huber, o.s.oc, o.s.uc, o.L.dstep, (double)o.L.N[0], (double)o.L.N[1], (double)o.L.N[2],
                        (double)o.top_k, o.score_only ? 1.0 : 0.0, o.accept_valid};
  memcpy(out13, v, sizeof v);
  return 0;
}
// every sample of the grid at pose16 through align_point<true> (s_src = 0, centre 0) and through score_point: returns how many
// differ in their code or in the bits of the one sum; seen4 = samples per code 0, 1, 2 and the samples in all
int ms_point(const unsigned long long *keys, const unsigned char *vox, size_t n, const drf_options_t *cam, const float *depth, const float *pose16,
             const drf_score_options_t *opt, unsigned long long seen4[4]) {
  dr::ScoreOpt o;
  if (dr::score_options(opt, cam->truncation_distance, cam->voxel_size, o)) return -1;
  const dr::HostMapSource fetch(std::vector<unsigned long long>(keys, keys + n), vox);
  const dr::LocateGrid lg = dr::locate_grid(*cam, o.step);
  const dr::AlignEval e = dr::score_eval(dr::map_motion(pose16, cam->voxel_size), o, (double)cam->voxel_size);
  int bad = 0;
  seen4[0] = seen4[1] = seen4[2] = seen4[3] = 0;
  for (long p = 0; p < dr::locate_positions(lg); ++p) {
    double g[3];
    if (!dr::locate_pixel(lg, e.vs, (int)p, depth, g)) continue;
    double acc[28] = {0.0}, cost = 0.0;
    const int a = dr::align_point<true>(e, g[0], g[1], g[2], 0.0f, fetch, acc);
    const int b = dr::score_point(e, g[0], g[1], g[2], fetch, cost);
    if (a != b || memcmp(&acc[27], &cost, 8) != 0) ++bad;
    ++seen4[a]; ++seen4[3];
  }
  return bad;
}
// cost[n_poses], counts[n_poses][4], score[n_poses]; 1 if the options are refused, 2 if a pose is
int ms_score(const unsigned long long *keys, const unsigned char *vox, size_t n, const drf_options_t *cam, const float *depth, const float *poses16, size_t n_poses,
             const drf_score_options_t *opt, double *cost, uint32_t *counts, double *score) {
  dr::ScoreOpt o;
  if (dr::score_options(opt, cam->truncation_distance, cam->voxel_size, o)) return 1;
  std::vector<double> table(n_poses * 12);
  for (size_t i = 0; i < n_poses; ++i) {
    if (dr::transform_pose_fault(poses16 + 16 * i)) return 2;
    const dr::MapMotion m = dr::map_motion(poses16 + 16 * i, cam->voxel_size);
    memcpy(&table[12 * i], m.R, 72);
    memcpy(&table[12 * i + 9], m.tv, 24);
  }
  const dr::HostMapSource fetch(std::vector<unsigned long long>(keys, keys + n), vox);
  const dr::SearchLattice plain = {{1, 1, 1}, {0, 0, 0}, 0.0, 1};
  dr::score_candidates_host(dr::locate_grid(*cam, o.step), depth, fetch, plain, table.data(), n_poses, o, cam->voxel_size, cost, counts, score);
  return 0;
}
// The search over render(pose16, depth_out, user).  0: ran (res->status says how it ended); 1: an option is refused (name receives
// it); 2: an anchor, a rotation or a product is (name receives the text's start); 3: the count of candidates is.  all_scores may be null.
typedef void (*ms_render_fn)(const float *pose16, float *depth_out, void *user);
int ms_search(const unsigned long long *keys, const unsigned char *vox, size_t n, const drf_options_t *cam, const float *depth, ms_render_fn render, void *user,
              const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot, const drf_search_options_t *opt, const drf_track_options_t *topt,
              const drf_locate_options_t *lopt, float pose16_out[16], drf_search_result_t *res, double *all_scores, char *name) {
  dr::SearchOpt so;
  dr::TrackOpt to;
  dr::LocateOpt lo;
  const char *bad = dr::search_options(opt, cam->truncation_distance, cam->voxel_size, so);
  if (!bad) bad = dr::track_options(topt, cam->voxel_size, to);
  if (!bad) bad = dr::locate_options(lopt, cam->truncation_distance, lo);
  if (bad) {
    if (name) { strncpy(name, bad, 31); name[31] = 0; }
    return 1;
  }
  const size_t nc = dr::search_count(n_anchors, n_rot, so.L);
  if (nc == 0) return 3;
  std::vector<double> table;
  const std::string why = dr::search_table(anchors16, n_anchors, rotations9, n_rot, cam->voxel_size, table);
  if (!why.empty()) {
    if (name) { strncpy(name, why.c_str(), 31); name[31] = 0; }
    return 2;
  }
  const dr::HostMapSource fetch(std::vector<unsigned long long>(keys, keys + n), vox);
  std::vector<double> cost(nc), score(nc);
  std::vector<uint32_t> counts(4 * nc);
  dr::score_candidates_host(dr::locate_grid(*cam, so.s.step), depth, fetch, so.L, table.data(), nc, so.s, cam->voxel_size, cost.data(), counts.data(), score.data());
  if (all_scores) memcpy(all_scores, score.data(), nc * 8);
  dr::search_refine(so, table.data(), dr::search_select(score.data(), nc, so.top_k), cost.data(), counts.data(), score.data(), nc, cam->voxel_size,
                    [&](const float *p16, drf_align_result_t &r) {
                      dr::track_frame_host(dr::locate_grid(*cam, to.step), depth, [&](const float *p, float *Dm) { render(p, Dm, user); }, p16, to, cam->voxel_size, r);
                    },
                    [&](const float *p16, drf_align_result_t &r) {
                      dr::locate_frame_host(dr::locate_grid(*cam, lo.step), depth, fetch, dr::map_motion(p16, cam->voxel_size), lo, cam->voxel_size, r);
                    },
                    pose16_out, *res);
  return 0;
}

}  // extern "C"
