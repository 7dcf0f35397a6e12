// C entry points over the coarse-to-fine half of the tracking in tandem_amd/csrc/pose_host.h for tests/test_map_track_pyramid.py
// (plain g++, no HIP): mtp_options, what the call makes of a drf_track_pyramid_options_t on a W x H camera; mtp_level, the level's
// camera; mtp_reduce, the reduction (track_reduce_host); mtp_system, one evaluation at a level (track_pyramid_system_host: the rule
// of drf_track_pyramid_system run on the host); mtp_frame, the whole tracking over a renderer of full-resolution colour and depth
// the caller supplies (track_pyramid_frame_host: the CPU reference of drf_track_pyramid_frame).  The camera is a drf_options_t.
#include "../../tandem_amd/csrc/fusion_host.h"

extern "C" {

// 0 and out4 = {levels, coarse_renders, max_renders, max_jump}; 1: refused, name says which
int mtp_options(const drf_track_pyramid_options_t *opt, float voxel_size, int W, int H, double out4[4], char *name) {
  dr::TrackPyramidOpt o;
  if (const char *bad = dr::track_pyramid_options(opt, voxel_size, W, H, o)) {
    if (name) { strncpy(name, bad, 31); name[31] = 0; }
    return 1;
  }
  out4[0] = o.levels; out4[1] = o.coarse_renders; out4[2] = o.c.t.max_renders; out4[3] = o.c.t.max_jump;
  return 0;
}
// level L's camera: ints = {W, H, step, Wg, Hg}, floats = {fx, fy, cx, cy, min_depth, max_depth}, and max_jump_L / max_renders_L of
// the options; 1: the level does not fit
int mtp_level(const drf_options_t *cam, const drf_track_pyramid_options_t *opt, int L, int ints[5], float floats[6], float *max_jump, int *max_renders) {
  dr::TrackPyramidOpt o;
  if (dr::track_pyramid_options(opt, cam->voxel_size, cam->width, cam->height, o) || !dr::track_level_fits(cam->width, cam->height, L)) return 1;
  const dr::LocateGrid g = dr::track_level_grid(dr::locate_grid(*cam, o.c.t.step), L);
  ints[0] = g.W; ints[1] = g.H; ints[2] = g.step; ints[3] = g.Wg; ints[4] = g.Hg;
  floats[0] = g.fx; floats[1] = g.fy; floats[2] = g.cx; floats[3] = g.cy; floats[4] = g.min_depth; floats[5] = g.max_depth;
  const dr::TrackColourOpt lo = dr::track_level_options(o, L);
  *max_jump = lo.t.max_jump; *max_renders = lo.t.max_renders;
  return 0;
}
// the reduction of a W x H pair to level L (bgr null: depth alone); 1: L outside 0..4
int mtp_reduce(int W, int H, int L, float max_jump, const unsigned char *bgr, const float *depth, unsigned char *bgr_out, float *depth_out) {
  if (L < 0 || L >= dr::kTrackMaxLevels) return 1;
  dr::track_reduce_host(W, H, L, max_jump, bgr, depth, bgr_out, depth_out);
  return 0;
}
// the system at level L; 1 if the options or the level are refused, 2 if a pose is
int mtp_system(const drf_options_t *cam, int L, const unsigned char *bgr, const float *depth, const unsigned char *model_bgr, const float *model_depth,
               const float *model_pose16, const float *pose16, const drf_track_pyramid_options_t *opt, double sums[28], unsigned long long counts[5]) {
  dr::TrackPyramidOpt o;
  if (dr::track_pyramid_options(opt, cam->voxel_size, cam->width, cam->height, o) || !dr::track_level_fits(cam->width, cam->height, L)) return 1;
  if (dr::transform_pose_fault(pose16) || dr::transform_pose_fault(model_pose16)) return 2;
  uint64_t c[5] = {0, 0, 0, 0, 0};
  dr::track_pyramid_system_host(dr::locate_grid(*cam, o.c.t.step), L, bgr, depth, model_bgr, model_depth, model_pose16, pose16, o, cam->voxel_size, sums, c);
  for (int i = 0; i < 5; ++i) counts[i] = c[i];
  return 0;
}
// the tracking from pose16 over render(pose16, bgr_out, depth_out, user), full resolution; trace receives the sums of the first
// min(evaluations, trace_cap) evaluations in the order they ran; stats = {stats8[8], level4[5][4], last5[5]}: 33 words.
// bgr null: geometry only.
typedef void (*mtp_render_fn)(const float *pose16, unsigned char *bgr_out, float *depth_out, void *user);
int mtp_frame(const drf_options_t *cam, const unsigned char *bgr, const float *depth, mtp_render_fn render, void *user, const float *pose16,
              const drf_track_pyramid_options_t *opt, drf_align_result_t *res, double *trace, size_t trace_cap, unsigned long long stats33[33]) {
  dr::TrackPyramidOpt o;
  if (dr::track_pyramid_options(opt, cam->voxel_size, cam->width, cam->height, o)) return 1;
  if (dr::transform_pose_fault(pose16)) return 2;
  std::vector<std::array<double, 28>> tr;
  uint64_t stats8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, level4[dr::kTrackMaxLevels][4], last5[5] = {0, 0, 0, 0, 0};
  dr::track_pyramid_frame_host(dr::locate_grid(*cam, o.c.t.step), bgr, depth, [&](const float *p16, unsigned char *Cm, float *Dm) { render(p16, Cm, Dm, user); }, pose16, o,
                               cam->voxel_size, *res, stats8, level4, last5, &tr);
  for (size_t i = 0; i < tr.size() && i < trace_cap; ++i) memcpy(trace + 28 * i, tr[i].data(), 224);
  for (int i = 0; i < 8; ++i) stats33[i] = stats8[i];
  for (int L = 0; L < dr::kTrackMaxLevels; ++L)
    for (int i = 0; i < 4; ++i) stats33[8 + 4 * L + i] = level4[L][i];
  for (int i = 0; i < 5; ++i) stats33[28 + i] = last5[i];
  return 0;
}

}  // extern "C"
