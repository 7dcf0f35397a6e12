// C entry points over the exposure half of the tracking in tandem_amd/csrc/pose_host.h for tests/test_map_track_exposure.py (plain
// g++, no HIP): mte_options, what the call makes of a drf_track_exposure_options_t on a W x H camera; mte_system, one evaluation
// of the 45 sums at a level, a pose and an exposure (track_exposure_system_at_host: the rule of drf_track_exposure_system run on
// the host); mte_step, one step of the 8 x 8 system (exposure_step); mte_frame, the whole tracking over a renderer of
// full-resolution colour and depth the caller supplies (track_exposure_frame_host: the CPU reference of drf_track_exposure_frame).
// The camera is a drf_options_t.
#include "../../tandem_amd/csrc/fusion_host.h"

extern "C" {

// 0 and out6 = {gain_init, offset_init, gain_min, gain_max, eps_gain, eps_offset}; 1: refused, name says which
int mte_options(const drf_track_exposure_options_t *opt, float voxel_size, int W, int H, double out6[6], char *name) {
  dr::TrackExposureOpt o;
  if (const char *bad = dr::track_exposure_options(opt, voxel_size, W, H, o)) {
    if (name) { strncpy(name, bad, 31); name[31] = 0; }
    return 1;
  }
  out6[0] = o.gain_init; out6[1] = o.offset_init; out6[2] = o.gain_min; out6[3] = o.gain_max; out6[4] = o.eps_gain; out6[5] = o.eps_offset;
  return 0;
}
// the system at level L; 1 if the options or the level are refused, 2 if a pose is, 3 if a colour image is missing
int mte_system(const drf_options_t *cam, int L, const unsigned char *bgr, const float *depth, const unsigned char *model_bgr, const float *model_depth,
               const float *model_pose16, const float *pose16, double gain, double offset, const drf_track_exposure_options_t *opt, double sums[45],
               unsigned long long counts[5]) {
  dr::TrackExposureOpt o;
  if (dr::track_exposure_options(opt, cam->voxel_size, cam->width, cam->height, o) || !dr::track_exposure_level_fits(cam->width, cam->height, L)) return 1;
  if (!bgr || !model_bgr) return 3;
  if (dr::transform_pose_fault(pose16) || dr::transform_pose_fault(model_pose16)) return 2;
  uint64_t c[5] = {0, 0, 0, 0, 0};
  dr::track_exposure_system_at_host(dr::locate_grid(*cam, o.p.c.t.step), L, bgr, depth, model_bgr, model_depth, model_pose16, pose16, gain, offset, o, cam->voxel_size, sums,
                                    c);
  for (int i = 0; i < 5; ++i) counts[i] = c[i];
  return 0;
}
// one step from sums[45] at the centre c: x6 = {gain, offset, gain_min, gain_max, eps_gain, eps_offset} (gain and offset are
// updated), Rt12 = R (9, row-major) then tv (3), updated; returns the status or -1, *held counts a held exposure
int mte_step(const double sums[45], const double c[3], double eps_rot, double eps_trans, double x6[6], double Rt12[12], unsigned long long *held) {
  dr::ExposureState x;
  x.gain = x6[0]; x.offset = x6[1]; x.gain_min = x6[2]; x.gain_max = x6[3]; x.eps_gain = x6[4]; x.eps_offset = x6[5];
  dr::MapMotion m;
  memcpy(m.R, Rt12, sizeof m.R);
  memcpy(m.tv, Rt12 + 9, sizeof m.tv);
  const int s = dr::exposure_step(sums, c, eps_rot, eps_trans, x, m);
  x6[0] = x.gain; x6[1] = x.offset;
  memcpy(Rt12, m.R, sizeof m.R);
  memcpy(Rt12 + 9, m.tv, sizeof m.tv);
  *held = x.held;
  return s;
}
// the tracking from pose16 over render(pose16, bgr_out, depth_out, user), full resolution; trace receives the pose sums of the
// first min(evaluations, trace_cap) evaluations in the order they ran; stats = {stats8[8], level4[5][4]}: 28 words.
typedef void (*mte_render_fn)(const float *pose16, unsigned char *bgr_out, float *depth_out, void *user);
int mte_frame(const drf_options_t *cam, const unsigned char *bgr, const float *depth, mte_render_fn render, void *user, const float *pose16,
              const drf_track_exposure_options_t *opt, drf_exposure_result_t *res, double *trace, size_t trace_cap, unsigned long long stats28[28]) {
  dr::TrackExposureOpt o;
  if (dr::track_exposure_options(opt, cam->voxel_size, cam->width, cam->height, o)) return 1;
  if (!bgr) return 3;
  if (dr::transform_pose_fault(pose16)) return 2;
  std::vector<std::array<double, 28>> tr;
  uint64_t stats8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, level4[dr::kTrackMaxLevels][4];
  dr::track_exposure_frame_host(dr::locate_grid(*cam, o.p.c.t.step), bgr, depth, [&](const float *p16, unsigned char *Cm, float *Dm) { render(p16, Cm, Dm, user); }, pose16, o,
                                cam->voxel_size, *res, stats8, level4, &tr);
  for (size_t i = 0; i < tr.size() && i < trace_cap; ++i) memcpy(trace + 28 * i, tr[i].data(), 224);
  for (int i = 0; i < 8; ++i) stats28[i] = stats8[i];
  for (int L = 0; L < dr::kTrackMaxLevels; ++L)
    for (int i = 0; i < 4; ++i) stats28[8 + 4 * L + i] = level4[L][i];
  return 0;
}

}  // extern "C"
