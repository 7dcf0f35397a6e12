// C entry points over the tracking half of tandem_amd/csrc/fusion_host.h for tests/test_map_track.py (plain g++, no HIP):
// mt_model, the model map of a model depth image (track_model_host), mt_system, one evaluation against a model depth the caller
// supplies (track_system_host: the rule of drf_track_system run on the host), mt_frame, the whole tracking over a renderer the
// caller supplies as a function (track_frame_host: the CPU reference of drf_track_frame) with the sums of every evaluation, and
// mt_options, what the call makes of a drf_track_options_t.  The camera is a drf_options_t (width, height, fx, fy, cx, cy,
// voxel_size and the sensor's depth range are read).
#include "../../tandem_amd/csrc/fusion_host.h"

extern "C" {

// 0 and the resolved options to out10 = {max_renders, inner_iters, step, dist_max, max_jump, huber, centre_depth, eps_rot, eps_trans,
// min_valid}; 1: refused, and name (if given, 32 bytes) receives the option's name
int mt_options(const drf_track_options_t *opt, float voxel_size, double out10[10], char *name) {
  dr::TrackOpt o;
  if (const char *bad = dr::track_options(opt, voxel_size, o)) {
    if (name) { strncpy(name, bad, 31); name[31] = 0; }
    return 1;
  }
  out10[0] = o.max_renders; out10[1] = o.a.max_iters; out10[2] = o.step; out10[3] = o.dist_max; out10[4] = o.max_jump; out10[5] = o.a.huber;
  out10[6] = o.centre_depth; out10[7] = o.a.eps_rot; out10[8] = o.a.eps_trans; out10[9] = o.a.min_valid;
  return 0;
}
// the model map of Dm: height x width x (nx, ny, nz, z)
int mt_model(const drf_options_t *cam, const float *Dm, float max_jump, float *out4) {
  std::vector<dr::TrackPixel> map((size_t)cam->width * cam->height);
  dr::track_model_host(dr::locate_grid(*cam, 1), max_jump, Dm, map.data());
  memcpy(out4, map.data(), map.size() * sizeof(dr::TrackPixel));
  return 0;
}
// the system at pose16 against model_depth, a ray-cast at model_pose16; 1 if the options are refused, 2 if a pose is
int mt_system(const drf_options_t *cam, const float *depth, const float *model_depth, const float *model_pose16, const float *pose16,
              const drf_track_options_t *opt, double sums[28], unsigned long long counts[4]) {
  dr::TrackOpt o;
  if (dr::track_options(opt, cam->voxel_size, o)) return 1;
  if (dr::transform_pose_fault(pose16) || dr::transform_pose_fault(model_pose16)) return 2;
  const dr::LocateGrid lg = dr::locate_grid(*cam, o.step);
  std::vector<dr::TrackPixel> map((size_t)cam->width * cam->height);
  dr::track_model_host(lg, o.max_jump, model_depth, map.data());
  double c_src[3];
  dr::locate_centre_src(o.centre_depth, cam->voxel_size, c_src);
  uint64_t c[4];
  dr::track_system_host(lg, depth, dr::track_model(model_pose16, o, cam->voxel_size, map.data()),
                        dr::align_eval(dr::map_motion(pose16, cam->voxel_size), c_src, o.a, cam->voxel_size), sums, c);
  for (int i = 0; i < 4; ++i) counts[i] = c[i];
  return 0;
}
// the tracking from pose16 over render(pose16, depth_out, user); trace receives the sums of the first min(iterations, trace_cap)
// evaluations, stats6 = {the four counters of the last evaluation, evaluations, renders}
typedef void (*mt_render_fn)(const float *pose16, float *depth_out, void *user);
int mt_frame(const drf_options_t *cam, const float *depth, mt_render_fn render, void *user, const float *pose16, const drf_track_options_t *opt,
             drf_align_result_t *res, double *trace, size_t trace_cap, unsigned long long stats6[6]) {
  dr::TrackOpt o;
  if (dr::track_options(opt, cam->voxel_size, o)) return 1;
  if (dr::transform_pose_fault(pose16)) return 2;
  std::vector<std::array<double, 28>> tr;
  uint64_t last4[4] = {0, 0, 0, 0}, stats2[2] = {0, 0};
  dr::track_frame_host(dr::locate_grid(*cam, o.step), depth, [&](const float *p16, float *Dm) { render(p16, Dm, user); }, pose16, o, cam->voxel_size, *res, last4,
                       stats2, &tr);
  for (size_t i = 0; i < tr.size() && i < trace_cap; ++i) memcpy(trace + 28 * i, tr[i].data(), 224);
  for (int i = 0; i < 4; ++i) stats6[i] = last4[i];
  stats6[4] = stats2[0]; stats6[5] = stats2[1];
  return 0;
}

}  // extern "C"
