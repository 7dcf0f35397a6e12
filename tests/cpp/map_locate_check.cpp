// C entry points over the localisation half of tandem_amd/csrc/fusion_host.h for tests/test_map_locate.py (plain g++, no HIP):
// ml_system, one evaluation of the system at a pose (locate_system_host: the rule of drf_locate_system run on the host), ml_frame,
// the whole refinement (locate_frame_host: the CPU reference of drf_locate_frame) with the sums of every evaluation, and
// ml_options, what the call makes of a drf_locate_options_t.  The map is ascending keys and n x 4096 bytes; the camera is a
// drf_options_t (width, height, fx, fy, cx, cy, voxel_size, truncation_distance and the sensor's depth range are read).
#include "../../tandem_amd/csrc/fusion_host.h"

extern "C" {

// 0 and the resolved options to out9 = {max_iters, min_weight, step, band, huber, centre_depth, eps_rot, eps_trans, min_valid}; 1: refused,
// and name (if given, 32 bytes) receives the option's name
int ml_options(const drf_locate_options_t *opt, float truncation_distance, double out9[9], char *name) {
  dr::LocateOpt o;
  if (const char *bad = dr::locate_options(opt, truncation_distance, o)) {
    if (name) { strncpy(name, bad, 31); name[31] = 0; }
    return 1;
  }
  out9[0] = o.a.max_iters; out9[1] = o.a.min_weight; out9[2] = o.step; out9[3] = o.a.band; out9[4] = o.a.huber; out9[5] = o.centre_depth;
  out9[6] = o.a.eps_rot; out9[7] = o.a.eps_trans; out9[8] = o.a.min_valid;
  return 0;
}
// the system at pose16; 1 if the options are refused, 2 if the pose is
int ml_system(const unsigned long long *keys, const unsigned char *vox, size_t n, const drf_options_t *cam, const float *depth, const float *pose16,
              const drf_locate_options_t *opt, double sums[28], unsigned long long counts[4]) {
  dr::LocateOpt o;
  if (dr::locate_options(opt, cam->truncation_distance, o)) return 1;
  if (dr::transform_pose_fault(pose16)) return 2;
  const std::vector<unsigned long long> k(keys, keys + n);
  const dr::HostMapSource map(k, vox);
  double c_src[3];
  dr::locate_centre_src(o.centre_depth, cam->voxel_size, c_src);
  uint64_t c[4];
  dr::locate_system_host(dr::locate_grid(*cam, o.step), depth, map, dr::align_eval(dr::map_motion(pose16, cam->voxel_size), c_src, o.a, cam->voxel_size), sums, c);
  for (int i = 0; i < 4; ++i) counts[i] = c[i];
  return 0;
}
// the refinement from pose16; trace receives the sums of the first min(iterations, trace_cap) evaluations
int ml_frame(const unsigned long long *keys, const unsigned char *vox, size_t n, const drf_options_t *cam, const float *depth, const float *pose16,
             const drf_locate_options_t *opt, drf_align_result_t *res, double *trace, size_t trace_cap) {
  dr::LocateOpt o;
  if (dr::locate_options(opt, cam->truncation_distance, o)) return 1;
  if (dr::transform_pose_fault(pose16)) return 2;
  const std::vector<unsigned long long> k(keys, keys + n);
  const dr::HostMapSource map(k, vox);
  std::vector<std::array<double, 28>> tr;
  dr::locate_frame_host(dr::locate_grid(*cam, o.step), depth, map, dr::map_motion(pose16, cam->voxel_size), o, cam->voxel_size, *res, &tr);
  for (size_t i = 0; i < tr.size() && i < trace_cap; ++i) memcpy(trace + 28 * i, tr[i].data(), 224);
  return 0;
}

}  // extern "C"
