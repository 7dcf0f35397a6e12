// C entry points over the colour half of the tracking in tandem_amd/csrc/fusion_host.h for tests/test_map_track_colour.py (plain
// g++, no HIP): mtc_options, what the call makes of a drf_track_colour_options_t; mtc_model, the model map and the model intensity
// map Ym of a model colour and depth image (track_model_colour_host); mtc_system, one evaluation with the photometric term
// (track_colour_system_host: the rule of drf_track_colour_system run on the host); mtc_geometric, the same images through the
// geometric track_system_host; mtc_frame, the whole tracking over a renderer of colour and depth the caller supplies
// (track_colour_frame_host: the CPU reference of drf_track_colour_frame).  The camera is a drf_options_t.
#include "../../tandem_amd/csrc/fusion_host.h"

extern "C" {

// 0 and out11 = {the ten of mt_options, photo_weight}, weight_bits = photo_weight's fp32 pattern; 1: refused, name says which
int mtc_options(const drf_track_colour_options_t *opt, float voxel_size, double out11[11], unsigned *weight_bits, char *name) {
  dr::TrackColourOpt o;
  if (const char *bad = dr::track_colour_options(opt, voxel_size, o)) {
    if (name) { strncpy(name, bad, 31); name[31] = 0; }
    return 1;
  }
  out11[0] = o.t.max_renders; out11[1] = o.t.a.max_iters; out11[2] = o.t.step; out11[3] = o.t.dist_max; out11[4] = o.t.max_jump; out11[5] = o.t.a.huber;
  out11[6] = o.t.centre_depth; out11[7] = o.t.a.eps_rot; out11[8] = o.t.a.eps_trans; out11[9] = o.t.a.min_valid; out11[10] = o.photo_weight;
  if (weight_bits) memcpy(weight_bits, &o.photo_weight, 4);
  return 0;
}
// the model map of (Cm, Dm): height x width x (nx, ny, nz, z), and Ym: height x width
int mtc_model(const drf_options_t *cam, const unsigned char *Cm, const float *Dm, float max_jump, float *out4, float *Ym) {
  std::vector<dr::TrackPixel> map((size_t)cam->width * cam->height);
  dr::track_model_colour_host(dr::locate_grid(*cam, 1), max_jump, Dm, Cm, map.data(), Ym);
  memcpy(out4, map.data(), map.size() * sizeof(dr::TrackPixel));
  return 0;
}
// track_photo_term alone on an intensity map Ym the caller supplies (height x width; it need not come from a model map, so its
// border may carry colour): 1 and out4 = {r, n0, n1, n2} if the term exists, 0 if it is skipped
int mtc_term(const drf_options_t *cam, const float *Ym, const float *model_pose16, const double m[3], double up, double vp, float yf, float photo_weight,
             double out4[4]) {
  dr::TrackModel t;
  t.m = dr::map_motion(model_pose16, cam->voxel_size);
  t.lim2 = 0.0; t.map = nullptr;
  dr::TrackColour tc;
  tc.Ym = Ym; tc.weight = (double)photo_weight;
  out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
  return dr::track_photo_term(t, tc, dr::locate_grid(*cam, 1), m, up, vp, yf, out4[0], out4 + 1) ? 1 : 0;
}
// the system at pose16 against (model_bgr, model_depth), a ray-cast at model_pose16; 1 if the options are refused, 2 if a pose is
int mtc_system(const drf_options_t *cam, const unsigned char *bgr, const float *depth, const unsigned char *model_bgr, const float *model_depth,
               const float *model_pose16, const float *pose16, const drf_track_colour_options_t *opt, double sums[28], unsigned long long counts[5]) {
  dr::TrackColourOpt o;
  if (dr::track_colour_options(opt, cam->voxel_size, o)) return 1;
  if (dr::transform_pose_fault(pose16) || dr::transform_pose_fault(model_pose16)) return 2;
  const dr::LocateGrid lg = dr::locate_grid(*cam, o.t.step);
  const size_t npix = (size_t)cam->width * cam->height;
  std::vector<dr::TrackPixel> map(npix);
  std::vector<float> Ym(npix);
  dr::track_model_colour_host(lg, o.t.max_jump, model_depth, model_bgr, map.data(), Ym.data());
  double c_src[3];
  dr::locate_centre_src(o.t.centre_depth, cam->voxel_size, c_src);
  uint64_t c[5];
  dr::track_colour_system_host(lg, bgr, depth, dr::track_model(model_pose16, o.t, cam->voxel_size, map.data()), dr::track_colour(o, Ym.data()),
                               dr::align_eval(dr::map_motion(pose16, cam->voxel_size), c_src, o.t.a, cam->voxel_size), sums, c);
  for (int i = 0; i < 5; ++i) counts[i] = c[i];
  return 0;
}
// drf_track_system's host rule on the same depth images
int mtc_geometric(const drf_options_t *cam, const float *depth, const float *model_depth, const float *model_pose16, const float *pose16,
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
// the tracking from pose16 over render(pose16, bgr_out, depth_out, user); trace receives the sums of the first min(iterations,
// trace_cap) evaluations, stats7 = {the five counters of the last evaluation, evaluations, renders}.  colour = 0 runs the
// geometric track_frame_host over the same renderer (stats7[4] stays 0).
typedef void (*mtc_render_fn)(const float *pose16, unsigned char *bgr_out, float *depth_out, void *user);
int mtc_frame(const drf_options_t *cam, const unsigned char *bgr, const float *depth, mtc_render_fn render, void *user, const float *pose16,
              const drf_track_colour_options_t *opt, int colour, drf_align_result_t *res, double *trace, size_t trace_cap, unsigned long long stats7[7]) {
  dr::TrackColourOpt o;
  if (dr::track_colour_options(opt, cam->voxel_size, o)) return 1;
  if (dr::transform_pose_fault(pose16)) return 2;
  std::vector<std::array<double, 28>> tr;
  uint64_t last5[5] = {0, 0, 0, 0, 0}, stats2[2] = {0, 0};
  const dr::LocateGrid lg = dr::locate_grid(*cam, o.t.step);
  if (colour) {
    dr::track_colour_frame_host(lg, bgr, depth, [&](const float *p16, unsigned char *Cm, float *Dm) { render(p16, Cm, Dm, user); }, pose16, o, cam->voxel_size, *res,
                                last5, stats2, &tr);
  } else {
    std::vector<unsigned char> Cm((size_t)cam->width * cam->height * 3);
    dr::track_frame_host(lg, depth, [&](const float *p16, float *Dm) { render(p16, Cm.data(), Dm, user); }, pose16, o.t, cam->voxel_size, *res, last5, stats2, &tr);
  }
  for (size_t i = 0; i < tr.size() && i < trace_cap; ++i) memcpy(trace + 28 * i, tr[i].data(), 224);
  for (int i = 0; i < 5; ++i) stats7[i] = last5[i];
  stats7[5] = stats2[0]; stats7[6] = stats2[1];
  return 0;
}

}  // extern "C"
