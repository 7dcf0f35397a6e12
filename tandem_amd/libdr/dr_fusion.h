// dr_fusion.h -- header-compatible replacement for TANDEM's
//   tandem/libdr/dr_fusion/src/dr_fusion/dr_fusion.h
// Same structs, class, members and signatures; every call forwards to the C ABI of libdr_mi355x.so.
// Protocol violations print and exit(EXIT_FAILURE) like tsdf_volume.cu:520-524,635-653,703-713.
#ifndef DR_FUSION_DR_FUSION_H
#define DR_FUSION_DR_FUSION_H

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "dr_mi355x.h"

struct DrFusionOptions {  // dr_fusion.h:18-36 -- layout-identical to drf_options_t
  float voxel_size;
  int num_buckets;
  int bucket_size;
  int num_blocks;
  int block_size;
  int max_sdf_weight;
  float truncation_distance;
  float max_sensor_depth;
  float min_sensor_depth;
  int num_render_streams;

  float fx;
  float fy;
  float cx;
  float cy;
  int height;
  int width;
};
static_assert(sizeof(DrFusionOptions) == sizeof(drf_options_t), "DrFusionOptions must match drf_options_t");

struct DrMesh {  // dr_fusion.h:38-42
  size_t num = 0;
  float *vert = nullptr;
  float *cols = nullptr;
};

class DrFusion {  // dr_fusion.h:44-73
public:
  DrFusion(struct DrFusionOptions const &options) : n_render_(options.num_render_streams), impl(nullptr) {
    check(drf_create(reinterpret_cast<const drf_options_t *>(&options), 0, &impl));
    // the reference mallocs 2 x 720 MB here (dr_fusion.cpp:36-37); allocated lazily with the first mesh instead
    dr_mesh_vert = nullptr;
    dr_mesh_cols = nullptr;
  }
  ~DrFusion() { drf_destroy(impl); free(dr_mesh_vert); free(dr_mesh_cols); }
  DrFusion(const DrFusion &) = delete;
  DrFusion &operator=(const DrFusion &) = delete;

  void IntegrateScanAsync(unsigned char *bgr, float *depth, float const *pose) { check(drf_integrate_scan_async(impl, bgr, depth, pose)); }
  void RenderAsync(std::vector<float const *> camera_poses) { check(drf_render_async(impl, camera_poses.data(), (int) camera_poses.size())); }
  void GetRenderResult(std::vector<unsigned char *> &bgr, std::vector<float *> &depth) {
    if ((!bgr.empty()) || (!depth.empty())) { fprintf(stderr, "Input vectors must be empty.\n"); exit(EXIT_FAILURE); }  // tsdf_volume.cu:715-718
    std::vector<uint8_t *> b(n_render_ > 0 ? n_render_ : 1);
    std::vector<float *> d(n_render_ > 0 ? n_render_ : 1);
    check(drf_get_render_result(impl, b.data(), d.data(), n_render_));
    for (int i = 0; i < n_render_; i++) { bgr.push_back(b[i]); depth.push_back(d[i]); }
  }
  void SaveMeshToFile(std::string const &filename, float lower_corner[3], float upper_corner[3]) { check(drf_save_mesh(impl, filename.c_str(), lower_corner, upper_corner)); }
  struct DrMesh GetMesh(float lower_corner[3], float upper_corner[3]) {  // caller owns vert / cols (dr_fusion.cpp:95-148)
    check(drf_extract_mesh_async(impl, lower_corner, upper_corner));
    size_t ntri = 0;
    check(drf_mesh_num_triangles(impl, &ntri));
    DrMesh m;
    m.vert = (float *) malloc(sizeof(float) * (ntri ? ntri : 1) * 9);
    m.cols = (float *) malloc(sizeof(float) * (ntri ? ntri : 1) * 9);
    check(drf_get_mesh_sync(impl, 3 * ntri, &m.num, m.vert, m.cols));
    return m;
  }
  void ExtractMeshAsync(float lower_corner[3], float upper_corner[3]) { check(drf_extract_mesh_async(impl, lower_corner, upper_corner)); }
  void GetMeshSync() {
    if (!dr_mesh_vert) {
      dr_mesh_vert = (float *) malloc(sizeof(float) * dr_mesh_num_max * 3);
      dr_mesh_cols = (float *) malloc(sizeof(float) * dr_mesh_num_max * 3);
    }
    check(drf_get_mesh_sync(impl, dr_mesh_num_max, &dr_mesh_num, dr_mesh_vert, dr_mesh_cols));
  }
  void Synchronize() { check(drf_synchronize(impl)); }

  // Extension (no reference counterpart): stream voxel blocks to host memory so the map may outgrow num_blocks
  // (dr_mi355x.h, INTEGRATION.md "Streaming").  radius 0 = off; otherwise at least drf_streaming_min_radius of the options.
  void SetStreaming(float radius, size_t host_capacity_blocks) { check(drf_set_streaming(impl, radius, host_capacity_blocks)); }
  void StreamOutRegion(float lower_corner[3], float upper_corner[3]) { check(drf_stream_out_region(impl, lower_corner, upper_corner)); }
  void StreamInRegion(float lower_corner[3], float upper_corner[3]) { check(drf_stream_in_region(impl, lower_corner, upper_corner)); }
  // DRF_MESH_MAP: SaveMeshToFile / ExtractMeshAsync / GetMeshSync / GetMesh cover the host store too (DRF_MESH_RESIDENT: the pool only)
  void SetMeshScope(int scope) { check(drf_set_mesh_scope(impl, scope)); }
  // DRF_RENDER_MAP: RenderAsync at any pose reads resident and host-stored blocks together (capacity 0 = the default staging)
  void SetRenderScope(int scope, size_t capacity = 0) { check(drf_set_render_scope(impl, scope, capacity)); }
  // 2..64: a DRF_RENDER_MAP render that exceeds the staging runs in up to max_passes depth bands (0: off, the default)
  void SetRenderBands(int max_passes) { check(drf_set_render_bands(impl, max_passes)); }

  // Map files (dr_mi355x.h "map files", INTEGRATION.md "Map files"): the whole map, host store included, to a file and into a
  // DrFusion whose map is empty.  Failures exit like every other member.
  void SaveMapToFile(std::string const &filename) { check(drf_save_map(impl, filename.c_str(), 0)); }
  void LoadMapFromFile(std::string const &filename) { check(drf_load_map(impl, filename.c_str(), 0)); }
  // a saved map of the same world merged into the map this DrFusion holds, voxel by voxel (dr_mi355x.h drf_merge_map)
  void MergeMapFromFile(std::string const &filename) { check(drf_merge_map(impl, filename.c_str(), 0)); }
  // the map file src resampled in this DrFusion's world frame and written to dst: T16 row-major, p_here = R p_file + t, rigid
  // (dr_mi355x.h drf_transform_map); this DrFusion's own map is not touched, MergeMapFromFile(dst) or LoadMapFromFile(dst) follow
  void TransformMapFile(std::string const &src, float const *T16, std::string const &dst) { check(drf_transform_map(impl, src.c_str(), T16, dst.c_str(), 0)); }
  // the map file src registered to the map file ref from T_init16 (null: the identity): T16_out, src-world to ref-world, goes
  // straight into TransformMapFile(src, T16_out, dst) (dr_mi355x.h drf_align_map; it refines, T_init16 must be within a few voxels).
  // A registration that finds no pose (degenerate, lost) exits like every other violation; returns the evaluations made.
  int AlignMapFiles(std::string const &src, std::string const &ref, float const *T_init16, float *T16_out) {
    static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    drf_align_result_t res;
    check(drf_align_map(impl, src.c_str(), ref.c_str(), T_init16 ? T_init16 : identity, nullptr, T16_out, &res));
    if (res.status == DRF_ALIGN_DEGENERATE || res.status == DRF_ALIGN_LOST) { fprintf(stderr, "%s\n", dr_last_error()); exit(EXIT_FAILURE); }
    return res.iterations;
  }
  // a depth frame (height x width floats, metres) located in the map this object holds, from the rough camera-to-world pose
  // pose_init16: pose16_out is the pose IntegrateScanAsync takes to continue the map (dr_mi355x.h drf_locate_frame; it refines,
  // pose_init16 must bring the points inside the truncation band; from farther off TrackDepthFrame goes first).  Returns the status, DRF_ALIGN_*: a frame that finds no pose
  // (DRF_ALIGN_DEGENERATE, DRF_ALIGN_LOST: pose16_out is then no better than pose_init16, dr_last_error() says why) is an answer a
  // tracker acts on, not a violation.
  int LocateDepthFrame(float const *depth, float const *pose_init16, float *pose16_out) {
    drf_align_result_t res;
    check(drf_locate_frame(impl, depth, pose_init16, nullptr, pose16_out, &res));
    return res.status;
  }
  // a depth frame tracked against the ray-cast model of the map this object holds, from a pose that is only good to decimetres and
  // degrees (dr_mi355x.h drf_track_frame: projective association, point-to-plane; opt null = its defaults).  It ends within
  // LocateDepthFrame's reach: track first, then locate from pose16_out.  Returns the status, DRF_ALIGN_*; DRF_ALIGN_MAX_ITERS is a
  // usable pose too.
  int TrackDepthFrame(float const *depth, float const *pose_init16, float *pose16_out, drf_track_options_t const *opt = nullptr) {
    drf_align_result_t res;
    check(drf_track_frame(impl, depth, pose_init16, opt, pose16_out, &res));
    return res.status;
  }
  // the same with the frame's colour image (bgr as IntegrateScanAsync takes it) and a photometric term next to the geometric one
  // (dr_mi355x.h drf_track_colour_frame): it holds the motion inside a plane, which TrackDepthFrame leaves open -- on a single wall
  // TrackDepthFrame is DRF_ALIGN_DEGENERATE and this call is not.  opt null = its defaults.  Returns the status, DRF_ALIGN_*.
  int TrackColourFrame(unsigned char const *bgr, float const *depth, float const *pose_init16, float *pose16_out,
                       drf_track_colour_options_t const *opt = nullptr) {
    drf_align_result_t res;
    check(drf_track_colour_frame(impl, bgr, depth, pose_init16, opt, pose16_out, &res));
    return res.status;
  }
  // the same coarse to fine over an image pyramid (dr_mi355x.h drf_track_pyramid_frame): the cure where the map's texture is finer
  // than a rendered pixel; no global search.  bgr null = geometry only, opt null = 3 levels.  Returns level 0's status.
  int TrackPyramidFrame(unsigned char const *bgr, float const *depth, float const *pose_init16, float *pose16_out,
                        drf_track_pyramid_options_t const *opt = nullptr) {
    drf_align_result_t res;
    check(drf_track_pyramid_frame(impl, bgr, depth, pose_init16, opt, pose16_out, &res));
    return res.status;
  }
  // the same for a frame whose exposure differs from the map's (dr_mi355x.h drf_track_exposure_frame): gain and offset of
  // frame ~ gain * model + offset are solved next to the pose and handed out (either may be null).  bgr is required; opt null = 3
  // levels, the gain from 1 within [0.25, 4].  Returns level 0's status.  Compensate the frame with them before IntegrateScanAsync.
  int TrackExposureFrame(unsigned char const *bgr, float const *depth, float const *pose_init16, float *pose16_out, double *gain_out = nullptr,
                         double *offset_out = nullptr, drf_track_exposure_options_t const *opt = nullptr) {
    drf_exposure_result_t res;
    check(drf_track_exposure_frame(impl, bgr, depth, pose_init16, opt, pose16_out, &res));
    if (gain_out) *gain_out = res.gain;
    if (offset_out) *offset_out = res.offset;
    return res.pose.status;
  }
  // one evaluation of its 8 x 8 system at `level`, a pose and an exposure against a model pair: sums[45], counts[5]
  void TrackExposureSystem(int level, unsigned char const *bgr, float const *depth, unsigned char const *model_bgr, float const *model_depth,
                           float const *model_pose16, float const *pose16, double gain, double offset, double *sums45, unsigned long long *counts5,
                           drf_track_exposure_options_t const *opt = nullptr) {
    uint64_t c[5];
    check(drf_track_exposure_system(impl, level, bgr, depth, model_bgr, model_depth, model_pose16, pose16, gain, offset, opt, sums45, c));
    for (int i = 0; i < 5; ++i) counts5[i] = c[i];
  }
  // n poses16 (n x 16 floats, camera-to-world) scored against the resident map in one kernel (dr_mi355x.h drf_score_poses): score[n],
  // lower is better; cost and counts (n x 4: samples, valid, unobserved, outside) may be null.  opt null = its defaults.
  void ScorePoses(float const *depth, float const *poses16, size_t n, double *score, double *cost = nullptr, uint32_t *counts = nullptr,
                  drf_score_options_t const *opt = nullptr) {
    check(drf_score_poses(impl, depth, poses16, n, opt, cost, counts, score));
  }
  // a depth frame found in the map from a lattice of poses (dr_mi355x.h drf_search_frame): every anchor turned by every rotation
  // (n_rot x 9 doubles, row-major, about the world axes) and moved by the offsets of opt is scored, the best few are tracked and
  // located, one is picked.  The guess that TrackDepthFrame and LocateDepthFrame need when a session has only a place-recognition
  // hit or a stale pose.  Returns the status, DRF_ALIGN_*; DRF_ALIGN_LOST: pose16_out is the best-scoring candidate, no more.
  int SearchDepthFrame(float const *depth, float const *anchors16, size_t n_anchors, double const *rotations9, size_t n_rot, float *pose16_out,
                       drf_search_options_t const *opt = nullptr, drf_search_result_t *result = nullptr, drf_track_options_t const *track_opt = nullptr,
                       drf_locate_options_t const *locate_opt = nullptr) {
    drf_search_result_t res;
    check(drf_search_frame(impl, depth, anchors16, n_anchors, rotations9, n_rot, opt, track_opt, locate_opt, pose16_out, &res, nullptr));
    if (result) *result = res;
    return res.status;
  }
  // ScorePoses with the appearance term from the voxel colours (dr_mi355x.h drf_score_colour_poses): bgr is the frame's colour image
  // as IntegrateScanAsync takes it; photo[n] is the colour sum, score carries both.
  void ScoreColourPoses(uint8_t const *bgr, float const *depth, float const *poses16, size_t n, double *score, double *cost = nullptr, double *photo = nullptr,
                        uint32_t *counts = nullptr, drf_score_colour_options_t const *opt = nullptr) {
    check(drf_score_colour_poses(impl, bgr, depth, poses16, n, opt, cost, photo, counts, score));
  }
  // SearchDepthFrame where geometry alone is ambiguous -- one wall, a corridor (dr_mi355x.h drf_search_colour_frame): selection and
  // winner by the colour score, tracking with the frame's colour image (the pyramid's rule).  Returns the status, DRF_ALIGN_*.
  int SearchColourFrame(uint8_t const *bgr, float const *depth, float const *anchors16, size_t n_anchors, double const *rotations9, size_t n_rot, float *pose16_out,
                        drf_search_colour_options_t const *opt = nullptr, drf_search_colour_result_t *result = nullptr,
                        drf_track_pyramid_options_t const *track_opt = nullptr, drf_locate_options_t const *locate_opt = nullptr) {
    drf_search_colour_result_t res;
    check(drf_search_colour_frame(impl, bgr, depth, anchors16, n_anchors, rotations9, n_rot, opt, track_opt, locate_opt, pose16_out, &res, nullptr));
    if (result) *result = res;
    return res.status;
  }
  // DRF_LOCATE_MAP: LocateDepthFrame reads resident and host-stored blocks together, without moving one (capacity 0 = the default
  // staging); DRF_LOCATE_RESIDENT, the default: the pool only
  void SetLocateScope(int scope, size_t capacity = 0) { check(drf_set_locate_scope(impl, scope, capacity)); }
  // DRF_SEARCH_MAP: the score stage of ScorePoses / SearchDepthFrame and their colour forms reads resident and host-stored blocks
  // together, without moving one (capacity 0 = the default staging); DRF_SEARCH_RESIDENT, the default: the pool only.  A search of
  // the whole map wants the render, the locate and the search scope set (dr_mi355x.h drf_set_search_scope)
  void SetSearchScope(int scope, size_t capacity = 0) { check(drf_set_search_scope(impl, scope, capacity)); }
  // the last search call: stagings made, blocks in the largest, blocks staged in total, score launches that read a staging
  void SearchStageStats(uint64_t out[4]) { check(drf_search_stage_stats(impl, out)); }

  // Incremental mesh (dr_mi355x.h "incremental mesh", INTEGRATION.md "Incremental mesh"): GetMeshUpdateSync fills dr_mesh_num /
  // dr_mesh_vert / dr_mesh_cols with the triangles of the listed blocks only, and the members below name the blocks: block i has
  // coordinates dr_mesh_update_coords[3 i ..] and owns triangles [dr_mesh_update_first[i], dr_mesh_update_first[i + 1]).
  // dr_mesh_update_full: every block is listed, drop what was kept before.
  void ExtractMeshUpdateAsync(float lower_corner[3], float upper_corner[3]) { check(drf_extract_mesh_update_async(impl, lower_corner, upper_corner)); }
  void GetMeshUpdateSync() {
    size_t nblk = 0, ntri = 0;
    int full = 0;
    check(drf_mesh_update_size(impl, &nblk, &ntri, &full));
    if (!dr_mesh_vert) {
      dr_mesh_vert = (float *) malloc(sizeof(float) * dr_mesh_num_max * 3);
      dr_mesh_cols = (float *) malloc(sizeof(float) * dr_mesh_num_max * 3);
    }
    dr_mesh_update_coords.resize(3 * nblk + 3);
    dr_mesh_update_first.resize(nblk + 1);
    check(drf_get_mesh_update_sync(impl, nblk, dr_mesh_num_max, &dr_mesh_update_blocks, dr_mesh_update_coords.data(), dr_mesh_update_first.data(),
                                   &dr_mesh_num, dr_mesh_vert, dr_mesh_cols, &full));
    dr_mesh_update_coords.resize(3 * dr_mesh_update_blocks);
    dr_mesh_update_full = full != 0;
  }
  void ResetMeshUpdate() { check(drf_mesh_update_reset(impl)); }

  bool dr_mesh_update_full = false;
  size_t dr_mesh_update_blocks = 0;
  std::vector<int32_t> dr_mesh_update_coords;
  std::vector<uint64_t> dr_mesh_update_first;

  size_t dr_mesh_num = 0;
  const size_t dr_mesh_num_max = 60000000;
  float *dr_mesh_vert;
  float *dr_mesh_cols;

private:
  static void check(int status) {
    if (status != DR_OK) { fprintf(stderr, "%s\n", dr_last_error()); exit(EXIT_FAILURE); }
  }
  int n_render_;
  drf_t *impl;
};

#endif  // DR_FUSION_DR_FUSION_H
