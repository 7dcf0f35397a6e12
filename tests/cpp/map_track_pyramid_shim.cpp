// The shim's TrackPyramidFrame (tandem_amd/libdr/dr_fusion.h) as a TANDEM translation unit would call it: a DrFusion loads MAP,
// tracks the colour and depth image of FRAME coarse to fine from FRAME's rough pose, and prints the status and the pose as one JSON
// line, which tests/test_fusion_track_pyramid_gpu.py holds to the library's own answer.
// FRAME is raw: 16 pose floats, a drf_track_pyramid_options_t, then 96 x 128 depths and 96 x 128 x 3 colour bytes.
//   map_track_pyramid_shim VOXEL_SIZE FX FY CX CY NUM_BLOCKS MAP FRAME
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dr_fusion.h"

int main(int argc, char **argv) {
  if (argc != 9) { fprintf(stderr, "usage: map_track_pyramid_shim VOXEL_SIZE FX FY CX CY NUM_BLOCKS MAP FRAME\n"); return 2; }
  DrFusionOptions o;
  o.voxel_size = strtof(argv[1], nullptr); o.num_blocks = atoi(argv[6]); o.num_buckets = o.num_blocks; o.bucket_size = 10; o.block_size = 8; o.max_sdf_weight = 64;
  o.truncation_distance = 4 * o.voxel_size; o.max_sensor_depth = 10.0f; o.min_sensor_depth = 0.1f; o.num_render_streams = 1;
  o.fx = strtof(argv[2], nullptr); o.fy = strtof(argv[3], nullptr); o.cx = strtof(argv[4], nullptr); o.cy = strtof(argv[5], nullptr); o.height = 96; o.width = 128;
  float pose[16], tracked[16];
  drf_track_pyramid_options_t opt;
  std::vector<float> depth((size_t)o.height * o.width);
  std::vector<unsigned char> bgr(depth.size() * 3);
  FILE *f = fopen(argv[8], "rb");
  if (!f || fread(pose, 4, 16, f) != 16 || fread(&opt, sizeof opt, 1, f) != 1 || fread(depth.data(), 4, depth.size(), f) != depth.size() ||
      fread(bgr.data(), 1, bgr.size(), f) != bgr.size()) {
    fprintf(stderr, "map_track_pyramid_shim: cannot read %s\n", argv[8]);
    return 2;
  }
  fclose(f);
  DrFusion fusion(o);
  fusion.LoadMapFromFile(argv[7]);
  const int st = fusion.TrackPyramidFrame(bgr.data(), depth.data(), pose, tracked, &opt);
  printf("{\"track_status\": %d, \"tracked\": [", st);
  for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", tracked[i]);
  printf("]}\n");
  return 0;
}
