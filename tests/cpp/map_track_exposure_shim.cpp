// The shim's TrackExposureFrame and TrackExposureSystem (tandem_amd/libdr/dr_fusion.h) as a TANDEM translation unit would call
// them: a DrFusion loads MAP, tracks the colour and depth image of FRAME under a change of exposure from FRAME's rough pose, evaluates
// the system once at the pose and exposure it found against the frame itself as the model, and prints the status, the pose, the
// gain, the offset and that system's cost as one JSON line, which tests/test_fusion_track_exposure_gpu.py holds to the library's own
// answer.
// FRAME is raw: 16 pose floats, a drf_track_exposure_options_t, then 96 x 128 depths and 96 x 128 x 3 colour bytes.
//   map_track_exposure_shim VOXEL_SIZE FX FY CX CY NUM_BLOCKS MAP FRAME
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dr_fusion.h"

int main(int argc, char **argv) {
  if (argc != 9) { fprintf(stderr, "usage: map_track_exposure_shim VOXEL_SIZE FX FY CX CY NUM_BLOCKS MAP FRAME\n"); return 2; }
  DrFusionOptions o;
  o.voxel_size = strtof(argv[1], nullptr); o.num_blocks = atoi(argv[6]); o.num_buckets = o.num_blocks; o.bucket_size = 10; o.block_size = 8; o.max_sdf_weight = 64;
  o.truncation_distance = 4 * o.voxel_size; o.max_sensor_depth = 10.0f; o.min_sensor_depth = 0.1f; o.num_render_streams = 1;
  o.fx = strtof(argv[2], nullptr); o.fy = strtof(argv[3], nullptr); o.cx = strtof(argv[4], nullptr); o.cy = strtof(argv[5], nullptr); o.height = 96; o.width = 128;
  float pose[16], tracked[16];
  drf_track_exposure_options_t opt;
  std::vector<float> depth((size_t)o.height * o.width);
  std::vector<unsigned char> bgr(depth.size() * 3);
  FILE *f = fopen(argv[8], "rb");
  if (!f || fread(pose, 4, 16, f) != 16 || fread(&opt, sizeof opt, 1, f) != 1 || fread(depth.data(), 4, depth.size(), f) != depth.size() ||
      fread(bgr.data(), 1, bgr.size(), f) != bgr.size()) {
    fprintf(stderr, "map_track_exposure_shim: cannot read %s\n", argv[8]);
    return 2;
  }
  fclose(f);
  DrFusion fusion(o);
  fusion.LoadMapFromFile(argv[7]);
  double gain = 0.0, offset = 0.0, sums[45];
  unsigned long long counts[5];
  const int st = fusion.TrackExposureFrame(bgr.data(), depth.data(), pose, tracked, &gain, &offset, &opt);
  fusion.TrackExposureSystem(0, bgr.data(), depth.data(), bgr.data(), depth.data(), tracked, tracked, gain, offset, sums, counts, &opt);
  printf("{\"track_status\": %d, \"gain\": %.17g, \"offset\": %.17g, \"cost\": %.17g, \"photometric\": %llu, \"tracked\": [", st, gain, offset, sums[27], counts[4]);
  for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", tracked[i]);
  printf("]}\n");
  return 0;
}
