// The shim's LocateDepthFrame (tandem_amd/libdr/dr_fusion.h) as a TANDEM translation unit would call it: a DrFusion loads MAP,
// locates the depth image of FRAME in it from FRAME's rough pose, and prints the status and the refined pose as one JSON line, which
// tests/test_fusion_map_locate_gpu.py holds to the library's own answer.  FRAME is raw: 16 pose floats, then height x width depths.
//   map_locate_shim VOXEL_SIZE MAP FRAME
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dr_fusion.h"

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: map_locate_shim VOXEL_SIZE MAP FRAME\n"); return 2; }
  DrFusionOptions o;
  o.voxel_size = strtof(argv[1], nullptr); o.num_buckets = 4000; o.bucket_size = 10; o.num_blocks = 4000; o.block_size = 8; o.max_sdf_weight = 64;
  o.truncation_distance = 4 * o.voxel_size; o.max_sensor_depth = 10.0f; o.min_sensor_depth = 0.1f; o.num_render_streams = 1;
  o.fx = 110.0f; o.fy = 110.0f; o.cx = 63.5f; o.cy = 47.5f; o.height = 96; o.width = 128;
  float pose[16], out[16];
  std::vector<float> depth((size_t)o.height * o.width);
  FILE *f = fopen(argv[3], "rb");
  if (!f || fread(pose, 4, 16, f) != 16 || fread(depth.data(), 4, depth.size(), f) != depth.size()) { fprintf(stderr, "map_locate_shim: cannot read %s\n", argv[3]); return 2; }
  fclose(f);
  DrFusion fusion(o);
  fusion.LoadMapFromFile(argv[2]);
  const int status = fusion.LocateDepthFrame(depth.data(), pose, out);
  printf("{\"status\": %d, \"pose\": [", status);
  for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", out[i]);
  printf("]}\n");
  return 0;
}
