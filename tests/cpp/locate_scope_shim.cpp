// The shim's SetLocateScope (tandem_amd/libdr/dr_fusion.h) as a TANDEM translation unit would call it: a DrFusion loads MAP, turns
// streaming on and sends every block to the host store, locates the depth image of FRAME in resident scope (which sees nothing) and
// then in map scope, and prints both statuses and the refined pose as one JSON line, which tests/test_fusion_locate_scope_gpu.py
// holds to the answer of an engine whose pool holds the map.  FRAME is raw: fx fy cx cy, 16 pose floats, height x width depths.
//   locate_scope_shim VOXEL_SIZE MAP FRAME
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dr_fusion.h"

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: locate_scope_shim VOXEL_SIZE MAP FRAME\n"); return 2; }
  DrFusionOptions o;
  o.voxel_size = strtof(argv[1], nullptr); o.num_buckets = 40000; o.bucket_size = 10; o.num_blocks = 40000; o.block_size = 8; o.max_sdf_weight = 64;
  o.truncation_distance = 4 * o.voxel_size; o.max_sensor_depth = 10.0f; o.min_sensor_depth = 0.1f; o.num_render_streams = 1;
  o.height = 96; o.width = 128;
  float k[4], pose[16], gone[16], out[16];
  std::vector<float> depth((size_t)o.height * o.width);
  FILE *f = fopen(argv[3], "rb");
  if (!f || fread(k, 4, 4, f) != 4 || fread(pose, 4, 16, f) != 16 || fread(depth.data(), 4, depth.size(), f) != depth.size()) {
    fprintf(stderr, "locate_scope_shim: cannot read %s\n", argv[3]);
    return 2;
  }
  fclose(f);
  o.fx = k[0]; o.fy = k[1]; o.cx = k[2]; o.cy = k[3];
  DrFusion fusion(o);
  fusion.LoadMapFromFile(argv[2]);
  float radius = 0.0f;
  if (drf_streaming_min_radius(reinterpret_cast<const drf_options_t *>(&o), &radius) != DR_OK) return 2;
  fusion.SetStreaming(radius, 0);
  float lo[3] = {-500.0f, -500.0f, -500.0f}, hi[3] = {500.0f, 500.0f, 500.0f};
  fusion.StreamOutRegion(lo, hi);
  const int resident_status = fusion.LocateDepthFrame(depth.data(), pose, gone);
  fusion.SetLocateScope(DRF_LOCATE_MAP);
  const int status = fusion.LocateDepthFrame(depth.data(), pose, out);
  printf("{\"resident_status\": %d, \"status\": %d, \"pose\": [", resident_status, status);
  for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", out[i]);
  printf("]}\n");
  return 0;
}
