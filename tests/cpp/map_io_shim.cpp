// The shim's map file members (tandem_amd/libdr/dr_fusion.h) as a TANDEM translation unit would call them: one synthetic scan
// into a DrFusion, SaveMapToFile, LoadMapFromFile on a second DrFusion, one render of each compared byte for byte.
//   map_io_shim PATH
#include <cmath>
#include <cstring>

#include "dr_fusion.h"

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: map_io_shim PATH\n"); return 2; }
  const int H = 96, W = 128;
  DrFusionOptions o;
  o.voxel_size = 0.02f; o.num_buckets = 20000; o.bucket_size = 10; o.num_blocks = 20000; o.block_size = 8; o.max_sdf_weight = 64;
  o.truncation_distance = 0.08f; o.max_sensor_depth = 10.0f; o.min_sensor_depth = 0.1f; o.num_render_streams = 1;
  o.fx = 110.0f; o.fy = 110.0f; o.cx = 63.5f; o.cy = 47.5f; o.height = H; o.width = W;
  std::vector<unsigned char> bgr((size_t)H * W * 3);
  std::vector<float> depth((size_t)H * W);
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) {  // a wavy wall about 1.5 m away, a border of invalid pixels
      const size_t i = (size_t)v * W + u;
      depth[i] = (u < 3 || v < 2) ? 0.0f : 1.5f + 0.2f * std::sin(0.07f * u) * std::cos(0.05f * v);
      bgr[3 * i] = (unsigned char)(2 * u); bgr[3 * i + 1] = (unsigned char)(2 * v); bgr[3 * i + 2] = (unsigned char)(u + v);
    }
  const float pose[16] = {1, 0, 0, 0.1f, 0, 1, 0, -0.05f, 0, 0, 1, 0.2f, 0, 0, 0, 1};
  const size_t nb = (size_t)H * W * 3, nd = (size_t)H * W * sizeof(float);
  std::vector<unsigned char> b1(nb), b2(nb);
  std::vector<float> d1((size_t)H * W), d2((size_t)H * W);
  {
    DrFusion a(o);
    a.IntegrateScanAsync(bgr.data(), depth.data(), pose);
    a.RenderAsync({pose});
    std::vector<unsigned char *> rb;
    std::vector<float *> rd;
    a.GetRenderResult(rb, rd);
    memcpy(b1.data(), rb[0], nb); memcpy(d1.data(), rd[0], nd);
    a.SaveMapToFile(argv[1]);
  }
  {
    DrFusion b(o);
    b.LoadMapFromFile(argv[1]);
    b.RenderAsync({pose});  // legal after a load, before any scan
    std::vector<unsigned char *> rb;
    std::vector<float *> rd;
    b.GetRenderResult(rb, rd);
    memcpy(b2.data(), rb[0], nb); memcpy(d2.data(), rd[0], nd);
  }
  size_t hit = 0;
  for (float z : d1) hit += z > 0.0f;
  if (hit < (size_t)H * W / 2) { fprintf(stderr, "map_io_shim: the render shows %zu pixels only\n", hit); return 1; }
  if (memcmp(b1.data(), b2.data(), nb) != 0 || memcmp(d1.data(), d2.data(), nd) != 0) { fprintf(stderr, "map_io_shim: the renders differ\n"); return 1; }
  printf("map_io_shim ok: %zu pixels rendered alike\n", hit);
  return 0;
}
