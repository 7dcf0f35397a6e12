// The shim's SetRenderBands (tandem_amd/libdr/dr_fusion.h) as a TANDEM translation unit would call it: one synthetic scan into a
// DrFusion whose pool holds the map, its render and its map file; a second, streaming DrFusion loads the file into its host
// store and renders the same pose in map scope with a staging of CAPACITY blocks (0 = the default) and up to 16 depth bands.
// The two renders must agree byte for byte.  (The shim exits on a refused call, so with a CAPACITY that the caller knows to be
// below the stored blocks in reach, success means the render was banded: tests/test_fusion_render_bands_gpu.py.)
//   render_bands_shim PATH CAPACITY
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "dr_fusion.h"

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: render_bands_shim PATH CAPACITY\n"); return 2; }
  const int H = 96, W = 128;
  DrFusionOptions o;
  o.voxel_size = 0.01f; o.num_buckets = 20000; o.bucket_size = 10; o.num_blocks = 20000; o.block_size = 8; o.max_sdf_weight = 64;
  o.truncation_distance = 0.04f; o.max_sensor_depth = 3.0f; o.min_sensor_depth = 0.1f; o.num_render_streams = 1;
  o.fx = 200.0f; o.fy = 200.0f; o.cx = 63.5f; o.cy = 47.5f; o.height = H; o.width = W;
  std::vector<unsigned char> bgr((size_t)H * W * 3);
  std::vector<float> depth((size_t)H * W);
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) {  // a near and a far wall side by side, a border of invalid pixels
      const size_t i = (size_t)v * W + u;
      depth[i] = (u < 3 || v < 2) ? 0.0f : (u < W / 2 ? 0.9f : 2.3f) + 0.05f * std::sin(0.07f * u) * std::cos(0.05f * v);
      bgr[3 * i] = (unsigned char)(2 * u); bgr[3 * i + 1] = (unsigned char)(2 * v); bgr[3 * i + 2] = (unsigned char)(u + v);
    }
  const float pose[16] = {1, 0, 0, 0.1f, 0, 1, 0, -0.05f, 0, 0, 1, 0.2f, 0, 0, 0, 1};
  const size_t nb = (size_t)H * W * 3, nd = (size_t)H * W * sizeof(float);
  std::vector<unsigned char> b1(nb), b2(nb);
  std::vector<float> d1((size_t)H * W), d2((size_t)H * W);
  std::vector<unsigned char *> rb;
  std::vector<float *> rd;
  {
    DrFusion a(o);
    a.IntegrateScanAsync(bgr.data(), depth.data(), pose);
    a.RenderAsync({pose});
    a.GetRenderResult(rb, rd);
    memcpy(b1.data(), rb[0], nb); memcpy(d1.data(), rd[0], nd);
    a.SaveMapToFile(argv[1]);
  }
  float radius = 0.0f;
  if (drf_streaming_min_radius(reinterpret_cast<const drf_options_t *>(&o), &radius) != 0) { fprintf(stderr, "render_bands_shim: no streaming radius\n"); return 1; }
  {
    DrFusion b(o);
    b.SetStreaming(radius, 0);
    b.LoadMapFromFile(argv[1]);  // streaming on: into the host store
    b.SetRenderScope(DRF_RENDER_MAP, (size_t)atol(argv[2]));
    b.SetRenderBands(16);
    b.RenderAsync({pose});  // legal after a load, before any scan
    rb.clear(); rd.clear();
    b.GetRenderResult(rb, rd);
    memcpy(b2.data(), rb[0], nb); memcpy(d2.data(), rd[0], nd);
  }
  size_t hit = 0;
  for (float z : d1) hit += z > 0.0f;
  if (hit < (size_t)H * W / 2) { fprintf(stderr, "render_bands_shim: the render shows %zu pixels only\n", hit); return 1; }
  if (memcmp(b1.data(), b2.data(), nb) != 0 || memcmp(d1.data(), d2.data(), nd) != 0) { fprintf(stderr, "render_bands_shim: the renders differ\n"); return 1; }
  printf("render_bands_shim ok: %zu pixels rendered alike\n", hit);
  return 0;
}
