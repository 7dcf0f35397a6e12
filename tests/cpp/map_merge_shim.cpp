// The shim's MergeMapFromFile (tandem_amd/libdr/dr_fusion.h) as a TANDEM translation unit would call it: one synthetic scan into
// a DrFusion that saves DIR/a.drfmap, a second scan from another pose into a second DrFusion that saves DIR/b.drfmap, merges
// a.drfmap and saves DIR/merged.drfmap; its render after the merge must show more of the wall than before.
// tests/test_fusion_map_merge_gpu.py holds the three files to the restatement of the rule.
//   map_merge_shim DIR
#include <cmath>
#include <cstring>

#include "dr_fusion.h"

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: map_merge_shim DIR\n"); return 2; }
  const std::string dir = argv[1];
  const int H = 96, W = 128;
  DrFusionOptions o;
  o.voxel_size = 0.02f; o.num_buckets = 20000; o.bucket_size = 10; o.num_blocks = 20000; o.block_size = 8; o.max_sdf_weight = 64;
  o.truncation_distance = 0.08f; o.max_sensor_depth = 10.0f; o.min_sensor_depth = 0.1f; o.num_render_streams = 1;
  o.fx = 110.0f; o.fy = 110.0f; o.cx = 63.5f; o.cy = 47.5f; o.height = H; o.width = W;
  std::vector<unsigned char> bgr((size_t)H * W * 3);
  std::vector<float> depth((size_t)H * W);
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) {  // a flat wall 1.5 m away, a border of invalid pixels
      const size_t i = (size_t)v * W + u;
      depth[i] = (u < 3 || v < 2) ? 0.0f : 1.5f;
      bgr[3 * i] = (unsigned char)(2 * u); bgr[3 * i + 1] = (unsigned char)(2 * v); bgr[3 * i + 2] = (unsigned char)(u + v);
    }
  // the same wall seen from two places half its width apart: the maps overlap and each holds blocks the other lacks
  const float pose_a[16] = {1, 0, 0, 0.1f, 0, 1, 0, -0.05f, 0, 0, 1, 0.2f, 0, 0, 0, 1};
  const float pose_b[16] = {1, 0, 0, 0.8f, 0, 1, 0, -0.05f, 0, 0, 1, 0.2f, 0, 0, 0, 1};
  const float pose_mid[16] = {1, 0, 0, 0.45f, 0, 1, 0, -0.05f, 0, 0, 1, 0.2f, 0, 0, 0, 1};
  {
    DrFusion a(o);
    a.IntegrateScanAsync(bgr.data(), depth.data(), pose_a);
    a.RenderAsync({pose_a});
    std::vector<unsigned char *> rb;
    std::vector<float *> rd;
    a.GetRenderResult(rb, rd);
    a.SaveMapToFile(dir + "/a.drfmap");
  }
  size_t before = 0, after = 0;
  {
    DrFusion b(o);
    b.IntegrateScanAsync(bgr.data(), depth.data(), pose_b);
    b.RenderAsync({pose_mid});
    std::vector<unsigned char *> rb;
    std::vector<float *> rd;
    b.GetRenderResult(rb, rd);
    for (size_t i = 0; i < (size_t)H * W; ++i) before += rd[0][i] > 0.0f;
    b.SaveMapToFile(dir + "/b.drfmap");
    b.MergeMapFromFile(dir + "/a.drfmap");
    b.RenderAsync({pose_mid});  // legal after a merge, before the next scan
    rb.clear(); rd.clear();
    b.GetRenderResult(rb, rd);
    for (size_t i = 0; i < (size_t)H * W; ++i) after += rd[0][i] > 0.0f;
    b.SaveMapToFile(dir + "/merged.drfmap");
  }
  if (!(after > before + (size_t)H * W / 10)) { fprintf(stderr, "map_merge_shim: %zu pixels before the merge, %zu after\n", before, after); return 1; }
  printf("map_merge_shim ok: %zu pixels before the merge, %zu after\n", before, after);
  return 0;
}
