// The shim's TransformMapFile (tandem_amd/libdr/dr_fusion.h) as a TANDEM translation unit would call it: one synthetic scan into a
// DrFusion that saves DIR/a.drfmap; a second DrFusion, whose world frame is the first one's moved by T, writes DIR/b.drfmap =
// a.drfmap in its own frame, loads it and renders it from T * pose: it must see the wall the first one saw from pose.  T goes to
// DIR/T.txt; tests/test_fusion_map_transform_gpu.py holds b.drfmap to the restatement of the rule.
//   map_transform_shim DIR
#include <cmath>
#include <cstring>

#include "dr_fusion.h"

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: map_transform_shim DIR\n"); return 2; }
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
  const float pose[16] = {1, 0, 0, 0.1f, 0, 1, 0, -0.05f, 0, 0, 1, 0.2f, 0, 0, 0, 1};
  // 30 degrees about y and a shift: the second session's frame
  const float c = std::cos(0.5235988f), s = std::sin(0.5235988f);
  const float T[16] = {c, 0, s, 0.37f, 0, 1, 0, -0.21f, -s, 0, c, 0.55f, 0, 0, 0, 1};
  float moved[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double a = 0.0;
      for (int k = 0; k < 4; ++k) a += (double)T[4 * i + k] * pose[4 * k + j];
      moved[4 * i + j] = (float)a;
    }
  FILE *tf = fopen((dir + "/T.txt").c_str(), "w");
  if (!tf) { fprintf(stderr, "map_transform_shim: cannot write T.txt\n"); return 1; }
  for (int i = 0; i < 16; ++i) fprintf(tf, "%.9g\n", T[i]);
  fclose(tf);
  size_t before = 0, after = 0;
  {
    DrFusion a(o);
    a.IntegrateScanAsync(bgr.data(), depth.data(), pose);
    a.RenderAsync({pose});
    std::vector<unsigned char *> rb;
    std::vector<float *> rd;
    a.GetRenderResult(rb, rd);
    for (size_t i = 0; i < (size_t)H * W; ++i) before += rd[0][i] > 0.0f;
    a.SaveMapToFile(dir + "/a.drfmap");
  }
  {
    DrFusion b(o);
    b.TransformMapFile(dir + "/a.drfmap", T, dir + "/b.drfmap");
    b.LoadMapFromFile(dir + "/b.drfmap");
    b.RenderAsync({moved});  // legal after a load, before the next scan
    std::vector<unsigned char *> rb;
    std::vector<float *> rd;
    b.GetRenderResult(rb, rd);
    for (size_t i = 0; i < (size_t)H * W; ++i) after += rd[0][i] > 0.0f;
  }
  if (!(before > (size_t)H * W / 2 && after > before * 8 / 10)) { fprintf(stderr, "map_transform_shim: %zu pixels in the first frame, %zu in the second\n", before, after); return 1; }
  printf("map_transform_shim ok: %zu pixels in the first frame, %zu in the second\n", before, after);
  return 0;
}
