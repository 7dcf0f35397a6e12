// The shim's ScoreColourPoses and SearchColourFrame (tandem_amd/libdr/dr_fusion.h) as a TANDEM translation unit would call them: a
// DrFusion of a HEIGHT x WIDTH camera loads MAP, scores FRAME's anchor with colour, searches the lattice of FRAME in it and prints
// the status, the winner's candidate, its final score and the pose as one JSON line, which tests/test_fusion_search_colour_gpu.py
// holds to the library's own answer.  FRAME is raw: 16 anchor floats, height x width x 3 colour bytes, height x width depths.  The
// options: half 3 3 1, top_k 3, pixel step 2, one tracking level, centre depth 1.5 m.
//   map_search_colour_shim VOXEL_SIZE FX FY CX CY NUM_BLOCKS HEIGHT WIDTH MAP FRAME
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dr_fusion.h"

int main(int argc, char **argv) {
  if (argc != 11) { fprintf(stderr, "usage: map_search_colour_shim VOXEL_SIZE FX FY CX CY NUM_BLOCKS HEIGHT WIDTH MAP FRAME\n"); return 2; }
  DrFusionOptions o;
  o.voxel_size = strtof(argv[1], nullptr); o.num_blocks = atoi(argv[6]); o.num_buckets = o.num_blocks; o.bucket_size = 10; o.block_size = 8; o.max_sdf_weight = 64;
  o.truncation_distance = 4 * o.voxel_size; o.max_sensor_depth = 10.0f; o.min_sensor_depth = 0.1f; o.num_render_streams = 1;
  o.fx = strtof(argv[2], nullptr); o.fy = strtof(argv[3], nullptr); o.cx = strtof(argv[4], nullptr); o.cy = strtof(argv[5], nullptr);
  o.height = atoi(argv[7]); o.width = atoi(argv[8]);
  if (o.height <= 0 || o.width <= 0 || o.height > 4096 || o.width > 4096) { fprintf(stderr, "map_search_colour_shim: bad camera\n"); return 2; }
  float anchor[16], out[16];
  std::vector<uint8_t> bgr((size_t)o.height * o.width * 3);
  std::vector<float> depth((size_t)o.height * o.width);
  FILE *f = fopen(argv[10], "rb");
  const bool ok = f && fread(anchor, 4, 16, f) == 16 && fread(bgr.data(), 1, bgr.size(), f) == bgr.size() && fread(depth.data(), 4, depth.size(), f) == depth.size();
  if (f) fclose(f);
  if (!ok) { fprintf(stderr, "map_search_colour_shim: cannot read %s\n", argv[10]); return 2; }
  DrFusion fusion(o);
  fusion.LoadMapFromFile(argv[9]);
  double score = 0.0, photo = 0.0;
  fusion.ScoreColourPoses(bgr.data(), depth.data(), anchor, 1, &score, nullptr, &photo);
  drf_search_colour_options_t so;
  memset(&so, 0, sizeof so);
  so.search.half[0] = so.search.half[1] = 3; so.search.half[2] = 1;
  so.search.top_k = 3;
  so.search.score.step = 2;
  drf_track_pyramid_options_t to;
  memset(&to, 0, sizeof to);
  to.levels = 1; to.colour.track.centre_depth = 1.5f; to.colour.track.eps_rot = 1e-3; to.colour.track.eps_trans = 0.02;
  drf_locate_options_t lo;
  memset(&lo, 0, sizeof lo);
  lo.centre_depth = 1.5f;
  const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  drf_search_colour_result_t res;
  const int status = fusion.SearchColourFrame(bgr.data(), depth.data(), anchor, 1, eye, 1, out, &so, &res, &to, &lo);
  const drf_search_colour_entry_t &e = res.entries[res.winner >= 0 ? res.winner : 0];
  printf("{\"status\": %d, \"anchor_score\": %.17g, \"anchor_photo\": %.17g, \"winner\": %d, \"index\": %llu, \"final_score\": %.17g, \"pose\": [", status, score, photo,
         res.winner, (unsigned long long)e.index, e.final_score);
  for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", out[i]);
  printf("]}\n");
  return 0;
}
