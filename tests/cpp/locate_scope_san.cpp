// The locate-scope rule of tandem_amd/csrc/fusion_host.h under AddressSanitizer and UBSan: a plain executable, nothing preloaded,
// nothing loaded into Python (tests/test_locate_scope.py builds and runs it).  It runs the checks of that test on cases of its own
// (a fixed generator): the selection is a superset of the blocks an evaluation reads, a staging serves a pose whose drift is
// below the slack, a pose a few slacks away reads a block the staging lacks, and the drift bounds the true displacement.
#include <cstdio>

#include "locate_scope_check.cpp"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {  // [0, 1)
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}
static void rigid(const double axis[3], double deg, const double t[3], float out[16]) {
  const double n = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
  const double x = axis[0] / n, y = axis[1] / n, z = axis[2] / n, a = deg * 3.14159265358979323846 / 180.0, c = std::cos(a), s = std::sin(a), C = 1.0 - c;
  const double R[9] = {c + x * x * C, x * y * C - z * s, x * z * C + y * s, y * x * C + z * s, c + y * y * C, y * z * C - x * s, z * x * C - y * s, z * y * C + x * s, c + z * z * C};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out[4 * i + j] = (float)R[3 * i + j];
    out[4 * i + 3] = (float)t[i];
  }
  out[12] = out[13] = out[14] = 0.0f;
  out[15] = 1.0f;
}
static void random_pose(double turn_deg, double move, float out[16]) {
  const double axis[3] = {uniform() - 0.5, uniform() - 0.5, uniform() - 0.5 + 1e-3};
  const double t[3] = {move * (uniform() - 0.5), move * (uniform() - 0.5), move * (uniform() - 0.5)};
  rigid(axis, turn_deg * (2.0 * uniform() - 1.0), t, out);
}
// pose b = pose a moved by the fraction s of a fixed twist
static void moved(const float a[16], const double axis[3], double deg, const double t[3], double s, float b[16]) {
  float d[16];
  const double ts[3] = {t[0] * s, t[1] * s, t[2] * s};
  rigid(axis, deg * s, ts, d);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) b[4 * i + j] = (float)((double)d[4 * i] * a[j] + (double)d[4 * i + 1] * a[4 + j] + (double)d[4 * i + 2] * a[8 + j]);
    b[4 * i + 3] = (float)(((double)d[4 * i] * a[3] + (double)d[4 * i + 1] * a[7] + (double)d[4 * i + 2] * a[11]) + (double)d[4 * i + 3]);
  }
  b[12] = b[13] = b[14] = 0.0f;
  b[15] = 1.0f;
}
static bool subset(const std::vector<u64> &part, const std::vector<u64> &whole) { return std::includes(whole.begin(), whole.end(), part.begin(), part.end()); }

int main() {
  drf_options_t o[2];
  memset(o, 0, sizeof o);
  for (int k = 0; k < 2; ++k) {
    o[k].voxel_size = 0.02f; o[k].num_buckets = 4000; o[k].bucket_size = 10; o[k].num_blocks = 4000; o[k].block_size = 8; o[k].max_sdf_weight = 64;
    o[k].truncation_distance = 0.08f; o[k].max_sensor_depth = 1.0f; o[k].min_sensor_depth = 0.1f; o[k].num_render_streams = 1;
    o[k].fx = 110.0f; o[k].fy = 110.0f; o[k].cx = 63.5f; o[k].cy = 47.5f; o[k].height = 96; o[k].width = 128;
  }
  o[1].fx = 95.0f; o[1].fy = 120.0f; o[1].cx = 20.25f; o[1].cy = 80.5f;  // an off-centre principal point
  const int B = 16;  // the store: every block of [-B, B)^3
  std::vector<u64> box;
  for (int x = -B; x < B; ++x)
    for (int y = -B; y < B; ++y)
      for (int z = -B; z < B; ++z) {
        const int c[3] = {x, y, z};
        u64 k;
        if (!pack_key_host(c, k)) return 1;
        box.push_back(k);
      }
  const double depths[6] = {0.1, 0.2, 0.45, 0.7, 0.9, 1.0};
  std::vector<u64> sel(box.size()), read(box.size());
  int vacuous = 0;
  for (int k = 0; k < 2; ++k) {
    const double slack = ls_slack(&o[k]);
    if (!(slack > 0.0)) { printf("no slack\n"); return 1; }
    for (int it = 0; it < 3; ++it) {
      float a[16], b[16], far[16];
      random_pose(180.0, 0.6, a);
      sel.resize(box.size()); read.resize(box.size());
      sel.resize((size_t)ls_select(box.data(), (int)box.size(), &o[k], a, sel.data(), (int)sel.size()));
      read.resize((size_t)ls_blocks_read(&o[k], a, depths, 6, read.data(), (int)read.size()));
      if (read.empty() || !subset(read, sel)) { printf("the selection misses a block read at its own pose\n"); return 1; }
      if (ls_drift(&o[k], a, a) != 0.0) { printf("drift(a, a) != 0\n"); return 1; }
      // a pose just inside the slack, by bisection on the fraction of a twist
      const double axis[3] = {uniform() - 0.5, uniform() - 0.5, uniform() - 0.5 + 1e-3}, t[3] = {uniform() - 0.5, uniform() - 0.5, uniform() - 0.5};
      double lo = 0.0, hi = 1.0;
      for (int i = 0; i < 40; ++i) {
        const double mid = 0.5 * (lo + hi);
        moved(a, axis, 20.0, t, mid, b);
        (ls_drift(&o[k], a, b) <= slack ? lo : hi) = mid;
      }
      moved(a, axis, 20.0, t, lo, b);
      const double drift = ls_drift(&o[k], a, b);
      if (!(drift <= slack && drift > 0.9 * slack) || ls_drift(&o[k], b, a) != drift || !ls_serves(&o[k], a, b, slack)) { printf("bisection: drift %g, slack %g\n", drift, slack); return 1; }
      if (ls_max_displacement(&o[k], a, b, depths, 6) > drift) { printf("the drift does not bound the displacement\n"); return 1; }
      read.resize(box.size());
      read.resize((size_t)ls_blocks_read(&o[k], b, depths, 6, read.data(), (int)read.size()));
      if (!subset(read, sel)) { printf("a pose within the slack reads a block the staging lacks\n"); return 1; }
      // four slacks away
      moved(a, axis, 20.0, t, 4.0 * lo, far);
      if (ls_serves(&o[k], a, far, slack)) { printf("a pose four slacks away is served\n"); return 1; }
      if (ls_max_displacement(&o[k], a, far, depths, 6) > ls_drift(&o[k], a, far)) { printf("the drift does not bound the displacement (far)\n"); return 1; }
      read.resize(box.size());
      read.resize((size_t)ls_blocks_read(&o[k], far, depths, 6, read.data(), (int)read.size()));
      if (!subset(read, sel)) ++vacuous;
    }
  }
  if (vacuous == 0) { printf("no far pose read a block outside the staging: the rule was not exercised\n"); return 1; }
  printf("far poses that needed a new staging: %d of 6\n", vacuous);
  printf("locate_scope_san ok\n");
  return 0;
}
