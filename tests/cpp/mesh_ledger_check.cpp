// mesh_ledger_check.cpp -- the bookkeeping of the incremental mesh (tandem_amd/csrc/fusion_host.h MeshUpdateLedger) as a stand-alone
// program: plain g++, no HIP, no device.  tests/test_mesh_ledger_host.py builds it with -Wall -Werror, and once more with
// -fsanitize=address,undefined, and runs it.  Every check is a CHECK(): a failed one prints its line and the program exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../tandem_amd/csrc/fusion_host.h"

using dr::MeshUpdateLedger;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "mesh_ledger_check.cpp:%d: CHECK(%s) failed\n", __LINE__, #c); } } while (0)

static const float kLower[3] = {-1.0f, -2.0f, 0.5f}, kUpper[3] = {3.0f, 2.0f, 4.25f};

// a rigid world-to-camera matrix that differs per k: a rotation about z and a translation
static void rigid_pose(int k, float T[16]) {
  const double a = 0.1 * (k + 1);
  const float c = (float)std::cos(a), s = (float)std::sin(a);
  const float m[16] = {c, -s, 0, 0.25f * k, s, c, 0, -0.5f * k, 0, 0, 1, (float)k, 0, 0, 0, 1};
  memcpy(T, m, sizeof m);
}
static void record(MeshUpdateLedger &l, int first, int n) {
  for (int k = first; k < first + n; ++k) {
    float T[16];
    rigid_pose(k, T);
    l.record_scan(T);
  }
}
// one whole update: decided, launched, fetched; returns whether it was full
static bool update(MeshUpdateLedger &l, const float *lower, const float *upper, unsigned long long redirects) {
  l.begin(lower, upper, redirects);
  const bool full = l.pending().full;
  l.launched();
  l.fetched();
  return full;
}
// a ledger with a fetched baseline {kLower, kUpper, 7 redirects}
static MeshUpdateLedger with_baseline() {
  MeshUpdateLedger l;
  CHECK(update(l, kLower, kUpper, 7));
  return l;
}

static void first_update_is_full() {
  MeshUpdateLedger l;
  CHECK(!l.baseline().valid && l.poses().empty());
  l.begin(kLower, kUpper, 0);
  CHECK(l.pending().valid && l.pending().full && l.pending().nblk == 0);
  MeshUpdateLedger scanned;  // scans before the first update change nothing about that
  record(scanned, 0, 3);
  scanned.begin(kLower, kUpper, 0);
  CHECK(scanned.pending().full);
}

static void same_box_and_redirects_after_rigid_scans_is_partial() {
  for (int n = 1; n <= DRF_MESH_UPDATE_MAX_SCANS; ++n) {
    MeshUpdateLedger l = with_baseline();
    record(l, 0, n);
    CHECK(l.poses().size() == (size_t)n);
    l.begin(kLower, kUpper, 7);
    CHECK(l.pending().valid && !l.pending().full);
    CHECK(l.poses().size() == (size_t)n);  // the launch reads them: begin() keeps them
    float T[16];
    rigid_pose(n - 1, T);
    CHECK(memcmp(l.poses()[n - 1].m, T, 48) == 0);  // rows 0..2 of the matrix given, bit for bit
  }
  MeshUpdateLedger l = with_baseline();  // no scan at all: partial (and the launch has nothing to mesh)
  l.begin(kLower, kUpper, 7);
  CHECK(!l.pending().full && l.poses().empty());
}

static void a_box_float_that_differs_bitwise_is_full() {
  for (int i = 0; i < 6; ++i) {
    MeshUpdateLedger l = with_baseline();
    record(l, 0, 2);
    float lo[3], up[3];
    memcpy(lo, kLower, 12); memcpy(up, kUpper, 12);
    float &f = i < 3 ? lo[i] : up[i - 3];
    f = std::nextafter(f, std::numeric_limits<float>::infinity());  // one ulp
    l.begin(lo, up, 7);
    CHECK(l.pending().full);
    CHECK(memcmp(l.pending().box, lo, 12) == 0 && memcmp(l.pending().box + 3, up, 12) == 0);
  }
  // bitwise, not by value: -0.0f == 0.0f, and yet the box differs
  const float z0[3] = {0.0f, 0.0f, 0.0f}, z1[3] = {-0.0f, 0.0f, 0.0f};
  MeshUpdateLedger l;
  CHECK(update(l, z0, kUpper, 0));
  CHECK(!update(l, z0, kUpper, 0));
  CHECK(update(l, z1, kUpper, 0));
}

static void a_redirect_count_that_differs_is_full() {
  MeshUpdateLedger l = with_baseline();
  record(l, 0, 1);
  CHECK(update(l, kLower, kUpper, 8));
  CHECK(l.baseline().redirects == 8);
  record(l, 1, 1);
  CHECK(!update(l, kLower, kUpper, 8));
}

static void force_full_makes_one_update_full() {
  MeshUpdateLedger l = with_baseline();
  record(l, 0, 1);
  l.force_full();
  CHECK(update(l, kLower, kUpper, 7));   // the next one is full
  record(l, 1, 1);
  CHECK(!update(l, kLower, kUpper, 7));  // the one after it is not
}

static void a_seventeenth_scan_overflows() {
  MeshUpdateLedger l = with_baseline();
  record(l, 0, DRF_MESH_UPDATE_MAX_SCANS + 1);
  CHECK(l.poses().size() == (size_t)DRF_MESH_UPDATE_MAX_SCANS);  // only sixteen are kept
  float T[16];
  rigid_pose(DRF_MESH_UPDATE_MAX_SCANS - 1, T);
  CHECK(memcmp(l.poses().back().m, T, 48) == 0);  // the first sixteen
  CHECK(update(l, kLower, kUpper, 7));
  CHECK(l.poses().empty());
  record(l, 0, DRF_MESH_UPDATE_MAX_SCANS);
  CHECK(!update(l, kLower, kUpper, 7));  // the overflow was that update's alone
}

static void a_pose_that_is_not_a_finite_rigid_motion_is_full() {
  float T[16];
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (int kind = 0; kind < 4; ++kind) {
    MeshUpdateLedger l = with_baseline();
    record(l, 0, 2);
    rigid_pose(5, T);
    if (kind == 0) T[0] *= 1.01f;  // scale: R R^T differs from I by more than 1e-3
    if (kind == 1) T[3] = nan;     // a translation that is not finite
    if (kind == 2) T[7] = inf;
    if (kind == 3) T[5] = nan;     // a rotation entry
    l.record_scan(T);
    CHECK(l.poses().size() == 2);  // it is not kept
    record(l, 2, 1);
    CHECK(l.poses().size() == 3);  // rigid scans after it still are
    CHECK(update(l, kLower, kUpper, 7));
    record(l, 0, 1);
    CHECK(!update(l, kLower, kUpper, 7));
  }
}

static void a_launch_that_threw_leaves_poses_and_flags() {
  {  // force-full survives a begin() that no launched() followed
    MeshUpdateLedger l = with_baseline();
    record(l, 0, 3);
    l.force_full();
    l.begin(kLower, kUpper, 7);
    CHECK(l.pending().full);
    l.begin(kLower, kUpper, 7);  // the caller tries again
    CHECK(l.pending().full && l.poses().size() == 3);
    l.launched();
    l.fetched();
    record(l, 0, 1);
    CHECK(!update(l, kLower, kUpper, 7));
  }
  {  // so does an overflow
    MeshUpdateLedger l = with_baseline();
    record(l, 0, DRF_MESH_UPDATE_MAX_SCANS + 1);
    l.begin(kLower, kUpper, 7);
    l.begin(kLower, kUpper, 7);
    CHECK(l.pending().full && l.poses().size() == (size_t)DRF_MESH_UPDATE_MAX_SCANS);
  }
  {  // and the poses of a partial one; the baseline has not moved
    MeshUpdateLedger l = with_baseline();
    record(l, 0, 4);
    l.begin(kLower, kUpper, 9);
    CHECK(l.pending().full);  // other redirects
    l.begin(kLower, kUpper, 7);
    CHECK(!l.pending().full && l.poses().size() == 4 && l.baseline().redirects == 7);
  }
}

static void scans_between_launch_and_fetch_belong_to_the_next_update() {
  MeshUpdateLedger l = with_baseline();
  record(l, 0, 2);
  l.begin(kLower, kUpper, 7);
  l.launched();
  CHECK(l.poses().empty());
  record(l, 2, 3);  // while the update is in flight
  l.fetched();
  CHECK(l.poses().size() == 3);
  float T[16];
  rigid_pose(2, T);
  CHECK(memcmp(l.poses()[0].m, T, 48) == 0);
  l.begin(kLower, kUpper, 7);
  CHECK(!l.pending().full && l.poses().size() == 3);
  // a non-rigid scan in flight makes the NEXT update full, not the pending one
  MeshUpdateLedger m = with_baseline();
  record(m, 0, 1);
  m.begin(kLower, kUpper, 7);
  m.launched();
  rigid_pose(0, T);
  T[0] = std::numeric_limits<float>::quiet_NaN();
  m.record_scan(T);
  CHECK(!m.pending().full);
  m.fetched();
  CHECK(update(m, kLower, kUpper, 7));
}

static void the_baseline_moves_only_at_fetched() {
  MeshUpdateLedger l = with_baseline();
  const float lo2[3] = {-8.0f, -8.0f, -8.0f}, up2[3] = {8.0f, 8.0f, 8.0f};
  record(l, 0, 1);
  l.begin(lo2, up2, 11);
  l.set_rows(42);
  CHECK(l.baseline().redirects == 7 && memcmp(l.baseline().box, kLower, 12) == 0 && memcmp(l.baseline().box + 3, kUpper, 12) == 0);
  l.launched();
  CHECK(l.baseline().redirects == 7 && memcmp(l.baseline().box, kLower, 12) == 0);
  CHECK(l.pending().nblk == 42 && l.pending().full);
  l.fetched();
  CHECK(l.baseline().valid && l.baseline().redirects == 11 && l.baseline().nblk == 42);
  CHECK(memcmp(l.baseline().box, lo2, 12) == 0 && memcmp(l.baseline().box + 3, up2, 12) == 0);
  // an update launched and never fetched is replaced: the old baseline still decides
  MeshUpdateLedger m = with_baseline();
  m.begin(lo2, up2, 7);
  m.launched();
  record(m, 0, 1);
  m.begin(kLower, kUpper, 7);
  CHECK(!m.pending().full);
}

int main() {
  first_update_is_full();
  same_box_and_redirects_after_rigid_scans_is_partial();
  a_box_float_that_differs_bitwise_is_full();
  a_redirect_count_that_differs_is_full();
  force_full_makes_one_update_full();
  a_seventeenth_scan_overflows();
  a_pose_that_is_not_a_finite_rigid_motion_is_full();
  a_launch_that_threw_leaves_poses_and_flags();
  scans_between_launch_and_fetch_belong_to_the_next_update();
  the_baseline_moves_only_at_fetched();
  if (failures) { printf("mesh_ledger_check: %d checks failed\n", failures); return 1; }
  printf("mesh_ledger_check ok\n");
  return 0;
}
