// engine_host_check.cpp -- the DrFusion engine's call order (CallOrder) and the locate scope's restaging rule (LocateStageCursor),
// tandem_amd/csrc/engine_host.h, as a stand-alone program: plain g++, no HIP, no device.  tests/test_engine_host.py builds it with
// -Wall -Werror, and once more with -fsanitize=address,undefined, and runs it.  Every check is a CHECK(): a failed one prints its
// line and the program exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../tandem_amd/csrc/fusion_host.h"

using dr::CallOrder;
using dr::HostBlockStore;
using dr::LocateStageCursor;

namespace dr { std::string &last_error_slot() { static std::string s; return s; } }

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "engine_host_check.cpp:%d: CHECK(%s) failed\n", __LINE__, #c); } } while (0)

// ------------------------------------------------------------------ CallOrder
// The engine's calls as they use the value: the check first, the transition once the call goes ahead.
static const char *kNames[] = {"IntegrateScanAsync", "RenderAsync", "GetRenderResult"};
static void scan(CallOrder &o) { o.expect(CallOrder::kIntegrate, "scan."); o.scan_begun(); }
static void render(CallOrder &o) { o.expect_render("render."); o.render_begun(); }
static void fetch(CallOrder &o) { o.expect(CallOrder::kGetRender, "fetch."); o.result_fetched(); }
static void other(CallOrder &o) { o.expect_integrate("drf_other"); }
static void load(CallOrder &o) { o.expect_integrate("drf_load_map"); o.map_loaded(); }

// what a call answers: -1 = it went ahead, otherwise the state (0..2) its refusal names; the code and the text are checked here
static int outcome(CallOrder &o, void (*call)(CallOrder &), const char *msg) {
  try {
    call(o);
    return -1;
  } catch (const dr::Error &e) {
    CHECK(e.code == DR_ERR_PROTOCOL);
    const std::string what = e.what(), head = std::string(msg) + " You should have called ";
    CHECK(what.compare(0, head.size(), head) == 0);
    for (int k = 0; k < 3; ++k)
      if (what == head + kNames[k]) return k;
    CHECK(!"the refusal names no call");
    return -2;
  }
}
// the state of a value, told by what it refuses and allows alone (none of the probes below changes it)
struct Seen { bool scan_ok, render_ok, fetch_ok, pending; };
static Seen probe(const CallOrder &o) {
  Seen s{true, true, true, o.render_pending()};
  try { o.expect(CallOrder::kIntegrate, "p"); } catch (const dr::Error &) { s.scan_ok = false; }
  try { o.expect_render("p"); } catch (const dr::Error &) { s.render_ok = false; }
  try { o.expect(CallOrder::kGetRender, "p"); } catch (const dr::Error &) { s.fetch_ok = false; }
  return s;
}
static bool same(const Seen &a, const Seen &b) { return a.scan_ok == b.scan_ok && a.render_ok == b.render_ok && a.fetch_ok == b.fetch_ok && a.pending == b.pending; }

static CallOrder at_integrate() { return CallOrder(); }
static CallOrder at_render() { CallOrder o; scan(o); return o; }
static CallOrder at_fetch() { CallOrder o; scan(o); render(o); return o; }

static void the_legal_cycle() {
  CallOrder o;
  for (int k = 0; k < 3; ++k) {
    CHECK(o.scan_may_come() && !o.render_pending());
    CHECK(outcome(o, other, "drf_other: call it where IntegrateScanAsync may be called.") == -1);
    CHECK(outcome(o, scan, "scan.") == -1);
    CHECK(!o.scan_may_come() && !o.render_pending());
    CHECK(outcome(o, render, "render.") == -1);
    CHECK(!o.scan_may_come() && o.render_pending());
    CHECK(outcome(o, fetch, "fetch.") == -1);
  }
  CHECK(o.scan_may_come());
}

static void every_illegal_call_names_the_call_that_should_have_come() {
  struct Call { void (*f)(CallOrder &); const char *msg; bool legal[3]; };  // legal[state]: kIntegrate, kRender, kGetRender
  const Call calls[] = {{scan, "scan.", {true, false, false}},
                        {render, "render.", {false, true, false}},
                        {fetch, "fetch.", {false, false, true}},
                        {other, "drf_other: call it where IntegrateScanAsync may be called.", {true, false, false}},
                        {load, "drf_load_map: call it where IntegrateScanAsync may be called.", {true, false, false}}};
  CallOrder (*const states[])() = {at_integrate, at_render, at_fetch};
  for (int st = 0; st < 3; ++st)
    for (const Call &c : calls) {
      CallOrder o = states[st]();
      const Seen before = probe(o);
      const int got = outcome(o, c.f, c.msg);
      if (c.legal[st]) { CHECK(got == -1); continue; }
      CHECK(got == st);                // the text names the call of the state it is in
      CHECK(same(probe(o), before));  // and a refused call leaves the state as it was
      CHECK(outcome(o, c.f, c.msg) == st);
    }
}

static void a_render_is_legal_straight_after_loaded_and_not_after_the_next_scan() {
  CallOrder o;
  CHECK(outcome(o, render, "render.") == 0);  // a new engine: no render before a scan
  CHECK(outcome(o, load, "drf_load_map: call it where IntegrateScanAsync may be called.") == -1);
  CHECK(o.scan_may_come() && !o.render_pending());
  CHECK(outcome(o, render, "render.") == -1);
  CHECK(o.render_pending());
  CHECK(outcome(o, fetch, "fetch.") == -1);
  CHECK(outcome(o, render, "render.") == -1);  // still the loaded map: no scan followed
  CHECK(outcome(o, fetch, "fetch.") == -1);
  CHECK(outcome(o, scan, "scan.") == -1);      // a scan is legal there as well, and ends the exception
  CHECK(outcome(o, render, "render.") == -1);
  CHECK(outcome(o, fetch, "fetch.") == -1);
  CHECK(outcome(o, render, "render.") == 0);
  CallOrder p = at_render();  // "loaded" is an exception where a scan may come only: not while a render is due or pending
  p.map_loaded();
  CHECK(outcome(p, fetch, "fetch.") == 1);
  render(p);
  CHECK(outcome(p, render, "render.") == 2);
}

static void render_pending_is_true_only_between_render_and_fetch() {
  CallOrder o;
  CHECK(!o.render_pending());
  load(o);
  CHECK(!o.render_pending());
  scan(o);
  CHECK(!o.render_pending());
  render(o);
  CHECK(o.render_pending());
  CHECK(outcome(o, scan, "scan.") == 2 && o.render_pending());
  fetch(o);
  CHECK(!o.render_pending());
}

// ------------------------------------------------------------------ LocateStageCursor
static drf_options_t camera() {
  drf_options_t o;
  memset(&o, 0, sizeof o);
  o.voxel_size = 0.02f; o.block_size = 8; o.num_blocks = 1024; o.num_buckets = 1024; o.bucket_size = 4; o.max_sdf_weight = 64;
  o.truncation_distance = 0.08f; o.max_sensor_depth = 2.0f; o.min_sensor_depth = 0.1f; o.num_render_streams = 1;
  o.width = 64; o.height = 48; o.fx = 60.0f; o.fy = 60.0f; o.cx = 31.5f; o.cy = 23.5f;
  return o;
}
// a camera at (x, 0, 0) that looks along +z
static void pose_at(double x, float T[16]) {
  const float m[16] = {1, 0, 0, (float)x, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  memcpy(T, m, sizeof m);
}
// a slab of blocks one metre in front of the camera at x: 4 x 3 x 3 = 36 of them, 0.16 m apart
static void put_slab(HostBlockStore &s, double x, float vs) {
  static const uint8_t zero[4096] = {};
  const long bx = std::lround(x / (8.0 * vs)), bz = std::lround(1.0 / (8.0 * vs));
  for (long i = 0; i < 4; ++i)
    for (long j = -1; j <= 1; ++j)
      for (long k = 0; k < 3; ++k) s.put(dr::pack_biased(bx + i - 2, j, bz + k), zero);
}
static const double kFar = 40.0;  // a second place: nothing of either slab is in reach of the other

static void an_empty_store_never_stages() {
  const drf_options_t o = camera();
  HostBlockStore store;
  LocateStageCursor c(store, o, dr::locate_stage_slack(o), 16);
  float p[16];
  pose_at(0.0, p);
  CHECK(c.begin(p).kind != LocateStageCursor::kTooMany);
  for (double x : {0.0, 0.001, 5.0, kFar}) {
    pose_at(x, p);
    const LocateStageCursor::Step s = c.at(p);
    CHECK(s.kind == LocateStageCursor::kKeep && s.count == 0);
  }
}

static void a_first_pose_over_capacity_is_refused_before_any_stage() {
  const drf_options_t o = camera();
  HostBlockStore store;
  put_slab(store, 0.0, o.voxel_size);
  float p[16];
  pose_at(0.0, p);
  const size_t n = dr::select_locate_blocks(store, o, p).size();
  CHECK(n == 36);
  LocateStageCursor small(store, o, dr::locate_stage_slack(o), n - 1);
  const LocateStageCursor::Step s = small.begin(p);
  CHECK(s.kind == LocateStageCursor::kTooMany && s.count == n);
  CHECK(small.keys().empty());  // nothing was selected, nothing can be staged
  LocateStageCursor fits(store, o, dr::locate_stage_slack(o), n);
  CHECK(fits.begin(p).kind == LocateStageCursor::kStage);
}

static void poses_inside_the_slack_give_one_stage_then_keep() {
  const drf_options_t o = camera();
  const double slack = dr::locate_stage_slack(o);
  CHECK(slack > 0.05);  // 8 sqrt(3) voxels less the pose's tolerance: about 0.26 m here
  HostBlockStore store;
  put_slab(store, 0.0, o.voxel_size);
  LocateStageCursor c(store, o, slack, 64);
  float p0[16], p[16];
  pose_at(0.0, p0);
  const LocateStageCursor::Step b = c.begin(p0);
  CHECK(b.kind == LocateStageCursor::kStage && b.count == 36);
  const std::vector<unsigned long long> first = dr::select_locate_blocks(store, o, p0);
  const LocateStageCursor::Step s0 = c.at(p0);
  CHECK(s0.kind == LocateStageCursor::kStage && s0.count == 36 && c.keys() == first);
  int stages = 1;
  for (int k = 1; k <= 20; ++k) {  // a refinement that creeps, every pose within the slack of the selection's
    pose_at(0.9 * slack * k / 20.0, p);
    CHECK(dr::locate_stage_serves(o, p0, p, slack));
    const LocateStageCursor::Step s = c.at(p);
    if (s.kind != LocateStageCursor::kKeep) ++stages;
    CHECK(s.kind == LocateStageCursor::kKeep && s.count == 36);
    CHECK(c.keys() == first && memcmp(c.pose(), p0, 64) == 0);
  }
  CHECK(stages == 1);
}

static void one_pose_beyond_the_slack_stages_the_new_selection() {
  const drf_options_t o = camera();
  const double slack = dr::locate_stage_slack(o);
  HostBlockStore store;
  put_slab(store, 0.0, o.voxel_size);
  put_slab(store, 1.6, o.voxel_size);  // further blocks: beside the first camera's pyramid, inside the moved one's
  LocateStageCursor c(store, o, slack, 128);
  float p0[16], p1[16];
  pose_at(0.0, p0);
  pose_at(1.0, p1);
  CHECK(!dr::locate_stage_serves(o, p0, p1, slack));
  c.begin(p0);
  CHECK(c.at(p0).kind == LocateStageCursor::kStage);
  const std::vector<unsigned long long> a = c.keys(), want = dr::select_locate_blocks(store, o, p1);
  CHECK(want != a && !want.empty());
  const LocateStageCursor::Step s = c.at(p1);
  CHECK(s.kind == LocateStageCursor::kStage && s.count == want.size() && c.keys() == want && memcmp(c.pose(), p1, 64) == 0);
  CHECK(c.at(p1).kind == LocateStageCursor::kKeep);  // and serves from there
  CHECK(c.at(p0).kind == LocateStageCursor::kStage && c.keys() == a);  // back beyond the slack: staged again
}

static void a_move_onto_an_empty_selection_is_a_release() {
  const drf_options_t o = camera();
  HostBlockStore store;
  put_slab(store, 0.0, o.voxel_size);
  LocateStageCursor c(store, o, dr::locate_stage_slack(o), 64);
  float p0[16], p1[16];
  pose_at(0.0, p0);
  pose_at(kFar, p1);
  c.begin(p0);
  CHECK(c.at(p0).kind == LocateStageCursor::kStage && c.keys().size() == 36);
  const LocateStageCursor::Step s = c.at(p1);
  CHECK(s.kind == LocateStageCursor::kStage && s.count == 0 && c.keys().empty());  // stage nothing: release, the resident kernel
  const LocateStageCursor::Step k = c.at(p1);
  CHECK(k.kind == LocateStageCursor::kKeep && k.count == 0);
}

static void a_move_onto_a_selection_over_capacity_is_refused_and_the_staging_stays_current() {
  const drf_options_t o = camera();
  const double slack = dr::locate_stage_slack(o);
  HostBlockStore store;
  put_slab(store, 0.0, o.voxel_size);
  put_slab(store, kFar, o.voxel_size);
  put_slab(store, kFar + 0.64, o.voxel_size);  // the second place holds more than the first
  float p0[16], p1[16], p[16];
  pose_at(0.0, p0);
  pose_at(kFar + 0.32, p1);
  const size_t n0 = dr::select_locate_blocks(store, o, p0).size(), n1 = dr::select_locate_blocks(store, o, p1).size();
  CHECK(n0 == 36 && n1 > n0);
  LocateStageCursor c(store, o, slack, n0);
  CHECK(c.begin(p0).kind == LocateStageCursor::kStage);
  CHECK(c.at(p0).kind == LocateStageCursor::kStage);
  const std::vector<unsigned long long> a = c.keys();
  const LocateStageCursor::Step s = c.at(p1);
  CHECK(s.kind == LocateStageCursor::kTooMany && s.count == n1);
  CHECK(c.keys() == a && memcmp(c.pose(), p0, 64) == 0);  // what is staged is still what the cursor reports
  pose_at(0.5 * slack, p);
  CHECK(c.at(p).kind == LocateStageCursor::kKeep);
  CHECK(c.at(p1).kind == LocateStageCursor::kTooMany);  // and asked again it refuses again
}

static void slack_zero_stages_at_every_pose_that_differs() {
  const drf_options_t o = camera();
  HostBlockStore store;
  put_slab(store, 0.0, o.voxel_size);
  LocateStageCursor c(store, o, 0.0, 64);
  float p[16];
  pose_at(0.0, p);
  c.begin(p);
  CHECK(c.at(p).kind == LocateStageCursor::kStage);
  CHECK(c.at(p).kind == LocateStageCursor::kKeep);  // the same pose: a drift of 0 is within a slack of 0
  for (int k = 1; k <= 5; ++k) {
    pose_at(1e-4 * k, p);
    const LocateStageCursor::Step s = c.at(p);
    CHECK(s.kind == LocateStageCursor::kStage && s.count == 36 && memcmp(c.pose(), p, 64) == 0);
    CHECK(c.at(p).kind == LocateStageCursor::kKeep);
  }
}

int main() {
  the_legal_cycle();
  every_illegal_call_names_the_call_that_should_have_come();
  a_render_is_legal_straight_after_loaded_and_not_after_the_next_scan();
  render_pending_is_true_only_between_render_and_fetch();
  an_empty_store_never_stages();
  a_first_pose_over_capacity_is_refused_before_any_stage();
  poses_inside_the_slack_give_one_stage_then_keep();
  one_pose_beyond_the_slack_stages_the_new_selection();
  a_move_onto_an_empty_selection_is_a_release();
  a_move_onto_a_selection_over_capacity_is_refused_and_the_staging_stays_current();
  slack_zero_stages_at_every_pose_that_differs();
  if (failures) { printf("engine_host_check: %d checks failed\n", failures); return 1; }
  printf("engine_host_check ok\n");
  return 0;
}
