"""-m gpu: drf_track_system / drf_track_frame.  The reference of every bit comparison is the numpy restatement of the rule in
tests/test_map_track.py (np_track_system) and, for whole trackings, track_frame_host through tests/cpp/map_track_check.cpp over
the CPU oracle's ray-cast, which tests/test_map_track.py holds to np_track_frame on every evaluation.  Engines of 5x7, 24x32 and
96x128; the map is the one-scan scene of 1 968 blocks.  DESIGN.md §7c "Tracking a depth frame against the ray-cast model"."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import ROOT, feed, options
from test_fusion_map_file_gpu import code_of, engine
from test_fusion_map_locate_gpu import DeviceDepth, result_dict
from test_fusion_map_transform_gpu import write
from test_map_align import CONVERGED, LOST, MAX_ITERS, assert_same_result, assert_same_system
from test_map_locate import build_check as build_locate_check
from test_map_locate import cpp_frame as cpp_locate_frame
from test_map_track import (BASIN_USED, H, PM, SYSTEM_OPTS, VS, W, basin_start, build_check, cpp_frame, np_track_system, pair_case, pair_poses, track_opts,
                            track_scene)

pytestmark = pytest.mark.gpu
f32 = np.float32


def scratch_bytes(height, width):
    """drf_track_stats()[5]: the groups' partial sums at step 1, 64 bytes of counters, and 24 bytes per pixel."""
    return 224 * (-(-height * width // 512)) + 64 + 24 * height * width


@pytest.fixture(scope="module")
def D(tmp_path_factory):
    """The scene, its map file, and the CPU runs of the basin start, computed once: the tracking, the localisation that follows
    it, and the localisation alone."""
    d = tmp_path_factory.mktemp("track")
    s = track_scene()
    s["file"] = str(d / "scene.drfmap")
    write(s["file"], VS, *s["blocks"])
    HT, HL = build_check(d), build_locate_check(d)
    s["start"] = basin_start(s, BASIN_USED)
    s["opt"] = track_opts(s)
    s["tracked"] = cpp_frame(HT, s["render"], s["cam"], s["depth"], s["start"], **s["opt"])
    s["tracked32"] = s["tracked"]["T"].astype(f32)
    s["located"] = cpp_locate_frame(HL, s["blocks"], s["cam"], s["depth"], s["tracked32"], centre_depth=s["centre_depth"])
    s["alone"] = cpp_locate_frame(HL, s["blocks"], s["cam"], s["depth"], s["start"], centre_depth=s["centre_depth"])
    s["HT"], s["dir"] = HT, d
    return s


def loaded(s, **kw):
    f = engine(s["cam"], **kw)
    f.load_map(s["file"])
    return f


def plain(r):
    return {k: v for k, v in r.items() if k in ("T", "sums", "samples", "valid0", "valid", "cost0", "cost", "iterations", "status")}


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("height,width", [(5, 7), (24, 32), (96, 128)], ids=["35", "768", "12288"])
def test_system_against_the_restatement(height, width):
    """The synthetic pairs of tests/test_map_track.py: every pose under every option set (strides 1 to 3, both centres, a dist_max
    that rejects), host pointers and device pointers, bit for bit; every count class occurs."""
    case = pair_case(7 + height, height, width)
    cam = case["cam"]
    f = engine(cam)
    dd, dm = DeviceDepth(f, case["depth"]), DeviceDepth(f, case["model"])
    seen = np.zeros(4, np.int64)
    for pname, pose in pair_poses(cam):
        for oname, opt in SYSTEM_OPTS:
            want = np_track_system(cam, case["depth"], case["model"], PM, pose, **opt)
            assert_same_system(f.track_system(case["depth"], case["model"], PM, pose, **opt), want, "%s, %s" % (pname, oname))
            step = opt.get("step", 1)
            assert f.track_stats() == (-(-width // step) * -(-height // step), want[1][0], want[1][1], 1, 0, scratch_bytes(height, width))
            assert_same_system(f.track_system(dd.ptr, dm.ptr, PM, pose, **opt), want, "%s, %s (device pointers)" % (pname, oname))
            seen += np.array(want[1]) > 0
    assert (seen > 0).all(), seen
    got = f.track_system(np.zeros((height, width), f32), case["model"], PM, PM)   # no sample: no gather, 28 zeros per group
    assert not got[0].any() and got[1] == (0, 0, 0, 0)
    dd.free()
    dm.free()
    f.close()


# ------------------------------------------------------------------ 2
def test_live_map():
    """Two scans fed.  The public render at Pm, left on the device, as the model of drf_track_system_device equals the first
    evaluation of drf_track_frame started at Pm, and both equal the restatement over the oracle's render."""
    from oracle.tsdf_oracle import TsdfOracle
    from synth import scene
    from test_map_locate import start_near
    s = scene.make_scans(2, H, W, seed=5)
    cam = options(s, H, W, VS)
    f, orc = engine(cam), TsdfOracle(**cam)
    bgr, depth, pose = s["scans"][1]
    Pm = start_near(pose.astype(np.float64), (1, -2, 1), 0.8, (1.0, 0.5, -0.8))
    feed(f, *s["scans"][0])
    f.IntegrateScanAsync(bgr, depth, pose)
    f.RenderAsync([Pm])                                                 # the second scan's render, at Pm
    rb, rd = f.GetRenderResult()
    for scan in s["scans"]:
        orc.integrate(*scan)
    od = orc.render(Pm)[1]
    assert np.array_equal(rd[0].view(np.uint32), od.view(np.uint32))
    dd = DeviceDepth(f, depth)
    opt = dict(centre_depth=2.0)
    want = np_track_system(cam, depth, od, Pm, Pm, **opt)
    got = f.track_system(dd.ptr, f.render_device_pointers()[1], Pm, Pm, **opt)
    assert_same_system(got, want, "the public render as the model")
    r = f.track_frame(depth, Pm, raise_on_failure=False, max_renders=1, inner_iters=1, **opt)
    assert f.track_stats()[:5] == (H * W, want[1][0], want[1][1], 1, 1)
    assert_same_system((r.sums, (r.samples, r.valid, r.samples - r.valid, 0)), (want[0], (want[1][0], want[1][1], want[1][2] + want[1][3], 0)), "the first evaluation")
    assert r.iterations == 1 and want[1][1] > 0.5 * want[1][0]
    dd.free()
    f.close()


# ------------------------------------------------------------------ 3
def test_the_basin_end_to_end(D):
    """drf_track_frame from the basin start, then drf_locate_frame from its pose: every field of both results is the CPU run's;
    drf_locate_frame alone from that start fails as the restatement says."""
    from test_map_locate import SCENE_MEASURED, scene_errors
    f = loaded(D)
    r = f.track_frame(D["depth"], D["start"], **D["opt"])
    st = f.track_stats()
    assert_same_result(result_dict(r), plain(D["tracked"]), "tracking")
    assert st[:5] == (H * W, r.samples, r.valid, r.iterations, D["tracked"]["renders"]) and st[5] == scratch_bytes(H, W)
    assert r.status == CONVERGED and np.array_equal(r.T32, D["tracked32"])
    dd = DeviceDepth(f, D["depth"])
    assert_same_result(result_dict(f.track_frame(dd.ptr, D["start"], **D["opt"])), plain(D["tracked"]), "tracking (device pointer)")
    dd.free()
    l = f.locate_frame(D["depth"], r.T32, centre_depth=D["centre_depth"])
    assert_same_result(result_dict(l), plain(D["located"]), "localisation after the tracking")
    a, t = scene_errors(l.T, D["pose"])
    print("tracked in %d renders and %d evaluations, located in %d: %.5f degrees, %.5f voxels from the scan's pose" % (st[4], st[3], l.iterations, a, t))
    assert l.status == CONVERGED and a <= 2 * SCENE_MEASURED[0] and t <= 2 * SCENE_MEASURED[1]
    alone = f.locate_frame(D["depth"], D["start"], raise_on_failure=False, centre_depth=D["centre_depth"])
    assert_same_result(result_dict(alone), plain(D["alone"]), "localisation alone")
    assert alone.status == LOST or scene_errors(alone.T, D["pose"])[1] > 1.0
    f.close()


def test_statuses(D):
    from tandem_amd.dr_fusion import AlignError
    f = loaded(D)
    r = f.track_frame(D["depth"], D["start"], **dict(D["opt"], max_renders=1))
    assert r.status == MAX_ITERS and r.iterations == 4 and f.track_stats()[4] == 1 and not np.array_equal(r.T32, D["start"])
    gone = D["start"].copy()
    gone[0, 3] += 50 * 8 * VS                                          # the map is 50 blocks away
    with pytest.raises(AlignError) as e:
        f.track_frame(D["depth"], gone, **D["opt"])
    assert e.value.result.status == LOST and e.value.result.valid == 0 and e.value.result.iterations == 1 and "lost" in str(e.value)
    assert np.array_equal(e.value.result.T32, gone)
    f.close()


# ------------------------------------------------------------------ 4
def test_the_map_is_untouched(D):
    from test_map_locate import start_near
    bgr, depth, pose = D["bgr"], D["depth"], D["pose"]
    view = start_near(pose.astype(np.float64), (0, 1, 0), 3.0, (2.0, 0.0, 0.0))

    def render(f):
        f.RenderAsync([view])
        rb, rd = f.GetRenderResult()
        return rb[0].copy(), rd[0].copy()

    def device_render(f):
        """the public render buffers as they lie on the device"""
        pb, pd = f.render_device_pointers()
        b, d = np.empty((H, W, 3), np.uint8), np.empty((H, W), f32)
        assert f._L.dr_memcpy_d2h(b.ctypes.data_as(C.c_void_p), C.c_void_p(pb), b.nbytes) == 0
        assert f._L.dr_memcpy_d2h(d.ctypes.data_as(C.c_void_p), C.c_void_p(pd), d.nbytes) == 0
        return (pb, pd), b, d

    f, g = loaded(D), loaded(D)
    before = (f.export_blocks(), f.stats(), render(f))
    held = device_render(f)
    assert np.array_equal(held[2].view(np.uint32), before[2][1].view(np.uint32))
    assert_same_result(result_dict(f.track_frame(depth, D["start"], **D["opt"])), plain(D["tracked"]), "tracking")
    f.track_system(depth, before[2][1], view, D["start"], step=2)
    again = device_render(f)
    assert again[0] == held[0] and np.array_equal(again[1], held[1]) and np.array_equal(again[2].view(np.uint32), held[2].view(np.uint32))
    after = (f.export_blocks(), f.stats(), render(f))
    assert before[1] == after[1] and before[0].keys() == after[0].keys()
    assert all(np.array_equal(before[0][k], after[0][k]) for k in before[0])
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1].view(np.uint32), after[2][1].view(np.uint32))
    assert np.array_equal(render(g)[1].view(np.uint32), before[2][1].view(np.uint32))
    moved = start_near(pose.astype(np.float64), (1, 0, 0), 2.0, (1.0, 2.0, 0.0))
    for e in (f, g):                                                    # a scan integrated after it: the same map as without
        feed(e, bgr, depth, moved)
    a, b = f.export_blocks(), g.export_blocks()
    assert f.stats() == g.stats() and a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    f.close()
    g.close()


# ------------------------------------------------------------------ 5
def test_streaming(D):
    """Streaming on, the half of the map with x below its median block sent to the host store.  Resident renders miss it and the
    counts say so; map-scope renders -- whole, and in depth bands through a staging a fifth of the size -- give the unbounded
    pool's result bit for bit; a staging too small is DR_ERR_CAPACITY with zeroed stats."""
    from tandem_amd.dr_fusion import RENDER_MAP, RENDER_RESIDENT, streaming_min_radius
    opt = dict(D["opt"], max_renders=2)
    whole = cpp_frame(D["HT"], D["render"], D["cam"], D["depth"], D["start"], **opt)
    f = loaded(D)
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))
    cut = float(np.median(D["blocks"][0][:, 0])) * 8 * VS
    f.stream_out_region((-500.0, -500.0, -500.0), (cut, 500.0, 500.0))
    stored = f.streaming_stats()["host"]
    assert 0 < stored < len(D["blocks"][0])
    f.set_render_scope(RENDER_RESIDENT)
    part = f.track_frame(D["depth"], D["start"], raise_on_failure=False, **opt)
    assert part.valid0 < whole["valid0"] and (part.samples, part.valid0) != (whole["samples"], whole["valid0"])
    f.set_render_scope(RENDER_MAP)
    r = f.track_frame(D["depth"], D["start"], **opt)
    assert_same_result(result_dict(r), plain(whole), "map scope")
    assert np.array_equal(r.T32, whole["T"].astype(f32)) and f.track_stats()[4] == 2
    # depth bands: a staging the planner (run here on the stored blocks) needs at least two passes for at the start's pose
    from test_fusion_render_bands import build_check_library
    from test_fusion_render_bands_gpu import MAX_PASSES, choose_capacity
    one = dict(D["opt"], max_renders=1)
    whole1 = cpp_frame(D["HT"], D["render"], D["cam"], D["depth"], D["start"], **one)
    cap, passes, n = choose_capacity(dict(lib=build_check_library(str(D["dir"] / "librb.so"))), f, [D["start"]], min_passes=2)
    f.set_render_scope(RENDER_MAP, cap)
    assert code_of(f.track_frame, D["depth"], D["start"]) == 5 and f.track_stats() == (0, 0, 0, 0, 0, 0)
    f.set_render_bands(MAX_PASSES)
    assert_same_result(result_dict(f.track_frame(D["depth"], D["start"], **one)), plain(whole1), "map scope, %d depth bands" % passes)
    f.set_render_bands(0)
    f.set_render_scope(RENDER_MAP, 4)
    assert code_of(f.track_frame, D["depth"], D["start"]) == 5 and f.track_stats() == (0, 0, 0, 0, 0, 0)
    assert f.streaming_stats()["host"] == stored
    f.close()


# ------------------------------------------------------------------ 6
def test_legality_in_its_order(D):
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import RENDER_MAP, streaming_min_radius
    f = loaded(D)
    L = f._L
    depth_a, pose_a = np.ascontiguousarray(D["depth"], f32), np.ascontiguousarray(D["start"], f32).reshape(16)
    dp, pp = depth_a.ctypes.data_as(_lib.f32p), pose_a.ctypes.data_as(_lib.f32p)
    sums_a, out_a = np.zeros(28), np.zeros(16, f32)
    sums, counts, out = sums_a.ctypes.data_as(_lib.f64p), (C.c_uint64 * 4)(), out_a.ctypes.data_as(_lib.f32p)
    nothing = lambda: f.track_stats() == (0, 0, 0, 0, 0, 0)  # noqa: E731
    f.track_system(D["depth"], D["depth"], D["start"], D["start"])
    assert not nothing()
    # null arguments (opt and res may be null)
    for args in ((None, dp, pp, pp, None, sums, counts), (dp, None, pp, pp, None, sums, counts), (dp, dp, None, pp, None, sums, counts),
                 (dp, dp, pp, None, None, sums, counts), (dp, dp, pp, pp, None, None, counts), (dp, dp, pp, pp, None, sums, None)):
        assert L.drf_track_system(f._h, *args) == 1 and nothing()
        assert L.drf_track_system_device(f._h, *args) == 1 and nothing()
    for args in ((None, pp, None, out, None), (dp, None, None, out, None), (dp, pp, None, None, None)):
        assert L.drf_track_frame(f._h, *args) == 1 and nothing()
        assert L.drf_track_frame_device(f._h, *args) == 1 and nothing()
    assert L.drf_track_stats(f._h, None) == 1
    one = _lib.TrackOptions(max_renders=1, inner_iters=1)
    assert L.drf_track_frame(f._h, dp, pp, C.byref(one), out, None) == 0 and not nothing()   # res null
    # a bad option is named
    for bad in (dict(step=-1), dict(max_renders=-1), dict(inner_iters=-1), dict(dist_max=float("nan")), dict(max_jump=-1.0), dict(huber=-1.0),
                dict(centre_depth=float("inf")), dict(eps_rot=-1.0), dict(min_valid=-1.0)):
        with pytest.raises(_lib.DrError) as e:
            f.track_frame(D["depth"], D["start"], **bad)
        assert e.value.code == 1 and list(bad)[0] in str(e.value) and nothing(), bad
    with pytest.raises(TypeError):
        f.track_frame(D["depth"], D["start"], no_such_option=1)
    # what is no rigid motion: the pose, and the model's pose
    scaled, nan, mirror = (D["start"].copy() for _ in range(3))
    scaled[:3, :3] *= 1.01
    nan[2, 3] = np.nan
    mirror[:3, 1] *= -1
    for bad in (scaled, nan, mirror):
        assert code_of(f.track_frame, D["depth"], bad) == 1 and nothing()
        assert code_of(f.track_system, D["depth"], D["depth"], D["start"], bad) == 1 and code_of(f.track_system, D["depth"], D["depth"], bad, D["start"]) == 1
    # the capacity stands behind the pose
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))
    f.stream_out_region((-500.0, -500.0, -500.0), (500.0, 500.0, 500.0))
    f.set_render_scope(RENDER_MAP, 4)
    assert code_of(f.track_frame, D["depth"], D["start"]) == 5 and nothing()
    assert code_of(f.track_frame, D["depth"], scaled) == 1
    # where a scan may not be integrated: after the options, before the pose and the capacity
    f.IntegrateScanAsync(np.zeros((H, W, 3), np.uint8), np.zeros((H, W), f32), np.eye(4, dtype=f32))
    assert code_of(f.track_frame, D["depth"], D["start"]) == 2 and code_of(f.track_frame, D["depth"], scaled) == 2 and nothing()
    assert code_of(f.track_system, D["depth"], D["depth"], D["start"], D["start"]) == 2
    with pytest.raises(_lib.DrError) as e:
        f.track_frame(D["depth"], scaled, step=-1)
    assert e.value.code == 1 and "step" in str(e.value)
    f.set_render_scope(RENDER_MAP, 0)
    f.RenderAsync([np.eye(4, dtype=f32)])
    assert code_of(f.track_frame, D["depth"], D["start"]) == 2         # between RenderAsync and GetRenderResult
    f.GetRenderResult()
    r = f.track_frame(D["depth"], D["start"], **D["opt"])              # afterwards the engine answers again, from the host store
    assert_same_result(result_dict(r), plain(D["tracked"]), "afterwards")
    f.close()


# ------------------------------------------------------------------ 7
def test_shim(D, tmp_path):
    """tandem_amd/libdr/dr_fusion.h TrackDepthFrame, then LocateDepthFrame, held to the library's own answers."""
    from tandem_amd import _lib
    f = loaded(D)
    want = f.track_frame(D["depth"], D["start"], **D["opt"])
    want_l = f.locate_frame(D["depth"], want.T32, raise_on_failure=False)   # the shim's LocateDepthFrame passes no options
    f.close()
    exe, frame = str(tmp_path / "map_track_shim"), str(tmp_path / "frame.bin")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_track_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    with open(frame, "wb") as fh:
        fh.write(np.ascontiguousarray(D["start"], f32).tobytes() + bytes(_lib.TrackOptions(**D["opt"])) + np.ascontiguousarray(D["depth"], f32).tobytes())
    cam = D["cam"]
    r = subprocess.run([exe, repr(VS)] + [repr(float(f32(cam[k]))) for k in ("fx", "fy", "cx", "cy")] + [str(cam["num_blocks"]), D["file"], frame],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["track_status"] == want.status == CONVERGED and np.array_equal(f32(js["tracked"]).reshape(4, 4), want.T32)
    assert js["locate_status"] == want_l.status and np.array_equal(f32(js["located"]).reshape(4, 4), want_l.T32)
