"""-m gpu: drf_track_colour_system / drf_track_colour_frame.  The reference of every bit comparison is the numpy restatement of the
rule in tests/test_map_track_colour.py (np_track_colour_system) and, for whole trackings, track_colour_frame_host through
tests/cpp/map_track_colour_check.cpp over the CPU oracle's ray-cast of colour and depth, which tests/test_map_track_colour.py holds
to np_track_colour_frame on every evaluation.  Engines of 5x7 up to 96x128; the maps are the one-scan scene of 1 968 blocks and
five scans of one textured plane.  DESIGN.md §7c "Tracking with colour"."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import test_map_track_colour as TC
from fusion_helpers import ROOT, feed
from test_fusion_map_file_gpu import code_of, engine
from test_fusion_map_locate_gpu import result_dict
from test_fusion_map_track_gpu import plain, scratch_bytes
from test_fusion_map_transform_gpu import write
from test_map_align import CONVERGED, DEGENERATE, assert_same_result, assert_same_system
from test_map_locate import camera, start_near
from test_map_track import H, PM, SYSTEM_OPTS, VS, W, basin_start, np_track_system, pair_poses, pose_near, track_opts, track_scene

pytestmark = pytest.mark.gpu
f32 = np.float32


def colour_scratch_bytes(height, width):
    """drf_track_colour_stats()[5]: the groups' partial sums at step 1, 64 bytes of counters, and 34 bytes per pixel."""
    return 224 * (-(-height * width // 512)) + 64 + 34 * height * width


class DeviceImage:
    """An image (float32 depth or uint8 colour) in device memory: .ptr is what the _device calls take."""

    def __init__(self, f, img, dtype):
        img = np.ascontiguousarray(img, dtype)
        self.L, self.p = f._L, C.c_void_p()
        assert self.L.dr_device_alloc(0, img.nbytes, C.byref(self.p)) == 0
        assert self.L.dr_memcpy_h2d(self.p, img.ctypes.data_as(C.c_void_p), img.nbytes) == 0
        self.ptr = int(self.p.value)

    def free(self):
        self.L.dr_device_free(self.p)


def plane_scans(cam):
    """Five scans of the textured plane of tests/test_map_track_colour.py: the identity and the camera moved sideways and up."""
    render = TC.textured_plane_renderer(cam)
    out = []
    for dx, dy in ((0.0, 0.0), (0.2, 0.0), (-0.2, 0.0), (0.0, 0.15), (0.0, -0.15)):
        p = np.eye(4, dtype=f32)
        p[0, 3], p[1, 3] = dx, dy
        out.append(render(p) + (p,))
    return out


@pytest.fixture(scope="module")
def D(tmp_path_factory):
    """The scene, its map file and the CPU run of the basin start with colour; the plane map in the CPU oracle and the CPU runs on it."""
    from oracle.tsdf_oracle import TsdfOracle
    d = tmp_path_factory.mktemp("track_colour")
    s = track_scene()
    s["file"] = str(d / "scene.drfmap")
    write(s["file"], VS, *s["blocks"])
    HC = TC.build_check(d)
    s["render_both"] = lambda pose: s["oracle"].render(pose)
    s["start"] = basin_start(s, 0)
    s["opt"] = track_opts(s)
    s["tracked"] = TC.cpp_frame(HC, s["render_both"], s["cam"], s["bgr"], s["depth"], s["start"], **s["opt"])
    pc = camera(VS, num_blocks=4000, num_buckets=4000, **TC.PLANE_CAM)
    orc = TsdfOracle(**pc)
    scans = plane_scans(pc)
    for scan in scans:
        orc.integrate(*scan)
    start = TC.plane_start(2)                                             # 8 voxels in the plane, 4 degrees about the normal
    both = lambda pose: orc.render(pose)                                  # noqa: E731
    s["plane"] = dict(cam=pc, scans=scans, start=start, bgr=scans[0][0], depth=scans[0][1],
                      colour=TC.cpp_frame(HC, both, pc, scans[0][0], scans[0][1], start, **TC.PLANE_OPTS),
                      geometric=TC.cpp_frame(HC, both, pc, scans[0][0], scans[0][1], start, colour=False, **TC.PLANE_OPTS))
    s["HC"], s["dir"] = HC, d
    return s


def loaded(s, **kw):
    f = engine(s["cam"], **kw)
    f.load_map(s["file"])
    return f


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("height,width", [(5, 7), (16, 32), (18, 32), (96, 128)], ids=["35", "512", "576", "12288"])
def test_system_against_the_restatement(height, width):
    """The synthetic pairs with colour: three poses under every option set (strides 1 to 3, a weight of its own, a dist_max that
    rejects), host pointers and device pointers, bit for bit, and the stats.  Then frame and model one grey: sums and the first
    four counts are drf_track_system's on the same engine, whose stats the colour calls have not touched."""
    case = TC.colour_pair(7 + height, height, width)
    cam = case["cam"]
    f = engine(cam)
    imgs = [DeviceImage(f, case["bgr"], np.uint8), DeviceImage(f, case["depth"], f32), DeviceImage(f, case["model_bgr"], np.uint8), DeviceImage(f, case["model"], f32)]
    poses = pair_poses(cam)
    for pname, pose in (poses[0], poses[2], poses[5]):
        for oname, opt in TC.COLOUR_OPTS:
            want = TC.np_track_colour_system(cam, case["bgr"], case["depth"], case["model_bgr"], case["model"], PM, pose, **opt)
            got = f.track_colour_system(case["bgr"], case["depth"], case["model_bgr"], case["model"], PM, pose, **opt)
            assert_same_system(got, want, "%s, %s" % (pname, oname))
            step = opt.get("step", 1)
            assert f.track_colour_stats() == (-(-width // step) * -(-height // step), want[1][0], want[1][1], 1, 0, colour_scratch_bytes(height, width))
            got = f.track_colour_system(imgs[0].ptr, imgs[1].ptr, imgs[2].ptr, imgs[3].ptr, PM, pose, **opt)
            assert_same_system(got, want, "%s, %s (device pointers)" % (pname, oname))
            if height >= 16 and oname == "defaults":
                assert want[1][4] > 0
    assert f.track_stats() == (0, 0, 0, 0, 0, 0)
    grey = np.full((height, width, 3), 93, np.uint8)
    for oname, opt in SYSTEM_OPTS[:3]:
        geo = f.track_system(case["depth"], case["model"], PM, pose_near(), **opt)
        held = f.track_stats()
        assert held[5] == scratch_bytes(height, width)
        col = f.track_colour_system(grey, case["depth"], grey, case["model"], PM, pose_near(), **opt)
        assert_same_system((col[0], col[1][:4]), geo, "uniform colour, %s" % oname)
        assert_same_system(geo, np_track_system(cam, case["depth"], case["model"], PM, pose_near(), **opt), "geometric, %s" % oname)
        if col[1][1] > 50:
            assert col[1][4] > 0, "the photometric terms were there"
        assert f.track_stats() == held
    got = f.track_colour_system(case["bgr"], np.zeros((height, width), f32), case["model_bgr"], case["model"], PM, PM)   # no sample
    assert not got[0].any() and got[1] == (0, 0, 0, 0, 0)
    for i in imgs:
        i.free()
    f.close()


# ------------------------------------------------------------------ 2
def test_live_map(D):
    """The scene's scan fed.  The public render at Pm, left on the device, as the model of drf_track_colour_system_device equals the
    first evaluation of drf_track_colour_frame started at Pm, and both equal the restatement over the oracle's render."""
    f = engine(D["cam"])
    bgr, depth, pose = D["bgr"], D["depth"], D["pose"]
    Pm = start_near(pose.astype(np.float64), (1, -2, 1), 0.8, (1.0, 0.5, -0.8))
    f.IntegrateScanAsync(bgr, depth, pose)
    f.RenderAsync([Pm])
    rb, rd = f.GetRenderResult()
    ob, od = D["oracle"].render(Pm)
    assert np.array_equal(rd[0].view(np.uint32), od.view(np.uint32)) and np.array_equal(rb[0], ob)
    db, dd = DeviceImage(f, bgr, np.uint8), DeviceImage(f, depth, f32)
    opt = dict(centre_depth=D["centre_depth"])
    want = TC.np_track_colour_system(D["cam"], bgr, depth, ob, od, Pm, Pm, **opt)
    pb, pd = f.render_device_pointers()
    got = f.track_colour_system(db.ptr, dd.ptr, pb, pd, Pm, Pm, **opt)
    assert_same_system(got, want, "the public render as the model")
    r = f.track_colour_frame(bgr, depth, Pm, raise_on_failure=False, max_renders=1, inner_iters=1, **opt)
    assert f.track_colour_stats()[:5] == (H * W, want[1][0], want[1][1], 1, 1)
    assert_same_system((r.sums, (r.samples, r.valid)), (want[0], want[1][:2]), "the first evaluation")
    assert r.iterations == 1 and want[1][1] > 0.5 * want[1][0] and want[1][4] > 0.5 * want[1][1]
    db.free()
    dd.free()
    f.close()


def test_the_basin_start_end_to_end(D):
    """drf_track_colour_frame from the basin start on the scene map, host and device pointers: every field is the CPU run's."""
    f = loaded(D)
    r = f.track_colour_frame(D["bgr"], D["depth"], D["start"], raise_on_failure=False, **D["opt"])
    st = f.track_colour_stats()
    assert_same_result(result_dict(r), plain(D["tracked"]), "tracking with colour")
    assert st[:5] == (H * W, r.samples, r.valid, r.iterations, D["tracked"]["renders"]) and st[5] == colour_scratch_bytes(H, W)
    assert np.array_equal(r.T32, D["tracked"]["T"].astype(f32))
    db, dd = DeviceImage(f, D["bgr"], np.uint8), DeviceImage(f, D["depth"], f32)
    r2 = f.track_colour_frame(db.ptr, dd.ptr, D["start"], raise_on_failure=False, **D["opt"])
    assert_same_result(result_dict(r2), plain(D["tracked"]), "tracking with colour (device pointers)")
    db.free()
    dd.free()
    f.close()


# ------------------------------------------------------------------ 3
def test_one_textured_plane_in_a_real_map(D):
    """Five scans of the textured plane integrated by the engine; the frame is the first scan, the start 8 voxels off inside the
    plane, half a voxel along the normal and 4 degrees about it.  The CPU oracle's map says beforehand (the fixture) what has to
    come out, and it does bit for bit: drf_track_frame is degenerate or leaves the pose more than a voxel off inside the plane
    (MEASURED on the oracle's map: MAX_ITERS, 4.33 degrees and 7.64 voxels); drf_track_colour_frame ends under one voxel (CONVERGED
    after 3 renders and 7 evaluations, 0.025 voxels in the plane, 0.033 along the normal)."""
    p = D["plane"]
    for name in ("colour", "geometric"):
        print(name, p[name]["status"], p[name]["renders"], p[name]["iterations"], TC.plane_errors(p[name]["T"]))
    assert p["geometric"]["status"] == DEGENERATE or TC.plane_errors(p["geometric"]["T"])[1] > 1.0
    assert p["colour"]["status"] == CONVERGED and TC.plane_errors(p["colour"]["T"])[1] < 1.0
    f = engine(p["cam"])
    for scan in p["scans"]:
        feed(f, *scan)
    geo = f.track_frame(p["depth"], p["start"], raise_on_failure=False, **TC.PLANE_OPTS)
    assert_same_result(result_dict(geo), plain(p["geometric"]), "geometric")
    assert geo.status == DEGENERATE or TC.plane_errors(geo.T)[1] > 1.0
    col = f.track_colour_frame(p["bgr"], p["depth"], p["start"], **TC.PLANE_OPTS)
    assert_same_result(result_dict(col), plain(p["colour"]), "colour")
    a, t, n = TC.plane_errors(col.T)
    print("with colour: status %d, %.5f degrees, %.5f voxels in the plane, %.5f along the normal" % (col.status, a, t, n))
    assert col.status == CONVERGED and t < 1.0
    f.close()


# ------------------------------------------------------------------ 4
def test_nothing_changed(D):
    """Map export, drf_stats, the public render on host and device, drf_track_stats of a geometric call made before -- field [5]
    included -- and the map after the next scan are what they are without the colour calls."""
    bgr, depth, pose = D["bgr"], D["depth"], D["pose"]
    view = start_near(pose.astype(np.float64), (0, 1, 0), 3.0, (2.0, 0.0, 0.0))

    def render(f):
        f.RenderAsync([view])
        rb, rd = f.GetRenderResult()
        return rb[0].copy(), rd[0].copy()

    def device_render(f):
        pb, pd = f.render_device_pointers()
        b, d = np.empty((H, W, 3), np.uint8), np.empty((H, W), f32)
        assert f._L.dr_memcpy_d2h(b.ctypes.data_as(C.c_void_p), C.c_void_p(pb), b.nbytes) == 0
        assert f._L.dr_memcpy_d2h(d.ctypes.data_as(C.c_void_p), C.c_void_p(pd), d.nbytes) == 0
        return (pb, pd), b, d

    f, g = loaded(D), loaded(D)
    before = (f.export_blocks(), f.stats(), render(f))
    held = device_render(f)
    two = dict(D["opt"], max_renders=2)
    geo = f.track_frame(depth, D["start"], raise_on_failure=False, **two)
    geo_stats = f.track_stats()
    assert geo_stats[5] == scratch_bytes(H, W)
    f.track_colour_frame(bgr, depth, D["start"], raise_on_failure=False, **two)
    f.track_colour_system(bgr, depth, before[2][0], before[2][1], view, D["start"], step=2)
    assert f.track_stats() == geo_stats
    again = device_render(f)
    assert again[0] == held[0] and np.array_equal(again[1], held[1]) and np.array_equal(again[2].view(np.uint32), held[2].view(np.uint32))
    geo2 = f.track_frame(depth, D["start"], raise_on_failure=False, **two)
    assert_same_result(result_dict(geo2), result_dict(geo), "the geometric call after the colour calls")
    assert f.track_stats() == geo_stats
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
    counts say so; map-scope renders -- whole, and in depth bands through a smaller staging -- give the unbounded pool's result bit
    for bit; a staging too small is DR_ERR_CAPACITY with zeroed stats."""
    from tandem_amd.dr_fusion import RENDER_MAP, RENDER_RESIDENT, streaming_min_radius
    opt = dict(D["opt"], max_renders=2)
    args = (D["bgr"], D["depth"], D["start"])
    whole = TC.cpp_frame(D["HC"], D["render_both"], D["cam"], *args, **opt)
    f = loaded(D)
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))
    cut = float(np.median(D["blocks"][0][:, 0])) * 8 * VS
    f.stream_out_region((-500.0, -500.0, -500.0), (cut, 500.0, 500.0))
    stored = f.streaming_stats()["host"]
    assert 0 < stored < len(D["blocks"][0])
    f.set_render_scope(RENDER_RESIDENT)
    part = f.track_colour_frame(*args, raise_on_failure=False, **opt)
    assert part.valid0 < whole["valid0"] and (part.samples, part.valid0) != (whole["samples"], whole["valid0"])
    f.set_render_scope(RENDER_MAP)
    r = f.track_colour_frame(*args, raise_on_failure=False, **opt)
    assert_same_result(result_dict(r), plain(whole), "map scope")
    assert np.array_equal(r.T32, whole["T"].astype(f32)) and f.track_colour_stats()[4] == 2
    from test_fusion_render_bands import build_check_library
    from test_fusion_render_bands_gpu import MAX_PASSES, choose_capacity
    one = dict(D["opt"], max_renders=1)
    whole1 = TC.cpp_frame(D["HC"], D["render_both"], D["cam"], *args, **one)
    cap, passes, n = choose_capacity(dict(lib=build_check_library(str(D["dir"] / "librb.so"))), f, [D["start"]], min_passes=2)
    f.set_render_scope(RENDER_MAP, cap)
    assert code_of(f.track_colour_frame, *args) == 5 and f.track_colour_stats() == (0, 0, 0, 0, 0, 0)
    f.set_render_bands(MAX_PASSES)
    assert_same_result(result_dict(f.track_colour_frame(*args, raise_on_failure=False, **one)), plain(whole1), "map scope, %d depth bands" % passes)
    f.set_render_bands(0)
    f.set_render_scope(RENDER_MAP, 4)
    assert code_of(f.track_colour_frame, *args) == 5 and f.track_colour_stats() == (0, 0, 0, 0, 0, 0)
    assert f.streaming_stats()["host"] == stored
    f.close()


# ------------------------------------------------------------------ 6
def test_legality_in_its_order(D):
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import RENDER_MAP, streaming_min_radius
    f = loaded(D)
    L = f._L
    depth_a, pose_a, bgr_a = np.ascontiguousarray(D["depth"], f32), np.ascontiguousarray(D["start"], f32).reshape(16), np.ascontiguousarray(D["bgr"], np.uint8)
    dp, pp, bp = depth_a.ctypes.data_as(_lib.f32p), pose_a.ctypes.data_as(_lib.f32p), C.c_void_p(bgr_a.ctypes.data)
    sums_a, out_a = np.zeros(28), np.zeros(16, f32)
    sums, counts, out = sums_a.ctypes.data_as(_lib.f64p), (C.c_uint64 * 5)(), out_a.ctypes.data_as(_lib.f32p)
    nothing = lambda: f.track_colour_stats() == (0, 0, 0, 0, 0, 0)  # noqa: E731
    f.track_colour_system(D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], D["start"])
    assert not nothing()
    # null arguments (opt and res may be null), the colour images among them
    full = (bp, dp, bp, dp, pp, pp, None, sums, counts)
    for k in (0, 1, 2, 3, 4, 5, 7, 8):
        args = full[:k] + (None,) + full[k + 1:]
        assert L.drf_track_colour_system(f._h, *args) == 1 and nothing(), k
        assert L.drf_track_colour_system_device(f._h, *args) == 1 and nothing(), k
    full = (bp, dp, pp, None, out, None)
    for k in (0, 1, 2, 4):
        args = full[:k] + (None,) + full[k + 1:]
        assert L.drf_track_colour_frame(f._h, *args) == 1 and nothing(), k
        assert L.drf_track_colour_frame_device(f._h, *args) == 1 and nothing(), k
    assert L.drf_track_colour_stats(f._h, None) == 1
    one = _lib.TrackColourOptions(_lib.TrackOptions(max_renders=1, inner_iters=1), 0.0)
    assert L.drf_track_colour_frame(f._h, bp, dp, pp, C.byref(one), out, None) == 0 and not nothing()   # res null
    # a bad option is named
    for bad in (dict(photo_weight=-1.0), dict(photo_weight=float("nan")), dict(photo_weight=float("inf")), dict(step=-1), dict(huber=-1.0), dict(max_jump=-1.0)):
        with pytest.raises(_lib.DrError) as e:
            f.track_colour_frame(D["bgr"], D["depth"], D["start"], **bad)
        assert e.value.code == 1 and list(bad)[0] in str(e.value) and nothing(), bad
    with pytest.raises(TypeError):
        f.track_colour_frame(D["bgr"], D["depth"], D["start"], no_such_option=1)
    # what is no rigid motion: the pose, and the model's pose
    scaled, nan = D["start"].copy(), D["start"].copy()
    scaled[:3, :3] *= 1.01
    nan[2, 3] = np.nan
    for bad in (scaled, nan):
        assert code_of(f.track_colour_frame, D["bgr"], D["depth"], bad) == 1 and nothing()
        assert code_of(f.track_colour_system, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], bad) == 1
        assert code_of(f.track_colour_system, D["bgr"], D["depth"], D["bgr"], D["depth"], bad, D["start"]) == 1
    # the capacity stands behind the pose
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))
    f.stream_out_region((-500.0, -500.0, -500.0), (500.0, 500.0, 500.0))
    f.set_render_scope(RENDER_MAP, 4)
    assert code_of(f.track_colour_frame, D["bgr"], D["depth"], D["start"]) == 5 and nothing()
    assert code_of(f.track_colour_frame, D["bgr"], D["depth"], scaled) == 1
    # where a scan may not be integrated: after the options, before the pose and the capacity
    f.IntegrateScanAsync(np.zeros((H, W, 3), np.uint8), np.zeros((H, W), f32), np.eye(4, dtype=f32))
    assert code_of(f.track_colour_frame, D["bgr"], D["depth"], D["start"]) == 2 and code_of(f.track_colour_frame, D["bgr"], D["depth"], scaled) == 2 and nothing()
    assert code_of(f.track_colour_system, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], D["start"]) == 2
    with pytest.raises(_lib.DrError) as e:
        f.track_colour_frame(D["bgr"], D["depth"], scaled, photo_weight=-2.0)
    assert e.value.code == 1 and "photo_weight" in str(e.value)
    f.set_render_scope(RENDER_MAP, 0)
    f.RenderAsync([np.eye(4, dtype=f32)])
    assert code_of(f.track_colour_frame, D["bgr"], D["depth"], D["start"]) == 2         # between RenderAsync and GetRenderResult
    f.GetRenderResult()
    r = f.track_colour_frame(D["bgr"], D["depth"], D["start"], raise_on_failure=False, **D["opt"])   # afterwards the engine answers again, from the host store
    assert_same_result(result_dict(r), plain(D["tracked"]), "afterwards")
    f.close()


# ------------------------------------------------------------------ 7
def test_shim(D, tmp_path):
    """tandem_amd/libdr/dr_fusion.h TrackColourFrame held to the library's own answer."""
    from tandem_amd import _lib
    opt = dict(D["opt"], max_renders=2)
    f = loaded(D)
    want = f.track_colour_frame(D["bgr"], D["depth"], D["start"], raise_on_failure=False, **opt)
    f.close()
    exe, frame = str(tmp_path / "map_track_colour_shim"), str(tmp_path / "frame.bin")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_track_colour_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    with open(frame, "wb") as fh:
        fh.write(np.ascontiguousarray(D["start"], f32).tobytes() + bytes(_lib.TrackColourOptions(_lib.TrackOptions(**opt), 0.0)) +
                 np.ascontiguousarray(D["depth"], f32).tobytes() + np.ascontiguousarray(D["bgr"], np.uint8).tobytes())
    cam = D["cam"]
    r = subprocess.run([exe, repr(VS)] + [repr(float(f32(cam[k]))) for k in ("fx", "fy", "cx", "cy")] + [str(cam["num_blocks"]), D["file"], frame],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["track_status"] == want.status and np.array_equal(f32(js["tracked"]).reshape(4, 4), want.T32)
