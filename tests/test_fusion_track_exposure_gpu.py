"""-m gpu: drf_track_exposure_system / drf_track_exposure_frame.  The reference of every bit comparison is the numpy restatement of
the rule in tests/test_map_track_exposure.py (np_exposure_system) and, for whole trackings, track_exposure_frame_host through
tests/cpp/map_track_exposure_check.cpp over the CPU oracle's ray-cast of colour and depth, which tests/test_map_track_exposure.py
holds to np_track_exposure_frame.  Engines of 5x7 up to 96x128; the maps are the textured plane of five scans and the one-scan
scene.  DESIGN.md §7c "Tracking under a change of exposure"."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import test_map_track_colour as TC
import test_map_track_exposure as TX
import test_map_track_pyramid as TP
from fusion_helpers import ROOT, feed
from test_fusion_map_file_gpu import engine
from test_fusion_map_locate_gpu import result_dict
from test_fusion_map_track_gpu import plain
from test_fusion_map_transform_gpu import write
from test_fusion_track_colour_gpu import DeviceImage, plane_scans
from test_fusion_track_pyramid_gpu import code_of, download
from test_map_align import CONVERGED, assert_same_result, bits
from test_map_locate import camera, start_near
from test_map_track import H, PM, VS, W, basin_start, pair_poses, track_opts, track_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
NOTHING = (0, 0, 0, 0, 0, 0, 0, 0)


def exposure_scratch_bytes(height, width):
    """drf_track_exposure_stats()[5] by the header's formula: the spans one behind the other, each at its element's alignment."""
    n = height * width
    g = -(-n // 512)
    lv = [max(1, (width >> L) * (height >> L)) for L in range(5)]
    spans = [(360 * g, 8), (48, 8), (4, 4), (16 * n, 32), (8 * n, 8), (4 * n, 4), (4 * lv[1], 4), (4 * n, 4), (4 * n, 4)] + [(4 * lv[L], 4) for L in range(1, 5)]
    spans += [(3 * n, 1), (3 * lv[1], 1), (3 * n, 1)] + [(3 * lv[L], 1) for L in range(1, 5)]
    at = 0
    for size, align in spans:
        at = -(-at // align) * align + size
    return at


def exposure_dict(r):
    d = result_dict(r)
    d.update(gain=r.gain, offset=r.offset, ext=r.ext, held=r.held, photometric=r.photometric)
    return d


def assert_same_exposure_run(f, r, want, what):
    """An ExposureResult of the engine and its statistics against a dict of TX.cpp_frame / TX.np_track_exposure_frame"""
    assert_same_result(result_dict(r), plain(want), what)
    assert np.array_equal(r.T32, want["T"].astype(f32)), what
    for k in ("gain", "offset", "ext"):
        assert np.array_equal(bits(getattr(r, k)), bits(want[k])), "%s: %s differs: %s against %s" % (what, k, getattr(r, k), want[k])
    assert (r.held, r.photometric) == (want["held"], want["photometric"]), what
    st = f.track_exposure_stats()
    assert st[:5] == want["stats8"][:5] and st[6:] == want["stats8"][6:] and st[5] > 0, "%s: %s against %s" % (what, st, want["stats8"])
    levels = {L: f.track_exposure_level_stats(L) for L in range(5)}
    assert {L: v for L, v in levels.items() if v[2]} == want["levels"], "%s: %s against %s" % (what, levels, want["levels"])


@pytest.fixture(scope="module")
def D(tmp_path_factory):
    """The plane map in the CPU oracle with the CPU run of the re-exposed frame on it; the scene, its map file and the CPU run on it."""
    from oracle.tsdf_oracle import TsdfOracle
    d = tmp_path_factory.mktemp("track_exposure")
    HX = TX.build_check(d)
    pc = camera(VS, num_blocks=4000, num_buckets=4000, **TC.PLANE_CAM)
    orc = TsdfOracle(**pc)
    scans = plane_scans(pc)
    for scan in scans:
        orc.integrate(*scan)
    start = TC.plane_start(3)                                             # the largest start of the CPU test: 12 voxels, 6 degrees
    frame = TX.re_expose(scans[0][0], 0.6, 60.0)
    plane = dict(cam=pc, scans=scans, start=start, bgr=frame, depth=scans[0][1],
                 tracked=TX.cpp_frame(HX, lambda pose: orc.render(pose), pc, frame, scans[0][1], start, **TX.PLANE_OPTS))
    s = track_scene()
    s["file"] = str(d / "scene.drfmap")
    write(s["file"], VS, *s["blocks"])
    s["start"] = basin_start(s, 0)
    s["opt"] = track_opts(s, max_renders=2, coarse_renders=2)
    s["bgr2"] = TX.re_expose(s["bgr"], 0.8, 25.0)
    s["tracked"] = TX.cpp_frame(HX, lambda pose: s["oracle"].render(pose), s["cam"], s["bgr2"], s["depth"], s["start"], levels=3, **s["opt"])
    s["plane"], s["HX"], s["dir"] = plane, HX, d
    return s


def loaded(s, **kw):
    f = engine(s["cam"], **kw)
    f.load_map(s["file"])
    return f


def plane_engine(D):
    p = D["plane"]
    f = engine(p["cam"])
    for scan in p["scans"]:
        feed(f, *scan)
    return f


# ------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("height,width", TX.SHAPES, ids=["35", "512", "576", "12288"])
def test_system_against_the_restatement(height, width):
    """The synthetic pairs at two exposures, levels 0 and 1 (5x7: level 0 alone), host and device pointers: the 45 sums and the five
    counters bit for bit, the statistics and the scratch formula.  At (1, 0) sums[0..27] and the counters are
    drf_track_pyramid_system's of the same engine (5x7, which that family refuses: drf_track_colour_system's)."""
    case = TC.colour_pair(7 + height, height, width)
    cam, d, bgr, mb, md = case["cam"], case["depth"], case["bgr"], case["model_bgr"], case["model"]
    f = engine(cam)
    imgs = [DeviceImage(f, bgr, np.uint8), DeviceImage(f, d, f32), DeviceImage(f, mb, np.uint8), DeviceImage(f, md, f32)]
    p = [i.ptr for i in imgs]
    poses = pair_poses(cam)
    ran = 0
    for L in (0, 1):
        if L > 0 and not TP.level_fits(cam, L):
            assert code_of(f.track_exposure_system, L, bgr, d, mb, md, PM, poses[0][1], levels=1) == 1 and f.track_exposure_stats() == NOTHING
            continue
        for pname, pose in (poses[0], poses[2]):
            for oname, opt in TC.COLOUR_OPTS[:2]:
                opt = dict(opt, levels=L + 1)
                step = opt.get("step", 1)
                for G, B in TX.EXPOSURES[:2]:
                    want = TX.np_exposure_system(cam, L, bgr, d, mb, md, PM, pose, G, B, **opt)
                    got = f.track_exposure_system(L, bgr, d, mb, md, PM, pose, G, B, **opt)
                    TX.assert_same_sums(got, want, "level %d, %s, %s at (%g, %g)" % (L, pname, oname, G, B))
                    st = f.track_exposure_stats()
                    assert st == (-(-(width >> L) // step) * -(-(height >> L) // step), want[1][0], want[1][1], 1, 0, exposure_scratch_bytes(height, width), 1, 0), st
                    assert f.track_exposure_level_stats(L) == (0, 0, 1, want[1][1])
                    got = f.track_exposure_system(L, p[0], p[1], p[2], p[3], PM, pose, G, B, **opt)
                    TX.assert_same_sums(got, want, "level %d, %s, %s at (%g, %g) (device pointers)" % (L, pname, oname, G, B))
                    if (G, B) == (1.0, 0.0):
                        if TP.level_fits(cam, L):
                            pyr = f.track_pyramid_system(L, bgr, d, mb, md, PM, pose, **opt)
                        else:
                            pyr = f.track_colour_system(bgr, d, mb, md, PM, pose, **{k: v for k, v in opt.items() if k != "levels"})
                        assert np.array_equal(bits(got[0][:28]), bits(pyr[0])) and got[1] == pyr[1], "the invariant: level %d, %s, %s" % (L, pname, oname)
                    ran += 1
    assert ran == (8 if height == 5 else 16)
    got = f.track_exposure_system(0, bgr, np.zeros((height, width), f32), mb, md, PM, PM, 0.7, 12.5, levels=1)   # no sample
    assert not got[0].any() and got[1] == (0, 0, 0, 0, 0)
    assert f.track_stats() == (0, 0, 0, 0, 0, 0)
    for i in imgs:
        i.free()
    f.close()


# ------------------------------------------------------------------ 3
def test_the_plane_in_a_real_map(D):
    """The five plane scans integrated by the engine, the frame re-exposed at (0.6, +60), the largest start of the CPU test: the
    result, the gain and the offset are the host reference's over the oracle's renders bit for bit, host and device pointers; the
    pose ends CONVERGED below one voxel in the plane -- and drf_track_pyramid_frame on the same inputs does not end below one
    voxel.  (Measured on the host reference: 0.022 voxels, gain 0.6018, offset 61.65 -- the map's colours are a fused average of
    five scans, not the analytic plane's, so the CPU test's tolerances on gain and offset are not asked for here; the pyramid
    call ends MAX_ITERS 2.48 voxels off.)"""
    p = D["plane"]
    f = plane_engine(D)
    r = f.track_exposure_frame(p["bgr"], p["depth"], p["start"], raise_on_failure=False, **TX.PLANE_OPTS)
    assert_same_exposure_run(f, r, p["tracked"], "the plane at (0.6, +60)")
    a, t, nrm = TC.plane_errors(r.T)
    print("exposure call: status %d, %.4f voxels in the plane, gain %.5f offset %.3f, stats %s" % (r.status, t, r.gain, r.offset, f.track_exposure_stats()))
    assert r.status == CONVERGED and t < 1.0
    db, dd = DeviceImage(f, p["bgr"], np.uint8), DeviceImage(f, p["depth"], f32)
    r = f.track_exposure_frame(db.ptr, dd.ptr, p["start"], raise_on_failure=False, **TX.PLANE_OPTS)
    assert_same_exposure_run(f, r, p["tracked"], "the plane at (0.6, +60) (device pointers)")
    pyr = f.track_pyramid_frame(p["bgr"], p["depth"], p["start"], raise_on_failure=False, **TC.PLANE_OPTS)
    tp = TC.plane_errors(pyr.T)[1]
    print("pyramid call: status %d, %.4f voxels in the plane" % (pyr.status, tp))
    assert tp > 1.0, "the call without an exposure ends more than one voxel off"
    db.free()
    dd.free()
    f.close()


def test_three_levels_on_the_scene_map(D):
    """The scene map, the frame re-exposed at (0.8, +25), three levels of two renders: every field, the exposure, the totals and
    the per-level outcomes are the CPU host run's over the oracle's renders."""
    f = loaded(D)
    r = f.track_exposure_frame(D["bgr2"], D["depth"], D["start"], raise_on_failure=False, levels=3, **D["opt"])
    assert_same_exposure_run(f, r, D["tracked"], "three levels on the scene")
    assert f.track_exposure_stats()[5] == exposure_scratch_bytes(H, W)
    f.close()


# ------------------------------------------------------------------ 4
def test_one_colour_equals_the_pyramid_call(D):
    """A map and a frame of one colour: the scene's scan fed with a black colour image, whose ray-cast is black at every pixel,
    exactly.  The gain's column is zero, every evaluation holds the exposure, and the call equals drf_track_pyramid_frame bit for
    bit; held equals the evaluations.  (Black, not the grey 93 of the CPU test, whose model the test hands over as one colour: the
    engine's ray-cast of a grey-93 map is 92 at a sixth of its pixels and 0 at its rim -- the rounding of the interpolated colour --
    so to the tracker that map is NOT of one colour, the exposure is solved from those few levels, and the call differs from the
    pyramid's: DESIGN.md "Tracking under a change of exposure" has the figures.)"""
    black = np.zeros((H, W, 3), np.uint8)
    f = engine(D["cam"])
    feed(f, black, D["depth"], D["pose"])
    pyr = f.track_pyramid_frame(black, D["depth"], D["start"], raise_on_failure=False, levels=3, **D["opt"])
    r = f.track_exposure_frame(black, D["depth"], D["start"], raise_on_failure=False, levels=3, **D["opt"])
    assert_same_result(result_dict(r), result_dict(pyr), "one colour")
    assert np.array_equal(r.T32, pyr.T32) and (r.gain, r.offset) == (1.0, 0.0)
    sx, sp = f.track_exposure_stats(), f.track_pyramid_stats()
    assert sx[:5] == sp[:5] and sx[6:] == sp[6:] and r.held == sx[3] > 3 and r.photometric > 1000
    assert {L: f.track_exposure_level_stats(L) for L in range(5)} == {L: f.track_pyramid_level_stats(L) for L in range(5)}
    f.close()


# ------------------------------------------------------------------ 5
def test_nothing_changed(D):
    """Map export, drf_stats, the public render on host and device and the other families' statistics are what they are without the
    exposure calls; streaming with map-scope renders gives the unbounded pool's bits (the plane, 48x64)."""
    bgr, depth, pose = D["bgr2"], D["depth"], D["pose"]
    view = start_near(pose.astype(np.float64), (0, 1, 0), 3.0, (2.0, 0.0, 0.0))

    def render(f):
        f.RenderAsync([view])
        rb, rd = f.GetRenderResult()
        return rb[0].copy(), rd[0].copy()

    def device_render(f):
        pb, pd = f.render_device_pointers()
        return (pb, pd), download(f, pb, (H, W, 3), np.uint8), download(f, pd, (H, W), f32)

    f = loaded(D)
    before = (f.export_blocks(), f.stats(), render(f))
    held = device_render(f)
    one = track_opts(D, max_renders=1)
    f.track_frame(depth, D["start"], raise_on_failure=False, **one)
    f.track_colour_frame(bgr, depth, D["start"], raise_on_failure=False, **one)
    f.track_pyramid_frame(bgr, depth, D["start"], raise_on_failure=False, levels=2, coarse_renders=1, **one)
    stats = (f.track_stats(), f.track_colour_stats(), f.track_pyramid_stats(), [f.track_pyramid_level_stats(L) for L in range(5)])
    f.track_exposure_frame(bgr, depth, D["start"], raise_on_failure=False, levels=3, **D["opt"])
    f.track_exposure_system(1, bgr, depth, before[2][0], before[2][1], view, D["start"], 0.8, 25.0, step=2)
    assert (f.track_stats(), f.track_colour_stats(), f.track_pyramid_stats(), [f.track_pyramid_level_stats(L) for L in range(5)]) == stats
    again = device_render(f)
    assert again[0] == held[0] and np.array_equal(again[1], held[1]) and np.array_equal(again[2].view(np.uint32), held[2].view(np.uint32))
    after = (f.export_blocks(), f.stats(), render(f))
    assert before[1] == after[1] and before[0].keys() == after[0].keys()
    assert all(np.array_equal(before[0][k], after[0][k]) for k in before[0])
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1].view(np.uint32), after[2][1].view(np.uint32))
    f.close()
    # streaming at 48x64: half of the plane map in the host store, map-scope renders
    from tandem_amd.dr_fusion import RENDER_MAP, streaming_min_radius
    p = D["plane"]
    f = plane_engine(D)
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))
    f.stream_out_region((-500.0, -500.0, -500.0), (0.0, 500.0, 500.0))
    stored = f.streaming_stats()["host"]
    assert stored > 0
    f.set_render_scope(RENDER_MAP)
    r = f.track_exposure_frame(p["bgr"], p["depth"], p["start"], raise_on_failure=False, **TX.PLANE_OPTS)
    assert_same_exposure_run(f, r, p["tracked"], "map scope")
    assert f.streaming_stats()["host"] == stored
    f.set_render_scope(RENDER_MAP, 4)
    assert code_of(f.track_exposure_frame, p["bgr"], p["depth"], p["start"]) == 5 and f.track_exposure_stats() == NOTHING
    f.close()


# ------------------------------------------------------------------ 6
def test_legality_in_its_order(D):
    from tandem_amd import _lib
    f = loaded(D)
    L = f._L
    depth_a, pose_a, bgr_a = np.ascontiguousarray(D["depth"], f32), np.ascontiguousarray(D["start"], f32).reshape(16), np.ascontiguousarray(D["bgr"], np.uint8)
    dp, pp, bp = depth_a.ctypes.data_as(_lib.f32p), pose_a.ctypes.data_as(_lib.f32p), C.c_void_p(bgr_a.ctypes.data)
    sums_a, out_a = np.zeros(45), np.zeros(16, f32)
    sums, counts, out = sums_a.ctypes.data_as(_lib.f64p), (C.c_uint64 * 5)(), out_a.ctypes.data_as(_lib.f32p)
    nothing = lambda: f.track_exposure_stats() == NOTHING and f.track_exposure_level_stats(0) == (0, 0, 0, 0)  # noqa: E731
    f.track_exposure_system(1, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], D["start"])
    assert not nothing()
    # null arguments (opt and res may be null); the colour images are required
    full = (bp, dp, bp, dp, pp, pp, 1.0, 0.0, None, sums, counts)
    for k in (0, 1, 2, 3, 4, 5, 9, 10):
        args = full[:k] + (None,) + full[k + 1:]
        assert L.drf_track_exposure_system(f._h, 1, *args) == 1 and nothing(), k
        assert L.drf_track_exposure_system_device(f._h, 1, *args) == 1 and nothing(), k
    full = (bp, dp, pp, None, out, None)
    for k in (0, 1, 2, 4):
        args = full[:k] + (None,) + full[k + 1:]
        assert L.drf_track_exposure_frame(f._h, *args) == 1 and nothing(), k
        assert L.drf_track_exposure_frame_device(f._h, *args) == 1 and nothing(), k
    assert L.drf_track_exposure_stats(f._h, None) == 1 and L.drf_track_exposure_level_stats(f._h, 0, None) == 1
    assert L.drf_track_exposure_level_stats(f._h, 5, (C.c_uint64 * 4)()) == 1 and L.drf_track_exposure_level_stats(f._h, -1, (C.c_uint64 * 4)()) == 1
    one = _lib.TrackExposureOptions(_lib.TrackPyramidOptions(_lib.TrackColourOptions(_lib.TrackOptions(max_renders=1, inner_iters=1), 0.0), 2, 1))
    assert L.drf_track_exposure_frame(f._h, bp, dp, pp, C.byref(one), out, None) == 0 and not nothing()   # res null
    assert f.track_exposure_stats()[3:5] == (2, 2)
    # a bad option is named: the pyramid options' own first, then the exposure's in their order; the colour image behind them
    for bad, name in ((dict(photo_weight=-1.0, gain_init=-1.0), "photo_weight"), (dict(levels=6, gain_min=9.0), "levels"), (dict(coarse_renders=-1, eps_gain=-1.0), "coarse_renders"),
                      (dict(gain_init=float("nan"), gain_min=-1.0), "gain_init"), (dict(offset_init=float("inf")), "offset_init"), (dict(gain_min=-1.0, gain_max=-1.0), "gain_min"),
                      (dict(gain_max=float("inf")), "gain_max"), (dict(eps_gain=-1.0, eps_offset=-1.0), "eps_gain"), (dict(eps_offset=float("nan")), "eps_offset"),
                      (dict(gain_min=2.0, gain_max=1.0), "gain_min"), (dict(gain_init=5.0, offset_init=900.0), "gain_init"), (dict(offset_init=-800.0), "offset_init")):
        with pytest.raises(_lib.DrError) as e:
            f.track_exposure_frame(D["bgr"], D["depth"], D["start"], **bad)
        assert e.value.code == 1 and ("option " + name) in str(e.value) and nothing(), bad
    xo = _lib.TrackExposureOptions(gain_init=9.0)
    assert L.drf_track_exposure_frame(f._h, None, dp, pp, C.byref(xo), out, None) == 1 and "option gain_init" in L.dr_last_error().decode()
    assert L.drf_track_exposure_frame(f._h, None, dp, pp, None, out, None) == 1 and "bgr is null" in L.dr_last_error().decode()
    for lvl in (-1, 4, 5):                                              # 96 >> 4 = 6 pixels
        assert code_of(f.track_exposure_system, lvl, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], D["start"]) == 1 and nothing()
    assert code_of(f.track_exposure_system, 1, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], D["start"], float("nan"), 0.0) == 1
    with pytest.raises(TypeError):
        f.track_exposure_frame(D["bgr"], D["depth"], D["start"], no_such_option=1)
    # what is no rigid motion: the pose, and the model's pose
    scaled = D["start"].copy()
    scaled[:3, :3] *= 1.01
    assert code_of(f.track_exposure_frame, D["bgr"], D["depth"], scaled) == 1 and nothing()
    assert code_of(f.track_exposure_system, 1, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], scaled) == 1
    assert code_of(f.track_exposure_system, 1, D["bgr"], D["depth"], D["bgr"], D["depth"], scaled, D["start"]) == 1
    # where a scan may not be integrated: after the options, before the pose
    f.IntegrateScanAsync(np.zeros((H, W, 3), np.uint8), np.zeros((H, W), f32), np.eye(4, dtype=f32))
    assert code_of(f.track_exposure_frame, D["bgr"], D["depth"], D["start"]) == 2 and code_of(f.track_exposure_frame, D["bgr"], D["depth"], scaled) == 2 and nothing()
    assert code_of(f.track_exposure_system, 1, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], D["start"]) == 2
    with pytest.raises(_lib.DrError) as e:
        f.track_exposure_frame(D["bgr"], D["depth"], scaled, gain_min=-1.0)
    assert e.value.code == 1 and "gain_min" in str(e.value)
    f.close()


def test_shim(D, tmp_path):
    """tandem_amd/libdr/dr_fusion.h TrackExposureFrame and TrackExposureSystem held to the library's own answers."""
    from tandem_amd import _lib
    f = loaded(D)
    want = f.track_exposure_frame(D["bgr2"], D["depth"], D["start"], raise_on_failure=False, levels=3, **D["opt"])
    system = f.track_exposure_system(0, D["bgr2"], D["depth"], D["bgr2"], D["depth"], want.T32, want.T32, want.gain, want.offset, levels=3, **D["opt"])
    f.close()
    exe, frame = str(tmp_path / "map_track_exposure_shim"), str(tmp_path / "frame.bin")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_track_exposure_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    opt = dict(D["opt"])
    coarse = opt.pop("coarse_renders")
    with open(frame, "wb") as fh:
        fh.write(np.ascontiguousarray(D["start"], f32).tobytes() +
                 bytes(_lib.TrackExposureOptions(_lib.TrackPyramidOptions(_lib.TrackColourOptions(_lib.TrackOptions(**opt), 0.0), 3, coarse))) +
                 np.ascontiguousarray(D["depth"], f32).tobytes() + np.ascontiguousarray(D["bgr2"], np.uint8).tobytes())
    cam = D["cam"]
    r = subprocess.run([exe, repr(VS)] + [repr(float(f32(cam[k]))) for k in ("fx", "fy", "cx", "cy")] + [str(cam["num_blocks"]), D["file"], frame],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["track_status"] == want.status and np.array_equal(f32(js["tracked"]).reshape(4, 4), want.T32)
    assert js["gain"] == want.gain and js["offset"] == want.offset and js["cost"] == float(system[0][27]) and js["photometric"] == system[1][4]
