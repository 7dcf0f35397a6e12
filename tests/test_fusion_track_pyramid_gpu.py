"""-m gpu: drf_track_reduce / drf_track_pyramid_system / drf_track_pyramid_frame.  The reference of every bit comparison is the numpy
restatement of the rule in tests/test_map_track_pyramid.py (np_reduce, np_pyramid_system) and, for whole trackings,
track_pyramid_frame_host through tests/cpp/map_track_pyramid_check.cpp over the CPU oracle's ray-cast of colour and depth, which
tests/test_map_track_pyramid.py holds to np_track_pyramid_frame on every evaluation.  Engines of 5x7 up to 96x128; the map is the
one-scan scene of 1 968 blocks.  DESIGN.md §7c "Tracking coarse to fine"."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import test_map_track_colour as TC
import test_map_track_pyramid as TP
from fusion_helpers import ROOT, feed
from test_fusion_map_file_gpu import engine
from test_fusion_map_locate_gpu import result_dict
from test_fusion_map_track_gpu import plain
from test_fusion_map_transform_gpu import write
from test_fusion_track_colour_gpu import DeviceImage
from test_map_align import LOST, assert_same_result, assert_same_system
from test_map_locate import camera, start_near
from test_map_track import H, PM, VS, W, basin_start, pair_poses, track_opts, track_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
NOTHING = (0, 0, 0, 0, 0, 0, 0, 0)


def code_of(call, *args, **kw):
    """the code of the DrError that the call raises"""
    from tandem_amd import _lib
    with pytest.raises(_lib.DrError) as e:
        call(*args, **kw)
    return e.value.code


def download(f, ptr, shape, dtype):
    out = np.empty(shape, dtype)
    assert f._L.dr_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes) == 0
    return out


def assert_same_pyramid_run(f, r, want, what):
    """An AlignResult of the engine and its statistics against a dict of TP.cpp_frame / TP.np_track_pyramid_frame"""
    assert_same_result(result_dict(r), plain(want), what)
    assert np.array_equal(r.T32, want["T"].astype(f32)), what
    st = f.track_pyramid_stats()
    assert st[:5] == want["stats8"][:5] and st[6:] == want["stats8"][6:] and st[5] > 0, "%s: %s against %s" % (what, st, want["stats8"])
    levels = {L: f.track_pyramid_level_stats(L) for L in range(5)}
    assert {L: v for L, v in levels.items() if v[2]} == want["levels"], "%s: %s against %s" % (what, levels, want["levels"])


@pytest.fixture(scope="module")
def D(tmp_path_factory):
    """The scene, its map file and the CPU runs of the pyramid over the oracle's renders."""
    d = tmp_path_factory.mktemp("track_pyramid")
    s = track_scene()
    s["file"] = str(d / "scene.drfmap")
    write(s["file"], VS, *s["blocks"])
    HP = TP.build_check(d)
    s["render_both"] = lambda pose: s["oracle"].render(pose)
    s["start"] = basin_start(s, 0)
    s["opt"] = track_opts(s, max_renders=2, coarse_renders=2)
    s["three"] = TP.cpp_frame(HP, s["render_both"], s["cam"], s["bgr"], s["depth"], s["start"], levels=3, **s["opt"])
    s["HP"], s["dir"] = HP, d
    return s


def loaded(s, **kw):
    f = engine(s["cam"], **kw)
    f.load_map(s["file"])
    return f


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("height,width", [(8, 8)] + TP.REDUCE_SHAPES, ids=["8x8", "16x32", "18x35", "96x128"])
def test_reduce_against_the_restatement(height, width):
    """The images of the CPU test at every level that keeps 8 pixels on a side (8x8: level 0 alone), host and device pointers, with
    colour and the depth alone, bit for bit; the levels below 8 pixels are refused."""
    bgr, depth = TP.reduce_pair(height, height, width)
    cam = camera(VS, height, width)
    f = engine(cam)
    db, dd = DeviceImage(f, bgr, np.uint8), DeviceImage(f, depth, f32)
    ob, od = DeviceImage(f, np.zeros((height, width, 3), np.uint8), np.uint8), DeviceImage(f, np.zeros((height, width), f32), f32)
    ran = 0
    for L in range(5):
        if not TP.level_fits(cam, L):
            assert code_of(f.track_reduce, L, 0.1, bgr, depth) == 1 and f.track_pyramid_stats() == NOTHING
            assert code_of(f.track_reduce, L, 0.1, (db.ptr, ob.ptr), (dd.ptr, od.ptr)) == 1
            continue
        for mj in (0.1 * (1 << L), 0.003):
            wc, wd = TP.np_reduce(bgr, depth, L, mj)
            gc, gd = f.track_reduce(L, mj, bgr, depth)
            assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)) and np.array_equal(gc, wc), (L, mj)
            st = f.track_pyramid_stats()
            assert st[:5] == (0, 0, 0, 0, 0) and st[5] > 0 and st[6:] == (0, 0)
            none, alone = f.track_reduce(L, mj, None, depth)
            assert none is None and np.array_equal(alone.view(np.uint32), wd.view(np.uint32)), "the depth alone"
            f.track_reduce(L, mj, (db.ptr, ob.ptr), (dd.ptr, od.ptr))
            assert np.array_equal(download(f, od.ptr, wd.shape, f32).view(np.uint32), wd.view(np.uint32)), "device pointers"
            assert np.array_equal(download(f, ob.ptr, wc.shape, np.uint8), wc), "device pointers"
            ran += 1
    assert ran == {8: 2, 16: 4, 18: 4, 96: 8}[height]
    for bad in (-1.0, float("nan"), float("inf")):
        assert code_of(f.track_reduce, 0, bad, bgr, depth) == 1
    for i in (db, dd, ob, od):
        i.free()
    f.close()


def test_named_reduction_cases_and_a_camera_too_small():
    """Every named block of the CPU test through the engine (8x8, levels 0 and -- refused -- above), and a 5x7 engine, which has
    no level 1 (nor a level 0 of 8 pixels)."""
    f = engine(camera(VS, 8, 8))
    for name, (L, mj, values, colours, _, _) in TP.REDUCE_CASES.items():
        bgr, depth = TP._block(L, values, colours)
        wc, wd = TP.np_reduce(bgr, depth, 0, mj)
        gc, gd = f.track_reduce(0, mj, bgr, depth)
        assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)) and np.array_equal(gc, wc), name
    f.close()
    f = engine(camera(VS, 16, 16))
    for name, (L, mj, values, colours, _, _) in TP.REDUCE_CASES.items():
        if L != 1:
            continue
        b8, d8 = TP._block(L, values, colours)
        bgr, depth = np.tile(b8, (2, 2, 1)), np.tile(d8, (2, 2))
        wc, wd = TP.np_reduce(bgr, depth, 1, mj)
        gc, gd = f.track_reduce(1, mj, bgr, depth)
        assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)) and np.array_equal(gc, wc), name
    f.close()
    f = engine(camera(VS, 5, 7))
    assert code_of(f.track_reduce, 1, 0.1, np.zeros((5, 7, 3), np.uint8), np.ones((5, 7), f32)) == 1
    assert code_of(f.track_pyramid_frame, None, np.ones((5, 7), f32), np.eye(4, dtype=f32)) == 1 and f.track_pyramid_stats() == NOTHING
    f.close()


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("height,width", TP.SYSTEM_SHAPES, ids=["%dx%d" % g for g in TP.SYSTEM_SHAPES])
def test_system_against_the_restatement(height, width):
    """Levels 1 to 3 where they keep 8 pixels, strides 1 to 3, with and without colour, host and device pointers: sums and every
    count class bit for bit, and the statistics."""
    case = TC.colour_pair(7 + height, height, width)
    cam, d, bgr, mb, md = case["cam"], case["depth"], case["bgr"], case["model_bgr"], case["model"]
    f = engine(cam)
    imgs = [DeviceImage(f, bgr, np.uint8), DeviceImage(f, d, f32), DeviceImage(f, mb, np.uint8), DeviceImage(f, md, f32)]
    pose = pair_poses(cam)[2][1]
    ran = 0
    for L in (1, 2, 3):
        if not TP.level_fits(cam, L):
            assert code_of(f.track_pyramid_system, L, bgr, d, mb, md, PM, pose, levels=1) == 1 and f.track_pyramid_stats() == NOTHING
            continue
        for step in (1, 2, 3):
            opt = dict(levels=L + 1, step=step, centre_depth=1.5)
            for colour in (True, False):
                want = TP.np_pyramid_system(cam, L, bgr if colour else None, d, mb if colour else None, md, PM, pose, **opt)
                got = f.track_pyramid_system(L, bgr if colour else None, d, mb if colour else None, md, PM, pose, **opt)
                assert_same_system(got, want, "level %d, step %d, colour %s" % (L, step, colour))
                st = f.track_pyramid_stats()
                assert st[:5] == (-(-(width >> L) // step) * -(-(height >> L) // step), want[1][0], want[1][1], 1, 0) and st[6:] == (1, 0)
                assert f.track_pyramid_level_stats(L) == (0, 0, 1, want[1][1])
                p = [i.ptr for i in imgs]
                got = f.track_pyramid_system(L, p[0] if colour else None, p[1], p[2] if colour else None, p[3], PM, pose, **opt)
                assert_same_system(got, want, "level %d, step %d, colour %s (device pointers)" % (L, step, colour))
                ran += 1
    assert ran >= 6 and f.track_stats() == (0, 0, 0, 0, 0, 0) and f.track_colour_stats() == (0, 0, 0, 0, 0, 0)
    for i in imgs:
        i.free()
    f.close()


# ------------------------------------------------------------------ 3
def test_one_level_is_the_single_level_call(D):
    """levels = 1 equals drf_track_colour_frame, with bgr null drf_track_frame, on the same engine: every field of res and
    pose16_out."""
    f = loaded(D)
    opt = track_opts(D, max_renders=3)
    col = f.track_colour_frame(D["bgr"], D["depth"], D["start"], raise_on_failure=False, **opt)
    pyr = f.track_pyramid_frame(D["bgr"], D["depth"], D["start"], raise_on_failure=False, levels=1, **opt)
    assert_same_result(result_dict(pyr), result_dict(col), "levels = 1 with colour")
    assert np.array_equal(pyr.T32, col.T32) and f.track_pyramid_stats()[:5] == f.track_colour_stats()[:5] and f.track_pyramid_stats()[6:] == (1, 0)
    geo = f.track_frame(D["depth"], D["start"], raise_on_failure=False, **opt)
    pyr = f.track_pyramid_frame(None, D["depth"], D["start"], raise_on_failure=False, levels=1, **opt)
    assert_same_result(result_dict(pyr), result_dict(geo), "levels = 1 without colour")
    assert np.array_equal(pyr.T32, geo.T32) and f.track_pyramid_stats()[:5] == f.track_stats()[:5]
    assert f.track_pyramid_level_stats(0) == (geo.status, f.track_stats()[4], geo.iterations, geo.valid)
    f.close()


# ------------------------------------------------------------------ 4
def test_three_levels_on_the_scene_map(D):
    """drf_track_pyramid_frame with three levels on the scene map, host and device pointers, with colour and without: every field,
    the totals and the per-level outcomes are the CPU host run's over the oracle's renders."""
    f = loaded(D)
    r = f.track_pyramid_frame(D["bgr"], D["depth"], D["start"], raise_on_failure=False, levels=3, **D["opt"])
    assert_same_pyramid_run(f, r, D["three"], "three levels")
    db, dd = DeviceImage(f, D["bgr"], np.uint8), DeviceImage(f, D["depth"], f32)
    r = f.track_pyramid_frame(db.ptr, dd.ptr, D["start"], raise_on_failure=False, levels=3, **D["opt"])
    assert_same_pyramid_run(f, r, D["three"], "three levels (device pointers)")
    want = TP.cpp_frame(D["HP"], D["render_both"], D["cam"], None, D["depth"], D["start"], levels=3, step=2, **D["opt"])
    r = f.track_pyramid_frame(None, dd.ptr, D["start"], raise_on_failure=False, levels=3, step=2, **D["opt"])
    assert_same_pyramid_run(f, r, want, "three levels, geometry only, step 2")
    db.free()
    dd.free()
    f.close()


def test_every_level_abandoned(D):
    """The 20-voxel start: levels 2 and 1 are abandoned, level 0 is LOST at the start pose; DR_OK with a note."""
    f = loaded(D)
    start = basin_start(D, 2)
    want = TP.cpp_frame(D["HP"], D["render_both"], D["cam"], D["bgr"], D["depth"], start, levels=3, **D["opt"])
    r = f.track_pyramid_frame(D["bgr"], D["depth"], start, raise_on_failure=False, levels=3, **D["opt"])
    assert_same_pyramid_run(f, r, want, "the far start")
    assert r.status == LOST and f.track_pyramid_stats()[6:] == (3, 2) and np.array_equal(r.T32, start)
    from tandem_amd.dr_fusion import AlignError
    with pytest.raises(AlignError) as e:                                # the note says what happened
        f.track_pyramid_frame(D["bgr"], D["depth"], start, levels=3, **D["opt"])
    assert "2 abandoned" in str(e.value) and "is lost" in str(e.value)
    f.close()


# ------------------------------------------------------------------ 5
def test_nothing_changed(D):
    """Map export, drf_stats, the public render on host and device, drf_track_stats / drf_track_colour_stats of calls made before
    and the map after the next scan are what they are without the pyramid calls."""
    bgr, depth, pose = D["bgr"], D["depth"], D["pose"]
    view = start_near(pose.astype(np.float64), (0, 1, 0), 3.0, (2.0, 0.0, 0.0))

    def render(f):
        f.RenderAsync([view])
        rb, rd = f.GetRenderResult()
        return rb[0].copy(), rd[0].copy()

    def device_render(f):
        pb, pd = f.render_device_pointers()
        return (pb, pd), download(f, pb, (H, W, 3), np.uint8), download(f, pd, (H, W), f32)

    f, g = loaded(D), loaded(D)
    before = (f.export_blocks(), f.stats(), render(f))
    held = device_render(f)
    one = track_opts(D, max_renders=1)
    geo = f.track_frame(depth, D["start"], raise_on_failure=False, **one)
    col = f.track_colour_frame(bgr, depth, D["start"], raise_on_failure=False, **one)
    stats = (f.track_stats(), f.track_colour_stats())
    f.track_pyramid_frame(bgr, depth, D["start"], raise_on_failure=False, levels=3, **D["opt"])
    f.track_pyramid_system(1, bgr, depth, before[2][0], before[2][1], view, D["start"], step=2)
    f.track_reduce(2, 0.4, bgr, depth)
    assert (f.track_stats(), f.track_colour_stats()) == stats
    again = device_render(f)
    assert again[0] == held[0] and np.array_equal(again[1], held[1]) and np.array_equal(again[2].view(np.uint32), held[2].view(np.uint32))
    assert_same_result(result_dict(f.track_frame(depth, D["start"], raise_on_failure=False, **one)), result_dict(geo), "the geometric call afterwards")
    assert_same_result(result_dict(f.track_colour_frame(bgr, depth, D["start"], raise_on_failure=False, **one)), result_dict(col), "the colour call afterwards")
    after = (f.export_blocks(), f.stats(), render(f))
    assert before[1] == after[1] and before[0].keys() == after[0].keys()
    assert all(np.array_equal(before[0][k], after[0][k]) for k in before[0])
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1].view(np.uint32), after[2][1].view(np.uint32))
    moved = start_near(pose.astype(np.float64), (1, 0, 0), 2.0, (1.0, 2.0, 0.0))
    for e in (f, g):                                                    # a scan integrated after it: the same map as without
        feed(e, bgr, depth, moved)
    a, b = f.export_blocks(), g.export_blocks()
    assert f.stats() == g.stats() and a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    f.close()
    g.close()


# ------------------------------------------------------------------ 6
def test_streaming(D):
    """Streaming on, the half of the map with x below its median block sent to the host store: map-scope renders give the
    unbounded pool's result bit for bit at every level; a staging too small is DR_ERR_CAPACITY with zeroed stats."""
    from tandem_amd.dr_fusion import RENDER_MAP, RENDER_RESIDENT, streaming_min_radius
    args = (D["bgr"], D["depth"], D["start"])
    f = loaded(D)
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))
    cut = float(np.median(D["blocks"][0][:, 0])) * 8 * VS
    f.stream_out_region((-500.0, -500.0, -500.0), (cut, 500.0, 500.0))
    stored = f.streaming_stats()["host"]
    assert 0 < stored < len(D["blocks"][0])
    f.set_render_scope(RENDER_RESIDENT)
    part = f.track_pyramid_frame(*args, raise_on_failure=False, levels=3, **D["opt"])
    assert (part.samples, part.valid0) != (D["three"]["samples"], D["three"]["valid0"]) or not np.array_equal(part.T, D["three"]["T"])
    f.set_render_scope(RENDER_MAP)
    r = f.track_pyramid_frame(*args, raise_on_failure=False, levels=3, **D["opt"])
    assert_same_pyramid_run(f, r, D["three"], "map scope")
    f.set_render_scope(RENDER_MAP, 4)
    assert code_of(f.track_pyramid_frame, *args, levels=3) == 5 and f.track_pyramid_stats() == NOTHING
    assert f.streaming_stats()["host"] == stored
    f.close()


# ------------------------------------------------------------------ 7
def test_legality_in_its_order(D):
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import RENDER_MAP, streaming_min_radius
    f = loaded(D)
    L = f._L
    depth_a, pose_a, bgr_a = np.ascontiguousarray(D["depth"], f32), np.ascontiguousarray(D["start"], f32).reshape(16), np.ascontiguousarray(D["bgr"], np.uint8)
    dp, pp, bp = depth_a.ctypes.data_as(_lib.f32p), pose_a.ctypes.data_as(_lib.f32p), C.c_void_p(bgr_a.ctypes.data)
    sums_a, out_a = np.zeros(28), np.zeros(16, f32)
    sums, counts, out = sums_a.ctypes.data_as(_lib.f64p), (C.c_uint64 * 5)(), out_a.ctypes.data_as(_lib.f32p)
    nothing = lambda: f.track_pyramid_stats() == NOTHING and f.track_pyramid_level_stats(0) == (0, 0, 0, 0)  # noqa: E731
    f.track_pyramid_system(1, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], D["start"])
    assert not nothing()
    # null arguments (the colour images, opt and res may be null; a model colour image must come with the frame's)
    full = (bp, dp, bp, dp, pp, pp, None, sums, counts)
    for k in (1, 2, 3, 4, 5, 7, 8):
        args = full[:k] + (None,) + full[k + 1:]
        assert L.drf_track_pyramid_system(f._h, 1, *args) == 1 and nothing(), k
        assert L.drf_track_pyramid_system_device(f._h, 1, *args) == 1 and nothing(), k
    full = (bp, dp, pp, None, out, None)
    for k in (1, 2, 4):
        args = full[:k] + (None,) + full[k + 1:]
        assert L.drf_track_pyramid_frame(f._h, *args) == 1 and nothing(), k
        assert L.drf_track_pyramid_frame_device(f._h, *args) == 1 and nothing(), k
    assert L.drf_track_reduce(f._h, 1, 0.1, bp, None, bp, dp) == 1 and L.drf_track_reduce(f._h, 1, 0.1, bp, dp, None, dp) == 1
    assert L.drf_track_reduce(f._h, 1, 0.1, None, dp, None, None) == 1 and L.drf_track_reduce_device(f._h, 1, 0.1, None, None, None, None) == 1
    assert L.drf_track_pyramid_stats(f._h, None) == 1 and L.drf_track_pyramid_level_stats(f._h, 0, None) == 1
    assert L.drf_track_pyramid_level_stats(f._h, 5, (C.c_uint64 * 4)()) == 1 and L.drf_track_pyramid_level_stats(f._h, -1, (C.c_uint64 * 4)()) == 1
    one = _lib.TrackPyramidOptions(_lib.TrackColourOptions(_lib.TrackOptions(max_renders=1, inner_iters=1), 0.0), 2, 1)
    assert L.drf_track_pyramid_frame(f._h, bp, dp, pp, C.byref(one), out, None) == 0 and not nothing()   # res null
    assert f.track_pyramid_stats()[3:5] == (2, 2)
    # a bad option is named: the colour options' own first, then levels, then coarse_renders
    for bad, name in ((dict(photo_weight=-1.0, levels=-1), "photo_weight"), (dict(step=-1, levels=9), "step"), (dict(levels=-1, coarse_renders=-1), "levels"),
                      (dict(levels=6), "levels"), (dict(levels=5), "levels"), (dict(coarse_renders=-1), "coarse_renders"), (dict(max_jump=float("nan")), "max_jump")):
        with pytest.raises(_lib.DrError) as e:
            f.track_pyramid_frame(D["bgr"], D["depth"], D["start"], **bad)
        assert e.value.code == 1 and ("option " + name) in str(e.value) and nothing(), bad
    r = f.track_pyramid_frame(D["bgr"], D["depth"], D["start"], raise_on_failure=False, levels=4, max_renders=1, coarse_renders=1, inner_iters=1)   # 96 >> 3 = 12
    assert f.track_pyramid_stats()[3:] == (4, 4, f.track_pyramid_stats()[5], 4, f.track_pyramid_stats()[7]) and r.iterations == 1
    for lvl in (-1, 4, 5):                                              # 96 >> 4 = 6 pixels
        assert code_of(f.track_pyramid_system, lvl, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], D["start"]) == 1 and nothing()
    with pytest.raises(TypeError):
        f.track_pyramid_frame(D["bgr"], D["depth"], D["start"], no_such_option=1)
    # what is no rigid motion: the pose, and the model's pose
    scaled, nan = D["start"].copy(), D["start"].copy()
    scaled[:3, :3] *= 1.01
    nan[2, 3] = np.nan
    for bad in (scaled, nan):
        assert code_of(f.track_pyramid_frame, D["bgr"], D["depth"], bad) == 1 and nothing()
        assert code_of(f.track_pyramid_system, 1, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], bad) == 1
        assert code_of(f.track_pyramid_system, 1, D["bgr"], D["depth"], D["bgr"], D["depth"], bad, D["start"]) == 1
    # the capacity stands behind the pose
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))
    f.stream_out_region((-500.0, -500.0, -500.0), (500.0, 500.0, 500.0))
    f.set_render_scope(RENDER_MAP, 4)
    assert code_of(f.track_pyramid_frame, D["bgr"], D["depth"], D["start"]) == 5 and nothing()
    assert code_of(f.track_pyramid_frame, D["bgr"], D["depth"], scaled) == 1
    # where a scan may not be integrated: after the options, before the pose and the capacity
    f.IntegrateScanAsync(np.zeros((H, W, 3), np.uint8), np.zeros((H, W), f32), np.eye(4, dtype=f32))
    assert code_of(f.track_pyramid_frame, D["bgr"], D["depth"], D["start"]) == 2 and code_of(f.track_pyramid_frame, D["bgr"], D["depth"], scaled) == 2 and nothing()
    assert code_of(f.track_pyramid_system, 1, D["bgr"], D["depth"], D["bgr"], D["depth"], D["start"], D["start"]) == 2
    assert code_of(f.track_reduce, 1, 0.1, D["bgr"], D["depth"]) == 2 and code_of(f.track_reduce, 7, 0.1, D["bgr"], D["depth"]) == 1
    with pytest.raises(_lib.DrError) as e:
        f.track_pyramid_frame(D["bgr"], D["depth"], scaled, levels=7)
    assert e.value.code == 1 and "levels" in str(e.value)
    f.close()


# ------------------------------------------------------------------ 8
def test_shim(D, tmp_path):
    """tandem_amd/libdr/dr_fusion.h TrackPyramidFrame held to the library's own answer."""
    from tandem_amd import _lib
    f = loaded(D)
    want = f.track_pyramid_frame(D["bgr"], D["depth"], D["start"], raise_on_failure=False, levels=3, **D["opt"])
    f.close()
    exe, frame = str(tmp_path / "map_track_pyramid_shim"), str(tmp_path / "frame.bin")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_track_pyramid_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    opt = dict(D["opt"])
    coarse = opt.pop("coarse_renders")
    with open(frame, "wb") as fh:
        fh.write(np.ascontiguousarray(D["start"], f32).tobytes() + bytes(_lib.TrackPyramidOptions(_lib.TrackColourOptions(_lib.TrackOptions(**opt), 0.0), 3, coarse)) +
                 np.ascontiguousarray(D["depth"], f32).tobytes() + np.ascontiguousarray(D["bgr"], np.uint8).tobytes())
    cam = D["cam"]
    r = subprocess.run([exe, repr(VS)] + [repr(float(f32(cam[k]))) for k in ("fx", "fy", "cx", "cy")] + [str(cam["num_blocks"]), D["file"], frame],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["track_status"] == want.status and np.array_equal(f32(js["tracked"]).reshape(4, 4), want.T32)
