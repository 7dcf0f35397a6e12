"""-m gpu: drf_locate_system / drf_locate_frame.  The reference of every bit comparison is np_locate_system / np_locate_frame, the
numpy restatement of the rule in tests/test_map_locate.py, and beside it locate_frame_host through tests/cpp/map_locate_check.cpp;
the maps reach an engine as files written by tandem_amd.map_file.write and load_map, so the restatement sees exactly the voxels
the engine holds (the live-map test: export_blocks).  96x128 engines, one of 168x200; maps of about 260 blocks (the integrated
scene: 1 968).  DESIGN.md §7c "Locating a depth frame in the map"."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import ROOT, feed
from test_fusion_map_file_gpu import code_of, engine
from test_fusion_map_transform_gpu import write
from test_map_align import CONVERGED, LOST, MAX_ITERS, assert_same_result, assert_same_system
from test_map_locate import (H, PLANES_STARTS, SCENE_MEASURED, SYSTEM_CASES, VS, W, build_check, cpp_frame, np_locate_frame, np_locate_system, planes_case, random_case,
                             scene_case, scene_errors, start_near)

pytestmark = pytest.mark.gpu


def result_dict(r):
    return dict(T=r.T, sums=r.sums, samples=r.samples, valid0=r.valid0, valid=r.valid, cost0=r.cost0, cost=r.cost, iterations=r.iterations, status=r.status)


@pytest.fixture(scope="module")
def CHK(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("map_locate_check"))


@pytest.fixture(scope="module")
def D(tmp_path_factory):
    """The cases and their map files, the references computed once: the random map, the planes, the integrated scene."""
    d = tmp_path_factory.mktemp("locate")
    out = dict(dir=d, rnd=random_case(3), planes=planes_case(), scene=scene_case())
    for name in ("rnd", "planes", "scene"):
        out[name]["file"] = str(d / (name + ".drfmap"))
        write(out[name]["file"], VS, *out[name]["blocks"])
    out["rnd_want"] = {name: np_locate_system(out["rnd"]["blocks"], out["rnd"]["cam"], out["rnd"]["depth"], out["rnd"]["pose"], **opt) for name, opt in SYSTEM_CASES}
    return out


def loaded(case, **kw):
    f = engine(case["cam"], **kw)
    f.load_map(case["file"])
    return f


class DeviceDepth:
    """A depth image in device memory: .ptr is what the _device calls take."""

    def __init__(self, f, depth):
        depth = np.ascontiguousarray(depth, np.float32)
        self.L, self.p = f._L, C.c_void_p()
        assert self.L.dr_device_alloc(0, depth.nbytes, C.byref(self.p)) == 0
        assert self.L.dr_memcpy_h2d(self.p, depth.ctypes.data_as(C.c_void_p), depth.nbytes) == 0
        self.ptr = int(self.p.value)

    def free(self):
        self.L.dr_device_free(self.p)


# ------------------------------------------------------------------ 1
def test_system_against_the_restatement(D):
    """12 288 positions, 24 groups; step 3: 1 376 positions, the last group 352 wide -- tail lanes, and a lane with fewer than 8
    positions; the host pointer and the device pointer give the same bits."""
    case = D["rnd"]
    f = loaded(case)
    dd = DeviceDepth(f, case["depth"])
    for name, opt in SYSTEM_CASES:
        want = D["rnd_want"][name]
        got = f.locate_system(case["depth"], case["pose"], **opt)
        assert_same_system(got, want, name)
        step = opt.get("step", 1)
        st = f.locate_stats()
        assert st[:4] == (-(-W // step) * -(-H // step), want[1][0], want[1][1], 1) and st[5] == 0, st
        assert st[4] == 224 * 24 + 32 + 4 * H * W, st
        assert_same_system(f.locate_system(dd.ptr, case["pose"], **opt), want, name + " (device pointer)")
    assert f.locate_stats()[0] == 1376
    # an image without a sample: no look-up, 28 zeros per group
    got = f.locate_system(np.zeros((H, W), np.float32), case["pose"])
    assert not got[0].any() and got[1] == (0, 0, 0, 0)
    dd.free()
    f.close()
    # an empty map
    f = engine(case["cam"])
    got = f.locate_system(case["depth"], case["pose"])
    assert_same_system(got, np_locate_system((np.zeros((0, 3), np.int64), np.zeros((0, 4096), np.uint8)), case["cam"], case["depth"], case["pose"]), "empty map")
    assert not got[0].any() and got[1][1] == 0 and got[1][2] == got[1][0] > 1000
    f.close()


def test_a_grid_whose_fold_crosses_its_stride(tmp_path):
    """168x200: 33 600 positions, 66 groups, the last 320 wide."""
    case = random_case(20 + 168, 168, 200)
    case["cam"].update(cx=99.5, cy=83.5)
    case["file"] = str(tmp_path / "m.drfmap")
    write(case["file"], VS, *case["blocks"])
    f = loaded(case)
    got = f.locate_system(case["depth"], case["pose"])
    assert f.locate_stats()[0] == 33600
    f.close()
    want = np_locate_system(case["blocks"], case["cam"], case["depth"], case["pose"])
    assert_same_system(got, want, "168x200")
    assert want[1][1] > 100


def test_far_blocks(tmp_path):
    """Map and camera moved by whole blocks beyond block coordinate 256: the table path of find_block."""
    case = random_case(3, shift=(300, -270, 5))
    assert np.abs(case["blocks"][0]).max() > 256
    case["file"] = str(tmp_path / "far.drfmap")
    write(case["file"], VS, *case["blocks"])
    f = loaded(case)
    got = f.locate_system(case["depth"], case["pose"])
    f.close()
    want = np_locate_system(case["blocks"], case["cam"], case["depth"], case["pose"])
    assert_same_system(got, want, "far blocks")
    assert want[1][1] > 100


# ------------------------------------------------------------------ 2
def test_refinement_against_the_host_and_the_restatement(D, CHK):
    pl, rnd, sc = D["planes"], D["rnd"], D["scene"]
    cases = (("planes", pl, start_near(pl["T_true"], *PLANES_STARTS[0][1:]), dict(centre_depth=pl["centre_depth"])),
             ("planes, one evaluation", pl, start_near(pl["T_true"], *PLANES_STARTS[1][1:]), dict(centre_depth=pl["centre_depth"], max_iters=1)),
             ("random", rnd, rnd["pose"], dict(max_iters=6, min_valid=0.01)),
             ("scene", sc, sc["start"], dict(centre_depth=sc["centre_depth"])))
    for name, case, start, opt in cases:
        f = loaded(case)
        r = f.locate_frame(case["depth"], start, raise_on_failure=False, **opt)
        st = f.locate_stats()
        dd = DeviceDepth(f, case["depth"])
        rd = f.locate_frame(dd.ptr, start, raise_on_failure=False, **opt)
        dd.free()
        f.close()
        got = result_dict(r)
        host, want = cpp_frame(CHK, case["blocks"], case["cam"], case["depth"], start, **opt), np_locate_frame(case["blocks"], case["cam"], case["depth"], start, **opt)
        print("%s: status %d after %d evaluations, %d of %d valid, cost %.3g -> %.3g" % (name, r.status, r.iterations, r.valid, r.samples, r.cost0, r.cost))
        assert_same_result(host, want, name + " (host against the restatement)")
        host.pop("trace")
        assert_same_result(got, host, name + " (library against the host)")
        assert_same_result(result_dict(rd), host, name + " (device pointer)")
        assert np.array_equal(r.T32, r.T.astype(np.float32))
        assert st[3] == r.iterations and st[2] == r.valid and st[1] == r.samples
    a, t = scene_errors(r.T, sc["pose"])
    print("scene: %.5f degrees, %.5f voxels from the scan's pose" % (a, t))
    assert r.status == CONVERGED and a <= 2 * SCENE_MEASURED[0] and t <= 2 * SCENE_MEASURED[1]


def test_statuses(D):
    from tandem_amd.dr_fusion import AlignError
    pl = D["planes"]
    f = loaded(pl)
    start = start_near(pl["T_true"], *PLANES_STARTS[0][1:])
    r = f.locate_frame(pl["depth"], start, centre_depth=pl["centre_depth"])
    assert r.status == CONVERGED
    r = f.locate_frame(pl["depth"], start, centre_depth=pl["centre_depth"], max_iters=1)
    assert r.status == MAX_ITERS and r.iterations == 1 and not np.array_equal(r.T32, start)
    gone = start.copy()
    gone[0, 3] += 50 * 8 * VS                                          # the map is 50 blocks away
    with pytest.raises(AlignError) as e:
        f.locate_frame(pl["depth"], gone)
    assert e.value.result.status == LOST and "lost" in str(e.value) and e.value.result.iterations == 1
    assert np.array_equal(e.value.result.T32, gone)
    f.close()


# ------------------------------------------------------------------ 3
def test_the_map_is_untouched(D):
    sc = D["scene"]
    bgr, depth, pose = sc["bgr"], sc["depth"], sc["pose"]
    view = start_near(pose.astype(np.float64), (0, 1, 0), 3.0, (2.0, 0.0, 0.0))

    def render(f):
        f.RenderAsync([view])
        rb, rd = f.GetRenderResult()
        return rb[0].copy(), rd[0].copy()

    f, g = loaded(sc), loaded(sc)
    before = (f.export_blocks(), f.stats(), render(f))
    want = np_locate_frame(sc["blocks"], sc["cam"], depth, sc["start"], centre_depth=sc["centre_depth"], max_iters=3)
    want.pop("trace")
    assert_same_result(result_dict(f.locate_frame(depth, sc["start"], centre_depth=sc["centre_depth"], max_iters=3)), want, "scene, 3 evaluations")
    f.locate_system(depth, sc["start"], step=2)
    after = (f.export_blocks(), f.stats(), render(f))
    assert before[1] == after[1] and before[0].keys() == after[0].keys()
    assert all(np.array_equal(before[0][k], after[0][k]) for k in before[0])
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1].view(np.uint32), after[2][1].view(np.uint32))
    assert np.array_equal(render(g)[1].view(np.uint32), before[2][1].view(np.uint32))
    # a scan integrated after it gives the same map as in an engine that never located
    moved = start_near(pose.astype(np.float64), (1, 0, 0), 2.0, (1.0, 2.0, 0.0))
    for e in (f, g):
        feed(e, bgr, depth, moved)
    a, b = f.export_blocks(), g.export_blocks()
    assert f.stats() == g.stats() and a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    f.close()
    g.close()


def test_live_map():
    """Two scans fed, the second scan's depth located from a perturbed pose without saving anything; the restatement over
    export_blocks."""
    from synth import scene
    from fusion_helpers import options
    s = scene.make_scans(2, H, W, seed=5)
    cam = options(s, H, W, VS)
    f = engine(cam)
    for scan in s["scans"]:
        feed(f, *scan)
    bgr, depth, pose = s["scans"][1]
    start = start_near(pose.astype(np.float64), (1, -2, 1), 0.8, (1.0, 0.5, -0.8))
    r = f.locate_frame(depth, start, raise_on_failure=False, max_iters=4, centre_depth=2.0)
    blk = f.export_blocks()
    f.close()
    coords = np.array(sorted(blk), np.int64).reshape(-1, 3)
    want = np_locate_frame((coords, np.stack([blk[tuple(c)] for c in coords.tolist()])), cam, depth, start, max_iters=4, centre_depth=2.0)
    want.pop("trace")
    assert_same_result(result_dict(r), want, "live map")
    a0, t0 = scene_errors(start.astype(np.float64), pose)
    a, t = scene_errors(r.T, pose)
    print("live map: %.3f deg %.3f voxels -> %.3f deg %.3f voxels, %d of %d valid" % (a0, t0, a, t, r.valid, r.samples))
    assert r.valid > 0.5 * r.samples and t < t0


# ------------------------------------------------------------------ 4
def test_streaming(D):
    from tandem_amd.dr_fusion import streaming_min_radius
    sc = D["scene"]
    opt = dict(centre_depth=sc["centre_depth"], max_iters=3)
    f = loaded(sc)
    want = result_dict(f.locate_frame(sc["depth"], sc["start"], **opt))
    want_sys = f.locate_system(sc["depth"], sc["start"])
    f.close()
    f = loaded(sc)
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))        # every block in reach is resident
    assert f.streaming_stats()["host"] == 0
    assert_same_result(result_dict(f.locate_frame(sc["depth"], sc["start"], **opt)), want, "streaming on, everything resident")
    assert f.locate_stats()[5] == 0
    f.stream_out_region((-50.0, -50.0, -50.0), (50.0, 50.0, 50.0))    # the blocks in view go to the host store
    stored = f.streaming_stats()["host"]
    assert stored == len(sc["blocks"][0]) and f.streaming_stats()["resident"] == 0
    got = f.locate_system(sc["depth"], sc["start"])
    assert got[1] == (want_sys[1][0], 0, want_sys[1][0], 0) and not got[0].any()
    assert f.locate_stats()[5] == stored
    r = f.locate_frame(sc["depth"], sc["start"], raise_on_failure=False, **opt)
    msg = f._L.dr_last_error().decode()                               # (the next call that succeeds clears it)
    assert r.status == LOST and r.iterations == 1 and r.valid == 0 and f.locate_stats()[5] == stored
    assert "lost" in msg and "%d blocks are in the host store" % stored in msg, msg
    f.stream_in_region((-50.0, -50.0, -50.0), (50.0, 50.0, 50.0))     # and back
    assert_same_result(result_dict(f.locate_frame(sc["depth"], sc["start"], **opt)), want, "streamed back in")
    f.close()


# ------------------------------------------------------------------ 5
def test_legality_in_its_order(D):
    from tandem_amd import _lib
    case = D["rnd"]
    f = loaded(case)
    L = f._L
    depth_a, pose_a = np.ascontiguousarray(case["depth"], np.float32), np.ascontiguousarray(case["pose"], np.float32).reshape(16)
    dp, pp = depth_a.ctypes.data_as(_lib.f32p), pose_a.ctypes.data_as(_lib.f32p)
    sums_a, out_a = np.zeros(28), np.zeros(16, np.float32)
    sums, counts, out = sums_a.ctypes.data_as(_lib.f64p), (C.c_uint64 * 4)(), out_a.ctypes.data_as(_lib.f32p)
    nothing = lambda: f.locate_stats() == (0, 0, 0, 0, 0, 0)  # noqa: E731
    f.locate_system(case["depth"], case["pose"])
    assert not nothing()
    # null arguments (opt and res may be null)
    for args in ((None, pp, None, sums, counts), (dp, None, None, sums, counts), (dp, pp, None, None, counts), (dp, pp, None, sums, None)):
        assert L.drf_locate_system(f._h, *args) == 1 and nothing()
        assert L.drf_locate_system_device(f._h, *args) == 1 and nothing()
    for args in ((None, pp, None, out, None), (dp, None, None, out, None), (dp, pp, None, None, None)):
        assert L.drf_locate_frame(f._h, *args) == 1 and nothing()
        assert L.drf_locate_frame_device(f._h, *args) == 1 and nothing()
    assert L.drf_locate_stats(f._h, None) == 1
    assert L.drf_locate_frame(f._h, dp, pp, None, out, None) == 0     # opt and res null
    # a bad option is named
    for bad in (dict(step=-1), dict(centre_depth=float("nan")), dict(huber=-1.0), dict(band=float("inf")), dict(max_iters=-3), dict(min_valid=-1.0)):
        with pytest.raises(_lib.DrError) as e:
            f.locate_frame(case["depth"], case["pose"], **bad)
        assert e.value.code == 1 and list(bad)[0] in str(e.value) and nothing(), bad
    with pytest.raises(TypeError):
        f.locate_frame(case["depth"], case["pose"], no_such_option=1)
    # what is no rigid motion
    scaled, nan, row, mirror = (case["pose"].copy() for _ in range(4))
    scaled[:3, :3] *= 1.01
    nan[2, 3] = np.nan
    row[3, 3] = 1.0 + 2.0 ** -20
    mirror[:3, 1] *= -1
    for bad in (scaled, nan, row, mirror):
        assert code_of(f.locate_system, case["depth"], bad) == 1 and code_of(f.locate_frame, case["depth"], bad) == 1 and nothing()
    # where a scan may not be integrated: after the options, before the pose
    f.IntegrateScanAsync(np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.float32), np.eye(4, dtype=np.float32))
    assert code_of(f.locate_frame, case["depth"], case["pose"]) == 2 and code_of(f.locate_system, case["depth"], scaled) == 2 and nothing()
    with pytest.raises(_lib.DrError) as e:
        f.locate_system(case["depth"], scaled, step=-1)
    assert e.value.code == 1
    assert L.drf_locate_frame(f._h, None, pp, None, out, None) == 1
    f.RenderAsync([np.eye(4, dtype=np.float32)])
    assert code_of(f.locate_system, case["depth"], case["pose"]) == 2  # between RenderAsync and GetRenderResult
    f.GetRenderResult()
    # afterwards the engine answers again (the empty scan changed nothing)
    assert_same_system(f.locate_system(case["depth"], case["pose"]), D["rnd_want"]["defaults"], "afterwards")
    f.close()


# ------------------------------------------------------------------ 6
def test_shim(D, tmp_path):
    """tandem_amd/libdr/dr_fusion.h LocateDepthFrame, held to the library's own answer."""
    pl = D["planes"]
    start = start_near(pl["T_true"], *PLANES_STARTS[0][1:])
    f = loaded(pl)
    want = f.locate_frame(pl["depth"], start)                          # the shim passes no options: centre_depth 0
    f.close()
    exe, frame = str(tmp_path / "map_locate_shim"), str(tmp_path / "frame.bin")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_locate_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    with open(frame, "wb") as fh:
        fh.write(np.ascontiguousarray(start, np.float32).tobytes() + np.ascontiguousarray(pl["depth"], np.float32).tobytes())
    r = subprocess.run([exe, repr(VS), pl["file"], frame], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["status"] == want.status == CONVERGED and np.array_equal(np.float32(js["pose"]).reshape(4, 4), want.T32)
