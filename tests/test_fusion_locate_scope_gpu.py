"""-m gpu: the locate scope (drf_set_locate_scope(DRF_LOCATE_MAP)): drf_locate_system / drf_locate_frame over the pool and the host
store together.  Every comparison is of bits: against an engine whose pool holds the whole map, and against np_locate_system /
np_locate_frame, the restatement of tests/test_map_locate.py, over the same blocks -- whatever the split between pool and store --
while no block moves.  96x128 engines with 2 cm voxels, one of 168x200.  DESIGN.md §7c "Locating in the whole map"."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import ROOT, feed
from guard_helpers import POISON_WORD, assert_same_bits, guarded
from test_fusion_map_file_gpu import code_of, engine
from test_fusion_map_locate_gpu import DeviceDepth, result_dict
from test_fusion_map_transform_gpu import write
from test_fusion_streaming_gpu import assert_same_blocks, two_places
from test_map_align import LOST, assert_same_result, assert_same_system
from test_map_locate import H, SYSTEM_CASES, VS, W, np_locate_frame, np_locate_system, np_options, np_system, motion, random_case, scene_case, start_near

pytestmark = pytest.mark.gpu

EVERYWHERE = ((-500.0, -500.0, -500.0), (500.0, 500.0, 500.0))
FRAME_OPT = dict(max_iters=3)


def radius(f):
    from tandem_amd.dr_fusion import streaming_min_radius
    return max(streaming_min_radius(f.options), 8.0)


def stored_engine(case, scope=True, region=EVERYWHERE, **kw):
    """The case's map loaded, streaming on, the blocks whose origin lies in `region` sent to the host store."""
    from tandem_amd.dr_fusion import LOCATE_MAP
    f = engine(case["cam"], **kw)
    f.load_map(case["file"])
    f.set_streaming(radius(f))
    f.stream_out_region(*region)
    if scope:
        f.set_locate_scope(LOCATE_MAP)
    return f


def as_blocks(blk):
    coords = np.array(sorted(blk), np.int64).reshape(-1, 3)
    return coords, np.stack([blk[tuple(c)] for c in coords.tolist()])


def with_file(case, path):
    case["file"] = str(path)
    write(case["file"], VS, *case["blocks"])
    return case


def frame_want(case, start, **opt):
    want = np_locate_frame(case["blocks"], case["cam"], case["depth"], start, **opt)
    want.pop("trace")
    want.pop("counts4", None)
    return want


@pytest.fixture(scope="module")
def D(tmp_path_factory):
    """The integrated scene and the random map with their files; the references, computed once and left alone.  near: a start whose
    whole refinement stays within the staging's slack (0.3 degrees and one voxel off the scan's pose: a drift of about 0.11 m
    against a slack of 0.22 m at these options)."""
    d = tmp_path_factory.mktemp("locate_scope")
    sc, rnd = with_file(scene_case(), d / "scene.drfmap"), with_file(random_case(3), d / "rnd.drfmap")
    sc["near"] = start_near(sc["pose"].astype(np.float64), (1, 1, -1), 0.3, (0.6, -0.3, 0.6))
    sc["opt"] = dict(centre_depth=sc["centre_depth"], **FRAME_OPT)
    out = dict(dir=d, scene=sc, rnd=rnd)
    out["scene_sys"] = {name: np_locate_system(sc["blocks"], sc["cam"], sc["depth"], sc["start"], **opt) for name, opt in SYSTEM_CASES}
    out["scene_frame"] = frame_want(sc, sc["near"], **sc["opt"])
    return out


def check_scene(f, D, stored, what):
    """Every system case and the refinement in map scope, host and device pointer: the restatement's bits, one staging per call."""
    sc = D["scene"]
    dd = DeviceDepth(f, sc["depth"])
    out = []
    for name, opt in SYSTEM_CASES:
        for depth in (sc["depth"], dd.ptr):
            got = f.locate_system(depth, sc["start"], **opt)
            assert_same_system(got, D["scene_sys"][name], "%s, %s" % (what, name))
            st = f.locate_stage_stats()
            assert st[0] == 1 and 0 < st[1] <= stored and st[2] == st[1] and st[3] == 1, st
            assert f.locate_stats()[5] == stored
        out.append((name, got[0]))
    for depth in (sc["depth"], dd.ptr):
        r = f.locate_frame(depth, sc["near"], **sc["opt"])
        assert_same_result(result_dict(r), D["scene_frame"], what + ", refinement")
        st = f.locate_stage_stats()
        assert st[0] == 1 and 0 < st[1] <= stored and st[3] == r.iterations == 3, st
    dd.free()
    return out + [("pose", r.T), ("pose32", r.T32), ("sums", r.sums)]


# ------------------------------------------------------------------ 1
def test_everything_stored(D):
    """Fails without the feature: the parent has no drf_set_locate_scope."""
    from tandem_amd.dr_fusion import LOCATE_MAP, LOCATE_RESIDENT
    sc = D["scene"]
    g = engine(sc["cam"])                                              # the whole map in the pool
    g.load_map(sc["file"])
    for name, opt in SYSTEM_CASES:
        assert_same_system(g.locate_system(sc["depth"], sc["start"], **opt), D["scene_sys"][name], "resident engine, " + name)
    assert_same_result(result_dict(g.locate_frame(sc["depth"], sc["near"], **sc["opt"])), D["scene_frame"], "resident engine, refinement")
    assert g.locate_stage_stats() == (0, 0, 0, 0)
    g.close()
    f = stored_engine(sc)
    stored = f.streaming_stats()["host"]
    assert stored == len(sc["blocks"][0]) and f.streaming_stats()["resident"] == 0
    check_scene(f, D, stored, "all stored")
    # flipped back: the resident scope reads nothing, as before
    f.set_locate_scope(LOCATE_RESIDENT)
    got = f.locate_system(sc["depth"], sc["start"])
    n = D["scene_sys"]["defaults"][1][0]
    assert got[1] == (n, 0, n, 0) and not got[0].any() and f.locate_stage_stats() == (0, 0, 0, 0) and f.locate_stats()[5] == stored
    f.set_locate_scope(LOCATE_MAP)
    assert_same_system(f.locate_system(sc["depth"], sc["start"]), D["scene_sys"]["defaults"], "map scope again")
    f.close()


# ------------------------------------------------------------------ 2
def test_a_split_through_the_samples(D):
    from tandem_amd.dr_fusion import LOCATE_MAP
    sc = D["scene"]
    want = D["scene_sys"]["defaults"]
    cut = float(np.median(sc["blocks"][0][:, 0])) * 8 * VS             # the half-space x <= cut, through the middle of the map
    f = stored_engine(sc, scope=False, region=((-500.0, -500.0, -500.0), (cut, 500.0, 500.0)))
    ss = f.streaming_stats()
    assert ss["host"] > 100 and ss["resident"] > 100
    got = f.locate_system(sc["depth"], sc["start"])
    print("split: %d stored, %d resident; resident scope sees %d of %d valid samples" % (ss["host"], ss["resident"], got[1][1], want[1][1]))
    assert 0 < got[1][1] < want[1][1]                                  # both sides are read
    f.set_locate_scope(LOCATE_MAP)
    check_scene(f, D, ss["host"], "split")
    assert f.streaming_stats() == ss
    f.close()


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("shift", [(300, -270, 5), (253, 0, 0)], ids=["beyond the grid", "across coordinate 256"])
def test_beyond_the_dense_grid(tmp_path, shift):
    """Stored blocks at |coordinate| >= 256 are found by the binary search of the staged keys; with a shift of 253 blocks the map's
    blocks [-3, 3] + 253 lie on both sides of coordinate 256 in one staging."""
    case = with_file(random_case(3, shift=shift), tmp_path / "far.drfmap")
    x = case["blocks"][0]
    assert (np.abs(x).max(1) >= 256).any() and ((np.abs(x).max(1) < 256).any() or shift[0] == 300)
    f = stored_engine(case)
    stored = f.streaming_stats()["host"]
    assert stored == len(x)
    for opt in ({}, dict(step=3)):
        want = np_locate_system(case["blocks"], case["cam"], case["depth"], case["pose"], **opt)
        assert want[1][1] > 10
        assert_same_system(f.locate_system(case["depth"], case["pose"], **opt), want, "shift %s %s" % (shift, opt))
        assert f.locate_stage_stats()[0] == 1 and 0 < f.locate_stage_stats()[1] <= stored
    opt = dict(max_iters=3, min_valid=0.01)
    r = f.locate_frame(case["depth"], case["pose"], raise_on_failure=False, **opt)
    assert_same_result(result_dict(r), frame_want(case, case["pose"], **opt), "shift %s, refinement" % (shift,))
    f.close()


# ------------------------------------------------------------------ 4
def test_tails(tmp_path, D):
    """168x200: 66 groups, the last 320 wide; 96x128 at step 3: 1 376 positions (the random map: test_beyond_the_dense_grid runs
    that grid beyond the dense grid, this one inside it)."""
    case = random_case(20 + 168, 168, 200)
    case["cam"].update(cx=99.5, cy=83.5)
    with_file(case, tmp_path / "m.drfmap")
    f = stored_engine(case)
    got = f.locate_system(case["depth"], case["pose"])
    assert f.locate_stats()[0] == 33600 and f.locate_stage_stats()[0] == 1
    f.close()
    want = np_locate_system(case["blocks"], case["cam"], case["depth"], case["pose"])
    assert_same_system(got, want, "168x200, stored")
    assert want[1][1] > 100
    rnd = D["rnd"]
    f = stored_engine(rnd)
    got = f.locate_system(rnd["depth"], rnd["pose"], step=3)
    assert f.locate_stats()[0] == 1376 and f.locate_stage_stats()[0] == 1
    f.close()
    assert_same_system(got, np_locate_system(rnd["blocks"], rnd["cam"], rnd["depth"], rnd["pose"], step=3), "step 3, stored")


# ------------------------------------------------------------------ 5
def test_restaging(D, parity_hooks, monkeypatch):
    """DR_LOCATE_STAGE_SLACK=0 (the parity library): every moved pose stages again, and nothing changes in the result."""
    sc = D["scene"]
    f = stored_engine(sc)
    r = f.locate_frame(sc["depth"], sc["near"], **sc["opt"])
    st = f.locate_stage_stats()
    assert_same_result(result_dict(r), D["scene_frame"], "default slack")
    assert r.iterations == 3 and st[0] == 1 and st[3] == 3 and st[2] == st[1], st
    monkeypatch.setenv("DR_LOCATE_STAGE_SLACK", "0")
    r0 = f.locate_frame(sc["depth"], sc["near"], **sc["opt"])
    st0 = f.locate_stage_stats()
    print("restaging: %s with the rule's slack, %s with none" % (st, st0))
    assert_same_result(result_dict(r0), D["scene_frame"], "no slack")
    assert_same_bits(r0.T, r.T, "pose")
    assert st0[0] == 3 and st0[3] == 3 and st0[1] > 0 and st0[1] < st0[2] <= 3 * st0[1], st0   # three distinct poses, three stagings
    got = f.locate_system(sc["depth"], sc["start"])                    # one pose: one staging, slack or none
    assert_same_system(got, D["scene_sys"]["defaults"], "no slack, one evaluation")
    assert f.locate_stage_stats()[0] == 1
    monkeypatch.delenv("DR_LOCATE_STAGE_SLACK")
    # a start a degree off moves farther than the slack allows: the rule itself stages again, with the same bits
    opt = dict(centre_depth=sc["centre_depth"], max_iters=3)
    r1 = f.locate_frame(sc["depth"], sc["start"], **opt)
    st1 = f.locate_stage_stats()
    print("a degree off: %s" % (st1,))
    assert_same_result(result_dict(r1), frame_want(sc, sc["start"], **opt), "a degree off")
    assert 1 <= st1[0] <= 3 and st1[3] == 3
    f.close()


# ------------------------------------------------------------------ 6
def test_capacity(D):
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import LOCATE_MAP
    sc = D["scene"]
    R, tv = motion(sc["start"], sc["cam"]["voxel_size"])
    det = np_system(sc["blocks"], sc["cam"], sc["depth"], R, tv, np_options(sc["cam"]), detail=True)[2]
    touched = {tuple(int(c) for c in b) for b in (np.floor(det["q"][det["valid"]]).astype(np.int64) >> 3)}
    assert len(touched) > 4                                            # blocks the evaluation reads, all of them stored
    f = stored_engine(sc)
    f.locate_system(sc["depth"], sc["start"])
    selected = f.locate_stage_stats()[1]
    assert selected >= len(touched)
    f.set_locate_scope(LOCATE_MAP, 4)
    before = (f.export_all_blocks(), f.streaming_stats())
    assert touched <= set(before[0])
    for call in (lambda: f.locate_system(sc["depth"], sc["start"]), lambda: f.locate_frame(sc["depth"], sc["start"])):
        with pytest.raises(_lib.DrError) as e:
            call()
        assert e.value.code == 5 and "drf_set_locate_scope" in str(e.value) and "drf_stream_in_region" in str(e.value), str(e.value)
        assert "holds 4 " in str(e.value) and "can read %d stored blocks" % selected in str(e.value), str(e.value)
        assert f.locate_stats() == (0, 0, 0, 0, 0, 0) and f.locate_stage_stats() == (0, 0, 0, 0)
    assert f.streaming_stats() == before[1]
    assert_same_blocks(f.export_all_blocks(), before[0], "after the refusals")
    f.set_locate_scope(LOCATE_MAP, 0)
    assert_same_system(f.locate_system(sc["depth"], sc["start"]), D["scene_sys"]["defaults"], "capacity 0")
    f.close()


# ------------------------------------------------------------------ 7
def test_the_map_is_untouched(D):
    from tandem_amd.dr_fusion import LOCATE_MAP, RENDER_MAP
    sc = D["scene"]
    cut = float(np.median(sc["blocks"][0][:, 0])) * 8 * VS
    region = ((-500.0, -500.0, -500.0), (cut, 500.0, 500.0))
    view = start_near(sc["pose"].astype(np.float64), (0, 1, 0), 3.0, (2.0, 0.0, 0.0))
    moved = start_near(sc["pose"].astype(np.float64), (1, 0, 0), 2.0, (1.0, 2.0, 0.0))

    def render(e):
        e.RenderAsync([view])
        rb, rd = e.GetRenderResult()
        return rb[0].copy(), rd[0].copy()

    f, g = stored_engine(sc, region=region), stored_engine(sc, scope=False, region=region)
    for e in (f, g):
        e.set_render_scope(RENDER_MAP)
    before = (f.export_blocks(), f.export_host_blocks(), f.streaming_stats())
    assert_same_result(result_dict(f.locate_frame(sc["depth"], sc["near"], **sc["opt"])), D["scene_frame"], "split, refinement")
    assert f.locate_stage_stats()[0] == 1
    f.locate_system(sc["depth"], sc["start"], step=2)
    assert f.streaming_stats() == before[2]
    assert_same_blocks(f.export_blocks(), before[0], "pool")
    assert_same_blocks(f.export_host_blocks(), before[1], "host store")
    a, b = render(f), render(g)                                        # the map-scope render uses the same staging right after
    assert f.render_stats()[0] > 0 and f.render_stats() == g.render_stats()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    for e in (f, g):
        feed(e, sc["bgr"], sc["depth"], moved)
    timeless = lambda s: {k: v for k, v in s.items() if k != "last_scan_us"}  # noqa: E731 -- a duration, not state
    assert timeless(f.streaming_stats()) == timeless(g.streaming_stats()) and f.stats() == g.stats()
    assert_same_blocks(f.export_all_blocks(), g.export_all_blocks(), "after the next scan")
    f.close()
    g.close()


# ------------------------------------------------------------------ 8
def test_nothing_to_stage(D):
    from tandem_amd.dr_fusion import LOCATE_MAP, LOCATE_RESIDENT
    sc = D["scene"]
    want = D["scene_sys"]["defaults"]
    f = engine(sc["cam"])
    f.load_map(sc["file"])
    f.set_locate_scope(LOCATE_MAP)                                     # streaming off
    assert_same_system(f.locate_system(sc["depth"], sc["start"]), want, "streaming off")
    assert f.locate_stage_stats() == (0, 0, 0, 0)
    f.set_streaming(radius(f))                                         # streaming on, an empty store
    assert f.streaming_stats()["host"] == 0
    assert_same_system(f.locate_system(sc["depth"], sc["start"]), want, "empty store")
    assert_same_result(result_dict(f.locate_frame(sc["depth"], sc["near"], **sc["opt"])), D["scene_frame"], "empty store, refinement")
    assert f.locate_stage_stats() == (0, 0, 0, 0)
    f.close()
    # stored blocks that all lie outside the selection: a sensor of 4 m, the camera 16 m from the map
    f = stored_engine(sc, max_sensor_depth=4.0)
    gone = sc["start"].copy()
    gone[0, 3] += 100 * 8 * VS
    got = f.locate_system(sc["depth"], gone)
    assert f.locate_stage_stats() == (0, 0, 0, 0) and f.locate_stats()[5] == len(sc["blocks"][0])
    r = f.locate_frame(sc["depth"], gone, raise_on_failure=False)
    msg = f._L.dr_last_error().decode()
    assert r.status == LOST and "0 of them staged" in msg and "%d blocks are in the host store" % len(sc["blocks"][0]) in msg, msg
    f.set_locate_scope(LOCATE_RESIDENT)
    assert_same_system(f.locate_system(sc["depth"], gone), got, "resident scope at the same pose")
    assert got[1][1] == 0 and got[1][2] == got[1][0] > 0
    f.close()


# ------------------------------------------------------------------ 9
def test_legality_in_its_order(D):
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import LOCATE_MAP
    sc = D["scene"]
    f = stored_engine(sc)
    L = f._L
    assert code_of(f.set_locate_scope, 2) == 1 and code_of(f.set_locate_scope, -1) == 1
    assert L.drf_locate_stage_stats(f._h, None) == 1
    assert L.drf_set_locate_scope(None, 1, 0) == 1 and L.drf_locate_stage_stats(None, (C.c_uint64 * 4)()) == 1
    assert_same_system(f.locate_system(sc["depth"], sc["start"]), D["scene_sys"]["defaults"], "an unknown scope changed nothing")
    # the order: option, protocol, pose, capacity
    f.set_locate_scope(LOCATE_MAP, 4)
    scaled = sc["start"].copy()
    scaled[:3, :3] *= 1.01
    assert code_of(f.locate_system, sc["depth"], sc["start"]) == 5
    assert code_of(f.locate_system, sc["depth"], scaled) == 1          # the pose before the capacity
    with pytest.raises(_lib.DrError) as e:
        f.locate_system(sc["depth"], scaled, step=-1)
    assert e.value.code == 1 and "step" in str(e.value)                # the option before the pose
    f.RenderAsync([np.eye(4, dtype=np.float32)])                       # (a loaded map may be rendered before its next scan)
    assert code_of(f.locate_system, sc["depth"], scaled) == 2          # the protocol before the pose
    assert code_of(f.locate_system, sc["depth"], sc["start"]) == 2     # ... and before the capacity
    assert code_of(f.set_locate_scope, LOCATE_MAP, 0) == 2             # the setter between RenderAsync and GetRenderResult
    f.GetRenderResult()
    assert code_of(f.locate_system, sc["depth"], sc["start"]) == 5     # the refused setter changed nothing
    assert f.locate_stage_stats() == (0, 0, 0, 0)
    f.close()


def test_live_loop_with_automatic_eviction():
    """synth.scene at two places 20 m apart, streaming with automatic eviction: the first scan's blocks are in the store when its
    depth is located from a perturbed pose; the restatement over export_all_blocks."""
    from tandem_amd.dr_fusion import LOCATE_MAP, DrFusion, DrFusionOptions, streaming_min_radius
    sc, scans, opt = two_places(2)
    f = DrFusion(DrFusionOptions(**opt))
    f.set_streaming(streaming_min_radius(f.options))
    f.set_locate_scope(LOCATE_MAP)
    for scan in scans:
        feed(f, *scan)
    bgr, depth, pose = scans[0]
    start = start_near(pose.astype(np.float64), (1, -2, 1), 0.3, (0.5, 0.4, -0.5))
    lo = dict(max_iters=3, centre_depth=2.0)
    ss = f.streaming_stats()
    r = f.locate_frame(depth, start, raise_on_failure=False, **lo)
    st = f.locate_stage_stats()
    assert f.streaming_stats() == ss and ss["host"] > 100
    blk = f.export_all_blocks()
    first = f.export_host_blocks()
    f.close()
    want = np_locate_frame(as_blocks(blk), opt, depth, start, **lo)
    want.pop("trace")
    want.pop("counts4", None)
    assert_same_result(result_dict(r), want, "live loop")
    print("live loop: %d stored, stagings %s, %d of %d valid" % (ss["host"], st, r.valid, r.samples))
    assert r.valid > 0.25 * r.samples and st[0] >= 1 and 0 < st[1] <= len(first) and st[3] == r.iterations


# ------------------------------------------------------------------ 10
def test_shim(D, tmp_path):
    """tandem_amd/libdr/dr_fusion.h SetLocateScope then LocateDepthFrame over a map that is all in the host store."""
    sc = D["scene"]
    g = engine(sc["cam"])
    g.load_map(sc["file"])
    want = g.locate_frame(sc["depth"], sc["near"])                     # the shim passes no options
    g.close()
    exe, frame = str(tmp_path / "locate_scope_shim"), str(tmp_path / "frame.bin")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/locate_scope_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    cam = sc["cam"]
    with open(frame, "wb") as fh:
        fh.write(np.float32([cam["fx"], cam["fy"], cam["cx"], cam["cy"]]).tobytes() + np.ascontiguousarray(sc["near"], np.float32).tobytes() +
                 np.ascontiguousarray(sc["depth"], np.float32).tobytes())
    r = subprocess.run([exe, repr(VS), sc["file"], frame], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["resident_status"] == LOST                               # everything is stored: the resident scope sees nothing
    assert js["status"] == want.status and np.array_equal(np.float32(js["pose"]).reshape(4, 4), want.T32)


# ------------------------------------------------------------------ 11
def test_under_guards(D, tmp_path, parity_hooks):
    """Cases 1 and 3 with every device allocation -- the staging, its table and flags, the call's scratch -- between guard bands
    and poisoned: no guard changes, no poison word reaches a result, and the bits are those of the unguarded run."""
    sc = D["scene"]
    far = with_file(random_case(3, shift=(253, 0, 0)), tmp_path / "far.drfmap")
    want_far = np_locate_system(far["blocks"], far["cam"], far["depth"], far["pose"])

    def run():
        f = stored_engine(sc)
        out = check_scene(f, D, len(sc["blocks"][0]), "guards")
        f.close()
        f = stored_engine(far)
        got = f.locate_system(far["depth"], far["pose"])
        f.close()
        assert_same_system(got, want_far, "across coordinate 256")
        return out + [("far", got[0])]

    with guarded():
        on = run()
    off = run()
    for (na, xa), (nb, xb) in zip(on, off):
        assert na == nb
        assert_same_bits(xa, xb, na)
        assert not (np.ascontiguousarray(xa).view(np.uint32) == POISON_WORD).any(), na
