"""-m gpu: the search scope (drf_set_search_scope(DRF_SEARCH_MAP)): the score stage of drf_score_poses, drf_score_colour_poses,
drf_search_frame and drf_search_colour_frame over the pool and the host store together.  Every comparison is of bits: against
np_score_poses / np_search_frame and the colour restatement, the references of tests/test_fusion_map_search_gpu.py and
tests/test_fusion_search_colour_gpu.py, over the same blocks whatever the split between pool and store, the staging's capacity and
the chunking are, and for whole searches against an engine whose pool holds the whole map -- while no block moves.  96x128 engines
with 2 cm voxels and the 48x64 wall.  The plans of case 3 are those of tests/test_search_scope.py, which says why they take the
random map at a sensor range of 0.6 m.  DESIGN.md §7c "Searching the whole map"."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import test_map_search_colour as SC
import test_search_scope as PL
from fusion_helpers import ROOT
from test_fusion_locate_scope_gpu import EVERYWHERE, stored_engine, with_file
from test_fusion_map_file_gpu import code_of, engine
from test_fusion_map_locate_gpu import DeviceDepth
from test_fusion_map_search_gpu import N_POSES, loaded, search_dict
from test_fusion_search_colour_gpu import colour_search_dict, wall_kw
from test_fusion_streaming_gpu import assert_same_blocks
from test_map_align import MAX_ITERS, bits
from test_map_locate import VS, random_case
from test_map_search import (assert_same_scores, assert_same_search, end_to_end_case, np_score_options, np_score_poses, np_search_frame, random_poses,
                             small_lattice)
from test_map_track import track_scene

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def map_engine(case, capacity=0, region=EVERYWHERE, everything=False, **kw):
    """stored_engine with the search scope set to the whole map; everything: the render and the locate scope too"""
    from tandem_amd.dr_fusion import LOCATE_MAP, RENDER_MAP, SEARCH_MAP
    f = stored_engine(case, scope=False, region=region, **kw)
    f.set_search_scope(SEARCH_MAP, capacity)
    if everything:
        f.set_render_scope(RENDER_MAP)
        f.set_locate_scope(LOCATE_MAP)
    return f


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    """The random map, its file, 259 poses and their restated scores at steps 1, 3 and 4; computed once and left alone"""
    case = with_file(random_case(3), tmp_path_factory.mktemp("search_scope_rnd") / "rnd.drfmap")
    case["poses"] = random_poses(case, N_POSES)
    case["want"] = {step: np_score_poses(case["blocks"], case["cam"], case["depth"], case["poses"], step=step) for step in (1, 3, 4)}
    return case


def lattice_case(directory, SS):
    """The case, the lattice and the CPU plan of tests/test_search_scope.py, its file, the restated search at pixel step 3"""
    case = with_file(PL.scope_case(), directory / "scope.drfmap")
    lat = PL.lattice_plan(SS, case)
    kw = dict(top_k=5, score_only=True, score=dict(step=3), **PL.LATTICE)
    want = np_search_frame(case["blocks"], None, case["cam"], case["depth"], lat["anchors"], lat["rot"], **kw)
    return case, lat, kw, want


@pytest.fixture(scope="module")
def LAT(tmp_path_factory):
    d = tmp_path_factory.mktemp("search_scope_lattice")
    return lattice_case(d, PL.build_check(d))


# ------------------------------------------------------------------ 1
def test_everything_stored(R):
    """Fails without the feature: the parent has no drf_set_search_scope.  The whole random map in the host store, 259 poses (no
    multiple of 4 or 64) at steps 1, 3 and 4, from a host and from a device pointer."""
    from tandem_amd.dr_fusion import SEARCH_MAP, SEARCH_RESIDENT
    f = map_engine(R)
    ss = f.streaming_stats()
    stored = ss["host"]
    assert stored == len(R["blocks"][0]) and ss["resident"] == 0
    dd = DeviceDepth(f, R["depth"])
    for step in (1, 3, 4):
        want = R["want"][step]
        for depth, what in ((R["depth"], "host"), (dd.ptr, "device")):
            assert_same_scores(f.score_poses(depth, R["poses"], step=step), want, "all stored, step %d, %s pointer" % (step, what))
            st, sg = f.search_stats(), f.search_stage_stats()
            assert st[0] == N_POSES and st[3] == 1 and st[7] == stored, st
            assert sg[0] >= 1 and 0 < sg[1] <= stored and sg[2] >= sg[1] and sg[3] >= sg[0], sg
    assert (R["want"][4][1][:, 1] == 0).any() and R["want"][4][1][:, 1].max() > 30
    # flipped back: the resident scope reads nothing, as before
    f.set_search_scope(SEARCH_RESIDENT)
    got = f.score_poses(R["depth"], R["poses"])
    o = np_score_options(R["cam"])
    assert not got[0].any() and (got[1][:, 1] == 0).all() and (got[1][:, 2] == got[1][:, 0]).all() and (got[2] == o["uc"]).all()
    assert f.search_stage_stats() == (0, 0, 0, 0) and f.search_stats()[7] == stored
    f.set_search_scope(SEARCH_MAP)
    assert_same_scores(f.score_poses(R["depth"], R["poses"]), R["want"][4], "map scope again")
    assert f.streaming_stats() == ss
    dd.free()
    f.close()


# ------------------------------------------------------------------ 2
def test_a_split_through_the_samples(R):
    from tandem_amd.dr_fusion import SEARCH_MAP
    want = R["want"][4]
    cut = float(np.median(R["blocks"][0][:, 0])) * 8 * VS               # the half-space x <= cut, through the middle of the map
    f = stored_engine(R, scope=False, region=((-500.0, -500.0, -500.0), (cut, 500.0, 500.0)))
    ss = f.streaming_stats()
    assert ss["host"] > 50 and ss["resident"] > 50
    got = f.score_poses(R["depth"], R["poses"])
    print("split: %d stored, %d resident; resident scope sees %d of %d valid samples over the poses" % (ss["host"], ss["resident"], got[1][:, 1].sum(), want[1][:, 1].sum()))
    assert 0 < got[1][:, 1].sum() < want[1][:, 1].sum()                 # both sides are read
    assert f.search_stage_stats() == (0, 0, 0, 0)
    f.set_search_scope(SEARCH_MAP)
    for step in (4, 1):
        assert_same_scores(f.score_poses(R["depth"], R["poses"], step=step), R["want"][step], "split, step %d" % step)
    sg = f.search_stage_stats()
    assert sg[0] >= 1 and 0 < sg[1] <= ss["host"], sg
    assert f.streaming_stats() == ss
    f.close()


# ------------------------------------------------------------------ 3
def test_many_passes_and_chunk_seams(LAT, parity_hooks, monkeypatch):
    """The lattice of tests/test_search_scope.py, 90 candidates, at the capacity of its CPU plan: at least 3 passes and an ix split.
    all_scores and the entries are the single-pass run's and the restatement's, with DR_SEARCH_CHUNK (the parity library) unset,
    16 and 1; the stagings made are the plan's passes."""
    from tandem_amd.dr_fusion import SEARCH_MAP
    case, lat, kw, want = LAT
    passes = lat["passes"]
    staged = sum(1 for _, _, k in passes if len(k))
    assert len(passes) >= 3 and max(lat["whole"]) > lat["capacity"] and staged == len(passes)
    assert want["n_candidates"] == lat["n"] == 90 and len(np.unique(bits(want["scores"]))) > 50
    f = map_engine(case, max_sensor_depth=PL.SCOPE_DEPTH)
    stored = f.streaming_stats()["host"]
    assert stored == len(case["blocks"][0])
    one = search_dict(f.search_frame(case["depth"], lat["anchors"], lat["rot"], all_scores=True, **kw))
    assert_same_search(one, want, "one pass")
    sg = f.search_stage_stats()
    assert sg[0] == 1 and lat["largest"] <= sg[1] == sg[2] <= stored and sg[3] == 1, sg   # the default capacity holds the union of all units
    f.set_search_scope(SEARCH_MAP, lat["capacity"])
    launches = {None: len(passes), "16": sum(-(-c // 16) for _, c, _ in passes), "1": lat["n"]}
    for chunk in (None, "16", "1"):
        if chunk:
            monkeypatch.setenv("DR_SEARCH_CHUNK", chunk)
        r = search_dict(f.search_frame(case["depth"], lat["anchors"], lat["rot"], all_scores=True, **kw))
        assert_same_search(r, want, "capacity %d, chunk %s" % (lat["capacity"], chunk))
        assert_same_search(r, one, "capacity %d, chunk %s, against one pass" % (lat["capacity"], chunk))
        sg, st = f.search_stage_stats(), f.search_stats()
        assert sg == (len(passes), max(len(k) for _, _, k in passes), sum(len(k) for _, _, k in passes), launches[chunk]), (chunk, sg)
        assert st[0] == lat["n"] and st[3] == launches[chunk] and st[7] == stored, st
    monkeypatch.delenv("DR_SEARCH_CHUNK")
    f.close()


# ------------------------------------------------------------------ 4
def test_the_colour_score(tmp_path):
    """The random map with random colours under a random colour image, all stored: cost, photo, counts and score are the colour
    restatement's; cost and counts are the geometric map-scope call's."""
    case = with_file(SC.random_colour_case(3), tmp_path / "colour.drfmap")
    poses = random_poses(case, 67)
    opt = dict(photo_weight=0.01, photo_cap=3.0)
    f = map_engine(case)
    for step in (3, 4):
        want = SC.np_score_colour_poses(case["blocks"], case["cam"], case["bgr"], case["depth"], poses, step=step, **opt)
        got = f.score_colour_poses(case["bgr"], case["depth"], poses, step=step, **opt)
        SC.assert_same_colour_scores(got, want, "colour, step %d" % step)
        sg = f.search_stage_stats()
        assert sg[0] >= 1 and sg[3] >= 1, sg
        geo = f.score_poses(case["depth"], poses, step=step)
        assert np.array_equal(bits(got[0]), bits(geo[0])) and np.array_equal(got[2], geo[1]), step
    assert want[2][:, 1].max() > 30 and len(np.unique(bits(want[1]))) > 30
    f.close()


# ------------------------------------------------------------------ 5
def test_far_blocks(tmp_path):
    """Map and camera moved by whole blocks beyond block coordinate 256, all stored: the sorted-key path of LocateFetchStaged."""
    case = with_file(random_case(3, shift=(300, -270, 5)), tmp_path / "far.drfmap")
    assert np.abs(case["blocks"][0]).max() > 256
    poses = random_poses(case, 13)
    f = map_engine(case)
    want = np_score_poses(case["blocks"], case["cam"], case["depth"], poses)
    assert_same_scores(f.score_poses(case["depth"], poses), want, "far blocks")
    assert f.search_stage_stats()[0] >= 1 and want[1][:, 1].max() > 10
    f.close()


# ------------------------------------------------------------------ 6
def test_a_whole_search(tmp_path):
    """The one-scan scene of 1 968 blocks, stored entirely, the search, render and locate scopes all set to the whole map:
    end_to_end_case's lattice with top_k 2 and accept_valid, so that one entry refines.  Status, winner, entries, the pose and
    all_scores are those of the same call on an engine whose pool holds the map (which the existing suite holds to the CPU)."""
    s = with_file(track_scene(), tmp_path / "scene.drfmap")
    anchors, rot, kw = end_to_end_case(s)
    kw.update(top_k=2, accept_valid=0.5)
    g = loaded(s)
    want = search_dict(g.search_frame(s["depth"], anchors, rot, all_scores=True, **kw))
    g.close()
    assert want["refined"] == 1 and want["winner"] == 0 and want["status"] <= MAX_ITERS and len(want["entries"]) == 2
    f = map_engine(s, everything=True)
    ss = f.streaming_stats()
    assert ss["host"] == len(s["blocks"][0]) == 1968 and ss["resident"] == 0
    before = f.export_host_blocks()
    dd = DeviceDepth(f, s["depth"])
    for depth, what in ((s["depth"], "host"), (dd.ptr, "device")):
        got = search_dict(f.search_frame(depth, anchors, rot, all_scores=True, **kw))
        assert_same_search(got, want, "scene, all stored, %s pointer" % what)
        sg, st = f.search_stage_stats(), f.search_stats()
        assert sg[0] >= 1 and 0 < sg[1] <= 1968 and st[7] == 1968 and st[4] > 0 and st[5] > 0, (sg, st)
    assert f.locate_stage_stats()[0] >= 1 and f.streaming_stats() == ss
    assert_same_blocks(f.export_host_blocks(), before, "host store")
    dd.free()
    f.close()


# ------------------------------------------------------------------ 7
def test_the_colour_search_on_the_wall(tmp_path):
    """The oracle-integrated wall, stored entirely, all three scopes on the whole map: the colour search, its final re-score
    included, is the resident engine's bit for bit."""
    w = with_file(SC.integrated_wall(), tmp_path / "wall.drfmap")
    anchor, eye = SC.wall_anchor()[None], np.eye(3).reshape(1, 9)
    g = loaded(w)
    want = colour_search_dict(g.search_colour_frame(w["bgr"], w["depth"], anchor, eye, all_scores=True, **wall_kw()))
    st_want = g.search_stats()
    g.close()
    assert want["refined"] == 3 and want["winner"] >= 0 and want["entries"][want["winner"]]["final_score"] > 0
    f = map_engine(w, everything=True)
    ss = f.streaming_stats()
    assert ss["host"] == len(w["blocks"][0]) and ss["resident"] == 0
    got = colour_search_dict(f.search_colour_frame(w["bgr"], w["depth"], anchor, eye, all_scores=True, **wall_kw()))
    SC.assert_same_colour_search(got, want, "wall, all stored")
    st, sg = f.search_stats(), f.search_stage_stats()
    assert st[:6] == st_want[:6] and st[7] == ss["host"], (st, st_want)   # the final re-score is not counted in [0] or [3]
    assert sg[0] >= 2 and sg[3] >= 2, sg                                  # the score stage and the final re-score each staged
    assert f.streaming_stats() == ss
    f.close()


# ------------------------------------------------------------------ 8
def test_refusals_and_legality_in_their_order(R, LAT):
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import SEARCH_MAP, SEARCH_RESIDENT
    f = map_engine(R)
    L = f._L
    # an unknown scope
    assert code_of(f.set_search_scope, 2) == 1 and code_of(f.set_search_scope, -1) == 1
    assert L.drf_search_stage_stats(f._h, None) == 1
    assert L.drf_set_search_scope(None, 1, 0) == 1 and L.drf_search_stage_stats(None, (C.c_uint64 * 4)()) == 1
    assert_same_scores(f.score_poses(R["depth"], R["poses"][:9]), tuple(w[:9] for w in R["want"][4]), "an unknown scope changed nothing")
    # a pending render
    f.RenderAsync([np.eye(4, dtype=f32)])                               # (a loaded map may be rendered before its next scan)
    assert code_of(f.set_search_scope, SEARCH_RESIDENT) == 2 and code_of(f.set_search_scope, SEARCH_MAP, 4) == 2
    assert code_of(f.score_poses, R["depth"], R["poses"][:9]) == 2
    f.GetRenderResult()
    assert_same_scores(f.score_poses(R["depth"], R["poses"][:9]), tuple(w[:9] for w in R["want"][4]), "the refused setter changed nothing")
    assert f.search_stage_stats()[0] >= 1
    # a capacity below one pose's selection: refused before anything is evaluated, nothing written
    f.set_search_scope(SEARCH_MAP, 4)
    before = (f.export_all_blocks(), f.streaming_stats())
    cost, counts, score = np.full(9, -7.0), np.full((9, 4), 77, np.uint32), np.full(9, -7.0)
    poses = np.ascontiguousarray(R["poses"][:9], f32).reshape(-1, 16)
    depth = np.ascontiguousarray(R["depth"], f32)
    rc = L.drf_score_poses(f._h, depth.ctypes.data_as(_lib.f32p), poses.ctypes.data_as(_lib.f32p), 9, None, cost.ctypes.data_as(_lib.f64p),
                           counts.ctypes.data_as(C.POINTER(C.c_uint32)), score.ctypes.data_as(_lib.f64p))
    msg = L.dr_last_error().decode()
    assert rc == 5 and "drf_set_search_scope" in msg and "drf_stream_in_region" in msg and "holds 4 " in msg and "stored blocks" in msg, msg
    assert (cost == -7.0).all() and (counts == 77).all() and (score == -7.0).all()
    assert f.search_stats() == (0,) * 8 and f.search_stage_stats() == (0, 0, 0, 0)
    scaled = R["poses"][:2].copy()
    scaled[1, :3, :3] *= 1.01
    assert code_of(f.score_poses, R["depth"], scaled) == 1              # a pose that is refused comes before the capacity
    with pytest.raises(_lib.DrError) as e:
        f.score_poses(R["depth"], R["poses"][:9], step=-1)
    assert e.value.code == 1 and "step" in str(e.value)                 # ... and an option before both
    assert f.streaming_stats() == before[1]
    assert_same_blocks(f.export_all_blocks(), before[0], "after the refusals")
    f.close()
    # the lattice: one below the largest single slab is refused with that count, the count itself is served
    case, lat, kw, want = LAT
    f = map_engine(case, capacity=lat["largest"] - 1, max_sensor_depth=PL.SCOPE_DEPTH)
    with pytest.raises(_lib.DrError) as e:
        f.search_frame(case["depth"], lat["anchors"], lat["rot"], **kw)
    assert e.value.code == 5 and "can read %d stored blocks" % lat["largest"] in str(e.value) and "holds %d " % (lat["largest"] - 1) in str(e.value), str(e.value)
    assert f.search_stats() == (0,) * 8 and f.search_stage_stats() == (0, 0, 0, 0)
    f.set_search_scope(SEARCH_MAP, lat["largest"])
    assert_same_search(search_dict(f.search_frame(case["depth"], lat["anchors"], lat["rot"], all_scores=True, **kw)), want, "capacity = the largest slab")
    f.close()
    # the scope has no effect with streaming off, or on with an empty store
    f = loaded(R)
    f.set_search_scope(SEARCH_MAP)
    assert_same_scores(f.score_poses(R["depth"], R["poses"]), R["want"][4], "streaming off")
    assert f.search_stage_stats() == (0, 0, 0, 0) and f.search_stats()[7] == 0
    from tandem_amd.dr_fusion import streaming_min_radius
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))
    assert f.streaming_stats()["host"] == 0
    assert_same_scores(f.score_poses(R["depth"], R["poses"]), R["want"][4], "an empty store")
    assert f.search_stage_stats() == (0, 0, 0, 0)
    f.close()


# ------------------------------------------------------------------ 9
def test_shim(tmp_path):
    """tandem_amd/libdr/dr_fusion.h SetSearchScope, SearchStageStats, ScorePoses and SearchDepthFrame over a map that is all in the
    host store, held to the answers of an engine whose pool holds it."""
    s = with_file(track_scene(), tmp_path / "scene.drfmap")
    anchors, rot, kw = end_to_end_case(s)
    g = loaded(s)
    want_score = g.score_poses(s["depth"], anchors)[2][0]
    want = g.search_frame(s["depth"], anchors, rot, half=(1, 1, 1), top_k=2, raise_on_failure=False)   # the shim passes no track or locate options
    g.close()
    exe, frame = str(tmp_path / "search_scope_shim"), str(tmp_path / "frame.bin")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/search_scope_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    with open(frame, "wb") as fh:
        fh.write(np.ascontiguousarray(anchors[0], f32).tobytes() + np.ascontiguousarray(s["depth"], f32).tobytes() + np.uint64(len(rot)).tobytes() + rot.tobytes())
    cam = s["cam"]
    r = subprocess.run([exe, repr(VS)] + [repr(float(f32(cam[k]))) for k in ("fx", "fy", "cx", "cy")] + [str(cam["num_blocks"]), s["file"], frame],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["resident_score"] == np_score_options(cam)["uc"]          # everything is stored: the resident scope sees nothing
    assert js["status"] == want.status and js["winner"] == want.winner and js["index"] == want.entries[max(want.winner, 0)].index
    assert js["anchor_score"] == want_score and js["stagings"] >= 1 and np.array_equal(f32(js["pose"]).reshape(4, 4), want.T32)
