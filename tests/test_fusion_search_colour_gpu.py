"""-m gpu: drf_score_colour_poses / drf_search_colour_frame.  The reference of every bit comparison is np_score_colour_poses /
np_search_colour_frame, the numpy restatement of the rule in tests/test_map_search_colour.py, for whole searches
search_colour_refine through tests/cpp/map_search_colour_check.cpp over the CPU oracle's ray-cast (which
tests/test_map_search_colour.py holds to the restatement), and for cost and counts drf_score_poses and drf_locate_system
themselves.  96x128 engines, one of 168x200 and the 48x64 wall; the random map with random colours, the oracle-integrated wall of
25 scans and the one-scan scene of 1 968 blocks.  DESIGN.md §7c "Searching with colour"."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import test_map_search_colour as SC
from fusion_helpers import ROOT
from test_fusion_map_file_gpu import engine
from test_fusion_map_search_gpu import N_POSES, code_of, loaded, search_dict
from test_fusion_track_colour_gpu import DeviceImage
from test_fusion_map_transform_gpu import write
from test_map_align import CONVERGED, LOST, MAX_ITERS, bits
from test_map_locate import NONE, random_case
from test_map_search import H, SCENE_STEP, VS, W, assert_same_scores, end_to_end_case, np_candidates, np_select, random_poses, scene_anchor, scene_lattice, small_lattice
from test_map_track import track_opts, track_scene

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def colour_scratch_bytes(height, width, step, table_entries, chunk=65536):
    """drf_search_stats()[6] of a colour call: 24 bytes of point, 4 of yf and a flag byte per padded grid position, the pose table,
    40 bytes per candidate of a chunk, a host-given depth image and colour image"""
    padded = 512 * -(-(-(-width // step) * -(-height // step)) // 512)
    return 29 * padded + 96 * max(table_entries, 1) + 40 * chunk + 7 * height * width


def colour_search_dict(r):
    return dict(search_dict(r), photos=None)


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    """The random map with random colours, its file, 259 poses and their restated colour scores at steps 1, 3 and 4"""
    d = tmp_path_factory.mktemp("search_colour_rnd")
    case = SC.random_colour_case(3)
    case["file"] = str(d / "rnd.drfmap")
    write(case["file"], VS, *case["blocks"])
    case["poses"] = random_poses(case, N_POSES)
    case["opt"] = dict(photo_weight=0.01, photo_cap=3.0)                  # both sides of both branches (tests/test_map_search_colour.py COLOUR_SETS)
    case["want"] = {step: SC.np_score_colour_poses(case["blocks"], case["cam"], case["bgr"], case["depth"], case["poses"], step=step, **case["opt"]) for step in (1, 3, 4)}
    return case


@pytest.fixture(scope="module")
def WALL(tmp_path_factory):
    """The oracle-integrated wall, its map file, the check library and the CPU run of the end-to-end search"""
    d = tmp_path_factory.mktemp("search_colour_wall")
    w = SC.integrated_wall()
    w["file"] = str(d / "wall.drfmap")
    write(w["file"], VS, *w["blocks"])
    w["HS"], w["dir"] = SC.build_check(d), d
    w["anchor"], w["eye"] = SC.wall_anchor()[None], np.eye(3).reshape(1, 9)
    w["want"] = SC.cpp_search(w["HS"], w["blocks"], w["render"], w["cam"], w["bgr"], w["depth"], w["anchor"], w["eye"], **SC.WALL_END_TO_END)
    return w


def wall_kw():
    kw = dict(SC.WALL_END_TO_END)
    track = dict(kw.pop("track"))
    kw.update(levels=track.pop("levels"), track=track)
    return kw


# ------------------------------------------------------------------ 1
def test_score_against_the_restatement_drf_score_poses_and_drf_locate_system(R):
    """259 poses at steps 1, 3 and 4: cost, photo, counts and score are the restatement's, from host and from device pointers; cost
    and counts are drf_score_poses' and, pose by pose, drf_locate_system's sums[27] and counts; the statistics; then the map of
    one colour under an image of that colour: photo +0.0 everywhere and the score drf_score_poses' bits."""
    f = loaded(R)
    db, dd = DeviceImage(f, R["bgr"], np.uint8), DeviceImage(f, R["depth"], f32)
    for step in (1, 3, 4):
        want = R["want"][step]
        got = f.score_colour_poses(R["bgr"], R["depth"], R["poses"], step=step, **R["opt"])
        SC.assert_same_colour_scores(got, want, "step %d" % step)
        st = f.search_stats()
        assert st == (N_POSES, -(-W // step) * -(-H // step), int(want[2][0, 0]), 1, 0, 0, st[6], 0), st
        assert st[6] >= colour_scratch_bytes(H, W, step, N_POSES)
        SC.assert_same_colour_scores(f.score_colour_poses(db.ptr, dd.ptr, R["poses"], step=step, **R["opt"]), want, "step %d (device pointers)" % step)
        geo = f.score_poses(dd.ptr, R["poses"], step=step)
        assert np.array_equal(bits(got[0]), bits(geo[0])) and np.array_equal(got[2], geo[1]), step
        for i, p in enumerate(R["poses"]):
            sums, c4 = f.locate_system(dd.ptr, p, step=step)
            assert tuple(int(v) for v in got[2][i]) == c4 and bits(got[0][i]) == bits(sums[27]), (step, i)
    assert (want[2][:, 1] == 0).any() and want[2][:, 1].max() > 30 and len(np.unique(bits(want[1]))) > 100
    got = f.score_colour_poses(R["bgr"], np.zeros((H, W), f32), R["poses"][:5])
    assert not got[0].any() and not got[1].any() and not got[2].any() and (got[3] == 8.0).all()
    db.free()
    dd.free()
    f.close()
    f = engine(R["cam"])                                                # an empty map
    got = f.score_colour_poses(R["bgr"], R["depth"], R["poses"][:5])
    SC.assert_same_colour_scores(got, SC.np_score_colour_poses(NONE, R["cam"], R["bgr"], R["depth"], R["poses"][:5]), "empty map")
    assert not got[0].any() and not got[1].any() and (got[2][:, 2] == got[2][:, 0]).all() and (got[3] == 8.0).all()
    f.close()


def test_uniform_colour_is_the_geometric_score(tmp_path):
    case = random_case(3)
    vox = np.array(case["blocks"][1], np.uint8).reshape(-1, 512, 8)
    vox[:, :, 4:7] = (40, 130, 220)
    case["blocks"] = (case["blocks"][0], vox.reshape(len(vox), 4096))
    case["file"] = str(tmp_path / "one.drfmap")
    write(case["file"], VS, *case["blocks"])
    bgr = np.ascontiguousarray(np.broadcast_to(np.array((40, 130, 220), np.uint8), (H, W, 3)))
    poses = random_poses(case, 67)
    f = loaded(case)
    for opt in (dict(step=1), dict(step=3, photo_weight=0.7, photo_cap=0.01)):
        got = f.score_colour_poses(bgr, case["depth"], poses, **opt)
        geo = f.score_poses(case["depth"], poses, step=opt["step"])
        assert (bits(got[1]) == 0).all(), opt
        assert np.array_equal(bits(got[0]), bits(geo[0])) and np.array_equal(got[2], geo[1]) and np.array_equal(bits(got[3]), bits(geo[2])), opt
    assert got[2][:, 1].max() > 30
    f.close()


# ------------------------------------------------------------------ 2
def test_a_grid_whose_fold_crosses_its_stride(tmp_path):
    """168x200 at step 1: 33 600 positions, 66 groups -- lanes 0 and 1 of both folds add two partials."""
    case = SC.random_colour_case(20 + 168, 168, 200)
    case["cam"].update(cx=99.5, cy=83.5)
    case["file"] = str(tmp_path / "m.drfmap")
    write(case["file"], VS, *case["blocks"])
    poses = random_poses(case, 9)
    f = loaded(case)
    got = f.score_colour_poses(case["bgr"], case["depth"], poses, step=1, photo_weight=0.01, photo_cap=3.0)
    assert f.search_stats()[1] == 33600
    f.close()
    want = SC.np_score_colour_poses(case["blocks"], case["cam"], case["bgr"], case["depth"], poses, step=1, photo_weight=0.01, photo_cap=3.0)
    SC.assert_same_colour_scores(got, want, "168x200")
    assert want[2][:, 1].max() > 100 and want[1].max() > 0


def test_far_blocks(tmp_path):
    case = SC.random_colour_case(3, shift=(300, -270, 5))
    assert np.abs(case["blocks"][0]).max() > 256
    case["file"] = str(tmp_path / "far.drfmap")
    write(case["file"], VS, *case["blocks"])
    poses = random_poses(case, 13)
    f = loaded(case)
    got = f.score_colour_poses(case["bgr"], case["depth"], poses)
    f.close()
    want = SC.np_score_colour_poses(case["blocks"], case["cam"], case["bgr"], case["depth"], poses)
    SC.assert_same_colour_scores(got, want, "far blocks")
    assert want[2][:, 1].max() > 10 and want[1].max() > 0


# ------------------------------------------------------------------ 3
def test_lattice_and_chunk_seams(R, parity_hooks, monkeypatch):
    """all_scores and the entries of a 2-anchor x 3-rotation x (3 x 5 x 3) lattice, 270 candidates, against the restatement; then
    with DR_SEARCH_CHUNK=64 and 1 (the parity library): the same bits and the same entries."""
    anchors, rot = small_lattice(R)
    kw = dict(half=(1, 2, 1), trans_step=0.08, top_k=5, score_only=True, score=dict(step=3), **R["opt"])
    want = SC.np_search_colour_frame(R["blocks"], None, R["cam"], R["bgr"], R["depth"], anchors, rot, **kw)
    assert want["n_candidates"] == 270 and len(np.unique(bits(want["scores"]))) > 150
    f = loaded(R)
    for chunk, chunks in ((None, 1), ("64", 5), ("1", 270)):
        if chunk:
            monkeypatch.setenv("DR_SEARCH_CHUNK", chunk)
        r = f.search_colour_frame(R["bgr"], R["depth"], anchors, rot, all_scores=True, **kw)
        SC.assert_same_colour_search(colour_search_dict(r), want, "chunk %s" % chunk)
        st = f.search_stats()
        assert st[0] == 270 and st[3] == chunks and st[4] == 0 and st[5] == 0, st
    monkeypatch.delenv("DR_SEARCH_CHUNK")
    f.close()


# ------------------------------------------------------------------ 4
def test_the_wall_end_to_end(WALL):
    """The 147-candidate wall lattice on the oracle-integrated wall loaded from a file, top_k 3: all_scores, every entry with its
    final_score, the winner and the pose equal the CPU run (search_colour_refine on the host over the oracle's ray-cast) bit for
    bit, from host and from device pointers; the winner is within a voxel in the plane and a quarter along the normal."""
    w, want = WALL, WALL["want"]
    f = loaded(w)
    r = f.search_colour_frame(w["bgr"], w["depth"], w["anchor"], w["eye"], all_scores=True, **wall_kw())
    st = f.search_stats()
    SC.assert_same_colour_search(colour_search_dict(r), want, "wall")
    db, dd = DeviceImage(f, w["bgr"], np.uint8), DeviceImage(f, w["depth"], f32)
    SC.assert_same_colour_search(colour_search_dict(f.search_colour_frame(db.ptr, dd.ptr, w["anchor"], w["eye"], all_scores=True, **wall_kw())), want, "wall (device pointers)")
    assert f.search_stats() == st
    ps, ls = f.track_pyramid_stats(), f.locate_stats()
    db.free()
    dd.free()
    f.close()
    t, nrm = SC.wall_errors(r.T32)
    print("wall: %d candidates in %d chunk(s), %d renders and %d evaluations over %d entries; winner entry %d (candidate %d), final score %.4f: %.4f voxels in the plane, %.4f along the normal" %
          (st[0], st[3], st[4], st[5], r.refined, r.winner, r.entries[r.winner].index, r.entries[r.winner].final_score, t, nrm))
    assert st[0] == 147 and st[1] == 768 and st[2] == 768 and st[3] == 1 and st[4] > 0 and st[5] > st[4] and r.refined == 3
    assert st[6] >= colour_scratch_bytes(48, 64, 2, 32)
    assert r.status in (CONVERGED, MAX_ITERS) and r.entries[0].index == SC.WALL_NEAREST and t <= 1.0 and nrm <= 0.25
    assert ps[3] > 0 and ps[6] == 1 and ls[3] > 0                           # the last refinement stages that ran: one level, a localisation


# ------------------------------------------------------------------ 5
def test_the_scene_score_stage(tmp_path):
    """The 10 648-candidate lattice of tests/test_map_search.py on the one-scan scene with the scan's own colour image: all_scores
    and the 8 best entries, score stage alone, against the restatement."""
    s = track_scene()
    s["file"] = str(tmp_path / "scene.drfmap")
    write(s["file"], VS, *s["blocks"])
    anchor = scene_anchor(s)
    rot, half = scene_lattice()
    o = SC.np_score_colour_options(s["cam"], step=SCENE_STEP)
    Rc, tv = np_candidates(s["cam"], anchor[None], rot, half)
    cost, photo, counts, score = SC.np_score_colour_candidates(s["blocks"], s["cam"], s["bgr"], s["depth"], Rc, tv, o, batch=512)
    f = loaded(s)
    r = f.search_colour_frame(s["bgr"], s["depth"], anchor[None], rot, half=half, top_k=8, score_only=True, score=dict(step=SCENE_STEP), all_scores=True)
    st = f.search_stats()
    f.close()
    assert r.n_candidates == 10648 and st[0] == 10648 and st[2] == 752 and st[3] == 1 and r.status == MAX_ITERS and r.winner == 0
    assert np.array_equal(bits(r.scores), bits(score))
    top = np_select(score, 8)
    assert [e.index for e in r.entries] == top.tolist()
    for e, c in zip(r.entries, top):
        assert bits(e.score) == bits(score[c]) and bits(e.cost) == bits(cost[c]) and bits(e.photo) == bits(photo[c]) and e.counts == tuple(int(v) for v in counts[c])
    assert photo.max() > 0 and len(np.unique(bits(photo))) > 1000


# ------------------------------------------------------------------ 6
def test_nothing_changed(WALL):
    """export_blocks, drf_stats, the public render (its device buffers too) and the streaming stats are identical before and after a
    colour score and a colour search; a geometric drf_search_frame before and after a colour call returns the same bits; with
    streaming on and half the map stored, stored blocks read as absent and the stats count them."""
    from tandem_amd.dr_fusion import streaming_min_radius
    w = WALL
    cam, view = w["cam"], np.eye(4, dtype=f32)
    Hc, Wc = cam["height"], cam["width"]

    def render(f):
        f.RenderAsync([view])
        rb, rd = f.GetRenderResult()
        return rb[0].copy(), rd[0].copy()

    def device_render(f):
        pb, pd = f.render_device_pointers()
        b, d = np.empty((Hc, Wc, 3), np.uint8), np.empty((Hc, Wc), f32)
        assert f._L.dr_memcpy_d2h(b.ctypes.data_as(C.c_void_p), C.c_void_p(pb), b.nbytes) == 0
        assert f._L.dr_memcpy_d2h(d.ctypes.data_as(C.c_void_p), C.c_void_p(pd), d.nbytes) == 0
        return (pb, pd), b, d

    geo_kw = dict(half=SC.WALL_HALF, top_k=3, score=dict(step=2), track=dict(centre_depth=1.5, **SC.TC.TRACK_EPS), locate=SC.WALL_LOCATE, all_scores=True,
                  raise_on_failure=False)
    f = loaded(w)
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))
    before = (f.export_blocks(), f.stats(), render(f), f.streaming_stats())
    held = device_render(f)
    geo0 = search_dict(f.search_frame(w["depth"], w["anchor"], w["eye"], **geo_kw))
    poses = np.stack([w["anchor"][0], view])
    whole = f.score_colour_poses(w["bgr"], w["depth"], poses, step=2)
    r = f.search_colour_frame(w["bgr"], w["depth"], w["anchor"], w["eye"], **wall_kw())
    assert r.status in (CONVERGED, MAX_ITERS) and f.search_stats()[7] == 0
    geo1 = search_dict(f.search_frame(w["depth"], w["anchor"], w["eye"], **geo_kw))
    from test_map_search import assert_same_search
    assert_same_search(geo1, geo0, "the geometric search before and after")
    again = device_render(f)
    assert again[0] == held[0] and np.array_equal(again[1], held[1]) and np.array_equal(again[2].view(np.uint32), held[2].view(np.uint32))
    after = (f.export_blocks(), f.stats(), render(f), f.streaming_stats())
    assert before[1] == after[1] and before[3] == after[3] and before[0].keys() == after[0].keys()
    assert all(np.array_equal(before[0][k], after[0][k]) for k in before[0])
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1].view(np.uint32), after[2][1].view(np.uint32))
    f.stream_out_region((-500.0, -500.0, -500.0), (0.0, 500.0, 500.0))     # the half x < 0
    stored = f.streaming_stats()
    part = f.score_colour_poses(w["bgr"], w["depth"], poses, step=2)
    assert f.search_stats()[7] == stored["host"] > 0 and f.streaming_stats() == stored
    left = f.export_blocks()
    rest = (np.array(sorted(left), np.int64).reshape(-1, 3), np.stack([left[k] for k in sorted(left)]))
    assert 0 < len(left) < len(w["blocks"][0])
    SC.assert_same_colour_scores(part, SC.np_score_colour_poses(rest, cam, w["bgr"], w["depth"], poses, step=2), "the resident part")
    assert part[2][1, 2] > whole[2][1, 2]
    f.close()


# ------------------------------------------------------------------ 7
def test_statuses_and_refusals_in_their_order(WALL):
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import AlignError
    w = WALL
    cam, anchors, rot = w["cam"], w["anchor"], w["eye"]
    Hc, Wc = cam["height"], cam["width"]
    kw = wall_kw()
    f = loaded(w)
    nothing = lambda: f.search_stats() == (0,) * 8  # noqa: E731
    # a map 50 blocks away: LOST, the best-scoring candidate handed out, a message
    gone = anchors.copy()
    gone[0, 2, 3] -= 50 * 8 * VS
    with pytest.raises(AlignError) as e:
        f.search_colour_frame(w["bgr"], w["depth"], gone, rot, **dict(kw, top_k=2))
    res = e.value.result
    assert res.status == LOST and res.winner == -1 and res.refined == 2 and "no candidate" in str(e.value) and not nothing()
    assert res.entries[0].index == 0 and all(en.track_status == LOST and en.locate_status == -1 and en.final_score == 0.0 for en in res.entries)
    # accept_valid stops at the first entry that reaches it
    r = f.search_colour_frame(w["bgr"], w["depth"], anchors, rot, accept_valid=0.5, **kw)
    assert r.refined == 1 and r.winner == 0 and r.entries[1].track_status == -1 and r.entries[0].final_score > 0
    # null arguments (the option structs, res and all_scores may be null); bgr is among them
    L = f._L
    bgr_a, depth_a, anc = np.ascontiguousarray(w["bgr"], np.uint8), np.ascontiguousarray(w["depth"], f32), np.ascontiguousarray(anchors, f32).reshape(-1, 16)
    bp, dp, ap, rp = C.c_void_p(bgr_a.ctypes.data), depth_a.ctypes.data_as(_lib.f32p), anc.ctypes.data_as(_lib.f32p), rot.ctypes.data_as(_lib.f64p)
    dvp = C.c_void_p(depth_a.ctypes.data)
    out_a, cost_a = np.zeros(16, f32), np.zeros(1)
    out, cost = out_a.ctypes.data_as(_lib.f32p), cost_a.ctypes.data_as(_lib.f64p)
    for b_, d_, a_, r_, o_ in ((None, 1, ap, rp, out), (bp, None, ap, rp, out), (bp, 1, None, rp, out), (bp, 1, ap, None, out), (bp, 1, ap, rp, None)):
        assert L.drf_search_colour_frame(f._h, b_, dp if d_ else None, a_, 1, r_, 1, None, None, None, o_, None, None) == 1 and nothing()
        assert L.drf_search_colour_frame_device(f._h, b_, dvp if d_ else None, a_, 1, r_, 1, None, None, None, o_, None, None) == 1 and nothing()
    for b_, d_, a_, c_ in ((None, 1, ap, cost), (bp, None, ap, cost), (bp, 1, None, cost), (bp, 1, ap, None)):
        assert L.drf_score_colour_poses(f._h, b_, dp if d_ else None, a_, 1, None, c_, None, None, None) == 1 and nothing()
        assert L.drf_score_colour_poses_device(f._h, b_, dvp if d_ else None, a_, 1, None, c_, None, None, None) == 1 and nothing()
    one = _lib.SearchColourOptions(_lib.SearchOptions(score_only=1), 0.0, 0.0)
    assert L.drf_search_colour_frame(f._h, bp, dp, ap, 1, rp, 1, C.byref(one), None, None, out, None, None) == 0 and not nothing()   # res and all_scores null
    assert L.drf_score_colour_poses(f._h, bp, dp, ap, 1, None, None, cost, None, None) == 0 and f.search_stats()[0] == 1                # photo alone
    # a bad option is named: the score's, the search's, the colour fields, the tracking's, the localisation's -- in that order
    for bad, which in ((dict(score=dict(step=-1)), "step"), (dict(top_k=33, photo_weight=-1.0), "top_k"), (dict(photo_weight=-1.0, photo_cap=-1.0), "photo_weight"),
                       (dict(photo_cap=float("nan"), levels=9), "photo_cap"), (dict(levels=9, locate=dict(min_valid=-1.0)), "levels"),
                       (dict(track=dict(max_jump=-1.0)), "max_jump"), (dict(track_photo_weight=-1.0), "photo_weight"), (dict(locate=dict(min_valid=-1.0)), "min_valid")):
        with pytest.raises(_lib.DrError) as e:
            f.search_colour_frame(w["bgr"], w["depth"], anchors, rot, **bad)
        assert e.value.code == 1 and which in str(e.value) and nothing(), bad
    for bad, which in ((dict(huber=-1.0, photo_cap=-1.0), "huber"), (dict(photo_cap=-1.0), "photo_cap"), (dict(photo_weight=float("inf")), "photo_weight")):
        with pytest.raises(_lib.DrError) as e:
            f.score_colour_poses(w["bgr"], w["depth"], anchors, **bad)
        assert e.value.code == 1 and which in str(e.value) and nothing()
    # no candidate, or more than 2^24
    assert code_of(f.search_colour_frame, w["bgr"], w["depth"], anchors[:0], rot) == 1 and code_of(f.search_colour_frame, w["bgr"], w["depth"], anchors, rot[:0]) == 1
    assert code_of(f.search_colour_frame, w["bgr"], w["depth"], anchors, rot, half=(200, 200, 200)) == 1 and nothing()
    assert L.drf_score_colour_poses(f._h, bp, dp, ap, 0, None, cost, None, None, None) == 1 and nothing()
    # what is no rigid motion
    scaled = anchors.copy()
    scaled[0, :3, :3] *= 1.01
    with pytest.raises(_lib.DrError) as e:
        f.search_colour_frame(w["bgr"], w["depth"], scaled, rot, **kw)
    assert e.value.code == 1 and "anchor 0" in str(e.value) and nothing()
    with pytest.raises(_lib.DrError) as e:
        f.score_colour_poses(w["bgr"], w["depth"], np.concatenate([anchors, scaled]))
    assert e.value.code == 1 and "pose 1" in str(e.value) and nothing()
    # where a scan may not be integrated: after the options, before the poses
    f.IntegrateScanAsync(np.zeros((Hc, Wc, 3), np.uint8), np.zeros((Hc, Wc), f32), np.eye(4, dtype=f32))
    assert code_of(f.search_colour_frame, w["bgr"], w["depth"], anchors, rot, **kw) == 2 and code_of(f.search_colour_frame, w["bgr"], w["depth"], scaled, rot, **kw) == 2
    assert code_of(f.score_colour_poses, w["bgr"], w["depth"], anchors) == 2 and code_of(f.search_colour_frame, w["bgr"], w["depth"], anchors, rot, photo_cap=-1.0) == 1
    assert nothing()
    f.RenderAsync([np.eye(4, dtype=f32)])
    assert code_of(f.search_colour_frame, w["bgr"], w["depth"], anchors, rot, **kw) == 2
    f.GetRenderResult()
    assert f.search_colour_frame(w["bgr"], w["depth"], anchors, rot, score_only=True).status == MAX_ITERS
    f.close()


def test_shim(WALL, tmp_path):
    """tandem_amd/libdr/dr_fusion.h ScoreColourPoses and SearchColourFrame, held to the library's own answers."""
    w = WALL
    f = loaded(w)
    ws = f.score_colour_poses(w["bgr"], w["depth"], w["anchor"])
    want = f.search_colour_frame(w["bgr"], w["depth"], w["anchor"], w["eye"], raise_on_failure=False, **wall_kw())
    f.close()
    exe, frame = str(tmp_path / "map_search_colour_shim"), str(tmp_path / "frame.bin")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_search_colour_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    with open(frame, "wb") as fh:
        fh.write(np.ascontiguousarray(w["anchor"][0], f32).tobytes() + np.ascontiguousarray(w["bgr"], np.uint8).tobytes() + np.ascontiguousarray(w["depth"], f32).tobytes())
    cam = w["cam"]
    r = subprocess.run([exe, repr(VS)] + [repr(float(f32(cam[k]))) for k in ("fx", "fy", "cx", "cy")] + [str(cam["num_blocks"]), str(cam["height"]), str(cam["width"]),
                       w["file"], frame], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["status"] == want.status and js["winner"] == want.winner and js["index"] == want.entries[max(want.winner, 0)].index
    assert js["anchor_score"] == ws[3][0] and js["anchor_photo"] == ws[1][0] and js["final_score"] == want.entries[max(want.winner, 0)].final_score
    assert np.array_equal(f32(js["pose"]).reshape(4, 4), want.T32)
