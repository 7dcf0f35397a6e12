"""-m gpu: drf_score_poses / drf_search_frame.  The reference of every bit comparison is np_score_poses / np_search_frame, the numpy
restatement of the rule in tests/test_map_search.py, for whole searches search_refine through tests/cpp/map_search_check.cpp over
the CPU oracle's ray-cast (which tests/test_map_search.py holds to the restatement), and for the score drf_locate_system itself:
cost and counts are its sums[27] and counts pose by pose.  96x128 engines, one of 168x200; the random map of about 260 blocks and
the one-scan scene of 1 968.  DESIGN.md §7c "Searching a pose lattice"."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import ROOT
from test_fusion_map_file_gpu import engine
from test_fusion_map_locate_gpu import DeviceDepth
from test_fusion_map_transform_gpu import write
from test_map_align import CONVERGED, LOST, MAX_ITERS, bits
from test_map_locate import NONE, SCENE_MEASURED, random_case, scene_errors
from test_map_search import (H, SCENE_STEP, VS, W, assert_same_scores, assert_same_search, build_check, candidate_pose16, cpp_search, end_to_end_case, np_candidates,
                             np_score_options, np_score_poses, np_search_frame, random_poses, scene_anchor, scene_lattice, small_lattice)
from test_map_track import track_opts, track_scene

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
N_POSES = 259   # no multiple of 4 (the workgroup's waves) or 64; every seventh pose looks away, every eleventh sits 300 blocks off


def scratch_bytes(height, width, step, table_entries, chunk=65536):
    """drf_search_stats()[6]: 24 bytes of point per padded grid position, the pose table, 32 bytes per candidate of a chunk, a
    host-given depth image, a flag byte per position"""
    padded = 512 * -(-(-(-width // step) * -(-height // step)) // 512)
    return 24 * padded + 96 * max(table_entries, 1) + 32 * chunk + 4 * height * width + padded


def code_of(call, *args, **kw):
    from tandem_amd import _lib
    with pytest.raises(_lib.DrError) as e:
        call(*args, **kw)
    return e.value.code


def loaded(case, **kw):
    f = engine(case["cam"], **kw)
    f.load_map(case["file"])
    return f


def search_dict(r):
    """a SearchResult of tandem_amd.dr_fusion as a dict shaped like np_search_frame's"""
    return dict(status=r.status, winner=r.winner, refined=r.refined, n_candidates=r.n_candidates, T32=r.T32, scores=r.scores, entries=[e._asdict() for e in r.entries])


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    """The random map, its file, 259 poses and their restated scores at steps 1, 3 and 4"""
    d = tmp_path_factory.mktemp("search_rnd")
    case = random_case(3)
    case["file"] = str(d / "rnd.drfmap")
    write(case["file"], VS, *case["blocks"])
    case["poses"] = random_poses(case, N_POSES)
    case["want"] = {step: np_score_poses(case["blocks"], case["cam"], case["depth"], case["poses"], step=step) for step in (1, 3, 4)}
    return case


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    """The scene, its map file, the check library"""
    d = tmp_path_factory.mktemp("search_scene")
    s = track_scene()
    s["file"] = str(d / "scene.drfmap")
    write(s["file"], VS, *s["blocks"])
    s["HS"], s["dir"] = build_check(d), d
    return s


# ------------------------------------------------------------------ 1
def test_score_against_the_restatement_and_drf_locate_system(R):
    """259 poses at steps 1 (24 groups), 3 (1 376 positions, the last group 352 wide) and 4: cost, counts and score are the
    restatement's; host and device pointers give the same bits; pose by pose cost and counts are drf_locate_system's sums[27] and
    counts; the statistics; an image without a sample; an empty map."""
    f = loaded(R)
    dd = DeviceDepth(f, R["depth"])
    for step in (1, 3, 4):
        want = R["want"][step]
        got = f.score_poses(R["depth"], R["poses"], step=step)
        assert_same_scores(got, want, "step %d" % step)
        st = f.search_stats()
        assert st == (N_POSES, -(-W // step) * -(-H // step), int(want[1][0, 0]), 1, 0, 0, st[6], 0), st
        assert st[6] >= scratch_bytes(H, W, step, N_POSES)
        assert_same_scores(f.score_poses(dd.ptr, R["poses"], step=step), want, "step %d (device pointer)" % step)
        for i, p in enumerate(R["poses"]):
            sums, c4 = f.locate_system(dd.ptr, p, step=step)
            assert tuple(int(v) for v in got[1][i]) == c4 and bits(got[0][i]) == bits(sums[27]), (step, i)
    assert (want[1][:, 1] == 0).any() and want[1][:, 1].max() > 30 and len(np.unique(bits(want[2]))) > 100
    o = np_score_options(R["cam"])
    got = f.score_poses(np.zeros((H, W), f32), R["poses"][:5])
    assert not got[0].any() and not got[1].any() and (got[2] == o["uc"]).all()
    dd.free()
    f.close()
    f = engine(R["cam"])                                                # an empty map
    got = f.score_poses(R["depth"], R["poses"][:5])
    assert_same_scores(got, np_score_poses(NONE, R["cam"], R["depth"], R["poses"][:5]), "empty map")
    assert not got[0].any() and (got[1][:, 2] == got[1][:, 0]).all() and (got[1][:, 0] > 100).all() and (got[2] == o["uc"]).all()
    f.close()


def test_a_grid_whose_fold_crosses_its_stride(tmp_path):
    """168x200 at step 1: 33 600 positions, 66 groups, the last 320 wide -- lanes 0 and 1 of the fold add two partials."""
    case = random_case(20 + 168, 168, 200)
    case["cam"].update(cx=99.5, cy=83.5)
    case["file"] = str(tmp_path / "m.drfmap")
    write(case["file"], VS, *case["blocks"])
    poses = random_poses(case, 9)
    f = loaded(case)
    got = f.score_poses(case["depth"], poses, step=1)
    assert f.search_stats()[1] == 33600
    sums, c4 = f.locate_system(case["depth"], poses[0])
    f.close()
    want = np_score_poses(case["blocks"], case["cam"], case["depth"], poses, step=1)
    assert_same_scores(got, want, "168x200")
    assert want[1][:, 1].max() > 100 and bits(got[0][0]) == bits(sums[27]) and tuple(int(v) for v in got[1][0]) == c4


def test_far_blocks(tmp_path):
    """Map and camera moved by whole blocks beyond block coordinate 256: the table path of find_block."""
    case = random_case(3, shift=(300, -270, 5))
    assert np.abs(case["blocks"][0]).max() > 256
    case["file"] = str(tmp_path / "far.drfmap")
    write(case["file"], VS, *case["blocks"])
    poses = random_poses(case, 13)
    f = loaded(case)
    got = f.score_poses(case["depth"], poses)
    f.close()
    want = np_score_poses(case["blocks"], case["cam"], case["depth"], poses)
    assert_same_scores(got, want, "far blocks")
    assert want[1][:, 1].max() > 10


# ------------------------------------------------------------------ 2
def test_lattice_and_chunk_seams(R, parity_hooks, monkeypatch):
    """all_scores and the entries of a 2-anchor x 3-rotation x (3 x 5 x 3) lattice, 270 candidates, against the restatement; then
    with DR_SEARCH_CHUNK=64 (the parity library): four full chunks and a tail of 14, the same bits and the same entries."""
    anchors, rot = small_lattice(R)
    kw = dict(half=(1, 2, 1), trans_step=0.08, top_k=5, score_only=True, score=dict(step=3))
    want = np_search_frame(R["blocks"], None, R["cam"], R["depth"], anchors, rot, **kw)
    assert want["n_candidates"] == 270 and len(np.unique(bits(want["scores"]))) > 150
    f = loaded(R)
    for chunk, chunks in ((None, 1), ("64", 5), ("1", 270)):
        if chunk:
            monkeypatch.setenv("DR_SEARCH_CHUNK", chunk)
        r = f.search_frame(R["depth"], anchors, rot, all_scores=True, **kw)
        assert_same_search(search_dict(r), want, "chunk %s" % chunk)
        st = f.search_stats()
        assert st[0] == 270 and st[3] == chunks and st[4] == 0 and st[5] == 0, st
    monkeypatch.delenv("DR_SEARCH_CHUNK")
    f.close()


# ------------------------------------------------------------------ 3
def test_the_scene_end_to_end(S):
    """The 10 648-candidate lattice of tests/test_map_search.py around the anchor 51.9 voxels and 14.3 degrees off, top_k 8, on the
    map loaded from a file: all_scores, every entry and the result equal the CPU run (search_refine on the host over the oracle's
    ray-cast) bit for bit, and the pose is within 2 x SCENE_MEASURED of the scan's."""
    anchor = scene_anchor(S)
    rot, half = scene_lattice()
    kw = dict(half=half, top_k=8, score=dict(step=SCENE_STEP), track=track_opts(S), locate=dict(centre_depth=S["centre_depth"]))
    want = cpp_search(S["HS"], S["blocks"], S["render"], S["cam"], S["depth"], anchor[None], rot, **kw)
    f = loaded(S)
    r = f.search_frame(S["depth"], anchor[None], rot, all_scores=True, **kw)
    st = f.search_stats()
    assert_same_search(search_dict(r), want, "scene")
    dd = DeviceDepth(f, S["depth"])
    assert_same_search(search_dict(f.search_frame(dd.ptr, anchor[None], rot, all_scores=True, **kw)), want, "scene (device pointer)")
    dd.free()
    f.close()
    a, t = scene_errors(r.T32.astype(f64), S["pose"])
    print("scene: %d candidates in %d chunk(s), %d renders and %d evaluations over %d entries; winner entry %d (candidate %d): %.5f degrees %.5f voxels off" %
          (st[0], st[3], st[4], st[5], r.refined, r.winner, r.entries[r.winner].index, a, t))
    for k, e in enumerate(r.entries):
        print("  entry %d: candidate %d score %.4f track %d locate %d, %d of %d valid, %.4f deg %.4f voxels" %
              ((k, e.index, e.score, e.track_status, e.locate_status, e.valid, e.samples) + scene_errors(e.T, S["pose"])))
    assert st[0] == 10648 and st[1] == 768 and st[2] == 752 and st[3] == 1 and st[4] > 0 and st[5] > st[4] and r.n_candidates == 10648 and r.refined == 8
    assert r.status == CONVERGED and a <= 2 * SCENE_MEASURED[0] and t <= 2 * SCENE_MEASURED[1]


# ------------------------------------------------------------------ 4
def test_the_map_is_untouched(S):
    """export_blocks, drf_stats, the public render (its device buffers too) and the streaming stats are identical before and after a
    score and a search; with streaming on and half the map stored, stored blocks read as absent and the stats count them."""
    from tandem_amd.dr_fusion import streaming_min_radius
    anchors, rot, kw = end_to_end_case(S)
    view = S["pose"]

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

    f = loaded(S)
    f.set_streaming(max(streaming_min_radius(f.options), 8.0))
    before = (f.export_blocks(), f.stats(), render(f), f.streaming_stats())
    held = device_render(f)
    poses = np.stack([anchors[0], np.asarray(S["pose"], f32)])           # the scan's own pose sees both halves
    whole = f.score_poses(S["depth"], poses)
    r = f.search_frame(S["depth"], anchors, rot, **kw)
    assert r.status == CONVERGED and f.search_stats()[7] == 0
    again = device_render(f)
    assert again[0] == held[0] and np.array_equal(again[1], held[1]) and np.array_equal(again[2].view(np.uint32), held[2].view(np.uint32))
    after = (f.export_blocks(), f.stats(), render(f), f.streaming_stats())
    assert before[1] == after[1] and before[3] == after[3] and before[0].keys() == after[0].keys()
    assert all(np.array_equal(before[0][k], after[0][k]) for k in before[0])
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1].view(np.uint32), after[2][1].view(np.uint32))
    cut = float(np.median(S["blocks"][0][:, 0])) * 8 * VS
    f.stream_out_region((-500.0, -500.0, -500.0), (cut, 500.0, 500.0))
    stored = f.streaming_stats()
    part = f.score_poses(S["depth"], poses)
    assert f.search_stats()[7] == stored["host"] > 0 and f.streaming_stats() == stored
    left = f.export_blocks()                                            # the resident part, as the restatement sees it
    rest = (np.array(sorted(left), np.int64).reshape(-1, 3), np.stack([left[k] for k in sorted(left)]))
    assert 0 < len(left) < len(S["blocks"][0])
    assert_same_scores(part, np_score_poses(rest, S["cam"], S["depth"], poses), "the resident part")
    assert part[1][1, 2] > whole[1][1, 2]
    f.close()


# ------------------------------------------------------------------ 5
def test_statuses_and_refusals_in_their_order(S):
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import AlignError, pose_rotations
    anchors, rot, kw = end_to_end_case(S)
    f = loaded(S)
    nothing = lambda: f.search_stats() == (0,) * 8  # noqa: E731
    # a map 50 blocks away: LOST, the best-scoring candidate handed out, a message
    gone = anchors.copy()
    gone[0, 0, 3] += 50 * 8 * VS
    with pytest.raises(AlignError) as e:
        f.search_frame(S["depth"], gone, rot, **dict(kw, top_k=2))
    res = e.value.result
    R_, tv = np_candidates(S["cam"], gone, rot, kw["half"])
    assert res.status == LOST and res.winner == -1 and res.refined == 2 and "no candidate" in str(e.value) and not nothing()
    assert res.entries[0].index == 0 and np.array_equal(res.T32, candidate_pose16(S["cam"], R_[0], tv[0]))
    assert all(en.track_status == LOST and en.locate_status == -1 for en in res.entries)
    # accept_valid stops at the first entry that reaches it
    r = f.search_frame(S["depth"], anchors, rot, accept_valid=0.5, **kw)
    assert r.status == CONVERGED and r.refined == 1 and r.winner == 0 and r.entries[1].track_status == -1
    # null arguments (the option structs, res and all_scores may be null)
    L = f._L
    depth_a, anc = np.ascontiguousarray(S["depth"], f32), np.ascontiguousarray(anchors, f32).reshape(-1, 16)
    dp, ap, rp = depth_a.ctypes.data_as(_lib.f32p), anc.ctypes.data_as(_lib.f32p), rot.ctypes.data_as(_lib.f64p)
    out_a, cost_a = np.zeros(16, f32), np.zeros(1)
    out, cost = out_a.ctypes.data_as(_lib.f32p), cost_a.ctypes.data_as(_lib.f64p)
    for args in ((None, ap, 1, rp, 4, None, None, None, out, None, None), (dp, None, 1, rp, 4, None, None, None, out, None, None),
                 (dp, ap, 1, None, 4, None, None, None, out, None, None), (dp, ap, 1, rp, 4, None, None, None, None, None, None)):
        assert L.drf_search_frame(f._h, *args) == 1 and nothing()
        assert L.drf_search_frame_device(f._h, *args) == 1 and nothing()
    for args in ((None, ap, 1, None, cost, None, None), (dp, None, 1, None, cost, None, None), (dp, ap, 1, None, None, None, None)):
        assert L.drf_score_poses(f._h, *args) == 1 and nothing()
        assert L.drf_score_poses_device(f._h, *args) == 1 and nothing()
    assert L.drf_search_stats(f._h, None) == 1
    one = _lib.SearchOptions(score_only=1)
    assert L.drf_search_frame(f._h, dp, ap, 1, rp, 4, C.byref(one), None, None, out, None, None) == 0 and not nothing()   # res and all_scores null
    assert L.drf_score_poses(f._h, dp, ap, 1, None, cost, None, None) == 0 and f.search_stats()[0] == 1
    # a bad option is named: the score's, the search's, the tracking's, the localisation's
    for bad, which in ((dict(score=dict(step=-1)), "step"), (dict(score=dict(unobserved_cost=float("nan"))), "unobserved_cost"), (dict(trans_step=-1.0), "trans_step"),
                       (dict(half=(0, -1, 0)), "half"), (dict(top_k=33), "top_k"), (dict(accept_valid=float("inf")), "accept_valid"),
                       (dict(track=dict(max_jump=-1.0)), "max_jump"), (dict(locate=dict(min_valid=-1.0)), "min_valid")):
        with pytest.raises(_lib.DrError) as e:
            f.search_frame(S["depth"], anchors, rot, **bad)
        assert e.value.code == 1 and which in str(e.value) and nothing(), bad
    with pytest.raises(_lib.DrError) as e:
        f.score_poses(S["depth"], anchors, huber=-1.0)
    assert e.value.code == 1 and "huber" in str(e.value) and nothing()
    # no candidate, or more than 2^24
    assert code_of(f.search_frame, S["depth"], anchors[:0], rot) == 1 and code_of(f.search_frame, S["depth"], anchors, rot[:0]) == 1 and nothing()
    assert code_of(f.search_frame, S["depth"], anchors, rot, half=(200, 200, 200)) == 1 and nothing()
    assert L.drf_score_poses(f._h, dp, ap, 0, None, cost, None, None) == 1 and L.drf_score_poses(f._h, dp, ap, (1 << 24) + 1, None, cost, None, None) == 1 and nothing()
    # what is no rigid motion: an anchor, a rotation, a pose
    scaled, nan = anchors.copy(), anchors.copy()
    scaled[0, :3, :3] *= 1.01
    nan[0, 2, 3] = np.nan
    mirror = rot.copy()
    mirror[2] = np.diag([1.0, -1.0, 1.0]).reshape(9)
    for a_, r_, text in ((scaled, rot, "anchor 0"), (nan, rot, "anchor 0"), (anchors, mirror, "rotation 2")):
        with pytest.raises(_lib.DrError) as e:
            f.search_frame(S["depth"], a_, r_, **kw)
        assert e.value.code == 1 and text in str(e.value) and nothing()
    two = np.concatenate([anchors, scaled])
    with pytest.raises(_lib.DrError) as e:
        f.score_poses(S["depth"], two)
    assert e.value.code == 1 and "pose 1" in str(e.value) and nothing()
    # where a scan may not be integrated: after the options, before the poses
    f.IntegrateScanAsync(np.zeros((H, W, 3), np.uint8), np.zeros((H, W), f32), np.eye(4, dtype=f32))
    assert code_of(f.search_frame, S["depth"], anchors, rot, **kw) == 2 and code_of(f.search_frame, S["depth"], scaled, rot, **kw) == 2 and nothing()
    assert code_of(f.score_poses, S["depth"], anchors) == 2 and code_of(f.search_frame, S["depth"], anchors, rot, top_k=33) == 1
    f.RenderAsync([np.eye(4, dtype=f32)])
    assert code_of(f.search_frame, S["depth"], anchors, rot, **kw) == 2   # between RenderAsync and GetRenderResult
    f.GetRenderResult()
    assert f.search_frame(S["depth"], anchors, pose_rotations(), score_only=True).status == MAX_ITERS
    f.close()


# ------------------------------------------------------------------ 6
def test_shim(S, tmp_path):
    """tandem_amd/libdr/dr_fusion.h ScorePoses and SearchDepthFrame, held to the library's own answers."""
    anchors, rot, kw = end_to_end_case(S)
    f = loaded(S)
    want_score = f.score_poses(S["depth"], anchors)[2][0]
    want = f.search_frame(S["depth"], anchors, rot, half=(1, 1, 1), top_k=2, raise_on_failure=False)   # the shim passes no track or locate options
    f.close()
    exe, frame = str(tmp_path / "map_search_shim"), str(tmp_path / "frame.bin")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_search_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    with open(frame, "wb") as fh:
        fh.write(np.ascontiguousarray(anchors[0], f32).tobytes() + np.ascontiguousarray(S["depth"], f32).tobytes() + np.uint64(len(rot)).tobytes() + rot.tobytes())
    cam = S["cam"]
    r = subprocess.run([exe, repr(VS)] + [repr(float(f32(cam[k]))) for k in ("fx", "fy", "cx", "cy")] + [str(cam["num_blocks"]), S["file"], frame],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["status"] == want.status and js["winner"] == want.winner and js["index"] == want.entries[max(want.winner, 0)].index
    assert js["anchor_score"] == want_score and np.array_equal(f32(js["pose"]).reshape(4, 4), want.T32)
