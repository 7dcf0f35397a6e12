"""-m gpu: drf_score_colour_poses and drf_search_colour_frame under the guarded allocator of the parity library
(tests/guard_helpers.py): the colour score's device scratch -- the points, yf, the flags, the pose table, 40 bytes per candidate of
a chunk, the depth and colour images -- and the scratch of the refinement stages lie between guard bands and start as poison,
quiet NaNs.  No guard may change, the results are bit-identical to the unguarded call and to the references of
tests/test_map_search_colour.py, and no poison word appears in them: a candidate whose 40 bytes no wave wrote, or a yf that
k_search_points_colour left out, would reach the scores as a NaN."""
import numpy as np
import pytest

import test_map_search_colour as SC
from guard_helpers import POISON_WORD, assert_same_bits, guarded
from test_fusion_map_file_gpu import engine
from test_fusion_search_colour_gpu import colour_search_dict, wall_kw
from test_fusion_map_transform_gpu import write
from test_map_search import VS, random_poses

pytestmark = pytest.mark.gpu


def test_colour_search_under_guards(tmp_path, parity_hooks, monkeypatch):
    """The random map with random colours at 96x128: 67 poses at step 1 and at step 3 (a last group with tail lanes) in chunks of
    16 -- four full chunks and a tail of 3, whose launch has a workgroup with one live wave -- and the end-to-end search of 147
    candidates on the oracle-integrated wall, whose tracking renders into its own scratch and whose final re-score is a plain
    table of 3 poses."""
    case = SC.random_colour_case(3)
    path = str(tmp_path / "m.drfmap")
    write(path, VS, *case["blocks"])
    poses = random_poses(case, 67)
    opt = dict(photo_weight=0.01, photo_cap=3.0)
    want = [SC.np_score_colour_poses(case["blocks"], case["cam"], case["bgr"], case["depth"], poses, step=step, **opt) for step in (1, 3)]
    w = SC.integrated_wall()
    wpath = str(tmp_path / "wall.drfmap")
    write(wpath, VS, *w["blocks"])
    anchor, eye = SC.wall_anchor()[None], np.eye(3).reshape(1, 9)
    want_search = SC.cpp_search(SC.build_check(tmp_path), w["blocks"], w["render"], w["cam"], w["bgr"], w["depth"], anchor, eye, **SC.WALL_END_TO_END)
    assert want[0][2][:, 1].max() > 0 and want_search["refined"] == 3 and want_search["winner"] >= 0
    monkeypatch.setenv("DR_SEARCH_CHUNK", "16")

    def run():
        f = engine(case["cam"])
        f.load_map(path)
        a = f.score_colour_poses(case["bgr"], case["depth"], poses, step=1, **opt)
        b = f.score_colour_poses(case["bgr"], case["depth"], poses, step=3, **opt)
        assert f.search_stats()[3] == 5
        f.close()
        SC.assert_same_colour_scores(a, want[0], "step 1")
        SC.assert_same_colour_scores(b, want[1], "step 3")
        f = engine(w["cam"])
        f.load_map(wpath)
        r = f.search_colour_frame(w["bgr"], w["depth"], anchor, eye, all_scores=True, **wall_kw())
        assert f.search_stats()[3] == 10                                   # 147 candidates in chunks of 16; the re-score is not counted
        f.close()
        SC.assert_same_colour_search(colour_search_dict(r), want_search, "search")
        return [("cost", a[0]), ("photo", a[1]), ("score", a[3]), ("cost, step 3", b[0]), ("photo, step 3", b[1]), ("score, step 3", b[3]), ("all scores", r.scores),
                ("pose32", r.T32), ("entries", np.stack([e.T for e in r.entries])), ("final", np.array([[e.final_score, e.final_photo, e.photo] for e in r.entries]))]

    with guarded():
        on = run()
    off = run()
    for (na, xa), (nb, xb) in zip(on, off):
        assert na == nb
        assert_same_bits(xa, xb, na)
        words = np.ascontiguousarray(xa).view(np.uint32)
        assert not (words == POISON_WORD).any(), na
