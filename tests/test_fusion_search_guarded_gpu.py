"""-m gpu: drf_score_poses and drf_search_frame under the guarded allocator of the parity library (tests/guard_helpers.py): the score
stage's device scratch -- the points, the flags, the pose table, 32 bytes per candidate of a chunk, the depth image -- and the
scratch of the refinement stages lie between guard bands and start as poison, quiet NaNs.  No guard may change, the results are
bit-identical to the unguarded call and to the restatement of tests/test_map_search.py, and no poison word appears in them: a
candidate whose 32 bytes no wave wrote, or a point that k_search_points left out, would reach the scores as a NaN."""
import numpy as np
import pytest

from guard_helpers import POISON_WORD, assert_same_bits, guarded
from test_fusion_map_file_gpu import engine
from test_fusion_map_search_gpu import search_dict
from test_fusion_map_transform_gpu import write
from test_map_search import VS, assert_same_scores, assert_same_search, build_check, cpp_search, end_to_end_case, np_score_poses, random_poses
from test_map_locate import random_case
from test_map_track import track_scene

pytestmark = pytest.mark.gpu


def test_search_under_guards(tmp_path, parity_hooks, monkeypatch):
    """The random map at 96x128: 67 poses at step 1 (24 groups, three of them without a sample) and at step 3 (a last group with
    tail lanes) in chunks of 16 -- four full chunks and a tail of 3, whose launch has a workgroup with one live wave -- and the
    end-to-end search of 108 candidates on the scene map, whose tracking renders into its own scratch."""
    case = random_case(3)
    path = str(tmp_path / "m.drfmap")
    write(path, VS, *case["blocks"])
    poses = random_poses(case, 67)
    want = [np_score_poses(case["blocks"], case["cam"], case["depth"], poses, step=step) for step in (1, 3)]
    s = track_scene()
    spath = str(tmp_path / "scene.drfmap")
    write(spath, VS, *s["blocks"])
    anchors, rot, kw = end_to_end_case(s)
    want_search = cpp_search(build_check(tmp_path), s["blocks"], s["render"], s["cam"], s["depth"], anchors, rot, **kw)
    assert want[0][1][:, 1].max() > 0 and want_search["refined"] == 3
    monkeypatch.setenv("DR_SEARCH_CHUNK", "16")

    def run():
        f = engine(case["cam"])
        f.load_map(path)
        a = f.score_poses(case["depth"], poses, step=1)
        b = f.score_poses(case["depth"], poses, step=3)
        assert f.search_stats()[3] == 5
        f.close()
        assert_same_scores(a, want[0], "step 1")
        assert_same_scores(b, want[1], "step 3")
        f = engine(s["cam"])
        f.load_map(spath)
        r = f.search_frame(s["depth"], anchors, rot, all_scores=True, **kw)
        f.close()
        assert_same_search(search_dict(r), want_search, "search")
        return [("cost", a[0]), ("score", a[2]), ("cost, step 3", b[0]), ("score, step 3", b[2]), ("all scores", r.scores), ("pose32", r.T32),
                ("entries", np.stack([e.T for e in r.entries]))]

    with guarded():
        on = run()
    off = run()
    for (na, xa), (nb, xb) in zip(on, off):
        assert na == nb
        assert_same_bits(xa, xb, na)
        words = np.ascontiguousarray(xa).view(np.uint32)
        assert not (words == POISON_WORD).any(), na
