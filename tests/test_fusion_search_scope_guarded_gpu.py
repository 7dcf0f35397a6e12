"""-m gpu: the search scope under the guarded allocator of the parity library (tests/guard_helpers.py): the staging's two slots, its
tables and flags and the score stage's scratch lie between guard bands and start as poison, quiet NaNs.  The whole random map in
the host store scored at 259 poses at pixel step 3, and the lattice of tests/test_search_scope.py at the capacity of its CPU plan
(at least 3 passes, an ix split) in chunks of 16.  No guard may change, the results are bit-identical to the unguarded run and to
the restatement of tests/test_map_search.py, and no poison word appears in them: a staged block the copy left out, or a candidate
whose record no wave wrote, would reach the scores as a NaN."""
import numpy as np
import pytest

import test_search_scope as PL
from guard_helpers import POISON_WORD, assert_same_bits, guarded
from test_fusion_locate_scope_gpu import with_file
from test_fusion_map_search_gpu import N_POSES, search_dict
from test_fusion_search_scope_gpu import lattice_case, map_engine
from test_map_locate import random_case
from test_map_search import assert_same_scores, assert_same_search, np_score_poses, random_poses

pytestmark = pytest.mark.gpu


def test_search_scope_under_guards(tmp_path, parity_hooks, monkeypatch):
    rnd = with_file(random_case(3), tmp_path / "rnd.drfmap")
    poses = random_poses(rnd, N_POSES)
    want_rnd = np_score_poses(rnd["blocks"], rnd["cam"], rnd["depth"], poses, step=3)
    case, lat, kw, want = lattice_case(tmp_path, PL.build_check(tmp_path))
    passes = lat["passes"]
    assert want_rnd[1][:, 1].max() > 30 and len(passes) >= 3 and max(lat["whole"]) > lat["capacity"]
    monkeypatch.setenv("DR_SEARCH_CHUNK", "16")

    def run():
        f = map_engine(rnd)
        a = f.score_poses(rnd["depth"], poses, step=3)
        sg = f.search_stage_stats()
        f.close()
        assert_same_scores(a, want_rnd, "all stored, step 3")
        assert sg[0] >= 1 and sg[3] >= -(-N_POSES // 16), sg
        f = map_engine(case, capacity=lat["capacity"], max_sensor_depth=PL.SCOPE_DEPTH)
        r = f.search_frame(case["depth"], lat["anchors"], lat["rot"], all_scores=True, **kw)
        sg = f.search_stage_stats()
        f.close()
        assert_same_search(search_dict(r), want, "the lattice in passes")
        assert sg[0] == len(passes) and sg[3] == sum(-(-c // 16) for _, c, _ in passes), sg
        return [("cost", a[0]), ("score", a[2]), ("all scores", r.scores), ("pose32", r.T32), ("entries", np.stack([e.T for e in r.entries]))]

    with guarded():
        on = run()
    off = run()
    for (na, xa), (nb, xb) in zip(on, off):
        assert na == nb
        assert_same_bits(xa, xb, na)
        words = np.ascontiguousarray(xa).view(np.uint32)
        assert not (words == POISON_WORD).any(), na
