"""-m gpu: drf_track_colour_system and drf_track_colour_frame under the guarded allocator of the parity library
(tests/guard_helpers.py): the calls' device scratch -- partial sums, counters, the model map, the model depth, Ym, the frame and both
colour images -- lies between guard bands and starts as poison, quiet NaNs.  No guard may change, the results are bit-identical
to the unguarded call and to the references of tests/test_map_track_colour.py, and no poison word appears in them: a partial[i]
that no wave wrote, or a pixel of Ym that k_track_model_colour left out, would reach the sums as a NaN."""
import numpy as np
import pytest

import test_map_track_colour as TC
from guard_helpers import POISON_WORD, assert_same_bits, guarded
from test_fusion_map_file_gpu import engine
from test_fusion_map_locate_gpu import result_dict
from test_fusion_map_track_gpu import plain
from test_fusion_map_transform_gpu import write
from test_map_align import assert_same_result, assert_same_system
from test_map_track import PM, VS, basin_start, pose_near, track_opts, track_scene

pytestmark = pytest.mark.gpu


def test_track_colour_under_guards(tmp_path, parity_hooks):
    """The synthetic pair with colour at 96x128, one evaluation at step 3 (a last group with tail lanes, and scratch beyond it that
    nobody writes or reads), and a tracking of two renders on the scene map, whose ray-casts write colour and depth into the same
    scratch."""
    big = TC.colour_pair(7 + 96, 96, 128)
    pose = pose_near()
    so = dict(step=3, dist_max=0.016, centre_depth=1.5)
    want = TC.np_track_colour_system(big["cam"], big["bgr"], big["depth"], big["model_bgr"], big["model"], PM, pose, **so)
    s = track_scene()
    path = str(tmp_path / "scene.drfmap")
    write(path, VS, *s["blocks"])
    opt = track_opts(s, max_renders=2)
    start = basin_start(s, 0)
    want_frame = TC.cpp_frame(TC.build_check(tmp_path), lambda p: s["oracle"].render(p), s["cam"], s["bgr"], s["depth"], start, **opt)
    assert want[1][4] > 0 and want_frame["iterations"] >= 4

    def run():
        f = engine(big["cam"])
        got = f.track_colour_system(big["bgr"], big["depth"], big["model_bgr"], big["model"], PM, pose, **so)
        f.close()
        assert_same_system(got, want, "system")
        f = engine(s["cam"])
        f.load_map(path)
        r = f.track_colour_frame(s["bgr"], s["depth"], start, raise_on_failure=False, **opt)
        f.close()
        assert_same_result(result_dict(r), plain(want_frame), "tracking")
        return [("system", got[0]), ("pose", r.T), ("pose32", r.T32), ("sums", r.sums)]

    with guarded():
        on = run()
    off = run()
    for (na, xa), (nb, xb) in zip(on, off):
        assert na == nb
        assert_same_bits(xa, xb, na)
        words = np.ascontiguousarray(xa).view(np.uint32)
        assert not (words == POISON_WORD).any(), na
