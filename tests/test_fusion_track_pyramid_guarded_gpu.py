"""-m gpu: drf_track_reduce, drf_track_pyramid_system and drf_track_pyramid_frame under the guarded allocator of the parity library
(tests/guard_helpers.py): the calls' device scratch -- partial sums, counters, the model map, the full-resolution model and its
level, Ym, the frame and its pyramid -- lies between guard bands and starts as poison, quiet NaNs.  No guard may change, the
results are bit-identical to the unguarded call and to the references of tests/test_map_track_pyramid.py, and no poison word
appears in them: a level pixel that k_track_reduce left out, or a tail lane that read past its span, would reach the sums as a
NaN or move a guard."""
import numpy as np
import pytest

import test_map_track_colour as TC
import test_map_track_pyramid as TP
from guard_helpers import POISON_WORD, assert_same_bits, guarded
from test_fusion_map_file_gpu import engine
from test_fusion_map_locate_gpu import result_dict
from test_fusion_map_track_gpu import plain
from test_fusion_map_transform_gpu import write
from test_map_align import assert_same_result, assert_same_system
from test_map_locate import camera
from test_map_track import PM, VS, basin_start, pose_near, track_opts, track_scene

pytestmark = pytest.mark.gpu


def test_track_pyramid_under_guards(tmp_path, parity_hooks):
    """One reduction at 18x35 (remainders on both axes: the last wave of every level has tail lanes), one level-1 system at 18x35
    -- the deepest level an 18x35 camera has; a level-2 system, which 96x128 has, beside it -- and a two-render pyramid of three
    levels on the scene map, whose ray-casts write colour and depth into the same scratch."""
    bgr, depth = TP.reduce_pair(18, 18, 35)
    want_reduce = TP.np_reduce(bgr, depth, 1, 0.2)
    small = TC.colour_pair(7 + 18, 18, 35)
    big = TC.colour_pair(7 + 96, 96, 128)
    pose = pose_near()
    so = dict(levels=3, step=2, centre_depth=1.5)
    want1 = TP.np_pyramid_system(small["cam"], 1, small["bgr"], small["depth"], small["model_bgr"], small["model"], PM, pose, levels=2, step=1, centre_depth=1.5)
    want2 = TP.np_pyramid_system(big["cam"], 2, big["bgr"], big["depth"], big["model_bgr"], big["model"], PM, pose, **so)
    s = track_scene()
    path = str(tmp_path / "scene.drfmap")
    write(path, VS, *s["blocks"])
    opt = track_opts(s, max_renders=2, coarse_renders=2)
    start = basin_start(s, 0)
    want_frame = TP.cpp_frame(TP.build_check(tmp_path), lambda p: s["oracle"].render(p), s["cam"], s["bgr"], s["depth"], start, levels=3, **opt)
    assert want2[1][4] > 0 and want_frame["stats8"][6] == 3

    def run():
        f = engine(camera(VS, 18, 35))
        gc, gd = f.track_reduce(1, 0.2, bgr, depth)
        f.close()
        assert np.array_equal(gd.view(np.uint32), want_reduce[1].view(np.uint32)) and np.array_equal(gc, want_reduce[0])
        f = engine(small["cam"])
        got1 = f.track_pyramid_system(1, small["bgr"], small["depth"], small["model_bgr"], small["model"], PM, pose, levels=2, step=1, centre_depth=1.5)
        f.close()
        assert_same_system(got1, want1, "level 1 at 18x35")
        f = engine(big["cam"])
        got2 = f.track_pyramid_system(2, big["bgr"], big["depth"], big["model_bgr"], big["model"], PM, pose, **so)
        f.close()
        assert_same_system(got2, want2, "level 2 at 96x128")
        f = engine(s["cam"])
        f.load_map(path)
        r = f.track_pyramid_frame(s["bgr"], s["depth"], start, raise_on_failure=False, levels=3, **opt)
        f.close()
        assert_same_result(result_dict(r), plain(want_frame), "tracking")
        return [("reduced depth", gd), ("system 1", got1[0]), ("system 2", got2[0]), ("pose", r.T), ("pose32", r.T32), ("sums", r.sums)]

    with guarded():
        on = run()
    off = run()
    for (na, xa), (nb, xb) in zip(on, off):
        assert na == nb
        assert_same_bits(xa, xb, na)
        words = np.ascontiguousarray(xa).view(np.uint32)
        assert not (words == POISON_WORD).any(), na
