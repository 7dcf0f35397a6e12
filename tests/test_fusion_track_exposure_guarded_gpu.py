"""-m gpu: drf_track_exposure_system and drf_track_exposure_frame under the guarded allocator of the parity library
(tests/guard_helpers.py): the calls' device scratch -- 45 partial sums per group, counters, the model map, the full-resolution model
and its level, Ym, the frame and its pyramid -- lies between guard bands and starts as poison, quiet NaNs.  No guard may change, the
results are bit-identical to the unguarded call and to the references of tests/test_map_track_exposure.py, and no poison word
appears in sums, pose, gain or offset: a row of 45 that k_track_exposure left short, or a fold that read past the last group,
would reach the sums as a NaN or move a guard."""
import numpy as np
import pytest

import test_map_track_colour as TC
import test_map_track_exposure as TX
from guard_helpers import POISON_WORD, assert_same_bits, guarded
from test_fusion_map_file_gpu import engine
from test_fusion_map_locate_gpu import result_dict
from test_fusion_map_track_gpu import plain
from test_fusion_map_transform_gpu import write
from test_map_align import assert_same_result
from test_map_track import PM, VS, basin_start, pose_near, track_opts, track_scene

pytestmark = pytest.mark.gpu


def test_track_exposure_under_guards(tmp_path, parity_hooks):
    """One level-1 system at 18x35 (remainders on both axes: the last wave has tail lanes, one group of 45), one level-2 system at
    96x128, and a two-render tracking of three levels on the scene map with the frame re-exposed, whose ray-casts write colour and
    depth into the same scratch."""
    small = TC.colour_pair(7 + 18, 18, 35)
    big = TC.colour_pair(7 + 96, 96, 128)
    pose = pose_near()
    so = dict(levels=3, step=2, centre_depth=1.5)
    want1 = TX.np_exposure_system(small["cam"], 1, small["bgr"], small["depth"], small["model_bgr"], small["model"], PM, pose, 0.7, 12.5, levels=2, step=1, centre_depth=1.5)
    want2 = TX.np_exposure_system(big["cam"], 2, big["bgr"], big["depth"], big["model_bgr"], big["model"], PM, pose, 1.6, -40.0, **so)
    s = track_scene()
    path = str(tmp_path / "scene.drfmap")
    write(path, VS, *s["blocks"])
    opt = track_opts(s, max_renders=2, coarse_renders=2)
    start = basin_start(s, 0)
    frame = TX.re_expose(s["bgr"], 0.8, 25.0)
    want_frame = TX.cpp_frame(TX.build_check(tmp_path), lambda p: s["oracle"].render(p), s["cam"], frame, s["depth"], start, levels=3, **opt)
    assert want2[1][4] > 0 and want_frame["stats8"][6] == 3 and want_frame["photometric"] > 0

    def run():
        f = engine(small["cam"])
        got1 = f.track_exposure_system(1, small["bgr"], small["depth"], small["model_bgr"], small["model"], PM, pose, 0.7, 12.5, levels=2, step=1, centre_depth=1.5)
        f.close()
        TX.assert_same_sums(got1, want1, "level 1 at 18x35")
        f = engine(big["cam"])
        got2 = f.track_exposure_system(2, big["bgr"], big["depth"], big["model_bgr"], big["model"], PM, pose, 1.6, -40.0, **so)
        f.close()
        TX.assert_same_sums(got2, want2, "level 2 at 96x128")
        f = engine(s["cam"])
        f.load_map(path)
        r = f.track_exposure_frame(frame, s["depth"], start, raise_on_failure=False, levels=3, **opt)
        f.close()
        assert_same_result(result_dict(r), plain(want_frame), "tracking")
        assert r.gain == want_frame["gain"] and r.offset == want_frame["offset"] and np.array_equal(r.ext, want_frame["ext"])
        return [("system 1", got1[0]), ("system 2", got2[0]), ("pose", r.T), ("pose32", r.T32), ("sums", r.sums), ("ext", r.ext),
                ("exposure", np.array([r.gain, r.offset]))]

    with guarded():
        on = run()
    off = run()
    for (na, xa), (nb, xb) in zip(on, off):
        assert na == nb
        assert_same_bits(xa, xb, na)
        words = np.ascontiguousarray(xa).view(np.uint32)
        assert not (words == POISON_WORD).any(), na
