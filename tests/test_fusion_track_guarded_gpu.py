"""-m gpu: drf_track_system and drf_track_frame under the guarded allocator of the parity library (tests/guard_helpers.py): the call's
device scratch -- partial sums, counters, the model map, the model depth, the frame -- lies between guard bands and starts as poison,
quiet NaNs.  No guard may change, the results are bit-identical to the unguarded call and to the references of
tests/test_map_track.py, and no poison word appears in them: a partial[i] that no wave wrote, or a model pixel that k_track_model
left out, would reach the sums as a NaN."""
import numpy as np
import pytest

from guard_helpers import POISON_WORD, assert_same_bits, guarded
from test_fusion_map_file_gpu import engine
from test_fusion_map_locate_gpu import result_dict
from test_fusion_map_track_gpu import plain
from test_fusion_map_transform_gpu import write
from test_map_align import assert_same_result, assert_same_system
from test_map_track import PM, VS, basin_start, build_check, cpp_frame, np_track_system, pair_case, pose_near, track_opts, track_scene

pytestmark = pytest.mark.gpu


def test_track_under_guards(tmp_path, parity_hooks):
    """The synthetic pair at 96x128: one evaluation at step 1 (24 groups, three of them without a sample) and at step 3 (a last
    group with tail lanes, and scratch beyond it that nobody writes or reads); 5x7, where the one group is mostly tail; and a
    tracking of two renders on the scene map, whose ray-casts write into the same scratch."""
    big, small = pair_case(7 + 96, 96, 128), pair_case(7 + 5, 5, 7)
    pose = pose_near()
    systems = [(big, {}), (big, dict(step=3, dist_max=0.016, centre_depth=1.5)), (small, {})]
    want = [np_track_system(c["cam"], c["depth"], c["model"], PM, pose, **o) for c, o in systems]
    s = track_scene()
    path = str(tmp_path / "scene.drfmap")
    write(path, VS, *s["blocks"])
    opt = track_opts(s, max_renders=2)
    start = basin_start(s, 0)
    want_frame = cpp_frame(build_check(tmp_path), s["render"], s["cam"], s["depth"], start, **opt)
    assert want[0][1][1] > 0 and want_frame["iterations"] >= 4

    def run():
        out = []
        for k, (c, o) in enumerate(systems):
            f = engine(c["cam"])
            got = f.track_system(c["depth"], c["model"], PM, pose, **o)
            f.close()
            assert_same_system(got, want[k], "system %d" % k)
            out.append(("system %d" % k, got[0]))
        f = engine(s["cam"])
        f.load_map(path)
        r = f.track_frame(s["depth"], start, **opt)
        f.close()
        assert_same_result(result_dict(r), plain(want_frame), "tracking")
        return out + [("pose", r.T), ("pose32", r.T32), ("sums", r.sums)]

    with guarded():
        on = run()
    off = run()
    for (na, xa), (nb, xb) in zip(on, off):
        assert na == nb
        assert_same_bits(xa, xb, na)
        words = np.ascontiguousarray(xa).view(np.uint32)
        assert not (words == POISON_WORD).any(), na
