"""-m gpu: the refusals that drf_locate_*, drf_track_* and drf_track_colour_* open with, in their one order -- the options, the
call order, blocks in the host store while streaming is off, the pose, the model pose (DESIGN.md "Where the frame-pose code
lives").  Every call below is wrong in several ways at once and must name the first of them; one fault after the other is then
taken away.  A 96 x 128 engine over a map of two unobserved blocks; no call gets as far as an evaluation."""
import numpy as np
import pytest

from test_fusion_map_file_gpu import engine
from test_fusion_map_transform_gpu import H, VS, W, options, write

pytestmark = pytest.mark.gpu
f32 = np.float32
ALL_LO, ALL_HI = (-500.0, -500.0, -500.0), (500.0, 500.0, 500.0)
DEPTH, BGR = np.full((H, W), 2.0, f32), np.full((H, W, 3), 90, np.uint8)
GOOD = np.eye(4, dtype=f32)
BAD = GOOD.copy()
BAD[:3, :3] *= 1.01  # no rigid motion

# name -> (call(f, pose, model_pose, **opt), its statistics, does it take a model pose)
CALLS = {
    "locate_system": (lambda f, p, m, **o: f.locate_system(DEPTH, p, **o), "locate_stats", False),
    "locate_frame": (lambda f, p, m, **o: f.locate_frame(DEPTH, p, **o), "locate_stats", False),
    "track_system": (lambda f, p, m, **o: f.track_system(DEPTH, DEPTH, m, p, **o), "track_stats", True),
    "track_frame": (lambda f, p, m, **o: f.track_frame(DEPTH, p, **o), "track_stats", False),
    "track_colour_system": (lambda f, p, m, **o: f.track_colour_system(BGR, DEPTH, BGR, DEPTH, m, p, **o), "track_colour_stats", True),
    "track_colour_frame": (lambda f, p, m, **o: f.track_colour_frame(BGR, DEPTH, p, **o), "track_colour_stats", False),
    "track_pyramid_system": (lambda f, p, m, **o: f.track_pyramid_system(1, BGR, DEPTH, BGR, DEPTH, m, p, **o), "track_pyramid_stats", True),
    "track_pyramid_frame": (lambda f, p, m, **o: f.track_pyramid_frame(BGR, DEPTH, p, **o), "track_pyramid_stats", False),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_refusals_in_their_order(name, tmp_path):
    from tandem_amd import _lib
    call, stats, has_model = CALLS[name]
    path = str(tmp_path / "two.drfmap")
    write(path, VS, [(0, 0, 12), (1, 0, 12)], np.zeros((2, 4096), np.uint8))
    f = engine(options())

    def refused(pose, model_pose, **opt):
        with pytest.raises(_lib.DrError) as e:
            call(f, pose, model_pose, **opt)
        got = getattr(f, stats)()
        assert got == (0,) * len(got)
        assert str(e.value).count("drf_" + name) == 1, str(e.value)
        return e.value.code, str(e.value)

    f.load_map(path)
    f.stream_out_region(ALL_LO, ALL_HI)  # streaming is off and the store holds the map
    assert f.streaming_stats()["host"] == 2
    f.RenderAsync([GOOD])                # and a render is pending
    # everything is wrong: the option is named
    code, msg = refused(BAD, BAD, step=-1)
    assert code == 1 and "option step" in msg, msg
    # the option mended: the call order
    code, msg = refused(BAD, BAD)
    assert code == 2 and "IntegrateScanAsync may be called" in msg and "host store" not in msg, msg
    f.GetRenderResult()
    # the call order mended: the store
    code, msg = refused(BAD, BAD)
    assert code == 2 and "2 blocks are in the host store while streaming is off" in msg, msg
    f.stream_in_region(ALL_LO, ALL_HI)
    # the store mended: the pose, before the model pose
    code, msg = refused(BAD, BAD)
    assert code == 1 and "the pose" in msg and "model pose" not in msg, msg
    if has_model:
        code, msg = refused(GOOD, BAD)
        assert code == 1 and "the model pose" in msg, msg
    f.close()
