"""-m gpu: the one staging of host-stored blocks (csrc/render_ops.h MapStage) under its three readers on ONE engine -- a map-scope
render, the tracking's model render, the locate scope -- one after the other.  Each reader is tested alone against an unbounded pool
elsewhere (test_fusion_render_scope_gpu.py, test_fusion_map_track_gpu.py, test_fusion_locate_scope_gpu.py); here they share the
staging, and every image, pose and result must still be the unbounded pool's, bit for bit, every statistic what the call gives
alone on a fresh engine, and the map untouched.  96x128, 2 cm voxels.  DESIGN.md "Where rendering and the frame pose live"."""
import numpy as np
import pytest

from fusion_helpers import feed, places, unbounded
from test_fusion_map_locate_gpu import result_dict
from test_fusion_streaming_gpu import assert_same_blocks
from test_map_align import assert_same_result

pytestmark = pytest.mark.gpu

TRACK_OPT = dict(max_renders=2)
LOCATE_OPT = dict(max_iters=3, centre_depth=2.0)


def render(f, pose):
    f.RenderAsync([pose])
    rb, rd = f.GetRenderResult()
    return rb[0].copy(), rd[0].copy()


def same_image(a, b, what):
    assert np.array_equal(a[0], b[0]), what + ": colour differs"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), what + ": depth differs"


def same_pose(a, b, what):
    assert_same_result(result_dict(a), result_dict(b), what)
    assert np.array_equal(a.T32.view(np.uint32), b.T32.view(np.uint32)), what + ": the float pose differs"


def test_one_staging_three_readers():
    from tandem_amd.dr_fusion import LOCATE_MAP, RENDER_MAP, DrFusion, DrFusionOptions, streaming_min_radius
    (near, far), opt = places(2, scans_per_place=3)
    bgr, depth, pose = near[0]
    start = pose.copy()
    start[:3, 3] += np.array((0.02, -0.02, 0.02), np.float32)  # a voxel off the scan's pose on every axis: both refinements move
    before, last = near + far[:1], far[1:]                     # `last`: the scan in front of render 1 and the one in front of render 2

    def engine_a():
        """Streaming on: place 0 is in the host store once the camera is at place 1.  Both scopes over the map; the locate scope may
        stage more than the render scope, so the staging is sized by the larger need of the two."""
        f = DrFusion(DrFusionOptions(**opt))
        f.set_streaming(streaming_min_radius(f.options))
        for s in before:
            feed(f, *s)
        stored = f.streaming_stats()["host"]
        assert stored > 100
        f.set_render_scope(RENDER_MAP, stored)
        f.set_locate_scope(LOCATE_MAP, 4 * stored)
        return f

    # B: the pool holds the whole map
    B = DrFusion(DrFusionOptions(**unbounded(opt)))
    for s in before:
        feed(B, *s)
    B.IntegrateScanAsync(*last[0])
    want = dict(render1=render(B, pose), track=B.track_frame(depth, start, raise_on_failure=False, **TRACK_OPT),
                locate=B.locate_frame(depth, start, raise_on_failure=False, **LOCATE_OPT))
    B.IntegrateScanAsync(*last[1])
    want["render2"] = render(B, pose)
    assert np.isfinite(want["render1"][1]).any() and (want["render1"][1] > 0).sum() > 1000  # place 0 is in the picture
    B.close()

    # A: the four calls in a row
    A = engine_a()
    A.IntegrateScanAsync(*last[0])
    same_image(render(A, pose), want["render1"], "render 1")
    stats = dict(render1=A.render_stats())
    ss = A.streaming_stats()
    pool, store = A.export_blocks(), A.export_host_blocks()
    assert len(store) > 100 and all(c[0] * 8 * 0.02 > 10.0 for c in pool) and any(c[0] * 8 * 0.02 < 10.0 for c in store)  # place 0: all of it stored
    assert stats["render1"][0] > 100                                    # and the render staged it
    same_pose(A.track_frame(depth, start, raise_on_failure=False, **TRACK_OPT), want["track"], "tracking")
    stats["track"] = A.track_stats()
    assert A.render_stats() == stats["render1"]                         # the model's render leaves the public render's statistics
    same_pose(A.locate_frame(depth, start, raise_on_failure=False, **LOCATE_OPT), want["locate"], "localisation")
    stats["locate"] = A.locate_stage_stats()
    assert stats["locate"][0] >= 1 and stats["locate"][1] > 100 and stats["track"][4] == 2
    assert A.streaming_stats() == ss
    assert_same_blocks(A.export_blocks(), pool, "the pool after tracking and localisation")
    assert_same_blocks(A.export_host_blocks(), store, "the host store after tracking and localisation")
    A.IntegrateScanAsync(*last[1])
    same_image(render(A, pose), want["render2"], "render 2")
    stats["render2"] = A.render_stats()
    assert A.track_stats() == stats["track"] and A.locate_stage_stats() == stats["locate"]
    A.close()

    # A': every call alone on a fresh engine gives the same statistics
    def alone(what):
        f = engine_a()
        f.IntegrateScanAsync(*last[0])
        if what == "render1":
            render(f, pose)
            got = f.render_stats()
        elif what == "track":
            render(f, last[0][2])                                       # (the scan's own render: a resident one, nothing staged)
            f.track_frame(depth, start, raise_on_failure=False, **TRACK_OPT)
            got = f.track_stats()
        elif what == "locate":
            render(f, last[0][2])
            f.locate_frame(depth, start, raise_on_failure=False, **LOCATE_OPT)
            got = f.locate_stage_stats()
        else:
            render(f, last[0][2])
            f.IntegrateScanAsync(*last[1])
            render(f, pose)
            got = f.render_stats()
        f.close()
        return got

    for what in ("render1", "track", "locate", "render2"):
        assert alone(what) == stats[what], what
