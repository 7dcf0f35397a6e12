"""-m gpu: the render scope (drf_set_render_scope(DRF_RENDER_MAP)) of a streaming DrFusion engine: RenderAsync at ANY pose
against the CPU oracle, whose pool never runs out -- depth (as uint32) and colour bit for bit -- while no block moves.
DESIGN.md §7c "Rendering the whole map"."""
import numpy as np
import pytest

import fusion_helpers
from fusion_helpers import BIG, box_of, canon, options, shifted
from test_fusion_streaming_gpu import assert_same_blocks, two_places

pytestmark = pytest.mark.gpu


def same_render(got_bgr, got_depth, want, what):
    ob, od = want
    assert np.array_equal(got_depth.view(np.uint32), od.view(np.uint32)), f"{what}: ray-cast depth differs at {(got_depth.view(np.uint32) != od.view(np.uint32)).sum()} px"
    assert np.array_equal(got_bgr, ob), f"{what}: ray-cast colour differs"


def step(f, o, bgr, depth, pose, render_poses, what):
    """The step() of tests/fusion_helpers.py with the poses to render given: every render and the update count must agree."""
    f.IntegrateScanAsync(bgr, depth, pose)
    f.RenderAsync(render_poses)
    rb, rd = f.GetRenderResult()
    assert o.integrate(bgr, depth, pose) == 0
    for i, p in enumerate(render_poses):
        same_render(rb[i], rd[i], o.render(p), f"{what}, render {i}")
    assert f.stats()["updated_last"] == o.stats()["updated_last"], what


def hit_blocks(opt, pose, depth):
    """Block of the centre voxel of every pixel's final sample (depth > 0), restated from the ray-cast in fp32."""
    F = np.float32
    v, u = np.nonzero(depth > 0)
    d = depth[v, u].astype(F)
    x = (u.astype(F) - F(opt["cx"])) * d / F(opt["fx"])
    y = (v.astype(F) - F(opt["cy"])) * d / F(opt["fy"])
    T = np.asarray(pose, F).reshape(4, 4)
    vs = F(opt["voxel_size"])
    out = []
    for i in range(3):
        a = T[i, 0] * x + T[i, 1] * y + T[i, 2] * d + T[i, 3] * F(1.0)
        out.append(np.trunc(a / vs + np.sign(a).astype(F) * F(0.5)).astype(np.int64) >> 3)
    return [tuple(int(c) for c in b) for b in np.stack(out, -1)]


@pytest.fixture(scope="module")
def room():
    """The room loop of tests/test_fusion_streaming_gpu.py (60 frames, 96x128, 2 cm, 2 m, a pool of 5600 blocks, minimum radius)
    with three render streams in map scope: frame k renders poses k, max(k - 30, 0) and max(k - 38, 0).  What the loop saw is
    recorded here and asserted by the first test; the later tests go on from its end state."""
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import RENDER_MAP, DrFusion, DrFusionOptions, streaming_min_radius
    fr, frames, H, W = fusion_helpers.room_frames()
    N = len(frames)
    opt = options(fr, H, W, 0.02, max_sensor_depth=2.0, num_blocks=5600, num_buckets=5600, num_render_streams=3)
    f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**dict(opt, num_blocks=BIG, num_buckets=BIG))
    g = DrFusion(DrFusionOptions(**dict(opt, num_render_streams=1)))  # the default: resident scope
    r = streaming_min_radius(f.options)
    f.set_streaming(r, BIG)
    g.set_streaming(r, BIG)
    f.set_render_scope(RENDER_MAP)
    s = dict(f=f, o=o, g=g, opt=opt, frames=frames, peak=0, staged=0, waited=0, error=None, g_last=None)
    try:
        for k, (bgr, depth, pose) in enumerate(frames):
            step(f, o, bgr, depth, pose, [pose, frames[max(k - 30, 0)][2], frames[max(k - 38, 0)][2]], f"frame {k}")
            rs = f.render_stats()
            s["staged"] += rs[0]
            s["waited"] += rs[3]
            s["peak"] = max(s["peak"], f.streaming_stats()["resident"])
            g.IntegrateScanAsync(bgr, depth, pose)
            g.RenderAsync([pose if k < N - 1 else frames[21][2]])
            s["g_last"] = g.GetRenderResult()
    except Exception as e:  # reported by the first test; the later ones then have no end state
        s["error"] = e
    yield s
    f.close()
    g.close()


def test_room_loop_with_look_backs_renders_as_the_unbounded_map(room):
    """Cannot pass without the render scope: the look-back poses see blocks that live in the host store."""
    if room["error"] is not None:
        raise room["error"]
    f, o, g, opt, frames = room["f"], room["o"], room["g"], room["opt"], room["frames"]
    want = o.export_blocks()
    assert len(want) > opt["num_blocks"]
    assert_same_blocks(f.export_all_blocks(), want, "whole map")
    assert room["peak"] <= opt["num_blocks"]
    assert room["staged"] > 0, "no render of the loop staged a stored block"
    stored, resident = set(f.export_host_blocks()), set(f.export_blocks())
    assert stored and not (stored & resident)
    # pose 21 looks at stored AND resident blocks, pose 29 at stored blocks only (the oracle's hits, by block)
    h21 = hit_blocks(opt, frames[21][2], o.render(frames[21][2])[1])
    n_stored, n_res = sum(b in stored for b in h21), sum(b in resident for b in h21)
    assert n_stored + n_res == len(h21)
    assert n_stored >= 500 and n_res >= 500, (n_stored, n_res)
    h29 = hit_blocks(opt, frames[29][2], o.render(frames[29][2])[1])
    assert len(h29) > 500 and all(b in stored for b in h29), (len(h29), sum(b in stored for b in h29))
    # the default stays what it was: in resident scope the same engine state renders pose 21 with holes
    gb, gd = room["g_last"]
    ob, od = o.render(frames[21][2])
    assert not np.array_equal(gd[0].view(np.uint32), od.view(np.uint32)), "resident scope should miss the stored blocks at pose 21"
    assert_same_blocks(g.export_all_blocks(), want, "whole map of the resident-scope engine")


def test_capacity_and_protocol_errors_leave_everything_as_it_was(room):
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import RENDER_MAP, RENDER_RESIDENT
    assert room["error"] is None, "needs the end state of the room loop"
    f, o, frames = room["f"], room["o"], room["frames"]
    bgr, depth, pose = frames[0]  # the loop closes: frame 0 follows frame 59
    f.IntegrateScanAsync(bgr, depth, pose)
    assert o.integrate(bgr, depth, pose) == 0
    st, res, host = f.streaming_stats(), f.export_blocks(), f.export_host_blocks()
    far = [frames[29][2]] * 3
    f.set_render_scope(RENDER_MAP, 64)
    with pytest.raises(_lib.DrError) as e:
        f.RenderAsync(far)
    assert e.value.code == 5
    assert f.streaming_stats() == st
    assert_same_blocks(f.export_blocks(), res, "resident after the refused render")
    assert_same_blocks(f.export_host_blocks(), host, "host store after the refused render")
    with pytest.raises(_lib.DrError) as e:                            # the protocol still expects RenderAsync
        f.IntegrateScanAsync(bgr, depth, pose)
    assert e.value.code == 2
    f.set_render_scope(RENDER_RESIDENT)
    f.RenderAsync([pose] * 3)                                         # accepted without a new scan
    with pytest.raises(_lib.DrError) as e:                            # between RenderAsync and GetRenderResult
        f.set_render_scope(RENDER_MAP)
    assert e.value.code == 2
    rb, rd = f.GetRenderResult()
    assert f.render_stats() == (0, 0, 0, 0)
    for i in range(3):
        same_render(rb[i], rd[i], o.render(pose), f"resident render {i} at the scan pose")
    with pytest.raises(_lib.DrError) as e:
        f.set_render_scope(2)
    assert e.value.code == 1
    assert f._L.drf_render_stats(f._h, None) == 1
    # a larger capacity: the same far render goes through and equals the oracle's
    f.set_render_scope(RENDER_MAP, 0)
    bgr, depth, pose = frames[1]
    step(f, o, bgr, depth, pose, far, "after the refused render")
    assert f.render_stats()[0] > 64


def test_far_render_beside_a_pending_map_mesh_is_read_only(room):
    from tandem_amd.dr_fusion import MESH_MAP, MESH_RESIDENT, RENDER_MAP
    assert room["error"] is None, "needs the end state of the room loop"
    f, o, opt, frames = room["f"], room["o"], room["opt"], room["frames"]
    f.set_render_scope(RENDER_MAP)
    lo, hi = box_of(o.export_blocks(), opt["voxel_size"])
    want_mesh = o.extract_mesh(lo, hi)  # the state the extraction is launched on
    assert len(want_mesh[0]) > 3000
    f.set_mesh_scope(MESH_MAP)
    f.ExtractMeshAsync(lo, hi)
    bgr, depth, pose = frames[2]
    f.IntegrateScanAsync(bgr, depth, pose)
    assert o.integrate(bgr, depth, pose) == 0
    before = (f.streaming_stats(), f.export_blocks(), f.export_host_blocks(), f.mesh_stats())
    assert before[0]["host"] > 0 and before[3][1] > 0
    far = [frames[31][2], frames[29][2], pose]
    f.RenderAsync(far)
    rb, rd = f.GetRenderResult()
    assert f.render_stats()[0] > 0
    for i, p in enumerate(far):
        same_render(rb[i], rd[i], o.render(p), f"render {i} beside the pending mesh")
    gv, gc = f.GetMeshSync()
    assert gv.shape == want_mesh[0].shape
    assert np.array_equal(canon(gv, gc), canon(*want_mesh)), "the pending map-scope mesh"
    assert f.streaming_stats() == before[0]
    assert_same_blocks(f.export_blocks(), before[1], "resident after the render")
    assert_same_blocks(f.export_host_blocks(), before[2], "host store after the render")
    assert f.mesh_stats() == before[3]
    f.set_mesh_scope(MESH_RESIDENT)
    for k in (3, 4):
        bgr, depth, pose = frames[k]
        step(f, o, bgr, depth, pose, [pose, frames[30][2], frames[k + 20][2]], f"frame {k} of the second lap")
    assert_same_blocks(f.export_all_blocks(), o.export_blocks(), "whole map after the second lap's frames")


def test_two_places_render_back_through_empty_superblocks():
    """Hazard (b): the first place is stored, and the pool's superblock flags call its whole neighbourhood empty."""
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import RENDER_MAP, DrFusion, DrFusionOptions, streaming_min_radius
    sc, scans, opt = two_places(4)
    opt.update(num_render_streams=2)
    f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**opt)
    f.set_streaming(streaming_min_radius(f.options))
    f.set_render_scope(RENDER_MAP)
    home = scans[0][2]
    step(f, o, *scans[0], [home, home], "scan at the origin")
    assert f.render_stats() == (0, 0, 0, 0)
    step(f, o, *scans[1], [home, scans[1][2]], "first far scan, looking back")  # its evictions are pending: the render waits
    rs = f.render_stats()
    assert rs[0] > 0 and rs[1] == rs[0] * (8 + 4096) and rs[2] == 0 and rs[3] == 1, rs
    for i in (2, 3):
        step(f, o, *scans[i], [scans[i][2], scans[i][2]], f"far scan {i}, scan pose only")
        assert f.render_stats() == (0, 0, 0, 0)
    step(f, o, *scans[4], [scans[4][2], home], "last far scan, looking back")
    rs = f.render_stats()
    assert rs[0] > 0 and rs[3] == 0, rs                              # nothing was evicted by this scan: no wait
    stored, resident = set(f.export_host_blocks()), set(f.export_blocks())
    hits = hit_blocks(opt, home, o.render(home)[1])
    assert len(hits) > 1000 and all(b in stored for b in hits)
    sup = lambda blocks: {tuple(c >> 3 for c in b) for b in blocks}  # noqa: E731 -- level-1 superblocks (8^3 blocks)
    assert not (sup(hits) & sup(resident)), "the render back must cross superblocks without a resident block"
    assert_same_blocks(f.export_all_blocks(), o.export_blocks(), "whole map")
    f.close()


def test_near_render_stages_without_waiting_for_pending_evictions():
    """A render close enough to the last scan cannot read a block that scan evicted, so it does not wait for the scan -- while
    it still stages the stored blocks within its reach.  Those lie in the hysteresis shell (radius, radius + 8 vs] of the scan's
    centre p: stored by an earlier, farther scan and not brought back.  The scan's camera centre is placed radius + 4 vs from
    such a block, against the direction of the image's last corner ray (only there does the view reach D rho), and the render
    10 voxels along that ray."""
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import RENDER_MAP, DrFusion, DrFusionOptions, streaming_min_radius
    sc, scans, opt = two_places(1)
    vs = opt["voxel_size"]
    f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**opt)
    R = streaming_min_radius(f.options)
    f.set_streaming(R)
    f.set_render_scope(RENDER_MAP)
    for i, s in enumerate(scans):  # the origin, then 20 m away: the first place is stored
        step(f, o, *s, [s[2]], f"scan {i}")
    stored = np.array(sorted(f.export_host_blocks()), np.int64)
    assert len(stored) > 100
    centres = (stored * 8 + 3.5) * vs
    c = centres[np.argmin(np.linalg.norm(centres - centres.mean(0), axis=1))]  # a stored block in the middle of the first place
    u = np.array([(opt["width"] - 1 - opt["cx"]) / opt["fx"], (opt["height"] - 1 - opt["cy"]) / opt["fy"], 1.0])
    u /= np.linalg.norm(u)  # the last pixel's ray of a camera that looks along +z
    p = c - (R + 4 * vs) * u
    bgr, depth, pose0 = sc["scans"][0]
    pose = np.array(pose0, np.float32).reshape(4, 4).copy()
    pose[:3, 3] = p
    p = pose[:3, 3].astype(np.float64)
    d = np.linalg.norm(centres - p, axis=1)
    assert ((d > R + 0.5 * vs) & (d <= R + 7.5 * vs)).any(), "no stored block in the hysteresis shell of the scan"
    q = np.eye(4, dtype=np.float32)  # looking along +z: the block lies on the corner ray, render_reach - 2 vs away
    q[:3, 3] = p + 10 * vs * u
    out_before = f.streaming_stats()["streamed_out"]
    f.IntegrateScanAsync(bgr, depth, pose)
    f.RenderAsync([q])
    rb, rd = f.GetRenderResult()
    rs = f.render_stats()
    assert o.integrate(bgr, depth, pose) == 0
    same_render(rb[0], rd[0], o.render(q), "render near the scan, evictions pending")
    assert rs[0] > 0 and rs[2] == 0 and rs[3] == 0, rs
    # the scan did evict (the second place): its chain was pending when the render selected its blocks
    assert f.streaming_stats()["streamed_out"] > out_before
    assert_same_blocks(f.export_all_blocks(), o.export_blocks(), "whole map")
    f.close()


def test_stored_blocks_beyond_the_dense_grid():
    """Hazard (c): the scene of test_blocks_in_the_overflow_table straddles block coordinate 256; once it is stored the pool's
    table is empty, and only the staging knows that the literal pass is needed."""
    from synth import scene
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import RENDER_MAP, DrFusion, DrFusionOptions, streaming_min_radius
    H, W, vs = 96, 128, 0.02
    sc = scene.make_scans(4, H, W, seed=6)
    opt = options(sc, H, W, vs)
    S = np.eye(4, dtype=np.float32)
    c, s = np.cos(1.45), np.sin(1.45)
    S[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    S[:3, 3] = (40.2, 0.3, -0.2)
    far_scans = shifted(sc["scans"], S)
    f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**opt)
    f.set_streaming(streaming_min_radius(f.options))
    f.set_render_scope(RENDER_MAP)
    for i in range(2):
        step(f, o, *far_scans[i], [far_scans[i][2]], f"shifted scan {i}")
    xs = [k[0] for k in f.export_blocks()]
    assert min(xs) < 256 <= max(xs)
    back = far_scans[1][2]
    for i in range(2):  # the unshifted scene, 40 m away: everything above is evicted
        step(f, o, *sc["scans"][i], [back], f"scan {i} at the origin, looking back")
        assert f.render_stats()[0] > 0
    stored = set(f.export_host_blocks())
    assert max(k[0] for k in stored) >= 256 > min(k[0] for k in stored)
    hits = hit_blocks(opt, back, o.render(back)[1])
    assert sum(b[0] >= 256 and b in stored for b in hits) > 100, "the render back must hit stored blocks beyond the border"
    assert_same_blocks(f.export_all_blocks(), o.export_blocks(), "whole map")
    f.close()


def test_nothing_to_stage():
    from synth import scene
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import RENDER_MAP, DrFusion, DrFusionOptions, streaming_min_radius
    H, W = 96, 128
    sc = scene.make_scans(3, H, W, seed=11)
    opt = options(sc, H, W, 0.02)
    for streaming in (False, True):
        f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**opt)
        if streaming:
            f.set_streaming(streaming_min_radius(f.options))
        f.set_render_scope(RENDER_MAP)
        for i, (bgr, depth, pose) in enumerate(sc["scans"]):
            step(f, o, bgr, depth, pose, [sc["scans"][0][2]], f"streaming {streaming}, scan {i}")
            assert f.render_stats() == (0, 0, 0, 0)
        if streaming:
            assert f.streaming_stats()["host"] == 0
        f.close()
