"""-m gpu: map-scope meshing (drf_set_mesh_scope(DRF_MESH_MAP)) of a DrFusion map whose blocks are split between the pool and
the host store.  The reference is an unbounded GPU engine fed the same scans: its mesh must come back byte for byte, in the
same triangle order, without a block moving.  The CPU oracle checks the triangle set.  DESIGN.md §7c "Meshing the whole map"."""
import numpy as np
import pytest

import fusion_helpers
from fusion_helpers import assert_same_mesh, box_of, canon, feed, options, places, rows, shifted, step, unbounded

pytestmark = pytest.mark.gpu

ALL_LO, ALL_HI = (-1e4, -1e4, -1e4), (1e4, 1e4, 1e4)


@pytest.fixture(scope="module")
def room_frames():
    return fusion_helpers.room_frames()


def room_loop(room_frames, S):
    """The room loop of tests/test_fusion_streaming_gpu.py (a pool of ~70 % of the map, streaming at the minimum radius), the
    scene moved by S; also an unbounded engine and the oracle fed the same frames."""
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, streaming_min_radius
    fr, frames, H, W = room_frames
    opt = options(fr, H, W, 0.02, max_sensor_depth=2.0, num_blocks=5600, num_buckets=5600)
    f, u, o = DrFusion(DrFusionOptions(**opt)), DrFusion(DrFusionOptions(**unbounded(opt))), TsdfOracle(**unbounded(opt))
    f.set_streaming(streaming_min_radius(f.options), 100000)
    for bgr, depth, pose in shifted(frames, S):
        feed(f, bgr, depth, pose)
        feed(u, bgr, depth, pose)
        assert o.integrate(bgr, depth, pose) == 0
    return f, u, o, opt


def check_room(f, u, o, opt):
    from tandem_amd.dr_fusion import MESH_MAP, MESH_RESIDENT
    blocks = u.export_blocks()
    assert len(blocks) > opt["num_blocks"]
    st = f.streaming_stats()
    assert st["host"] > 0 and st["resident"] + st["host"] == len(blocks), st
    lo, hi = box_of(blocks, opt["voxel_size"])
    want = u.GetMesh(lo, hi)
    assert len(want[0]) > 3000
    f.set_mesh_scope(MESH_MAP)
    got = f.GetMesh(lo, hi)
    assert_same_mesh(got, want, "map scope vs unbounded engine")
    assert np.array_equal(canon(*got), canon(*o.extract_mesh(lo, hi))), "map scope vs oracle"
    meshed, uploaded, chunks = f.mesh_stats()
    assert meshed == len(blocks) and uploaded >= st["host"] and chunks >= 2, f.mesh_stats()
    f.set_mesh_scope(MESH_RESIDENT)
    res = f.GetMesh(lo, hi)
    assert len(res[0]) < len(want[0]), "the resident-scope mesh should miss the stored blocks"
    assert f.mesh_stats() == (st["resident"], 0, 1)


def test_automatic_mode_room_loop_map_mesh_is_the_unbounded_engines(room_frames):
    f, u, o, opt = room_loop(room_frames, np.eye(4, dtype=np.float32))
    check_room(f, u, o, opt)
    f.close(); u.close()


def test_room_loop_in_the_overflow_table(room_frames):
    """The room moved beyond block coordinate 256 along x: every resident block lives in the open-addressing table."""
    S = np.eye(4, dtype=np.float32)
    S[:3, 3] = (50.0, 0.25, -0.5)
    f, u, o, opt = room_loop(room_frames, S)
    assert min(k[0] for k in u.export_blocks()) >= 256
    check_room(f, u, o, opt)
    f.close(); u.close()


@pytest.fixture(scope="module")
def many_places():
    """Four places 20 m apart into a pool that holds about one of them; each place goes to the host store with
    drf_stream_out_region before the next is scanned."""
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, streaming_min_radius
    pl, opt = places(4)
    o1 = TsdfOracle(**unbounded(opt))
    for s in pl[0]:
        o1.integrate(*s)
    one = len(o1.export_blocks())
    opt.update(num_blocks=int(1.2 * one), num_buckets=int(1.2 * one))
    f, u, o = DrFusion(DrFusionOptions(**opt)), DrFusion(DrFusionOptions(**unbounded(opt))), TsdfOracle(**unbounded(opt))
    f.set_streaming(streaming_min_radius(f.options))
    for p, scans in enumerate(pl):
        for s in scans:
            feed(f, *s)
            feed(u, *s)
            assert o.integrate(*s) == 0
        if p + 1 < len(pl):
            f.stream_out_region((20.0 * p - 10.0, -1e4, -1e4), (20.0 * p + 10.0, 1e4, 1e4))
    blocks = u.export_blocks()
    assert len(blocks) > 3 * opt["num_blocks"]
    yield f, u, o, opt, box_of(blocks, opt["voxel_size"])
    f.close(); u.close()


def test_many_chunks(many_places):
    from tandem_amd.dr_fusion import MESH_MAP
    f, u, o, opt, (lo, hi) = many_places
    st = f.streaming_stats()
    assert st["host"] > opt["num_blocks"], st
    want = u.GetMesh(lo, hi)
    f.set_mesh_scope(MESH_MAP)
    got = f.GetMesh(lo, hi)
    meshed, uploaded, chunks = f.mesh_stats()
    assert chunks >= 3 and uploaded > st["host"], f.mesh_stats()
    assert meshed == st["resident"] + st["host"]
    assert_same_mesh(got, want, "map scope vs unbounded engine")
    assert np.array_equal(canon(*got), canon(*o.extract_mesh(lo, hi))), "map scope vs oracle"
    assert f.streaming_stats() == st


def test_save_mesh_in_map_scope_writes_the_unbounded_engines_file(many_places, tmp_path):
    from tandem_amd.dr_fusion import MESH_MAP
    f, u, o, opt, (lo, hi) = many_places
    f.set_mesh_scope(MESH_MAP)
    f.SaveMeshToFile(tmp_path / "map.obj", lo, hi)
    u.SaveMeshToFile(tmp_path / "ref.obj", lo, hi)
    a, b = (tmp_path / "map.obj").read_bytes(), (tmp_path / "ref.obj").read_bytes()
    assert len(a) > 100000 and a == b


def test_a_cut_through_a_surface():
    """One place, then the half-space x >= x_cut to the host store: the plane crosses the surface.  The map mesh is the
    unbounded engine's; the resident-scope mesh is a strict subset that lacks the seam cells on the resident side."""
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MESH_MAP, MESH_RESIDENT
    pl, opt = places(1, scans_per_place=3, seed=5)
    vs = opt["voxel_size"]
    f, u, o = DrFusion(DrFusionOptions(**opt)), DrFusion(DrFusionOptions(**unbounded(opt))), TsdfOracle(**unbounded(opt))
    for s in pl[0]:
        feed(f, *s)
        feed(u, *s)
        assert o.integrate(*s) == 0
    blocks = u.export_blocks()
    lo, hi = box_of(blocks, vs)
    want = u.GetMesh(lo, hi)
    wx = want[0].reshape(-1, 3, 3)[:, :, 0]
    bcut = int(np.floor(np.median(wx) / (8 * vs)))  # a block plane through the middle of the surface
    x_cut = bcut * 8 * vs
    f.stream_out_region(((bcut * 8 - 4) * vs, -1e4, -1e4), ALL_HI)
    st = f.streaming_stats()
    assert st["host"] > 0 and st["resident"] > 0
    assert max(k[0] for k in f.export_blocks()) < bcut <= min(k[0] for k in f.export_host_blocks())
    f.set_mesh_scope(MESH_MAP)
    got = f.GetMesh(lo, hi)
    assert_same_mesh(got, want, "map scope vs unbounded engine")
    assert np.array_equal(canon(*got), canon(*o.extract_mesh(lo, hi))), "map scope vs oracle"
    f.set_mesh_scope(MESH_RESIDENT)
    res = f.GetMesh(lo, hi)
    R = {r.tobytes() for r in rows(*res)}
    Wt = rows(*want)
    W = {r.tobytes() for r in Wt}
    assert R < W, "the resident-scope mesh must be a strict subset of the whole map's"
    missing = np.array([r.tobytes() not in R for r in Wt])
    mx = Wt[:, :9].view(np.float32)[:, 0::3]
    # cells owned by the last resident voxel layer span x in [x_cut - 1.5 vs, x_cut - 0.5 vs]; the first stored layer's start at x_cut - 0.5 vs
    seam = missing & (mx.min(axis=1) < x_cut - 0.6 * vs) & (mx.min(axis=1) > x_cut - 8 * vs)
    assert seam.sum() > 0, "no triangle within one block of the cut on the resident side is missing"
    assert not (missing & (mx.max(axis=1) < x_cut - 8 * vs)).any(), "triangles far from the cut went missing"
    f.close(); u.close()


def test_map_extraction_is_read_only():
    """Pool order, host store and streaming stats are unchanged by a map-scope extraction, and integrating further frames
    still matches the oracle bit for bit."""
    from synth import scene
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MESH_MAP, streaming_min_radius
    H, W = 96, 128
    sc = scene.make_scans(4, H, W, seed=3)
    S = np.eye(4, dtype=np.float32)
    S[:3, 3] = (20.0, 0.0, 0.0)
    scans = [sc["scans"][0]] + shifted(sc["scans"][:4], S)
    opt = options(sc, H, W, 0.02, max_sensor_depth=6.0)
    c = TsdfOracle(**unbounded(opt))
    c.integrate(*scans[0])
    n1 = len(c.export_blocks())
    c2, n2 = TsdfOracle(**unbounded(opt)), []
    for s in scans[1:3]:
        c2.integrate(*s)
        n2.append(len(c2.export_blocks()))
    pool = max(n1 + n2[0], n2[-1])  # the first scan of the second place allocates before the first place leaves
    opt.update(num_blocks=pool, num_buckets=pool)
    f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**unbounded(opt))
    f.set_streaming(streaming_min_radius(f.options))
    for i, s in enumerate(scans[:3]):
        step(f, o, *s, f"scan {i}")
    st = f.streaming_stats()
    assert st["host"] == n1 and st["resident"] == n2[-1], (st, n1, n2)
    res, host = f.export_blocks(), f.export_host_blocks()
    f.set_mesh_scope(MESH_MAP)
    lo, hi = (-3.0, -3.0, -1.0), (23.0, 3.0, 7.0)
    got = f.GetMesh(lo, hi)
    assert np.array_equal(canon(*got), canon(*o.extract_mesh(lo, hi)))
    assert f.streaming_stats() == st
    after = f.export_blocks()
    assert list(after.keys()) == list(res.keys()), "the pool's slot order changed"
    assert all(np.array_equal(after[k], res[k]) for k in res)
    h2 = f.export_host_blocks()
    assert h2.keys() == host.keys() and all(np.array_equal(h2[k], host[k]) for k in host)
    for i, s in enumerate(scans[3:]):
        step(f, o, *s, f"scan {i + 3} after the extraction")
    all_f, all_o = f.export_all_blocks(), o.export_blocks()
    assert all_f.keys() == all_o.keys() and all(np.array_equal(all_f[k], all_o[k]) for k in all_o)
    f.close()


def test_empty_host_store_is_the_resident_pass():
    from synth import scene
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MESH_MAP, MESH_RESIDENT
    H, W = 96, 128
    sc = scene.make_scans(2, H, W, seed=1)
    f = DrFusion(DrFusionOptions(**options(sc, H, W, 0.02)))
    for s in sc["scans"]:
        feed(f, *s)
    lo, hi = (-2.0, -2.0, 0.0), (2.0, 2.0, 4.0)
    res = f.GetMesh(lo, hi)
    st_res = f.mesh_stats()
    f.set_mesh_scope(MESH_MAP)
    got = f.GetMesh(lo, hi)
    assert len(res[0]) > 1000
    assert_same_mesh(got, res, "map scope with an empty host store")
    assert f.mesh_stats() == st_res and f.mesh_stats()[1] == 0
    f.set_mesh_scope(MESH_RESIDENT)
    f.close()


def test_protocol():
    from synth import scene
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MESH_MAP, MESH_RESIDENT
    H, W = 96, 128
    sc = scene.make_scans(2, H, W, seed=1)
    f = DrFusion(DrFusionOptions(**options(sc, H, W, 0.02)))
    feed(f, *sc["scans"][0])
    f.stream_out_region((0.0, -1e4, -1e4), ALL_HI)
    assert f.streaming_stats()["host"] > 0
    lo, hi = (-2.0, -2.0, 0.0), (2.0, 2.0, 4.0)
    for bad in (-1, 2, 100):
        with pytest.raises(_lib.DrError) as e:
            f.set_mesh_scope(bad)
        assert e.value.code == 1
    assert f._L.drf_mesh_stats(f._h, None) == 1
    f.set_mesh_scope(MESH_MAP)
    f.ExtractMeshAsync(lo, hi)
    for scope in (MESH_RESIDENT, MESH_MAP):
        with pytest.raises(_lib.DrError) as e:
            f.set_mesh_scope(scope)
        assert e.value.code == 2
    v, c = f.GetMeshSync()
    stats = f.mesh_stats()
    assert stats[1] > 0, "the scope stayed DRF_MESH_MAP"
    # outside the integrate window (after IntegrateScanAsync, before GetRenderResult)
    f.stream_in_region(ALL_LO, ALL_HI)  # streaming is off: the next scan needs the store empty
    f.IntegrateScanAsync(*sc["scans"][1])
    with pytest.raises(_lib.DrError) as e:
        f.ExtractMeshAsync(lo, hi)
    assert e.value.code == 2
    assert f.mesh_stats() == stats
    f.RenderAsync([sc["scans"][1][2]])
    f.GetRenderResult()
    f.close()
