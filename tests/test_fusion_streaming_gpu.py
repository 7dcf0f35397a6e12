"""-m gpu: DrFusion with voxel-block streaming (drf_set_streaming, drf_stream_{out,in}_region) against the CPU oracle, whose
pool never runs out: the whole map -- resident blocks and host store merged -- bit-identical after every scan, identical
update counts, and bit-identical ray-casts at the scan pose.  DESIGN.md "Streaming voxel blocks"."""
import numpy as np
import pytest

from fusion_helpers import canon, options, shifted, step

pytestmark = pytest.mark.gpu

ALL_LO, ALL_HI = (-1e4, -1e4, -1e4), (1e4, 1e4, 1e4)


def assert_same_blocks(a, b, what=""):
    """Two {block coordinate: 4096 bytes} dicts, bit for bit."""
    assert a.keys() == b.keys(), f"{what}: block sets differ: {len(a)} vs {len(b)}, e.g. {sorted(a.keys() ^ b.keys())[:3]}"
    bad = [k for k in a if not np.array_equal(a[k], b[k])]
    assert not bad, f"{what}: {len(bad)} of {len(a)} blocks differ, e.g. {bad[:3]}"


def test_round_trip_out_and_in_is_exact():
    from synth import scene
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions
    H, W = 96, 128
    sc = scene.make_scans(5, H, W, seed=11)
    opt = options(sc, H, W, 0.02)
    f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**opt)
    for i, (bgr, depth, pose) in enumerate(sc["scans"][:2]):
        step(f, o, bgr, depth, pose, f"scan {i}")
    before = f.export_blocks()
    n = len(before)
    f.stream_out_region(ALL_LO, ALL_HI)
    st = f.streaming_stats()
    assert f.export_blocks() == {} and st["resident"] == 0 and st["host"] == n and st["streamed_out"] == n
    assert_same_blocks(f.export_host_blocks(), before, "host store")
    f.stream_in_region(ALL_LO, ALL_HI)
    st = f.streaming_stats()
    assert st["resident"] == n and st["host"] == 0 and st["streamed_in"] == n and st["bytes_moved"] == 2 * 4096 * n
    assert_same_blocks(f.export_blocks(), before, "after the round trip")
    # half out and back: the pool is compacted, the next allocations reuse the vacated slots
    f.stream_out_region(ALL_LO, (1e4, 1e4, 2.0))
    assert 0 < f.streaming_stats()["host"] < n
    f.stream_in_region(ALL_LO, ALL_HI)
    assert_same_blocks(f.export_blocks(), before, "after the second round trip")
    for i, (bgr, depth, pose) in enumerate(sc["scans"][2:]):
        step(f, o, bgr, depth, pose, f"scan {i + 2}")
    assert_same_blocks(f.export_blocks(), o.export_blocks(), "final")
    f.close()


def test_automatic_mode_walks_the_room_loop_in_a_bounded_pool():
    """The synth.room loop at 2 m depth: a pool of ~70 % of the final map overflows without streaming; with streaming at the
    minimum radius the loop finishes, every ray-cast and update count equals the oracle's, and blocks go out and come back."""
    import torch  # noqa: F401  (synth.room renders with torch)
    from synth import room
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, streaming_min_radius
    H, W, N = 96, 128, 60
    poses = room.loop_poses(N, seed=0)
    fr = room.render_frames(poses, H, W)
    frames = [(fr["bgr"][k].numpy(), fr["depth"][k].numpy(), poses[k]) for k in range(N)]
    opt = options(fr, H, W, 0.02, max_sensor_depth=2.0, num_blocks=5600, num_buckets=5600)
    g = DrFusion(DrFusionOptions(**opt))
    with pytest.raises(_lib.DrError) as e:
        for bgr, depth, pose in frames:
            g.IntegrateScanAsync(bgr, depth, pose)
            g.RenderAsync([pose])
            g.GetRenderResult()
    assert e.value.code == 5
    g.close()

    f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**dict(opt, num_blocks=100000, num_buckets=100000))  # the oracle's pool never runs out
    r = streaming_min_radius(f.options)
    f.set_streaming(r, 100000)
    peak = 0
    for k, (bgr, depth, pose) in enumerate(frames):
        step(f, o, bgr, depth, pose, f"frame {k}")
        peak = max(peak, f.streaming_stats()["resident"])
    want = o.export_blocks()
    assert len(want) > opt["num_blocks"]
    assert_same_blocks(f.export_all_blocks(), want, "whole map")
    st = f.streaming_stats()
    assert st["streamed_out"] > 0 and st["streamed_in"] > 0, st
    assert st["resident"] + st["host"] == len(want) and peak <= opt["num_blocks"]
    f.close()


def test_blocks_in_the_overflow_table():
    """Blocks with |coordinate| >= 256 live in the open-addressing table: evicting them must not leave keys behind (a key
    whose value is -1 reads as "already allocated" forever), and evicting grid blocks while the table holds blocks moves
    table blocks in the pool.  The scene of test_fusion_gpu.py::test_blocks_outside_the_dense_grid straddles the border."""
    from synth import scene
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, streaming_min_radius
    H, W, vs = 96, 128, 0.02
    sc = scene.make_scans(4, H, W, seed=6)
    opt = options(sc, H, W, vs)
    S = np.eye(4, dtype=np.float32)
    c, s = np.cos(1.45), np.sin(1.45)
    S[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    S[:3, 3] = (40.2, 0.3, -0.2)
    scans = shifted(sc["scans"], S)
    f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**opt)
    f.set_streaming(streaming_min_radius(f.options))
    border = 256 * 8 * vs  # origin of the first block outside the dense grid along +x
    for i in range(2):
        step(f, o, *scans[i], f"scan {i}")
    xs = [k[0] for k in f.export_blocks()]
    assert min(xs) < 256 <= max(xs)
    f.stream_out_region((border - 1e-3, -1e4, -1e4), ALL_HI)          # every table block
    assert max(k[0] for k in f.export_blocks()) < 256 and min(k[0] for k in f.export_host_blocks()) >= 256
    assert_same_blocks(f.export_all_blocks(), o.export_blocks(), "table blocks out")
    step(f, o, *scans[2], "scan 2")                                   # brings them back, allocates more of them
    assert f.streaming_stats()["host"] == 0
    f.stream_out_region(ALL_LO, (border - 0.5 * vs * 8, 1e4, 1e4))    # grid blocks out while the table is full
    assert min(k[0] for k in f.export_blocks()) >= 256
    assert_same_blocks(f.export_all_blocks(), o.export_blocks(), "grid blocks out")
    f.stream_in_region(ALL_LO, ALL_HI)
    assert_same_blocks(f.export_blocks(), o.export_blocks(), "all back")
    od = step(f, o, *scans[3], "scan 3")
    assert (od > 0).mean() > 0.3
    assert_same_blocks(f.export_all_blocks(), o.export_blocks(), "final")
    f.close()


def two_places(n_far):
    """Scan 0 of the scene at the origin, then n_far scans of it 20 m along +x: the first place is evicted automatically."""
    from synth import scene
    H, W = 96, 128
    sc = scene.make_scans(max(n_far, 1), H, W, seed=3)
    S = np.eye(4, dtype=np.float32)
    S[:3, 3] = (20.0, 0.0, 0.0)
    return sc, [sc["scans"][0]] + shifted(sc["scans"][:n_far], S), options(sc, H, W, 0.02, max_sensor_depth=6.0)


def count_blocks(opt, scans):
    from oracle.tsdf_oracle import TsdfOracle
    o, n = TsdfOracle(**opt), []
    for bgr, depth, pose in scans:
        o.integrate(bgr, depth, pose)
        n.append(len(o.export_blocks()))
    return n


def test_errors_leave_the_state_unchanged():
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, streaming_min_radius
    sc, scans, opt = two_places(4)
    n1 = count_blocks(opt, scans[:1])[0]
    n2 = count_blocks(opt, scans[1:])
    pool = max(n1 + n2[0], n2[-1])
    assert n1 + n2[-1] > pool, (n1, n2)
    opt.update(num_blocks=pool, num_buckets=pool)
    f = DrFusion(DrFusionOptions(**opt))
    r = streaming_min_radius(f.options)
    with pytest.raises(_lib.DrError) as e:
        f.set_streaming(0.99 * r)
    assert e.value.code == 1
    f.set_streaming(r)
    for bgr, depth, pose in scans:
        f.IntegrateScanAsync(bgr, depth, pose)
        f.RenderAsync([pose])
        f.GetRenderResult()
    st = f.streaming_stats()
    assert st["host"] == n1 and st["resident"] == n2[-1], (st, n1, n2)
    res, host = f.export_blocks(), f.export_host_blocks()
    with pytest.raises(_lib.DrError) as e:                            # does not fit: nothing moves
        f.stream_in_region(ALL_LO, ALL_HI)
    assert e.value.code == 5
    assert f.streaming_stats() == st
    assert_same_blocks(f.export_blocks(), res, "resident after the refused stream-in")
    assert_same_blocks(f.export_host_blocks(), host, "host after the refused stream-in")
    for radius in (0.0, 2 * r):                                       # the store holds blocks: the mode stays
        with pytest.raises(_lib.DrError) as e:
            f.set_streaming(radius)
        assert e.value.code == 2
    with pytest.raises(_lib.DrError) as e:
        f.bench_integrate([scans[0][0]], [scans[0][1]], [scans[0][2]])
    assert e.value.code == 6
    with pytest.raises(_lib.DrError) as e:
        f.bench_sequence(0, 0, np.eye(4, dtype=np.float32)[None])
    assert e.value.code == 6
    f.close()
    # streaming off with blocks in the host store: integrating would allocate fresh blocks over stored ones
    g = DrFusion(DrFusionOptions(**opt))
    g.IntegrateScanAsync(*scans[0])
    g.RenderAsync([scans[0][2]])
    g.GetRenderResult()
    g.stream_out_region(ALL_LO, ALL_HI)
    with pytest.raises(_lib.DrError) as e:
        g.IntegrateScanAsync(*scans[0])
    assert e.value.code == 2
    assert g._L.drf_stream_out_region(g._h, None, None) == 1 and g._L.drf_stream_in_region(g._h, None, None) == 1
    g.close()


def test_mesh_of_the_whole_map_after_bringing_it_back():
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, streaming_min_radius
    sc, scans, opt = two_places(2)
    f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**opt)
    f.set_streaming(streaming_min_radius(f.options))
    for i, s in enumerate(scans):
        step(f, o, *s, f"scan {i}")
    assert f.streaming_stats()["host"] > 0
    f.stream_in_region(ALL_LO, ALL_HI)
    assert_same_blocks(f.export_blocks(), o.export_blocks(), "all back")
    lo, hi = (-3.0, -3.0, -1.0), (23.0, 3.0, 7.0)
    want = o.extract_mesh(lo, hi)
    assert len(want[0]) > 1000
    gv, gc = f.GetMesh(lo, hi)
    assert gv.shape == want[0].shape
    assert np.array_equal(canon(gv, gc), canon(*want))
    f.close()
