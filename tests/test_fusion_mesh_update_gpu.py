"""-m gpu: incremental mesh updates (drf_extract_mesh_update_async / drf_get_mesh_update_sync).  The reference is the same
engine's full extraction (ExtractMeshAsync + GetMeshSync) over the same box at the same moment -- and, in map scope, an
unbounded engine fed the same scans, which tests/test_fusion_map_mesh_gpu.py ties to the CPU oracle: the patches, kept in a
MeshPatches store and assembled in packed-key order, must equal it byte for byte, triangle order included.
DESIGN.md §7c "Incremental mesh".  Scenes as in tests/test_fusion_map_mesh_gpu.py, helpers from tests/fusion_helpers.py."""
import numpy as np
import pytest

import fusion_helpers
from fusion_helpers import assert_same_mesh, box_of, feed, options, places, shifted, unbounded

pytestmark = pytest.mark.gpu

ROOM_LO, ROOM_HI = (-3.6, -2.6, -2.1), (3.6, 2.6, 2.1)  # synth.room is a 6 x 4 x 3 m box around the origin


def assert_box_holds(blocks, vs, lo, hi):
    c = np.array(list(blocks), np.int64)
    assert (c.min(0) * 8 * vs > np.array(lo) + 2 * vs).all() and ((c.max(0) + 1) * 8 * vs < np.array(hi) - 2 * vs).all(), "the fixed box does not hold the map"


@pytest.fixture(scope="module")
def room_frames():
    return fusion_helpers.room_frames()


def check_update(upd, patches, want, what, full=None):
    """Apply one update to the consumer's store and compare the assembly with the full extraction `want`."""
    is_full, coords, first, vert, cols = upd
    if full is not None:
        assert is_full == full, f"{what}: full = {is_full}"
    assert len(first) == len(coords) + 1 and int(first[-1]) * 3 == len(vert) == len(cols), what
    assert np.all(np.diff(first.astype(np.int64)) >= 0), what
    from tandem_amd.dr_fusion import pack_block_key
    keys = pack_block_key(coords.astype(np.int64))
    assert np.all(np.diff(keys) > 0), f"{what}: patches are not in ascending packed-key order"
    patches.apply(upd)
    assert_same_mesh(patches.assemble(), want, what)


def test_room_loop_updates_assemble_to_the_full_mesh(room_frames):
    """60 frames, an update every 3: the assembly equals GetMesh(box) at every update; the first update is full, the later
    ones are not, and together they mesh strictly fewer blocks than their scopes hold (the frustum is narrower than the room)."""
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MeshPatches
    fr, frames, H, W = room_frames
    f = DrFusion(DrFusionOptions(**options(fr, H, W, 0.02)))
    m = MeshPatches()
    scope = meshed = 0
    for k, s in enumerate(frames):
        feed(f, *s)
        if k % 3 != 2:
            continue
        upd = f.GetMeshUpdate(ROOM_LO, ROOM_HI)
        st = f.mesh_update_stats()
        assert st["full"] == (k == 2) and st["scans"] == 3 and st["meshed"] == len(upd[1]), (k, st)
        assert st["scope"] == f.stats()["blocks"]
        check_update(upd, m, f.GetMesh(ROOM_LO, ROOM_HI), f"frame {k}", full=(k == 2))
        if k > 2:
            scope += st["scope"]
            meshed += st["meshed"]
    blocks = f.export_blocks()
    assert len(m.assemble()[0]) > 3 * 3000
    assert_box_holds(blocks, 0.02, ROOM_LO, ROOM_HI)
    print(f"room loop: {meshed} blocks meshed again of {scope} in scope over 19 updates")
    assert 0 < meshed < scope
    f.close()


def test_nothing_happened_lists_nothing_and_launches_no_mesh_pass():
    from synth import scene
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MeshPatches
    H, W = 96, 128
    sc = scene.make_scans(2, H, W, seed=1)
    f = DrFusion(DrFusionOptions(**options(sc, H, W, 0.02)))
    for s in sc["scans"]:
        feed(f, *s)
    lo, hi = (-2.0, -2.0, 0.0), (2.0, 2.0, 4.0)
    m = MeshPatches()
    check_update(f.GetMeshUpdate(lo, hi), m, f.GetMesh(lo, hi), "first", full=True)
    assert f.mesh_stats()[2] == 1 and f.mesh_stats()[0] == f.stats()["blocks"]
    assert len(m.assemble()[0]) > 3000
    f.ExtractMeshUpdateAsync(lo, hi)
    assert f.mesh_update_size() == (0, 0, False)
    assert f.mesh_stats() == (0, 0, 0), "blocks meshed / uploads / chunks of the last extraction: no mesh pass may have run"
    st = f.mesh_update_stats()
    assert st == dict(scope=f.stats()["blocks"], meshed=0, scans=0, full=False), st
    full, coords, first, vert, cols = upd = f.GetMeshUpdateSync()
    assert not full and coords.shape == (0, 3) and list(first) == [0] and vert.shape == (0, 3) and cols.shape == (0, 3)
    check_update(upd, m, f.GetMesh(lo, hi), "second")
    f.close()


def test_locality_rescanning_one_place_lists_no_block_of_the_other():
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MeshPatches
    pl, opt = places(2, spacing=20.0, max_sensor_depth=10.0)
    f = DrFusion(DrFusionOptions(**opt))
    for scans in pl:
        for s in scans:
            feed(f, *s)
    blocks = f.export_blocks()
    lo, hi = box_of(blocks, opt["voxel_size"])
    nb = sum(1 for k in blocks if k[0] * 8 * opt["voxel_size"] > 10.0)
    assert 0 < nb < len(blocks), "both places hold blocks"
    m = MeshPatches()
    check_update(f.GetMeshUpdate(lo, hi), m, f.GetMesh(lo, hi), "baseline over both places", full=True)
    feed(f, *pl[0][0])
    upd = f.GetMeshUpdate(lo, hi)
    assert len(upd[1]) > 0 and not upd[0]
    assert (upd[1][:, 0] * 8 * opt["voxel_size"] < 10.0).all(), "a block of place B is listed after re-scanning place A"
    check_update(upd, m, f.GetMesh(lo, hi), "after re-scanning place A", full=False)
    st = f.mesh_update_stats()
    assert st["scope"] == f.stats()["blocks"] and st["meshed"] <= st["scope"] - nb
    f.close()


def cull_margin(coords, pose, opt):
    """k_cull's test in float64 for block coordinates (n, 3): +1 where it holds with at least 2 px / 4 cm to spare, -1 where
    it fails by as much, 0 where a rounding could decide."""
    vs = opt["voxel_size"]
    Ti = np.linalg.inv(np.asarray(pose, np.float64).reshape(4, 4))
    pc = (coords.astype(np.float64) * 8 * vs) @ Ti[:3, :3].T + Ti[:3, 3]
    ce = pc + 4 * vs
    with np.errstate(divide="ignore", invalid="ignore"):
        px = opt["fx"] * ce[:, 0] / ce[:, 2] + opt["cx"]
        py = opt["fy"] * ce[:, 1] / ce[:, 2] + opt["cy"]
    W, H = opt["width"], opt["height"]
    inside = (pc[:, 2] > 0.04) & (px > 1.5) & (py > 1.5) & (px < W - 2.5) & (py < H - 2.5)
    outside = (pc[:, 2] > 0.04) & ((px < -2.5) | (py < -2.5) | (px > W + 1.5) | (py > H + 1.5))
    return inside.astype(int) - outside.astype(int)


def test_neighbour_dependence_lists_the_untouched_block_across_the_face():
    """Three scans from different poses, then the first pose again.  Its visible set ends inside the mapped surface: block N
    fails k_cull's test for that pose (so no voxel of it is written -- checked on the exported voxels) while the block V that
    shares a face with it passes.  N's cells next to that face read V's voxels, so the update must list N although N itself is
    untouched; N = the first such block, in key order, that has triangles of its own."""
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MeshPatches, pack_block_key
    pl, opt = places(1, scans_per_place=3, seed=5)
    f = DrFusion(DrFusionOptions(**opt))
    for s in pl[0]:
        feed(f, *s)
    before = f.export_blocks()
    lo, hi = box_of(before, opt["voxel_size"])
    m = MeshPatches()
    check_update(f.GetMeshUpdate(lo, hi), m, f.GetMesh(lo, hi), "baseline", full=True)
    scan = pl[0][0]
    coords = np.array(sorted(before, key=lambda k: int(pack_block_key(np.array(k)))), np.int64)
    margin = dict(zip(map(tuple, coords), cull_margin(coords, scan[2], opt)))
    faces = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    N = V = None
    for c in map(tuple, coords):
        if margin[c] != -1 or c not in m.blocks:
            continue
        for d in faces:
            v = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
            if margin.get(v) == 1 and v in m.blocks:
                N, V = c, v
                break
        if N:
            break
    assert N is not None, "the scene holds no meshed block outside the frustum with a meshed face neighbour inside it"
    feed(f, *scan)
    after = f.export_blocks()
    assert np.array_equal(after[N], before[N]), f"block {N} was written by the scan"
    assert not np.array_equal(after[V], before[V]), f"block {V} was not written by the scan"
    upd = f.GetMeshUpdate(lo, hi)
    listed = set(map(tuple, upd[1].tolist()))
    assert V in listed, f"the visible block {V} is not listed"
    assert N in listed, f"the untouched block {N} across the face of {V} is not listed"
    assert f.mesh_update_stats()["meshed"] < f.mesh_update_stats()["scope"]
    old = {k: (v.copy(), c.copy()) for k, (v, c) in m.blocks.items()}
    check_update(upd, m, f.GetMesh(lo, hi), "after the scan", full=False)
    changed = [k for k in listed if (k in m.blocks) != (k in old) or (k in old and not np.array_equal(m.blocks[k][0], old[k][0]))]
    assert changed, "the scan changed no listed block's triangles"
    f.close()


def test_full_again_after_another_box_a_reset_and_too_many_scans():
    from synth import scene
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MeshPatches, MESH_UPDATE_MAX_SCANS
    H, W = 96, 128
    sc = scene.make_scans(4, H, W, seed=1)
    f = DrFusion(DrFusionOptions(**options(sc, H, W, 0.02)))
    for s in sc["scans"][:2]:
        feed(f, *s)
    lo, hi = (-2.0, -2.0, 0.0), (2.0, 2.0, 4.0)
    lo2 = (-2.0, -2.0, 0.01)
    m = MeshPatches()
    check_update(f.GetMeshUpdate(lo, hi), m, f.GetMesh(lo, hi), "first", full=True)
    nblk = f.stats()["blocks"]
    feed(f, *sc["scans"][2])
    check_update(f.GetMeshUpdate(lo, hi), m, f.GetMesh(lo, hi), "same box", full=False)
    # another box: every block again, on a lattice that differs
    feed(f, *sc["scans"][3])
    upd = f.GetMeshUpdate(lo2, hi)
    assert len(upd[1]) == f.stats()["blocks"] >= nblk
    check_update(upd, m, f.GetMesh(lo2, hi), "another box", full=True)
    assert not np.array_equal(m.assemble()[0], f.GetMesh(lo, hi)[0])
    check_update(f.GetMeshUpdate(lo2, hi), m, f.GetMesh(lo2, hi), "the new box is the baseline now", full=False)
    # reset
    f.mesh_update_reset()
    upd = f.GetMeshUpdate(lo2, hi)
    assert len(upd[1]) == f.stats()["blocks"] and f.mesh_update_stats()["full"]
    check_update(upd, m, f.GetMesh(lo2, hi), "after mesh_update_reset", full=True)
    # exactly the number of scans the engine records: still incremental
    for k in range(MESH_UPDATE_MAX_SCANS):
        feed(f, *sc["scans"][k % 4])
    upd = f.GetMeshUpdate(lo2, hi)
    assert f.mesh_update_stats()["scans"] == MESH_UPDATE_MAX_SCANS
    check_update(upd, m, f.GetMesh(lo2, hi), "MAX_SCANS scans", full=False)
    # one more than that
    for k in range(MESH_UPDATE_MAX_SCANS + 1):
        feed(f, *sc["scans"][k % 4])
    upd = f.GetMeshUpdate(lo2, hi)
    assert len(upd[1]) == f.stats()["blocks"]
    check_update(upd, m, f.GetMesh(lo2, hi), "MAX_SCANS + 1 scans", full=True)
    feed(f, *sc["scans"][0])
    check_update(f.GetMeshUpdate(lo2, hi), m, f.GetMesh(lo2, hi), "and incremental again", full=False)
    f.close()


def streaming_room_loop(room_frames, S):
    """The bounded-pool room loop of the map-mesh tests (a pool of ~70 % of the map, streaming at the minimum radius) in
    DRF_MESH_MAP, an update every 3 frames against the unbounded engine's full mesh."""
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MeshPatches, MESH_MAP, MESH_RESIDENT, streaming_min_radius
    fr, frames, H, W = room_frames
    opt = options(fr, H, W, 0.02, max_sensor_depth=2.0, num_blocks=5600, num_buckets=5600)
    f, u = DrFusion(DrFusionOptions(**opt)), DrFusion(DrFusionOptions(**unbounded(opt)))
    f.set_streaming(streaming_min_radius(f.options), 100000)
    f.set_mesh_scope(MESH_MAP)
    lo = tuple(float(a + b) for a, b in zip(ROOM_LO, S[:3, 3]))
    hi = tuple(float(a + b) for a, b in zip(ROOM_HI, S[:3, 3]))
    m = MeshPatches()
    with_store = scope = meshed = 0
    for k, s in enumerate(shifted(frames, S)):
        feed(f, *s)
        feed(u, *s)
        if k % 3 != 2:
            continue
        probe = k == 56  # late in the loop: the store is populated
        if probe:
            st, all_blocks, pool = f.streaming_stats(), f.export_all_blocks(), f.export_blocks()
            assert st["host"] > 0
            f.set_mesh_scope(MESH_RESIDENT)
            with pytest.raises(_lib.DrError) as e:
                f.ExtractMeshUpdateAsync(lo, hi)
            assert e.value.code == 2, "DRF_MESH_RESIDENT with a non-empty host store must be DR_ERR_PROTOCOL"
            f.set_mesh_scope(MESH_MAP)
        upd = f.GetMeshUpdate(lo, hi)
        us = f.mesh_update_stats()
        if probe:
            assert f.streaming_stats() == st
            after = f.export_blocks()
            assert list(after.keys()) == list(pool.keys()), "the pool's slot order changed"
            a2 = f.export_all_blocks()
            assert a2.keys() == all_blocks.keys() and all(np.array_equal(a2[q], all_blocks[q]) for q in a2)
        check_update(upd, m, u.GetMesh(lo, hi), f"frame {k}", full=(k == 2))
        if f.streaming_stats()["host"] > 0 and k > 2:
            with_store += 1
            scope += us["scope"]
            meshed += us["meshed"]
            assert us["scope"] == f.streaming_stats()["resident"] + f.streaming_stats()["host"]
    st = f.streaming_stats()
    blocks = u.export_blocks()
    assert len(blocks) > opt["num_blocks"] and st["resident"] + st["host"] == len(blocks)
    assert st["streamed_out"] > 0 and st["streamed_in"] > 0, st
    assert with_store >= 5 and 0 < meshed < scope, (with_store, meshed, scope)
    assert len(m.assemble()[0]) > 3 * 3000
    assert_box_holds(blocks, 0.02, lo, hi)
    f.close(); u.close()
    return blocks


def test_streaming_room_loop_in_map_scope(room_frames):
    streaming_room_loop(room_frames, np.eye(4, dtype=np.float32))


def test_streaming_room_loop_in_the_overflow_table(room_frames):
    """The room moved beyond block coordinate 256 along x: every resident block lives in the open-addressing table."""
    S = np.eye(4, dtype=np.float32)
    S[:3, 3] = (50.0, 0.25, -0.5)
    blocks = streaming_room_loop(room_frames, S)
    assert min(k[0] for k in blocks) >= 256


def test_several_chunks_after_rescanning_two_far_apart_places():
    """Four places 20 m apart into a pool that holds about one of them (tests/test_fusion_map_mesh_gpu.py::many_places): the
    staging caps follow the pool, so the map needs several chunks.  After a baseline, places 0 and 2 are scanned again: the
    update lists blocks of those two only, runs more than one chunk, and the assembly is the unbounded engine's mesh."""
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MeshPatches, MESH_MAP, streaming_min_radius
    pl, opt = places(4)
    o1 = TsdfOracle(**unbounded(opt))
    for s in pl[0]:
        o1.integrate(*s)
    one = len(o1.export_blocks())
    opt.update(num_blocks=int(1.2 * one), num_buckets=int(1.2 * one))
    f, u = DrFusion(DrFusionOptions(**opt)), DrFusion(DrFusionOptions(**unbounded(opt)))
    f.set_streaming(streaming_min_radius(f.options))
    f.set_mesh_scope(MESH_MAP)
    for p, scans in enumerate(pl):
        for s in scans:
            feed(f, *s)
            feed(u, *s)
        if p + 1 < len(pl):
            f.stream_out_region((20.0 * p - 10.0, -1e4, -1e4), (20.0 * p + 10.0, 1e4, 1e4))
    blocks = u.export_blocks()
    assert len(blocks) > 3 * opt["num_blocks"]
    lo, hi = box_of(blocks, opt["voxel_size"])
    m = MeshPatches()
    check_update(f.GetMeshUpdate(lo, hi), m, u.GetMesh(lo, hi), "baseline", full=True)
    assert f.mesh_stats()[2] >= 3 and f.mesh_update_stats()["scope"] == len(blocks) == f.mesh_update_stats()["meshed"]
    for p in (0, 2):  # the pool holds about one place: what is resident leaves before another place comes back in
        f.stream_out_region((-1e4, -1e4, -1e4), (1e4, 1e4, 1e4))
        for s in pl[p]:
            feed(f, *s)
            feed(u, *s)
    st = f.streaming_stats()
    upd = f.GetMeshUpdate(lo, hi)
    assert f.streaming_stats() == st
    place = np.round(upd[1][:, 0] * 8 * opt["voxel_size"] / 20.0).astype(int)
    assert set(place.tolist()) == {0, 2}, f"places listed: {sorted(set(place.tolist()))}"
    meshed, uploaded, chunks = f.mesh_stats()
    assert chunks >= 2 and meshed == len(upd[1]) < len(blocks), f.mesh_stats()
    check_update(upd, m, u.GetMesh(lo, hi), "after re-scanning places 0 and 2", full=False)
    f.close(); u.close()


def test_protocol_and_capacity():
    import ctypes as C
    from synth import scene
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, MeshPatches
    H, W = 96, 128
    sc = scene.make_scans(4, H, W, seed=1)
    f = DrFusion(DrFusionOptions(**options(sc, H, W, 0.02)))
    for s in sc["scans"][:2]:
        feed(f, *s)
    lo, hi = (-2.0, -2.0, 0.0), (2.0, 2.0, 4.0)
    lo_a, hi_a = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
    L, h = f._L, f._h

    def code(fn, *a):
        with pytest.raises(_lib.DrError) as e:
            fn(*a)
        return e.value.code

    # nothing pending
    assert code(f.GetMeshUpdateSync) == 2 and code(f.mesh_update_size) == 2
    # null pointers
    assert L.drf_extract_mesh_update_async(h, None, hi_a) == 1 and L.drf_extract_mesh_update_async(h, lo_a, None) == 1
    assert L.drf_mesh_update_stats(h, None) == 1 and L.drf_mesh_update_size(h, None, None, None) == 1
    # not between IntegrateScanAsync and GetRenderResult
    f.IntegrateScanAsync(*sc["scans"][2])
    assert code(f.ExtractMeshUpdateAsync, lo, hi) == 2
    f.RenderAsync([sc["scans"][2][2]])
    f.GetRenderResult()
    # a pending update: wrong getter, double launch of either kind, scope change
    m = MeshPatches()
    f.ExtractMeshUpdateAsync(lo, hi)
    assert code(f.GetMeshSync) == 2 and code(f.mesh_num_triangles) == 2
    assert code(f.ExtractMeshUpdateAsync, lo, hi) == 2 and code(f.ExtractMeshAsync, lo, hi) == 2
    assert code(f.set_mesh_scope, 1) == 2
    nb, nt, full = f.mesh_update_size()
    assert full and nb == f.stats()["blocks"] and nt > 1000
    coords, first = np.empty((nb, 3), np.int32), np.zeros(nb + 1, np.uint64)
    vert, cols = np.empty((3 * nt, 3), np.float32), np.empty((3 * nt, 3), np.float32)
    n, num, fl = C.c_size_t(), C.c_size_t(), C.c_int()
    args = (C.byref(n), coords.ctypes.data_as(C.POINTER(C.c_int32)), first.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(num),
            _lib.fptr(vert), _lib.fptr(cols), C.byref(fl))
    assert L.drf_get_mesh_update_sync(h, nb, 3 * nt, None, *args[1:]) == 1
    # too small: DR_ERR_CAPACITY, the update stays pending
    assert L.drf_get_mesh_update_sync(h, nb - 1, 3 * nt, *args) == 5
    assert L.drf_get_mesh_update_sync(h, nb, 3 * nt - 1, *args) == 5
    assert f.mesh_update_size() == (nb, nt, True)
    check_update(f.GetMeshUpdateSync(), m, f.GetMesh(lo, hi), "first, after two refusals", full=True)
    # a pending full extraction: the update's getter is the wrong one
    f.ExtractMeshAsync(lo, hi)
    assert code(f.GetMeshUpdateSync) == 2 and code(f.mesh_update_size) == 2 and code(f.ExtractMeshUpdateAsync, lo, hi) == 2
    f.GetMeshSync()
    # an incremental update refused for room: the baseline does not advance, the retry returns the same patches
    feed(f, *sc["scans"][3])
    f.ExtractMeshUpdateAsync(lo, hi)
    nb2, nt2, full2 = f.mesh_update_size()
    assert not full2 and 0 < nb2 < f.stats()["blocks"]
    assert L.drf_get_mesh_update_sync(h, nb2 - 1, 3 * nt, *args) == 5
    assert L.drf_get_mesh_update_sync(h, nb, max(3 * nt2 - 3, 0), *args) == 5
    assert f.mesh_update_size() == (nb2, nt2, False)
    stats = f.mesh_update_stats()
    upd = f.GetMeshUpdateSync()
    assert (len(upd[1]), len(upd[3]) // 3, upd[0]) == (nb2, nt2, False) and f.mesh_update_stats() == stats
    # a full extraction (and a saved mesh's extraction path) between two updates does not disturb the second
    want = f.GetMesh(lo, hi)
    check_update(upd, m, want, "incremental, after two refusals", full=False)
    feed(f, *sc["scans"][0])
    mid = f.GetMesh((-1.0, -1.0, 0.5), (1.0, 1.0, 3.0))
    assert 0 < len(mid[0]) < len(want[0])
    upd = f.GetMeshUpdate(lo, hi)
    assert not upd[0] and 0 < len(upd[1]) < f.stats()["blocks"]
    check_update(upd, m, f.GetMesh(lo, hi), "after a full extraction over another box", full=False)
    f.close()
