"""-m gpu: drf_merge_map.  The reference of every comparison is the numpy restatement of the rule in tests/test_map_merge.py
(np_merge_voxels / np_merge_maps) applied to what the engine exported and what the file holds: the merged map bit for bit, the
slot order, the six merge counters, continuation against an engine that loaded the merged map, independence of pool size, host
store and chunk size, every refusal leaving the engine as it was.  96x128 scans at voxel_size 0.02, synth.scene seed 11.
DESIGN.md §7c "Merging a map file"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fusion_helpers import ROOT, assert_same_mesh, box_of, feed, options, places, shifted, unbounded
from test_fusion_map_file_gpu import code_of, engine, file_blocks, render, same_image
from test_fusion_streaming_gpu import assert_same_blocks
from test_map_file import compose, pack
from test_map_merge import np_merge_maps

pytestmark = pytest.mark.gpu
H, W, VS = 96, 128, 0.02
MAXW = 64


def compose_map(blocks):
    """The bytes of the map file that holds {coord: 4096 bytes}."""
    keys = sorted(pack(c) for c in blocks)
    by_key = {pack(c): v for c, v in blocks.items()}
    vox = np.stack([by_key[k] for k in keys]) if keys else np.zeros((0, 4096), np.uint8)
    return compose(np.float32(VS), keys, vox)


def saved(f, path):
    f.save_map(path)
    return open(path, "rb").read()


def stats_of(st):
    """merge_stats() of a merge in which every combined block is resident, from np_merge_maps' counts."""
    return (st["file"], st["added"], st["combined"], 0, st["verbatim"], st["averaged"])


def weights(blocks):
    return np.stack(list(blocks.values())).reshape(-1, 8)[:, 7]


@pytest.fixture(scope="module")
def M(tmp_path_factory):
    """Map A = scans 0 and 1, map B = scans 2, 3 and 4 of synth.scene seed 11, each saved by an unbounded engine (FA, FB);
    want = the numpy merge of B's file into A, st its counts, merged = the file that holds it."""
    from synth import scene
    sc = scene.make_scans(5, H, W, seed=11)
    opt = options(sc, H, W, VS)
    d = tmp_path_factory.mktemp("merge")
    out = dict(scans=sc["scans"], opt=opt, dir=d)
    for name, idx in (("A", (0, 1)), ("B", (2, 3, 4))):
        U = engine(unbounded(opt))
        for i in idx:
            feed(U, *sc["scans"][i])
        out["F" + name] = str(d / (name + ".drfmap"))
        U.save_map(out["F" + name])
        out[name], _ = file_blocks(out["F" + name])
        assert_same_blocks(out[name], U.export_blocks(), name)
        U.close()
    out["want"], out["st"] = np_merge_maps(out["A"], out["B"], MAXW)
    st = out["st"]
    print("A %d blocks, B %d; shared %d, only A %d, only B %d; case 3 %d, case 2 %d, case 1 %d; weights up to %d" % (
        len(out["A"]), len(out["B"]), st["combined"], len(out["A"]) - st["combined"], st["added"], st["averaged"], st["verbatim"], st["unchanged"],
        max(weights(out["A"]).max(), weights(out["B"]).max())))
    assert min(st["added"], st["combined"], len(out["A"]) - st["combined"], st["averaged"], st["verbatim"], st["unchanged"]) > 0, st
    # what the CPU oracle gives for these scans: every class of block and voxel is populated
    assert (len(out["A"]), len(out["B"]), st["combined"], st["added"], st["averaged"], st["verbatim"]) == (2120, 2170, 1546, 624, 444401, 120852)
    out["merged"] = compose_map(out["want"])
    out["FM"] = str(d / "merged.drfmap")
    open(out["FM"], "wb").write(out["merged"])
    return out


def engine_with_a(M, **kw):
    f = engine(M["opt"], **kw)
    for i in range(2):
        feed(f, *M["scans"][i])
    return f


# ------------------------------------------------------------------ 1
def test_against_the_restatement(M, tmp_path):
    f = engine_with_a(M)
    before, stats = f.export_blocks(), f.stats()
    assert_same_blocks(before, M["A"], "A")
    f.merge_map(M["FB"])
    got = f.export_blocks()
    assert_same_blocks(got, M["want"], "merged")
    added = sorted(pack(c) for c in M["B"] if c not in M["A"])
    assert [pack(c) for c in got] == [pack(c) for c in before] + added, "the old slots in their order, then the added keys ascending"
    assert f.merge_stats() == stats_of(M["st"])
    assert f.stats() == dict(stats, blocks=len(M["want"]))
    assert saved(f, str(tmp_path / "m.drfmap")) == M["merged"]
    f.close()


# ------------------------------------------------------------------ 2
def test_continuation_equals_an_engine_that_loaded_the_merged_map(M, tmp_path):
    from tandem_amd.dr_fusion import RENDER_MAP
    scans = M["scans"]
    g, l = engine_with_a(M), engine(M["opt"])
    g.merge_map(M["FB"])
    l.load_map(M["FM"])
    assert g.merge_stats()[1] > 0 and g.merge_stats()[2] > 0 and g.merge_stats()[5] > 0
    for f in (g, l):
        f.set_render_scope(RENDER_MAP)
    view = render(g, scans[2][2])  # legal before any scan because of the merge
    assert (view[1] > 0).mean() > 0.3
    same_image(view, render(l, scans[2][2]), "map-scope render before any scan")
    for i in (3, 4):
        views = []
        for f in (g, l):
            f.IntegrateScanAsync(*scans[i])
            views.append(render(f, scans[i][2]))
        same_image(views[0], views[1], f"ray-cast after scan {i}")
        sg, sl = g.stats(), l.stats()
        assert sg["updated_last"] == sl["updated_last"] > 0 and sg["blocks"] == sl["blocks"] and sg["mismatches"] == sl["mismatches"]
        assert_same_blocks(g.export_blocks(), l.export_blocks(), f"blocks after scan {i}")
    lo, hi = box_of(g.export_blocks(), VS)
    pg, pl = str(tmp_path / "g.obj"), str(tmp_path / "l.obj")
    g.SaveMeshToFile(pg, lo, hi)
    l.SaveMeshToFile(pl, lo, hi)
    assert os.path.getsize(pg) > 100000 and open(pg, "rb").read() == open(pl, "rb").read()
    g.close(), l.close()


# ------------------------------------------------------------------ 3
def test_symmetry_below_the_weight_cap(M, tmp_path):
    assert weights(M["A"]).max() <= MAXW and weights(M["B"]).max() <= MAXW, "the rule is symmetric only while no weight exceeds W"
    f = engine(M["opt"])
    for i in (2, 3, 4):
        feed(f, *M["scans"][i])
    f.merge_map(M["FA"])
    st = f.merge_stats()
    assert st[0] == len(M["A"]) and st[1] == len(M["A"]) - M["st"]["combined"] > 0 and st[2] == M["st"]["combined"] > 0 and st[5] == M["st"]["averaged"] > 0
    assert saved(f, str(tmp_path / "ba.drfmap")) == M["merged"]
    f.close()


# ------------------------------------------------------------------ 4
def test_an_empty_target_is_a_load(M, tmp_path):
    e, l = engine(M["opt"]), engine(M["opt"])
    e.merge_map(M["FB"])
    l.load_map(M["FB"])
    n = len(M["B"])
    assert e.merge_stats() == (n, n, 0, 0, 0, 0) and n > 0
    assert list(e.export_blocks()) == list(l.export_blocks())
    assert saved(e, str(tmp_path / "e.drfmap")) == saved(l, str(tmp_path / "l.drfmap")) == open(M["FB"], "rb").read()
    e.close(), l.close()


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("chunk", [0, 64, 5])
def test_chunk_size_does_not_change_the_result(M, tmp_path, chunk):
    """The target loaded from A's file: slot i holds the i-th key, so with 64 or 5 blocks per chunk the chunks mix added and
    combined blocks (the fixture asserts both classes and B's blocks interleave them in key order)."""
    f = engine(M["opt"])
    f.load_map(M["FA"], chunk)
    f.merge_map(M["FB"], chunk)
    assert f.merge_stats() == stats_of(M["st"]) and min(f.merge_stats()[1:3]) > 0
    assert saved(f, str(tmp_path / "c.drfmap")) == M["merged"]
    f.close()


# ------------------------------------------------------------------ 6
def test_pool_store_and_scope_independence(tmp_path):
    from tandem_amd.dr_fusion import MESH_MAP, streaming_min_radius
    (p0, p1), popt = places(2)
    target, extra = [p0[0], p1[0]], [p0[1], p1[1]]
    U = engine(unbounded(popt))
    for s in extra:
        feed(U, *s)
    F = str(tmp_path / "f.drfmap")
    U.save_map(F)
    U.close()
    fb, _ = file_blocks(F)
    V = engine(unbounded(popt))
    for s in target:
        feed(V, *s)
    ta = V.export_blocks()
    want, st = np_merge_maps(ta, fb, MAXW)
    T = engine(popt)                                                   # streaming: the pool holds the second place only
    T.set_streaming(streaming_min_radius(T.options))
    S = engine(popt, num_blocks=len(want) + 3, num_buckets=len(want) + 3)  # streaming off, a pool that just fits
    for s in target:
        feed(T, *s)
        feed(S, *s)
    before, order = T.streaming_stats(), list(T.export_blocks())
    assert before["host"] > 0 and before["resident"] > 0
    host = T.export_host_blocks()
    for f in (T, V, S):
        f.merge_map(F, 64)
    mt = T.merge_stats()
    assert mt[1] > 0 and mt[2] > 0 and mt[3] > 0
    assert mt[:2] == (st["file"], st["added"]) and mt[2] + mt[3] == st["combined"] and mt[4:] == (st["verbatim"], st["averaged"])
    assert mt[3] == sum(c in host for c in fb)
    assert V.merge_stats() == S.merge_stats() == stats_of(st)
    after = T.streaming_stats()
    assert list(T.export_blocks()) == order and after["resident"] == before["resident"] and after["host"] == before["host"] + mt[1]
    assert [after[k] for k in ("streamed_out", "streamed_in", "bytes_moved")] == [before[k] for k in ("streamed_out", "streamed_in", "bytes_moved")]
    assert_same_blocks(T.export_all_blocks(), want, "streaming engine against the restatement")
    files = [saved(f, str(tmp_path / f"{i}.drfmap")) for i, f in enumerate((T, V, S))]
    assert files[0] == files[1] == files[2] == compose_map(want)
    lo, hi = box_of(want, VS)
    meshes = []
    for f in (T, V, S):
        f.set_mesh_scope(MESH_MAP)
        meshes.append(f.GetMesh(lo, hi))
    assert len(meshes[0][0]) > 1000
    assert_same_mesh(meshes[0], meshes[1], "map-scope mesh, streaming against unbounded")
    assert_same_mesh(meshes[2], meshes[1], "map-scope mesh, tight pool against unbounded")
    views = []
    for f in (T, V):                                                   # the next scan brings in what the merge stored
        f.IntegrateScanAsync(*p1[1])
        views.append(render(f, p1[1][2]))
    same_image(views[0], views[1], "the next scan's ray-cast")
    assert T.stats()["updated_last"] == V.stats()["updated_last"] > 0
    assert_same_blocks(T.export_all_blocks(), V.export_blocks(), "after the next scan")
    T.close(), V.close(), S.close()


# ------------------------------------------------------------------ 7
def crafted_block(rng, w):
    v = np.empty((512, 8), np.uint8)
    scale = rng.choice(np.array([0.08, 1.0, 30.0], np.float32), 512)
    v[:, :4] = (rng.uniform(-1.0, 1.0, 512).astype(np.float32) * scale).view(np.uint8).reshape(512, 4)
    v[:, 4:7] = rng.integers(0, 256, (512, 3), dtype=np.uint8)
    v[:, 7] = w
    return v.reshape(4096)


@pytest.mark.parametrize("maxw", [64, 255])
def test_crafted_weights(tmp_path, maxw):
    """40 pairs of 3-block files, one block shared: 20 480 weight pairs drawn from 0..255 on both sides, each of 0, 1, W, W + 1
    (where a weight can hold it) and 255 forced on both sides against each other in every pair of files."""
    rng = np.random.default_rng(maxw)
    special = sorted({0, 1, maxw, min(maxw + 1, 255), 255})
    sa, sb = (np.array(g).reshape(-1) for g in np.meshgrid(special, special, indexing="ij"))
    shared, only_a, only_b = (0, 0, 0), (1, -2, 3), (-1, 0, 30)
    opt = dict(voxel_size=VS, num_buckets=8, bucket_size=10, num_blocks=8, block_size=8, max_sdf_weight=maxw, truncation_distance=4 * VS,
               max_sensor_depth=10.0, min_sensor_depth=0.1, num_render_streams=0, fx=100.0, fy=100.0, cx=3.5, cy=3.5, height=8, width=8)
    pa, pb = str(tmp_path / "a.drfmap"), str(tmp_path / "b.drfmap")
    pairs, seen = 0, np.zeros(4, np.int64)
    for _ in range(40):
        wa, wb = rng.integers(0, 256, 512), rng.integers(0, 256, 512)
        wa[:len(sa)], wb[:len(sb)] = sa, sb
        A = {shared: crafted_block(rng, wa), only_a: crafted_block(rng, rng.integers(0, 256, 512))}
        B = {shared: crafted_block(rng, wb), only_b: crafted_block(rng, rng.integers(0, 256, 512))}
        A[(5, 5, 5)] = crafted_block(rng, 0)  # the third block of each file: one that is all empty, and shared too
        B[(5, 5, 5)] = crafted_block(rng, rng.integers(0, 2, 512))
        open(pa, "wb").write(compose_map(A))
        open(pb, "wb").write(compose_map(B))
        want, st = np_merge_maps(A, B, maxw)
        f = engine(opt)
        f.load_map(pa)
        f.merge_map(pb)
        got = f.export_blocks()
        assert_same_blocks(got, want, "crafted")
        assert f.merge_stats() == (3, 1, 2, 0, st["verbatim"], st["averaged"])
        f.close()
        a8, g8 = np.stack([A[shared], A[(5, 5, 5)]]).reshape(-1, 8), np.stack([got[shared], got[(5, 5, 5)]]).reshape(-1, 8)
        b8 = np.stack([B[shared], B[(5, 5, 5)]]).reshape(-1, 8)
        untouched = b8[:, 7] == 0
        assert np.array_equal(g8[untouched], a8[untouched]), "a voxel of case 1 changed"
        assert (g8[~untouched, 7] <= maxw).all(), "a merged weight exceeds W"
        over = ~untouched & (a8[:, 7] > 0) & (a8[:, 7].astype(int) + b8[:, 7] > 255)
        assert over.any() and (g8[over, 7] == maxw).all(), "a weight sum above 255 wrapped"
        pairs += 512
        seen += np.bincount(np.where(untouched, 1, np.where(a8[:, 7] == 0, 2, 3)), minlength=4)
    assert pairs >= 20000 and seen[1:].min() > 0


# ------------------------------------------------------------------ 8
def snapshot(f, path):
    return saved(f, path), list(f.export_blocks()), f.stats(), f.mesh_update_stats(), f.merge_stats()


def test_refusals_leave_things_as_they_were(M, tmp_path):
    from tandem_amd.dr_fusion import streaming_min_radius
    scans, FB = M["scans"], M["FB"]
    p = str(tmp_path / "snap.drfmap")
    lo, hi = box_of(M["want"], VS)
    n_union, n_added = len(M["want"]), M["st"]["added"]
    data = open(FB, "rb").read()
    nb = len(M["B"])
    other_vs, cut, flipped = (str(tmp_path / n) for n in ("vs.drfmap", "cut.drfmap", "flip.drfmap"))
    keys = sorted(pack(c) for c in M["B"])
    by_key = {pack(c): v for c, v in M["B"].items()}
    open(other_vs, "wb").write(compose(np.float32(0.01), keys, np.stack([by_key[k] for k in keys])))
    open(cut, "wb").write(data[:len(data) - 4096 - 11])
    bad = bytearray(data)
    bad[64 + 8 * nb + 4096 * (nb // 2) + 77] ^= 0x04
    open(flipped, "wb").write(bytes(bad))

    f = engine_with_a(M)
    assert f.GetMeshUpdate(lo, hi)[0] is True and f.GetMeshUpdate(lo, hi)[0] is False  # a baseline no refusal may void
    snap = snapshot(f, p)
    assert code_of(f.merge_map, other_vs) == 1
    for path in (cut, flipped, str(tmp_path / "missing.drfmap")):
        assert code_of(f.merge_map, path) == 4, path
    assert f._L.drf_merge_map(f._h, None, 0) == 1
    assert snapshot(f, p) == snap
    f.IntegrateScanAsync(scans[1][0], np.zeros((H, W), np.float32), scans[1][2])  # no valid depth: changes no voxel
    assert code_of(f.merge_map, FB) == 2
    f.RenderAsync([scans[1][2]])
    assert code_of(f.merge_map, FB) == 2                              # between RenderAsync and GetRenderResult
    f.GetRenderResult()
    after = snapshot(f, p)
    assert after[:2] == snap[:2] and after[2]["updated_total"] == snap[2]["updated_total"] and after[4] == snap[4]
    f.close()

    g = engine_with_a(M, num_blocks=n_union - 1, num_buckets=n_union - 1)  # one block too many for the pool
    assert g.GetMeshUpdate(lo, hi)[0] is True
    snap = snapshot(g, p)
    assert code_of(g.merge_map, FB) == 5
    assert snapshot(g, p) == snap
    assert g.GetMeshUpdate(lo, hi)[0] is False, "the refused merge voided the mesh baseline"
    g.close()

    h = engine(M["opt"])                                               # ... and for the host store
    r = streaming_min_radius(h.options)
    h.set_streaming(r, n_added - 1)
    for i in range(2):
        feed(h, *scans[i])
    st = h.streaming_stats()
    assert st["host"] == 0, "both scans lie within the radius"
    snap = snapshot(h, p)
    assert code_of(h.merge_map, FB) == 5
    assert snapshot(h, p) == snap and h.streaming_stats() == st
    h.close()
    h = engine(M["opt"])                                               # exactly enough: the added blocks go to the store
    h.set_streaming(r, n_added)
    for i in range(2):
        feed(h, *scans[i])
    h.merge_map(FB)
    assert h.streaming_stats()["host"] == n_added and h.merge_stats() == stats_of(M["st"])
    assert saved(h, p) == M["merged"]
    h.close()


# ------------------------------------------------------------------ 9
def test_the_mesh_update_after_a_merge_is_full(M):
    from tandem_amd.dr_fusion import MeshPatches
    lo, hi = box_of(M["want"], VS)
    f = engine_with_a(M)
    consumer = MeshPatches()
    up = f.GetMeshUpdate(lo, hi)
    assert up[0] is True
    consumer.apply(up)
    assert f.GetMeshUpdate(lo, hi)[0] is False
    f.ExtractMeshAsync(lo, hi)                                        # a pending extraction describes the map before the merge
    f.merge_map(M["FB"])
    assert_same_mesh(f.GetMeshSync(), consumer.assemble(), "the extraction that was pending across the merge")
    f.ExtractMeshUpdateAsync(lo, hi)
    assert f.mesh_update_size()[2] is True, "the first mesh update after a merge is full"
    consumer.apply(f.GetMeshUpdateSync())
    full = f.GetMesh(lo, hi)
    assert len(full[0]) > 1000
    assert_same_mesh(consumer.assemble(), full, "the consumer after the full update")
    f.close()


# ------------------------------------------------------------------ 10
def test_blocks_in_the_overflow_table(tmp_path):
    from synth import scene
    sc = scene.make_scans(4, H, W, seed=6)
    opt = options(sc, H, W, VS)
    S = np.eye(4, dtype=np.float32)
    c, s = np.cos(1.45), np.sin(1.45)
    S[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    S[:3, 3] = (40.2, 0.3, -0.2)
    scans = shifted(sc["scans"], S)
    f = engine(opt)
    for i in range(2):
        feed(f, *scans[i])
    p = str(tmp_path / "t.drfmap")
    f.save_map(p, 64)
    f.close()
    fb, _ = file_blocks(p)
    outside = [k for k in fb if max(abs(v) if v >= 0 else -v - 1 for v in k) >= 256]
    assert outside and len(outside) < len(fb), "the file straddles the border of the dense grid"
    g = engine(opt)
    feed(g, *scans[3])
    ga = g.export_blocks()
    want1, st1 = np_merge_maps(ga, fb, MAXW)
    g.merge_map(p, 64)
    assert g.merge_stats() == stats_of(st1)
    assert any(k not in ga for k in outside), "no block outside the dense grid was added"
    assert_same_blocks(g.export_blocks(), want1, "first merge")
    want2, st2 = np_merge_maps(want1, fb, MAXW)
    g.merge_map(p, 5)
    assert g.merge_stats() == stats_of(st2) and st2["added"] == 0 and st2["combined"] == len(fb) and st2["averaged"] > 0
    assert_same_blocks(g.export_blocks(), want2, "second merge")
    m = str(tmp_path / "m.drfmap")
    open(m, "wb").write(compose_map(want2))
    l = engine(opt)
    l.load_map(m)
    same_image(render(g, scans[2][2]), render(l, scans[2][2]), "ray-cast across the border")
    views = []
    for e in (g, l):
        e.IntegrateScanAsync(*scans[2])
        views.append(render(e, scans[2][2]))
    same_image(views[0], views[1], "ray-cast after the next scan")
    assert (views[0][1] > 0).mean() > 0.3
    assert_same_blocks(g.export_blocks(), l.export_blocks(), "after the next scan")
    g.close(), l.close()


# ------------------------------------------------------------------ 11
def test_shim_merges(tmp_path):
    """tandem_amd/libdr/dr_fusion.h: MergeMapFromFile on a DrFusion that holds one scan, of the file a second DrFusion saved."""
    import __graft_entry__ as g
    if not os.path.isfile(os.path.join(ROOT, "tandem_amd", "libdr_mi355x.so")):
        g.build()
    exe = str(tmp_path / "map_merge_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tandem_amd", "libdr"), os.path.join(ROOT, "tests/cpp/map_merge_shim.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_merge_shim ok" in r.stdout
    a, b, m = (file_blocks(str(tmp_path / n))[0] for n in ("a.drfmap", "b.drfmap", "merged.drfmap"))
    want, st = np_merge_maps(b, a, MAXW)
    assert st["added"] > 0 and st["averaged"] > 0
    assert_same_blocks(m, want, "the shim's merged map")


# ------------------------------------------------------------------ 12
def test_merge_command(M, tmp_path):
    out = str(tmp_path / "out.drfmap")
    r = subprocess.run([sys.executable, "-m", "tandem_amd.map_file", "merge", out, M["FA"], M["FB"]], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(out, "rb").read() == M["merged"]
    assert "added %d" % M["st"]["added"] in r.stdout
