"""-m gpu: drf_transform_map.  The reference of every byte comparison is np_transform_map, the numpy restatement of the rule in
tests/test_map_transform.py, written to a file by tandem_amd.map_file.write; beside it a pure integer remapping for the lattice
motions and an analytic plane for the meaning of T.  96x128 engines with a pool of a few thousand blocks.
DESIGN.md §7c "Moving a map into another frame"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fusion_helpers import ROOT, assert_same_mesh, box_of, feed, places
from test_fusion_map_file_gpu import code_of, engine
from test_map_merge import np_merge_maps
from test_map_transform import B, as_dict, cluster, lattice_move, LATTICE, np_transform_map, random_blocks, rigid

pytestmark = pytest.mark.gpu
H, W, VS = 96, 128, 0.02
T37 = rigid((1, 2, 3), 37.0, (0.313, -1.07, 2.5))


def options(vs=VS, **kw):
    d = dict(voxel_size=vs, num_buckets=4000, bucket_size=10, num_blocks=4000, block_size=8, max_sdf_weight=64, truncation_distance=4 * vs,
             max_sensor_depth=10.0, min_sensor_depth=0.1, num_render_streams=1, fx=110.0, fy=110.0, cx=63.5, cy=47.5, height=H, width=W)
    d.update(kw)
    return d


def write(path, vs, coords, vox):
    from tandem_amd import map_file
    map_file.write(path, vs, np.asarray(coords, np.int64).reshape(-1, 3), np.asarray(vox, np.uint8).reshape(-1, 4096))
    return open(path, "rb").read()


def stats_of(st):
    """transform_stats()[2:5] from the restatement's counts."""
    return (st["blocks"], st["voxels"], st["refused"])


@pytest.fixture(scope="module")
def M(tmp_path_factory):
    """The source map of about 40 blocks, its file, and what the restatement makes of it under T37 (computed once)."""
    rng = np.random.default_rng(37)
    coords = cluster(-1, 1) + [(6, -5, 3), (300, 7, -2)] + [(3, 2, 0), (3, 2, 1), (3, 3, 1), (-4, 0, 2), (-4, 1, 2), (-5, 1, 2), (2, -3, -3), (2, -3, -4), (0, 3, 0), (0, 4, 0), (1, 4, 0)]
    assert len(set(coords)) == len(coords) == 40
    vox = random_blocks(rng, len(coords))
    w = vox.reshape(-1, 8)[:, 7]
    assert (w == 0).any() and (w == 1).any() and (w == 255).any()
    d = tmp_path_factory.mktemp("transform")
    src = str(d / "src.drfmap")
    write(src, VS, coords, vox)
    wc, wv, st = np_transform_map(coords, vox, T37, VS)
    print("source %d blocks -> %d blocks, %d voxels, %d refused" % (len(coords), st["blocks"], st["voxels"], st["refused"]))
    assert st["blocks"] > len(coords) and st["voxels"] > 0 and st["refused"] > 0
    want = write(str(d / "want.drfmap"), VS, wc, wv)
    return dict(dir=d, src=src, coords=coords, vox=vox, wc=wc, wv=wv, st=st, want=want)


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("chunk", [0, 5, 1])
def test_against_the_restatement(M, tmp_path, chunk):
    f = engine(options())
    out = str(tmp_path / "out.drfmap")
    f.transform_map(M["src"], T37, out, chunk)
    st = f.transform_stats()
    f.close()
    got = open(out, "rb").read()
    assert len(got) == len(M["want"]), f"{(len(got) - 72) // 4104} blocks against {M['st']['blocks']}"
    assert got == M["want"]
    assert st[2:5] == stats_of(M["st"]) and st[0] == len(M["coords"]) and st[1] >= st[2] and st[5] == 4104 * len(M["coords"])
    assert not os.path.exists(out + ".part")


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("name,P,shift", LATTICE, ids=[m[0] for m in LATTICE])
def test_lattice_motions(tmp_path, name, P, shift):
    """A signed permutation and a whole number of voxels at voxel_size 2^-6: every weighted voxel moves with its 8 bytes; the
    expectation is the integer remapping alone (test_map_transform.lattice_move), not the restatement."""
    from tandem_amd import map_file
    vs = 2.0 ** -6
    rng = np.random.default_rng(6)
    coords = cluster(-1, 0) + [(4, -3, 2), (-9, 0, 5)]
    vox = random_blocks(rng, len(coords))
    src, out = str(tmp_path / "src.drfmap"), str(tmp_path / "out.drfmap")
    write(src, vs, coords, vox)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = P
    T[:3, 3] = np.asarray(shift, np.float64) * vs
    f = engine(options(vs))
    f.transform_map(src, T, out)
    st = f.transform_stats()
    f.close()
    want = lattice_move(coords, vox, P, shift)
    _, gc, gv = map_file.read(out)
    got = as_dict(gc, gv)
    assert got.keys() == want.keys(), name
    assert all(np.array_equal(got[k], want[k]) for k in want), name
    nw = int((vox.reshape(-1, 8)[:, 7] > 0).sum())
    assert st[2:5] == (len(want), nw, 0) and nw > 0


# ------------------------------------------------------------------ 3
def test_a_plane_lands_where_the_motion_puts_it(tmp_path):
    """Meaning, not only self-consistency: the source holds sdf = n.p - d at every lattice point of 4x4x4 blocks (float64,
    rounded once), constant colour, weight 5.  Trilinear interpolation is exact on a linear field, so every weighted output voxel at
    p must hold n.(R^T (p - t)) - d up to the rounding of eight fp32 terms and of f (under 1e-6 of the largest value; the bound
    allows ten times that).  Catches R against R^T and the sign of t."""
    from tandem_amd import map_file
    n = np.array([0.36, -0.48, 0.8])
    d = 0.137
    coords = np.array(cluster(0, 3), np.int64) - 2
    off = np.stack([np.arange(512) >> 6, (np.arange(512) >> 3) & 7, np.arange(512) & 7], axis=1)
    p = (coords[:, None, :] * 8 + off[None]).astype(np.float64) * np.float64(np.float32(VS))
    vox = np.zeros((len(coords), 512, 8), np.uint8)
    vox[:, :, :4] = np.ascontiguousarray((p @ n - d).astype(np.float32)).view(np.uint8).reshape(len(coords), 512, 4)
    vox[:, :, 4:7] = (40, 130, 220)
    vox[:, :, 7] = 5
    T = rigid((-2, 1, 0.5), 71.0, (0.41, 0.23, -0.37))
    src, out = str(tmp_path / "src.drfmap"), str(tmp_path / "out.drfmap")
    write(src, VS, coords, vox)
    f = engine(options())
    f.transform_map(src, T, out)
    st = f.transform_stats()
    f.close()
    _, gc, gv = map_file.read(out)
    gv = gv.reshape(len(gc), 512, 8)
    weighted = gv[:, :, 7] > 0
    q = ((gc[:, None, :] * 8 + off[None]).astype(np.float64) * np.float64(np.float32(VS)))[weighted]
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    want = ((q - t) @ R) @ n - d  # rows of (q - t) @ R are R^T (q - t)
    got = np.ascontiguousarray(gv[weighted][:, :4]).view(np.float32)[:, 0].astype(np.float64)
    bound = 1e-5 * max(np.abs(want).max(), VS)
    err = np.abs(got - want).max()
    print("plane: %d weighted voxels, max |sdf - plane| %.3g, bound %.3g" % (weighted.sum(), err, bound))
    assert err <= bound
    assert (gv[weighted][:, 4:7] == (40, 130, 220)).all() and (gv[weighted][:, 7] == 5).all()
    _, _, rst = np_transform_map(coords, vox, T, VS)
    assert int(weighted.sum()) == rst["voxels"] == st[3] > 0


# ------------------------------------------------------------------ 4
def test_the_engine_is_untouched(M, tmp_path):
    from tandem_amd.dr_fusion import streaming_min_radius
    (p0, p1), popt = places(2)
    f = engine(popt, num_blocks=6000, num_buckets=6000)
    f.set_streaming(streaming_min_radius(f.options))
    for s in (p0[0], p0[1], p1[0], p1[1]):
        feed(f, *s)
    assert f.streaming_stats()["host"] > 0 and f.streaming_stats()["resident"] > 0
    a, b, out = (str(tmp_path / n) for n in ("a.drfmap", "b.drfmap", "out.drfmap"))
    snapshot = lambda: (f.stats(), f.streaming_stats(), f.mesh_update_stats(), f.merge_stats(), list(f.export_blocks()), sorted(f.export_host_blocks()))  # noqa: E731
    f.save_map(a)
    lo, hi = box_of(f.export_blocks(), 0.02)
    mesh = f.GetMesh(lo, hi)
    assert len(mesh[0]) > 1000
    before = snapshot()
    f.transform_map(M["src"], T37, out)
    assert open(out, "rb").read() == M["want"]
    assert snapshot() == before
    f.save_map(b)
    assert open(a, "rb").read() == open(b, "rb").read()
    f.ExtractMeshAsync(lo, hi)                                        # pending across the call
    f.transform_map(M["src"], T37, out, 7)
    assert open(out, "rb").read() == M["want"]
    assert_same_mesh(f.GetMeshSync(), mesh, "the extraction that was pending across the transform")
    feed(f, *p1[1])                                                   # and it goes on
    assert f.stats()["updated_last"] > 0
    f.close()


# ------------------------------------------------------------------ 5
def test_transform_then_merge(M, tmp_path):
    """Engine A holds a map that shares some blocks with the moved file and has some of its own; merge_map of the moved file
    must give np_merge_maps(A, np_transform_map(...))."""
    rng = np.random.default_rng(12)
    moved = as_dict(M["wc"], M["wv"])
    shared = list(moved)[::3]
    own = [(40, 40, 40), (41, 40, 40), (-60, 2, 9)]
    assert not any(c in moved for c in own)
    ac = shared + own
    av = random_blocks(rng, len(ac))
    av.reshape(-1, 8)[:, 7] = np.minimum(av.reshape(-1, 8)[:, 7], 64)  # a map an engine with max_sdf_weight 64 can hold
    A = as_dict(np.array(ac), av)
    pa, out, pm = (str(tmp_path / n) for n in ("a.drfmap", "moved.drfmap", "merged.drfmap"))
    write(pa, VS, ac, av)
    f = engine(options())
    f.load_map(pa)
    f.transform_map(M["src"], T37, out)
    f.merge_map(out)
    want, st = np_merge_maps(A, moved, 64)
    assert st["combined"] == len(shared) > 0 and st["added"] > 0 and st["averaged"] > 0
    assert f.merge_stats() == (len(moved), st["added"], st["combined"], 0, st["verbatim"], st["averaged"])
    f.save_map(pm)
    f.close()
    wc = np.array(list(want), np.int64)
    assert open(pm, "rb").read() == write(str(tmp_path / "want.drfmap"), VS, wc, np.stack([want[tuple(c)] for c in wc]))


# ------------------------------------------------------------------ 6
def test_refusals(M, tmp_path):
    from tandem_amd import map_file
    f = engine(options())
    src = M["src"]
    out = str(tmp_path / "out.drfmap")
    gone = lambda: not os.path.exists(out) and not os.path.exists(out + ".part")  # noqa: E731
    T = np.ascontiguousarray(T37)
    Tp = T.ctypes.data_as(f._L.drf_transform_map.argtypes[2])
    raw = lambda s, t, d: f._L.drf_transform_map(f._h, s, t, d, 0)  # noqa: E731
    # DR_ERR_ARG: null arguments, one path twice, what is no rigid motion, another voxel_size, a block leaving the key range
    assert raw(None, Tp, os.fsencode(out)) == 1 and raw(os.fsencode(src), None, os.fsencode(out)) == 1 and raw(os.fsencode(src), Tp, None) == 1
    assert f._L.drf_transform_stats(f._h, None) == 1
    assert code_of(f.transform_map, src, T37, src) == 1
    scaled, nan, row, mirror, sheared = (T37.copy() for _ in range(5))
    scaled[:3, :3] *= 1.01
    nan[2, 3] = np.nan
    row[3, 3] = 1.0 + 2.0 ** -20
    mirror[:3, 1] *= -1
    sheared[0, 1] += 0.01
    for bad in (scaled, nan, row, mirror, sheared):
        assert code_of(f.transform_map, src, bad, out) == 1
    other = str(tmp_path / "other_vs.drfmap")
    write(other, 0.01, M["coords"], M["vox"])
    assert code_of(f.transform_map, other, T37, out) == 1
    edge = str(tmp_path / "edge.drfmap")
    write(edge, VS, [(B - 2, 0, 0), (0, 0, 0)], M["vox"][:2])
    push = np.eye(4, dtype=np.float32)
    push[0, 3] = 100 * VS
    assert code_of(f.transform_map, edge, push, out) == 1
    assert gone()
    # DR_ERR_IO: a source that fails the validation, one that is not there, a destination that cannot be created
    data = open(src, "rb").read()
    flipped, cut = str(tmp_path / "flip.drfmap"), str(tmp_path / "cut.drfmap")
    bad = bytearray(data)
    bad[64 + 8 * 40 + 4096 * 20 + 77] ^= 0x04
    open(flipped, "wb").write(bytes(bad))
    open(cut, "wb").write(data[:-4107])
    for path in (flipped, cut, str(tmp_path / "missing.drfmap")):
        assert code_of(f.transform_map, path, T37, out) == 4, path
        assert gone()
    nowhere = str(tmp_path / "no_such_directory" / "out.drfmap")
    assert code_of(f.transform_map, src, T37, nowhere) == 4
    assert "no_such_directory" in f._L.dr_last_error().decode() and not os.path.exists(nowhere + ".part")
    # DR_ERR_PROTOCOL: where a scan may not be integrated
    bgr, depth, pose = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.float32), np.eye(4, dtype=np.float32)
    f.IntegrateScanAsync(bgr, depth, pose)
    assert code_of(f.transform_map, src, T37, out) == 2
    f.RenderAsync([pose])
    assert code_of(f.transform_map, src, T37, out) == 2               # between RenderAsync and GetRenderResult
    f.GetRenderResult()
    assert gone()
    # an empty source, and one without a weighted voxel, give the 72 bytes of an empty map
    empty, hollow = str(tmp_path / "empty.drfmap"), str(tmp_path / "hollow.drfmap")
    write(empty, VS, np.zeros((0, 3), np.int64), np.zeros((0, 4096), np.uint8))
    weightless = M["vox"][:3].copy()
    weightless.reshape(-1, 8)[:, 7] = 0
    write(hollow, VS, [(0, 0, 0), (0, 0, 1), (7, 7, 7)], weightless)
    for path, nsrc in ((empty, 0), (hollow, 3)):
        f.transform_map(path, T37, out)
        assert os.path.getsize(out) == 72 and map_file.info(out)["blocks"] == 0
        st = f.transform_stats()
        assert st[0] == nsrc and st[2:5] == (0, 0, 0)
        os.remove(out)
    # after all of it the engine does what it did in test 1
    f.transform_map(src, T37, out)
    assert open(out, "rb").read() == M["want"] and f.transform_stats()[2:5] == stats_of(M["st"])
    f.close()


def test_a_source_that_does_not_fit_on_the_device(M, tmp_path, monkeypatch, parity_hooks):
    """DR_ERR_CAPACITY.  No test can fill an MI355X, so the parity build (the same sources) reads a lower limit for the same
    comparison: one block less than the source's 40, then exactly what the call takes."""
    out = str(tmp_path / "out.drfmap")
    monkeypatch.setenv("DR_TRANSFORM_MAX_BYTES", str(39 * 4104))
    f = engine(options())
    assert code_of(f.transform_map, M["src"], T37, out) == 5
    assert "device memory" in f._L.dr_last_error().decode()
    assert not os.path.exists(out) and not os.path.exists(out + ".part")
    monkeypatch.delenv("DR_TRANSFORM_MAX_BYTES")
    f.transform_map(M["src"], T37, out)                               # without the limit: the candidate count the exact limit needs
    ncand = f.transform_stats()[1]
    os.remove(out)
    monkeypatch.setenv("DR_TRANSFORM_MAX_BYTES", str(40 * 4104 + 20 * ncand + 16 - 1))
    assert code_of(f.transform_map, M["src"], T37, out) == 5
    monkeypatch.setenv("DR_TRANSFORM_MAX_BYTES", str(40 * 4104 + 20 * ncand + 16))
    f.transform_map(M["src"], T37, out)
    assert open(out, "rb").read() == M["want"]
    f.close()


# ------------------------------------------------------------------ 7
def test_shim_transforms(tmp_path):
    """tandem_amd/libdr/dr_fusion.h: TransformMapFile of the file a DrFusion saved, held to the restatement."""
    import __graft_entry__ as g
    from tandem_amd import map_file
    if not os.path.isfile(os.path.join(ROOT, "tandem_amd", "libdr_mi355x.so")):
        g.build()
    exe = str(tmp_path / "map_transform_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tandem_amd", "libdr"), os.path.join(ROOT, "tests/cpp/map_transform_shim.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_transform_shim ok" in r.stdout
    vs, ac, av = map_file.read(str(tmp_path / "a.drfmap"))
    T = np.loadtxt(str(tmp_path / "T.txt"), dtype=np.float32).reshape(4, 4)
    wc, wv, st = np_transform_map(ac, av, T, vs)
    assert st["voxels"] > 10000
    assert open(str(tmp_path / "b.drfmap"), "rb").read() == write(str(tmp_path / "want.drfmap"), vs, wc, wv)


def test_transform_command(M, tmp_path):
    out = str(tmp_path / "out.drfmap")
    r = subprocess.run([sys.executable, "-m", "tandem_amd.map_file", "transform", M["src"], out, "--pose"] + [repr(float(v)) for v in T37.reshape(16)],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(out, "rb").read() == M["want"]
    assert "written %d" % M["st"]["blocks"] in r.stdout
