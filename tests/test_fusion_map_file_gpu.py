"""-m gpu: drf_save_map / drf_load_map.  The file is parsed here by the restatement of tests/test_map_file.py; the loading
engine must go on exactly where the saving engine stood (blocks, ray-casts, update counts, meshes, all bit for bit against the
CPU oracle), the file must not depend on pool size, streaming history or chunk size, and every refusal must leave the engine
as it was.  96x128 scans at voxel_size 0.02.  DESIGN.md §7c "Saving and loading the map"."""
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import ROOT, assert_same_mesh, box_of, feed, options, places, shifted, step, unbounded
from test_fusion_streaming_gpu import ALL_HI, ALL_LO, assert_same_blocks
from test_map_file import pack, parse, unpack

pytestmark = pytest.mark.gpu
H, W, VS = 96, 128, 0.02


class Replay:
    """The oracle's recorded answers for scans[at:], behind the three calls fusion_helpers.step makes: one oracle run serves
    every engine of this file and stays unchanged."""

    def __init__(self, rec, at=0):
        self.rec, self.i = rec, at

    def integrate(self, bgr, depth, pose):
        assert np.array_equal(pose, self.rec[self.i]["pose"]), "replayed out of order"
        self.i += 1
        return 0

    def render(self, pose):
        assert np.array_equal(pose, self.rec[self.i - 1]["pose"])
        return self.rec[self.i - 1]["render"]

    def stats(self):
        return dict(updated_last=self.rec[self.i - 1]["updated_last"])

    def export_blocks(self):
        return self.rec[self.i - 1]["blocks"]


def record(opt, scans):
    from oracle.tsdf_oracle import TsdfOracle
    o, rec = TsdfOracle(**unbounded(opt)), []
    for bgr, depth, pose in scans:
        assert o.integrate(bgr, depth, pose) == 0
        rec.append(dict(pose=pose, render=o.render(pose), updated_last=o.stats()["updated_last"], blocks=o.export_blocks()))
    return rec


def engine(opt, **kw):
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions
    return DrFusion(DrFusionOptions(**dict(opt, **kw)))


def file_blocks(path):
    """{coord: 4096 bytes} and the keys of a map file, everything the format promises asserted (tests/test_map_file.py::parse)."""
    vs_bits, keys, vox, _ = parse(open(path, "rb").read())
    assert vs_bits == int(np.float32(VS).view(np.uint32))
    return {unpack(int(k)): vox[i] for i, k in enumerate(keys)}, [int(k) for k in keys]


def render(f, pose):
    f.RenderAsync([pose])
    rb, rd = f.GetRenderResult()
    return rb[0], rd[0]


def same_image(a, b, what):
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: depth differs at {(a[1] != b[1]).sum()} px"
    assert np.array_equal(a[0], b[0]), f"{what}: colour differs"


def code_of(call, *args):
    from tandem_amd import _lib
    with pytest.raises(_lib.DrError) as e:
        call(*args)
    return e.value.code


@pytest.fixture(scope="module")
def S11(tmp_path_factory):
    """synth.scene seed 11, 5 scans: the oracle's record of all of them, and file F = the map after 2 scans, saved by an
    unbounded engine U with streaming off, with U's blocks and U's ray-cast at the pose of scan 2."""
    from synth import scene
    sc = scene.make_scans(5, H, W, seed=11)
    opt = options(sc, H, W, VS)
    rec = record(opt, sc["scans"])
    U = engine(unbounded(opt))
    for i in range(2):
        step(U, Replay(rec, i), *sc["scans"][i], f"U scan {i}")
    F = str(tmp_path_factory.mktemp("map") / "F.drfmap")
    U.save_map(F)
    blocks = U.export_blocks()
    assert_same_blocks(blocks, rec[1]["blocks"], "U against the oracle")
    pose2 = sc["scans"][2][2]
    U.IntegrateScanAsync(sc["scans"][2][0], np.zeros((H, W), np.float32), pose2)  # no valid depth: changes nothing, makes a render legal
    view = render(U, pose2)
    assert_same_blocks(U.export_blocks(), blocks, "a scan without depth")
    U.close()
    # scan 1 once more after scans 0 and 1: a scan that allocates no block (test_load_in_chunks)
    again = [sc["scans"][0], sc["scans"][1], sc["scans"][1]]
    rec_again = record(opt, again)
    assert rec_again[2]["blocks"].keys() == blocks.keys()
    return dict(scans=sc["scans"], opt=opt, rec=rec, F=F, n=len(blocks), blocks=blocks, pose=pose2, view=view, again=again, rec_again=rec_again)


# ------------------------------------------------------------------ 1
def test_round_trip_and_continuation(S11, tmp_path):
    from tandem_amd.dr_fusion import MeshPatches
    scans, opt, rec = S11["scans"], S11["opt"], S11["rec"]
    A, oa = engine(opt), Replay(rec)
    for i in range(2):
        step(A, oa, *scans[i], f"A scan {i}")
    stats, order = A.stats(), list(A.export_blocks())
    p = str(tmp_path / "a.drfmap")
    A.save_map(p)
    got, keys = file_blocks(p)
    assert_same_blocks(got, A.export_blocks(), "file against export_blocks")
    assert A.stats() == stats and list(A.export_blocks()) == order, "the save changed the engine"
    assert open(p, "rb").read() == open(S11["F"], "rb").read(), "pool size changed the file"
    lo, hi = box_of(rec[-1]["blocks"], VS)
    B, ob = engine(opt), Replay(rec, 2)
    assert B.GetMeshUpdate(lo, hi)[0] is True and B.GetMeshUpdate(lo, hi)[0] is False  # a baseline the load has to void
    B.load_map(p)
    assert [pack(c) for c in B.export_blocks()] == keys, "slot i holds the block with the i-th key"
    assert_same_blocks(B.export_blocks(), A.export_blocks(), "loaded")
    assert B.stats() == dict(blocks=len(keys), updated_last=0, updated_total=0, mismatches=0)
    up = B.GetMeshUpdate(lo, hi)
    assert up[0] is True, "the first mesh update after a load is full"
    assert_same_mesh(MeshPatches().apply(up).assemble(), A.GetMesh(lo, hi), "mesh update after the load")
    for i in range(2, 5):
        step(A, oa, *scans[i], f"A scan {i}")
        step(B, ob, *scans[i], f"B scan {i}")
        assert A.stats()["updated_total"] - stats["updated_total"] == B.stats()["updated_total"]
    assert_same_blocks(A.export_blocks(), rec[4]["blocks"], "A final")
    assert_same_blocks(B.export_blocks(), rec[4]["blocks"], "B final")
    ma = A.GetMesh(lo, hi)
    assert len(ma[0]) > 1000
    assert_same_mesh(ma, B.GetMesh(lo, hi), "full-box mesh")
    A.close(), B.close()


# ------------------------------------------------------------------ 2
def test_the_file_is_a_function_of_the_map_alone(S11, tmp_path):
    from tandem_amd.dr_fusion import streaming_min_radius
    scans, opt, rec, n = S11["scans"], S11["opt"], S11["rec"], S11["n"]
    S = engine(opt)
    for i in range(2):
        step(S, Replay(rec, i), *scans[i], f"S scan {i}")
    S.stream_out_region(ALL_LO, (1e4, 1e4, 2.0))
    st, res, host = S.streaming_stats(), S.export_blocks(), S.export_host_blocks()
    assert 0 < st["host"] < n and st["resident"] + st["host"] == n
    _, keys = file_blocks(S11["F"])
    stored = [unpack(k) in host for k in keys]
    mixed = [c for c in range(0, n, 64) if 0 < sum(stored[c:c + 64]) < len(stored[c:c + 64])]
    assert mixed, "no chunk of 64 holds both resident and stored blocks"
    want = open(S11["F"], "rb").read()
    for chunk in (0, 64, 5):
        p = str(tmp_path / f"s{chunk}.drfmap")
        S.save_map(p, chunk)
        assert open(p, "rb").read() == want, f"chunk_blocks={chunk}"
        assert os.listdir(tmp_path) == [f"s{chunk}.drfmap"]
        os.remove(p)
    assert S.streaming_stats() == st
    assert list(S.export_blocks()) == list(res)
    assert_same_blocks(S.export_blocks(), res, "pool after the saves")
    assert_same_blocks(S.export_host_blocks(), host, "store after the saves")
    S.close()
    # automatic mode: the first place is evicted by the radius rule
    (near, far), popt = places(2)
    T, V = engine(popt), engine(unbounded(popt))
    T.set_streaming(streaming_min_radius(T.options))
    for s in near + far:
        feed(T, *s)
        feed(V, *s)
    assert T.streaming_stats()["host"] > 0 and T.streaming_stats()["resident"] > 0
    pt, pv = str(tmp_path / "t.drfmap"), str(tmp_path / "v.drfmap")
    T.save_map(pt, 64)
    V.save_map(pv)
    assert open(pt, "rb").read() == open(pv, "rb").read()
    assert_same_blocks(file_blocks(pt)[0], V.export_blocks(), "the streamed map's file")
    T.close(), V.close()


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("chunk", [0, 64, 5, "n"])
def test_load_in_chunks(S11, chunk):
    """num_blocks = n + 3: the last chunk is partial and the pool nearly full.  Scan 2 of the scene allocates 365 new blocks
    (2120 -> 2485 in the oracle), which no pool of n + 3 can take, so the scan that follows the load here is scan 1 once
    more: it allocates nothing, updates the voxels it updated before, and is held to the oracle by step like any other."""
    n = S11["n"]
    f = engine(S11["opt"], num_blocks=n + 3, num_buckets=n + 3)
    f.load_map(S11["F"], n if chunk == "n" else chunk)
    assert_same_blocks(f.export_blocks(), S11["blocks"], "loaded")
    same_image(render(f, S11["pose"]), S11["view"], "ray-cast of the loaded map")
    step(f, Replay(S11["rec_again"], 2), *S11["again"][2], "scan 1 again")
    assert f.stats()["updated_last"] > 0
    assert_same_blocks(f.export_blocks(), S11["rec_again"][2]["blocks"], "after the scan")
    f.close()


# ------------------------------------------------------------------ 4
def test_load_with_streaming_on(S11):
    from tandem_amd.dr_fusion import RENDER_MAP, streaming_min_radius
    n, rec = S11["n"], S11["rec"]
    f = engine(S11["opt"])
    f.set_streaming(streaming_min_radius(f.options), 0)
    before = f.streaming_stats()
    f.load_map(S11["F"], 64)
    st = f.streaming_stats()
    assert st["resident"] == 0 and st["host"] == n
    assert (st["streamed_out"], st["streamed_in"], st["bytes_moved"]) == (before["streamed_out"], before["streamed_in"], before["bytes_moved"])
    assert_same_blocks(f.export_host_blocks(), S11["blocks"], "store")
    assert (render(f, S11["pose"])[1] == 0).all(), "a resident-scope render sees nothing before the first scan"
    f.set_render_scope(RENDER_MAP)
    same_image(render(f, S11["pose"]), S11["view"], "map-scope render of the loaded store")
    assert f.render_stats()[0] > 0 and f.streaming_stats() == st
    o = Replay(rec, 2)
    for i in range(2, 5):
        step(f, o, *S11["scans"][i], f"scan {i}")
    assert f.streaming_stats()["streamed_in"] > 0
    assert_same_blocks(f.export_all_blocks(), rec[4]["blocks"], "whole map")
    f.close()


# ------------------------------------------------------------------ 5
def test_blocks_in_the_overflow_table(tmp_path):
    from synth import scene
    from oracle.tsdf_oracle import TsdfOracle
    sc = scene.make_scans(4, H, W, seed=6)
    opt = options(sc, H, W, VS)
    S = np.eye(4, dtype=np.float32)
    c, s = np.cos(1.45), np.sin(1.45)
    S[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    S[:3, 3] = (40.2, 0.3, -0.2)
    scans = shifted(sc["scans"], S)
    f, o = engine(opt), TsdfOracle(**opt)
    for i in range(2):
        step(f, o, *scans[i], f"scan {i}")
    xs = [k[0] for k in f.export_blocks()]
    assert min(xs) < 256 <= max(xs)
    p = str(tmp_path / "t.drfmap")
    f.save_map(p, 64)
    g = engine(opt)
    g.load_map(p, 64)
    assert_same_blocks(g.export_blocks(), f.export_blocks(), "loaded")
    assert_same_blocks(g.export_blocks(), o.export_blocks(), "against the oracle")
    od = step(g, o, *scans[2], "scan 2")
    assert (od > 0).mean() > 0.3
    assert_same_blocks(g.export_blocks(), o.export_blocks(), "final")
    f.close(), g.close()


# ------------------------------------------------------------------ 6
def assert_empty(f):
    st = f.streaming_stats()
    assert f.export_blocks() == {} and f.export_host_blocks() == {} and st["resident"] == 0 and st["host"] == 0
    assert f.stats() == dict(blocks=0, updated_last=0, updated_total=0, mismatches=0)


def test_refusals_leave_things_as_they_were(S11, tmp_path):
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import streaming_min_radius
    scans, opt, rec, n, F = S11["scans"], S11["opt"], S11["rec"], S11["n"], S11["F"]
    f = engine(opt)                                                   # a map that is not empty
    step(f, Replay(rec), *scans[0], "scan 0")
    assert code_of(f.load_map, F) == 2
    assert_same_blocks(f.export_blocks(), rec[0]["blocks"], "after the refused load")
    f.IntegrateScanAsync(*scans[1])                                   # save and load out of turn; the render still completes
    assert code_of(f.save_map, str(tmp_path / "x.drfmap")) == 2
    f.RenderAsync([scans[1][2]])
    assert code_of(f.save_map, str(tmp_path / "x.drfmap")) == 2 and code_of(f.load_map, F) == 2
    rb, rd = f.GetRenderResult()
    same_image((rb[0], rd[0]), rec[1]["render"], "the render around the refused save")
    assert os.listdir(tmp_path) == []
    assert code_of(f.save_map, str(tmp_path / "no" / "such" / "dir" / "x.drfmap")) == 4
    assert f._L.drf_save_map(f._h, None, 0) == 1 and f._L.drf_load_map(f._h, None, 0) == 1
    f.close()

    f = engine(opt, num_blocks=n - 1, num_buckets=n - 1)              # one block too many for the pool
    assert code_of(f.load_map, F) == 5
    assert_empty(f)
    step(f, Replay(rec), *scans[0], "scan 0 after the refused load")
    assert_same_blocks(f.export_blocks(), rec[0]["blocks"], "scan 0 after the refused load")
    f.close()

    f = engine(opt)                                                   # ... and for the host store
    r = streaming_min_radius(f.options)
    f.set_streaming(r, n - 1)
    assert code_of(f.load_map, F) == 5
    assert_empty(f)
    f.set_streaming(r, n)
    f.load_map(F)
    assert f.streaming_stats()["host"] == n
    f.close()

    bad = str(tmp_path / "bad.drfmap")                                # one voxel bit flipped
    data = bytearray(open(F, "rb").read())
    data[64 + 8 * n + 4096 * (n // 2) + 77] ^= 0x04
    open(bad, "wb").write(bytes(data))
    f = engine(opt)
    assert code_of(f.load_map, bad) == 4 and code_of(f.load_map, str(tmp_path / "missing.drfmap")) == 4
    assert_empty(f)
    f.load_map(F, 5)
    assert_same_blocks(f.export_blocks(), S11["blocks"], "the good file after the bad one")
    f.close()

    o1 = dict(opt, voxel_size=0.01, truncation_distance=0.04)         # another voxel size
    f, o = engine(o1), TsdfOracle(**o1)
    assert code_of(f.load_map, F) == 1
    assert_empty(f)
    step(f, o, *scans[0], "scan 0 at 1 cm")
    assert_same_blocks(f.export_blocks(), o.export_blocks(), "scan 0 at 1 cm")
    f.close()

    f = engine(opt)                                                   # the empty map
    e = str(tmp_path / "empty.drfmap")
    f.save_map(e)
    assert os.path.getsize(e) == 72 and file_blocks(e) == ({}, [])
    f.load_map(e)
    assert_empty(f)
    f.load_map(F)                                                     # still empty, so still loadable
    assert_same_blocks(f.export_blocks(), S11["blocks"], "after the empty file")
    f.close()


# ------------------------------------------------------------------ 7
def test_shim_saves_and_loads(tmp_path):
    """tandem_amd/libdr/dr_fusion.h: SaveMapToFile on one DrFusion, LoadMapFromFile on a second, one render of each compared."""
    import __graft_entry__ as g
    if not os.path.isfile(os.path.join(ROOT, "tandem_amd", "libdr_mi355x.so")):
        g.build()
    exe = str(tmp_path / "map_io_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tandem_amd", "libdr"), os.path.join(ROOT, "tests/cpp/map_io_shim.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    p = str(tmp_path / "shim.drfmap")
    r = subprocess.run([exe, p], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_io_shim ok" in r.stdout
    blocks, _ = file_blocks(p)
    assert len(blocks) > 50
