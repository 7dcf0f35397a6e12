"""-m gpu: drf_align_system / drf_align_map.  The reference of every bit comparison is np_align_system / np_align_maps, the numpy
restatement of the rule in tests/test_map_align.py, and beside it align_maps_host through tests/cpp/map_align_check.cpp; the maps
reach the library as files written by tandem_amd.map_file.write.  The meaning of the pose is held to the truth on three planes.
96x128 engines, maps of about 40 blocks (the planes: 275).  DESIGN.md §7c "Registering two maps"."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from fusion_helpers import ROOT, assert_same_mesh, box_of, feed, places
from test_fusion_map_file_gpu import code_of, engine
from test_fusion_map_transform_gpu import options, write
from test_map_align import (CONVERGED, DEGENERATE, LOST, MAX_ITERS, SMALL, T37, VS, assert_same_result, assert_same_system, build_check, cpp_align,
                            np_align_maps, np_align_system, plane_bound, planes_case, random_pair, twist_between)
from test_map_transform import _OFF

pytestmark = pytest.mark.gpu
EYE = np.eye(4, dtype=np.float32)
NONE = (np.zeros((0, 3), np.int64), np.zeros((0, 4096), np.uint8))


def result_dict(r):
    return dict(T=r.T, sums=r.sums, samples=r.samples, valid0=r.valid0, valid=r.valid, cost0=r.cost0, cost=r.cost, iterations=r.iterations, status=r.status)


@pytest.fixture(scope="module")
def CHK(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("map_align_check"))


@pytest.fixture(scope="module")
def D(tmp_path_factory):
    """The maps and their files: the random pair of about 40 source blocks, and the planes."""
    d = tmp_path_factory.mktemp("align")
    rnd, pl = random_pair(3), planes_case()
    files = {}
    for name, m in (("rnd_src", rnd[0]), ("rnd_ref", rnd[1]), ("pl_src", pl["src"]), ("pl_ref", pl["ref"])):
        files[name] = str(d / (name + ".drfmap"))
        write(files[name], VS, *m)
    return dict(dir=d, rnd=rnd, planes=pl, **files)


def run_system(f, tmp_path, name, src, ref, T, vs, same=False, **opt):
    ps, pr = str(tmp_path / (name + "_src.drfmap")), str(tmp_path / (name + "_ref.drfmap"))
    write(ps, vs, *src)
    if not same:
        write(pr, vs, *ref)
    got = f.align_system(ps, ps if same else pr, T, **opt)
    st = f.align_stats()
    assert st[:5] == (len(src[0]), len(ref[0]), got[1][0], got[1][1], 1), st
    assert st[5] == 4104 * (len(src[0]) + len(ref[0])) + 224 * len(src[0]) + 32
    return got


# ------------------------------------------------------------------ 1
def test_system_against_the_restatement(D, tmp_path):
    f = engine(options())
    src, ref = D["rnd"]
    for name, T, opt in (("T37", T37, {}), ("small", SMALL, {}), ("identity", EYE, {}), ("min_weight 3", SMALL, dict(min_weight=3)),
                         ("wide band, tight huber", SMALL, dict(band=0.05, huber=0.25))):
        want = np_align_system(src, ref, T, VS, **opt)
        got = f.align_system(D["rnd_src"], D["rnd_ref"], T, **opt)
        assert_same_system(got, want, name)
        assert want[1][1] > 0 and want[1][2] > 0, name
    # an empty source, an empty reference
    for name, s, r in (("empty source", NONE, ref), ("empty reference", src, NONE)):
        got = run_system(f, tmp_path, name.replace(" ", "_"), s, r, SMALL, VS)
        assert_same_system(got, np_align_system(s, r, SMALL, VS), name)
        assert not got[0].any() and got[1][1] == 0
    # the source against itself at the identity: f = 0, phi is the voxel itself, every residual is exactly 0
    got = run_system(f, tmp_path, "self", src, src, EYE, VS, same=True)
    assert_same_system(got, np_align_system(src, src, EYE, VS), "self")
    assert got[1][1] > 1000 and not got[0][21:].any(), got
    assert all(got[0][i] > 0 for i in (0, 6, 11, 15, 18, 20))
    f.close()


@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 130])
def test_block_counts_around_the_grid_and_fold_tails(tmp_path, n_src):
    src, ref = random_pair(10 + n_src, n_src=n_src)
    f = engine(options())
    got = run_system(f, tmp_path, "n", src, ref, SMALL, VS)
    f.close()
    want = np_align_system(src, ref, SMALL, VS)
    assert_same_system(got, want, f"{n_src} blocks")
    assert want[1][1] > 0


def test_lattice_motion(tmp_path):
    vs = 2.0 ** -6
    src, ref = random_pair(5, vs=vs)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = np.array([3, -5, 2]) * vs
    f = engine(options(vs))
    got = run_system(f, tmp_path, "lattice", src, ref, T, vs)
    f.close()
    want = np_align_system(src, ref, T, vs)
    assert_same_system(got, want, "lattice")
    assert want[1][1] > 100


# ------------------------------------------------------------------ 2
def test_registration_against_the_host_and_the_restatement(D, CHK):
    f = engine(options())
    cases = (("planes", D["pl_src"], D["pl_ref"], D["planes"]["src"], D["planes"]["ref"], EYE, {}),
             ("random", D["rnd_src"], D["rnd_ref"], D["rnd"][0], D["rnd"][1], SMALL, dict(max_iters=6, min_valid=0.01)),
             ("random, one evaluation", D["rnd_src"], D["rnd_ref"], D["rnd"][0], D["rnd"][1], SMALL, dict(max_iters=1, min_valid=0.01)),
             ("random, lost", D["rnd_src"], D["rnd_ref"], D["rnd"][0], D["rnd"][1], SMALL, dict(min_valid=0.9)))
    for name, ps, pr, src, ref, T0, opt in cases:
        r = f.align_map(ps, pr, T0, raise_on_failure=False, **opt)
        got = result_dict(r)
        host, want = cpp_align(CHK, src, ref, T0, VS, **opt), np_align_maps(src, ref, T0, VS, **opt)
        print("%s: status %d after %d evaluations, %d of %d valid, cost %.3g -> %.3g" % (name, r.status, r.iterations, r.valid, r.samples, r.cost0, r.cost))
        assert_same_result(host, want, name + " (host against the restatement)")
        host.pop("trace")
        assert_same_result(got, host, name + " (library against the host)")
        assert np.array_equal(r.T32, r.T.astype(np.float32))
        assert f.align_stats()[4] == r.iterations
    assert r.status == LOST and r.iterations == 1
    f.close()


# ------------------------------------------------------------------ 3
def test_planes_recover_the_known_pose(D):
    pl = D["planes"]
    bound, N, smin, smax, at_truth = plane_bound(pl)
    assert smin > 0.1 * smax
    f = engine(options())
    r = f.align_map(D["pl_src"], D["pl_ref"])
    f.close()
    d = twist_between(r.T, pl["T_true"], pl["src"][0], VS)
    print("planes: %d evaluations, %d valid, cost %.3g -> %.3g, |d| %.3g, bound %.3g" % (r.iterations, r.valid, r.cost0, r.cost, np.linalg.norm(d), bound))
    assert r.status == CONVERGED and r.iterations <= 20
    assert np.linalg.norm(d) <= bound


# ------------------------------------------------------------------ 4
def test_align_transform_merge(D, tmp_path):
    """The user's chain: the reference moved by T_true is a second session's map; registering it to the reference from the identity
    must undo T_true, and transform_map by that pose followed by merge_map into an engine that holds the reference must give the
    planes again."""
    from tandem_amd import map_file
    pl = D["planes"]
    Tt32 = pl["T_true"].astype(np.float32)
    moved, back, merged = (str(tmp_path / n) for n in ("moved.drfmap", "back.drfmap", "merged.drfmap"))
    f = engine(options())
    f.transform_map(D["pl_ref"], Tt32, moved)
    r = f.align_map(moved, D["pl_ref"])
    _, mc, mv = map_file.read(moved)
    truth = np.linalg.inv(Tt32.astype(np.float64))
    bound, N, smin, smax, at_truth = plane_bound(pl, src=(mc, mv), T_truth=truth, eps_scale=2.0)
    d = twist_between(r.T, truth, mc, VS)
    print("chain: %d evaluations, %d of %d valid, |T T_true - I| %.3g, |d| %.3g, bound %.3g" %
          (r.iterations, r.valid, r.samples, np.abs(r.T @ Tt32.astype(np.float64) - np.eye(4)).max(), np.linalg.norm(d), bound))
    assert r.status == CONVERGED
    assert np.linalg.norm(d) <= bound
    f.transform_map(moved, r.T32, back)
    f.load_map(D["pl_ref"])
    f.merge_map(back)
    st = f.merge_stats()
    assert st[2] > 0 and st[5] > 10000, st
    f.save_map(merged)
    f.close()
    _, gc, gv = map_file.read(merged)
    gv = gv.reshape(len(gc), 512, 8)
    p = (gc[:, None, :] * 8 + _OFF[None]).astype(np.float64) * np.float64(np.float32(VS))
    nearest = np.argmin(np.linalg.norm((gc * 8 + 4)[:, None, :] - 8.0 * pl["origins"][None], axis=-1), axis=1)
    nrm, org = pl["patch_normals"][nearest], pl["origins"][nearest] * 8 * np.float64(np.float32(VS))
    want = np.einsum("bvk,bk->bv", p, nrm) - np.einsum("bk,bk->b", org, nrm)[:, None]
    got = np.ascontiguousarray(gv[:, :, :4]).view(np.float32)[:, :, 0].astype(np.float64)
    both = gv[:, :, 7] == 10                                          # the voxels both maps observed
    sdf = np.ascontiguousarray(pl["ref"][1].reshape(-1, 8)[:, :4]).view(np.float32)
    eps = 1e-5 * float(np.abs(sdf).max()) / VS
    err = np.abs(got - want)[both].max()
    print("merged: %d voxels of weight 10, max |sdf - plane| %.3g m, bound %.3g m" % (both.sum(), err, 2 * eps * VS))
    assert both.sum() > 30000
    assert err <= 2 * eps * VS


# ------------------------------------------------------------------ 5
def test_the_engine_is_untouched(D, tmp_path):
    from tandem_amd.dr_fusion import streaming_min_radius
    (p0, p1), popt = places(2)
    f = engine(popt, num_blocks=6000, num_buckets=6000)
    f.set_streaming(streaming_min_radius(f.options))
    for s in (p0[0], p0[1], p1[0], p1[1]):
        feed(f, *s)
    assert f.streaming_stats()["host"] > 0 and f.streaming_stats()["resident"] > 0
    a, b = (str(tmp_path / n) for n in ("a.drfmap", "b.drfmap"))
    snapshot = lambda: (f.stats(), f.streaming_stats(), f.mesh_update_stats(), f.merge_stats(), f.transform_stats(), list(f.export_blocks()), sorted(f.export_host_blocks()))  # noqa: E731
    f.save_map(a)
    lo, hi = box_of(f.export_blocks(), 0.02)
    mesh = f.GetMesh(lo, hi)
    assert len(mesh[0]) > 1000
    before = snapshot()
    want_sys = np_align_system(*D["rnd"], SMALL, VS)
    want = np_align_maps(D["planes"]["src"], D["planes"]["ref"], EYE, VS)
    assert_same_system(f.align_system(D["rnd_src"], D["rnd_ref"], SMALL), want_sys, "system")
    assert snapshot() == before
    f.ExtractMeshAsync(lo, hi)                                        # pending across both calls
    assert_same_system(f.align_system(D["rnd_src"], D["rnd_ref"], SMALL), want_sys, "system, extraction pending")
    got = result_dict(f.align_map(D["pl_src"], D["pl_ref"]))
    want.pop("trace")
    assert_same_result(got, want, "registration, extraction pending")
    assert_same_mesh(f.GetMeshSync(), mesh, "the extraction that was pending across the registration")
    assert snapshot() == before
    f.save_map(b)
    assert open(a, "rb").read() == open(b, "rb").read()
    feed(f, *p1[1])                                                   # and it goes on
    assert f.stats()["updated_last"] > 0
    f.close()


# ------------------------------------------------------------------ 6
def test_refusals_in_their_order(D, tmp_path):
    from tandem_amd import _lib
    f = engine(options())
    L = f._L
    src, ref = D["rnd_src"], D["rnd_ref"]
    enc = os.fsencode
    eye_a = np.ascontiguousarray(EYE)
    Tp = lambda T: eye_a.ctypes.data_as(_lib.f32p)  # noqa: E731
    sums_a, T32_a = np.zeros(28), np.zeros(16, np.float32)
    sums, counts, T32 = sums_a.ctypes.data_as(_lib.f64p), (_lib.C.c_uint64 * 3)(), T32_a.ctypes.data_as(_lib.f32p)
    nothing_held = lambda: f.align_stats() == (0, 0, 0, 0, 0, 0)  # noqa: E731
    # null arguments
    for args in ((None, enc(ref), Tp(EYE), None, sums, counts), (enc(src), None, Tp(EYE), None, sums, counts), (enc(src), enc(ref), None, None, sums, counts),
                 (enc(src), enc(ref), Tp(EYE), None, None, counts), (enc(src), enc(ref), Tp(EYE), None, sums, None)):
        assert L.drf_align_system(f._h, *args) == 1 and nothing_held()
    for args in ((None, enc(ref), Tp(EYE), None, T32, None), (enc(src), None, Tp(EYE), None, T32, None), (enc(src), enc(ref), None, None, T32, None),
                 (enc(src), enc(ref), Tp(EYE), None, None, None)):
        assert L.drf_align_map(f._h, *args) == 1 and nothing_held()
    assert L.drf_align_stats(f._h, None) == 1
    with pytest.raises(_lib.DrError) as e:
        f.align_map(src, ref, EYE, huber=-1.0)
    assert e.value.code == 1 and "huber" in str(e.value)
    with pytest.raises(TypeError):
        f.align_map(src, ref, EYE, no_such_option=1)
    # what is no rigid motion
    scaled, nan, row, mirror = (T37.copy() for _ in range(4))
    scaled[:3, :3] *= 1.01
    nan[2, 3] = np.nan
    row[3, 3] = 1.0 + 2.0 ** -20
    mirror[:3, 1] *= -1
    for bad in (scaled, nan, row, mirror):
        assert code_of(f.align_system, src, ref, bad) == 1 and code_of(f.align_map, src, ref, bad) == 1 and nothing_held()
    # a file that fails the validation, on either side; it comes after the motion and before the voxel size
    data = open(src, "rb").read()
    flipped, cut, other = (str(tmp_path / n) for n in ("flip.drfmap", "cut.drfmap", "other_vs.drfmap"))
    bad = bytearray(data)
    bad[64 + 8 * 40 + 4096 * 20 + 77] ^= 0x04
    open(flipped, "wb").write(bytes(bad))
    open(cut, "wb").write(data[:-4107])
    write(other, 0.01, *D["rnd"][0])
    for path in (flipped, cut, str(tmp_path / "missing.drfmap")):
        assert code_of(f.align_map, path, ref, EYE) == 4 and code_of(f.align_map, src, path, EYE) == 4, path
        assert code_of(f.align_system, path, other, EYE) == 4 and code_of(f.align_system, other, path, EYE) == 4, path
        assert nothing_held()
    assert code_of(f.align_map, flipped, ref, scaled) == 1             # the motion is looked at first
    # another voxel_size, on either side
    assert code_of(f.align_map, other, ref, EYE) == 1 and code_of(f.align_map, src, other, EYE) == 1
    assert "voxel_size" in L.dr_last_error().decode() and nothing_held()
    # where a scan may not be integrated: before everything but the null arguments and the options
    H, W = 96, 128
    bgr, depth, pose = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.float32), np.eye(4, dtype=np.float32)
    f.IntegrateScanAsync(bgr, depth, pose)
    assert code_of(f.align_map, src, ref, EYE) == 2 and code_of(f.align_system, flipped, ref, scaled) == 2
    assert L.drf_align_map(f._h, None, enc(ref), Tp(EYE), None, T32, None) == 1
    f.RenderAsync([pose])
    assert code_of(f.align_system, src, ref, EYE) == 2                 # between RenderAsync and GetRenderResult
    f.GetRenderResult()
    assert nothing_held()
    # a registration that finds no pose is DR_OK with the status set and a message; the Python mirror raises unless told not to
    from tandem_amd.dr_fusion import AlignError
    with pytest.raises(AlignError) as e:
        f.align_map(src, ref, SMALL, min_valid=0.9)
    assert e.value.result.status == LOST and "lost" in str(e.value)
    assert np.array_equal(e.value.result.T32, SMALL)
    one = planes_case(only=2)
    deep = tmp_path.joinpath(*["a_directory_with_a_long_name_" + "x" * 90] * 4)   # paths of 500 characters: the message keeps its reason
    deep.mkdir(parents=True)
    one_src, one_ref = str(deep / "one_src.drfmap"), str(deep / "one_ref.drfmap")
    assert len(one_src) > 480
    write(one_src, VS, *one["src"])
    write(one_ref, VS, *one["ref"])
    r = f.align_map(one_src, one_ref, raise_on_failure=False)
    msg = L.dr_last_error().decode()
    assert r.status == DEGENERATE and "degenerate" in msg and one_src in msg and one_ref in msg
    r = f.align_map(D["pl_src"], D["pl_ref"], max_iters=1)
    assert r.status == MAX_ITERS and r.iterations == 1 and not np.array_equal(r.T32, EYE)
    # after all of it the engine does what it did in test 1
    assert_same_system(f.align_system(src, ref, SMALL), np_align_system(*D["rnd"], SMALL, VS), "afterwards")
    f.close()


def test_maps_that_do_not_fit_on_the_device(D, monkeypatch, parity_hooks):
    """DR_ERR_CAPACITY.  No test can fill an MI355X, so the parity build (the same sources) reads the lower limit drf_transform_map's
    test uses, for the same comparison: one byte less than the call takes, then exactly what it takes."""
    ns, nr = len(D["rnd"][0][0]), len(D["rnd"][1][0])
    need = 4104 * (ns + nr) + 224 * ns + 32
    f = engine(options())
    monkeypatch.setenv("DR_TRANSFORM_MAX_BYTES", str(need - 1))
    assert code_of(f.align_system, D["rnd_src"], D["rnd_ref"], SMALL) == 5
    assert "device memory" in f._L.dr_last_error().decode() and f.align_stats() == (0, 0, 0, 0, 0, 0)
    assert code_of(f.align_map, D["rnd_src"], D["rnd_ref"], SMALL) == 5
    monkeypatch.setenv("DR_TRANSFORM_MAX_BYTES", str(need))
    assert_same_system(f.align_system(D["rnd_src"], D["rnd_ref"], SMALL), np_align_system(*D["rnd"], SMALL, VS), "at the limit")
    assert f.align_stats()[5] == need
    f.close()


# ------------------------------------------------------------------ 7
def test_shim_and_command(D, tmp_path):
    """tandem_amd/libdr/dr_fusion.h AlignMapFiles and `python -m tandem_amd.map_file align`, held to the library's own answer."""
    import __graft_entry__ as g
    from tandem_amd import map_file
    if not os.path.isfile(os.path.join(ROOT, "tandem_amd", "libdr_mi355x.so")):
        g.build()
    f = engine(options())
    want = f.align_map(D["pl_src"], D["pl_ref"])
    f.close()
    exe = str(tmp_path / "map_align_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tandem_amd", "libdr"), os.path.join(ROOT, "tests/cpp/map_align_shim.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    out = str(tmp_path / "moved.drfmap")
    r = subprocess.run([exe, repr(VS), D["pl_src"], D["pl_ref"], out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["evaluations"] == want.iterations and np.array_equal(np.float32(js["pose"]).reshape(4, 4), want.T32)
    assert map_file.info(out)["blocks"] > 0
    far = planes_case(shift_ref=5)
    far_ref = str(tmp_path / "far_ref.drfmap")
    write(far_ref, VS, *far["ref"])
    r = subprocess.run([exe, repr(VS), D["pl_src"], far_ref, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "lost" in r.stderr, r.stdout + r.stderr
    cmd = [sys.executable, "-m", "tandem_amd.map_file", "align"]
    r = subprocess.run(cmd + [D["pl_src"], D["pl_ref"]], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["status"] == "converged" and js["iterations"] == want.iterations and (js["samples"], js["valid"]) == (want.samples, want.valid)
    assert np.array_equal(np.float32(js["pose"]).reshape(4, 4), want.T32) and js["cost"] == want.cost and js["cost0"] == want.cost0
    r = subprocess.run(cmd + [D["pl_src"], far_ref], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 1, r.stdout + r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["status"] == "lost"
    r = subprocess.run(cmd + [D["pl_src"], D["pl_ref"], "--max-iters", "1", "--init"] + [repr(float(v)) for v in EYE.reshape(16)],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 1 and json.loads(r.stdout.strip().splitlines()[-1])["status"] == "max_iters"
