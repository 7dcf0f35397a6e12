"""The host rule of the locate scope (drf_set_locate_scope(DRF_LOCATE_MAP); tandem_amd/csrc/fusion_host.h locate_stage_slack,
locate_pose_drift, select_locate_blocks), compiled by g++ from tests/cpp/locate_scope_check.cpp -- no GPU:
  * the selection at a pose holds every block an evaluation there reads (brute force over every pixel, depths from
    min_sensor_depth to max_sensor_depth and the eight corners), for two sets of intrinsics;
  * the staging made at pose A holds every block read at a pose B whose drift is just below the slack, and the rule is not vacuous:
    poses a few slacks away read blocks the staging lacks;
  * the drift is symmetric, zero for A = B and bounds the true displacement of the sample points;
  * the same checks under AddressSanitizer and UBSan in a stand-alone program; the C ABI, its Python mirror and the shim.
The options are 96x128 at 2 cm with max_sensor_depth 1 m, so that the store -- every block of the box [-16, 16)^3, 2.56 m each way --
holds whatever a pose of these tests can read.  DESIGN.md §7c "Locating in the whole map"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import ROOT, abi_module, check_symbols
from test_map_locate import Camera, camera, f32p, f64p, rigid, u64p

DEPTHS = np.array([0.1, 0.2, 0.45, 0.7, 0.9, 1.0])                      # min_sensor_depth .. max_sensor_depth
CAMS = [camera(max_sensor_depth=1.0), camera(max_sensor_depth=1.0, fx=95.0, fy=120.0, cx=20.25, cy=80.5)]
B = 16
BIAS = 1 << 20


def pack(c):
    c = np.asarray(c, np.int64) + BIAS
    return ((c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]).astype(np.uint64)


BOX = np.sort(pack(np.stack(np.meshgrid(*[np.arange(-B, B)] * 3, indexing="ij"), -1).reshape(-1, 3)))


@pytest.fixture(scope="module")
def LS(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("locate_scope")), "liblocate_scope_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/locate_scope_check.cpp"), "-o", so])
    h = C.CDLL(so)
    cam = C.POINTER(Camera)
    h.ls_slack.restype = h.ls_drift.restype = h.ls_max_displacement.restype = C.c_double
    h.ls_slack.argtypes = [cam]
    h.ls_drift.argtypes = [cam, f32p, f32p]
    h.ls_serves.argtypes = [cam, f32p, f32p, C.c_double]
    h.ls_round_trip.argtypes = [f32p, C.c_float, f32p]
    h.ls_select.argtypes = [u64p, C.c_int, cam, f32p, u64p, C.c_int]
    h.ls_blocks_read.argtypes = [cam, f32p, f64p, C.c_int, u64p, C.c_int]
    h.ls_max_displacement.argtypes = [cam, f32p, f32p, f64p, C.c_int]
    return h


def p16(pose):
    a = np.ascontiguousarray(pose, np.float32).reshape(16)
    return a, a.ctypes.data_as(f32p)


def selection(LS, cam, pose):
    out = np.zeros(len(BOX), np.uint64)
    n = LS.ls_select(BOX.ctypes.data_as(u64p), len(BOX), C.byref(Camera(**cam)), p16(pose)[1], out.ctypes.data_as(u64p), len(out))
    assert 0 < n <= len(BOX)
    assert (np.diff(out[:n].astype(np.int64)) > 0).all()                # ascending, each block once: what the kernel's search needs
    return set(out[:n].tolist())


def blocks_read(LS, cam, pose):
    out = np.zeros(len(BOX), np.uint64)
    n = LS.ls_blocks_read(C.byref(Camera(**cam)), p16(pose)[1], DEPTHS.ctypes.data_as(f64p), len(DEPTHS), out.ctypes.data_as(u64p), len(out))
    assert 0 < n <= len(BOX)
    return set(out[:n].tolist())


def drift(LS, cam, a, b):
    return LS.ls_drift(C.byref(Camera(**cam)), p16(a)[1], p16(b)[1])


def displacement(LS, cam, a, b):
    return LS.ls_max_displacement(C.byref(Camera(**cam)), p16(a)[1], p16(b)[1], DEPTHS.ctypes.data_as(f64p), len(DEPTHS))


def random_pose(rng):
    return rigid(rng.uniform(-1, 1, 3) + (0, 0, 1e-3), rng.uniform(-180, 180), rng.uniform(-0.3, 0.3, 3))


def moved(a, axis, deg, t, s):
    """Pose a moved by the fraction s of a twist, as a float32 pose."""
    return (rigid(axis, deg * s, np.asarray(t) * s).astype(np.float64) @ np.asarray(a, np.float64)).astype(np.float32)


def at_drift(LS, cam, a, axis, t, target):
    """The pose along the twist whose drift from a is just below target (bisection on the fraction)."""
    lo, hi = 0.0, 1.0
    assert drift(LS, cam, a, moved(a, axis, 20.0, t, hi)) > target
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if drift(LS, cam, a, moved(a, axis, 20.0, t, mid)) <= target:
            lo = mid
        else:
            hi = mid
    return moved(a, axis, 20.0, t, lo), lo


@pytest.mark.parametrize("k", [0, 1], ids=["centred", "off-centre principal point"])
def test_selection_is_a_superset_by_brute_force(LS, k):
    cam, rng = CAMS[k], np.random.default_rng(11 + k)
    box = set(BOX.tolist())
    for _ in range(8):
        pose = random_pose(rng)
        sel, read = selection(LS, cam, pose), blocks_read(LS, cam, pose)
        assert read <= box, "the store of this test must hold what the pose reads"
        assert read <= sel, "%d blocks read are not selected" % len(read - sel)
        assert len(sel) < len(box)                                      # a cut, not the whole store


@pytest.mark.parametrize("k", [0, 1], ids=["centred", "off-centre principal point"])
def test_a_staging_serves_the_poses_within_the_slack_and_not_much_more(LS, k):
    cam, rng = CAMS[k], np.random.default_rng(23 + k)
    cm = Camera(**cam)
    slack = LS.ls_slack(C.byref(cm))
    vs, s3 = cam["voxel_size"], np.sqrt(3.0)
    assert 0.9 * 8 * s3 * vs < slack < 8 * s3 * vs                      # the spare 8 sqrt(3) voxels less what a near-rigid pose takes
    box, lacking = set(BOX.tolist()), 0
    for _ in range(6):
        a = random_pose(rng)
        axis, t = rng.uniform(-1, 1, 3) + (0, 0, 1e-3), rng.uniform(-0.5, 0.5, 3)
        sel = selection(LS, cam, a)
        b, s = at_drift(LS, cam, a, axis, t, slack)
        d = drift(LS, cam, a, b)
        assert 0.97 * slack < d <= slack and LS.ls_serves(C.byref(cm), p16(a)[1], p16(b)[1], slack) == 1
        read = blocks_read(LS, cam, b)
        assert read <= sel, "drift %.4f <= slack %.4f, but %d blocks read at B are not in A's selection" % (d, slack, len(read - sel))
        far = moved(a, axis, 20.0, t, 4.0 * s)                          # a few slacks away
        assert drift(LS, cam, a, far) > 2.0 * slack and LS.ls_serves(C.byref(cm), p16(a)[1], p16(far)[1], slack) == 0
        read = blocks_read(LS, cam, far)
        assert read <= box
        lacking += bool(read - sel)
    print("poses a few slacks away that read a block outside the staging: %d of 6" % lacking)
    assert lacking >= 1, "no far pose needed a new staging: the rule was not exercised"


def test_drift_is_symmetric_zero_at_home_and_bounds_the_displacement(LS):
    rng = np.random.default_rng(5)
    for k, cam in enumerate(CAMS):
        for _ in range(6):
            a = random_pose(rng)
            b = moved(a, rng.uniform(-1, 1, 3) + (0, 0, 1e-3), rng.uniform(-30, 30), rng.uniform(-0.4, 0.4, 3), 1.0)
            dab, dba = drift(LS, cam, a, b), drift(LS, cam, b, a)
            assert dab == dba > 0.0 and drift(LS, cam, a, a) == 0.0 and drift(LS, cam, b, b) == 0.0
            true = displacement(LS, cam, a, b)
            assert 0.0 < true <= dab, (true, dab)
            assert dab < 4.0 * true + 1e-6                              # a bound, not a number without meaning
    nan = np.array(random_pose(rng), np.float32)
    nan[0, 3] = np.nan
    assert LS.ls_serves(C.byref(Camera(**CAMS[0])), p16(nan)[1], p16(nan)[1], 1.0) == 0   # a NaN serves nothing


def test_the_loop_pose_converts_within_the_voxel_set_aside(LS):
    """pose16 -> (Rd, tv) in lattice units -> pose16: the rotation comes back exactly, a translation within one float ulp; the
    sample points move by far less than the voxel that locate_stage_slack leaves out of the slack."""
    rng = np.random.default_rng(7)
    cam = CAMS[0]
    for scale in (0.3, 30.0, 300.0):
        a = np.array(random_pose(rng), np.float32)
        a[:3, 3] *= np.float32(scale / 0.3)
        a32, ap = p16(a)
        out = np.zeros(16, np.float32)
        LS.ls_round_trip(ap, C.c_float(cam["voxel_size"]), out.ctypes.data_as(f32p))
        out = out.reshape(4, 4)
        assert np.array_equal(out[:3, :3], a[:3, :3]) and np.array_equal(out[3], [0, 0, 0, 1])
        assert (np.abs(out[:3, 3] - a[:3, 3]) <= np.spacing(np.abs(a[:3, 3]))).all()
        assert drift(LS, cam, a, out) < 0.01 * cam["voxel_size"]


def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """The same checks under AddressSanitizer and UBSan: a plain executable with its own main and its own cases, nothing preloaded,
    nothing loaded into Python."""
    exe = str(tmp_path / "locate_scope_san")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/locate_scope_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "locate_scope_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


def test_abi_declares_exports_and_types_the_two_functions(tmp_path):
    L = abi_module()
    src = check_symbols(L, ["drf_set_locate_scope", "drf_locate_stage_stats"])
    assert "#define DRF_LOCATE_RESIDENT 0" in src and "#define DRF_LOCATE_MAP      1" in src
    assert "int drf_set_locate_scope(drf_t *h, int scope, size_t stage_capacity_blocks);" in src
    assert "int drf_locate_stage_stats(drf_t *h, uint64_t out[4]);" in src
    lib = L.lib()
    assert lib.drf_set_locate_scope(None, 1, 0) == 1 and lib.drf_locate_stage_stats(None, (C.c_uint64 * 4)()) == 1
    from tandem_amd import dr_fusion
    assert (dr_fusion.LOCATE_RESIDENT, dr_fusion.LOCATE_MAP) == (0, 1)
    assert callable(dr_fusion.DrFusion.set_locate_scope) and callable(dr_fusion.DrFusion.locate_stage_stats)
    # the shim carries SetLocateScope: the program of the GPU test compiles and links
    exe = str(tmp_path / "locate_scope_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/locate_scope_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert os.path.isfile(exe)
