"""CPU: the host half of drf_transform_map (include/dr_mi355x.h "map files", DESIGN.md §7c "Moving a map into another frame").
transform_voxel, transform_block and plan_transform of tandem_amd/csrc/fusion_host.h compiled with plain g++
(tests/cpp/map_transform_check.cpp) and held to np_transform_map, a numpy restatement of the rule written here -- the reference of
tests/test_fusion_map_transform_gpu.py too; the same under AddressSanitizer and UBSan as a stand-alone program
(tests/cpp/map_transform_san.cpp); the two new names of the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import abi_module, check_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 1 << 20
u8p, u64p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
_V = np.arange(512)
_OFF = np.stack([_V >> 6, (_V >> 3) & 7, _V & 7], axis=1).astype(np.int64)  # voxel index x*64 + y*8 + z -> (x, y, z)


# ------------------------------------------------------------------ the rule, restated
def np_keys(c):
    c = (np.asarray(c, np.int64).reshape(-1, 3) + B).astype(np.uint64)
    return (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]


def motion(T, vs):
    """Rd (3, 3) and tv (3,) in float64 from the float32 matrix and the float32 voxel size, as the rule states them."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    return T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64) / np.float64(np.float32(vs))


def np_region(coords, Rd, tv):
    """Destination blocks to evaluate: per source block the axis-aligned bounds of its lattice box [8b - 1, 8b + 8]^3 under
    g = R u + tv, plus one block all round; the union, ascending by key.  A generous stand-in for 'everywhere'."""
    ends = np.array([[x, y, z] for x in (-1.0, 8.0) for y in (-1.0, 8.0) for z in (-1.0, 8.0)])
    out = set()
    for c in np.asarray(coords, np.int64).reshape(-1, 3):
        g = (c * 8 + ends) @ Rd.T + tv
        lo, hi = np.floor(g.min(0) / 8).astype(np.int64) - 1, np.floor(g.max(0) / 8).astype(np.int64) + 1
        out.update((x, y, z) for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1))
    out = np.array(sorted(out), np.int64).reshape(-1, 3)
    return out[((out >= -B) & (out < B)).all(1)]


def np_transform_map(coords, voxels, T, vs):
    """The map {coords (n, 3) block coordinates, voxels (n, 4096) uint8} moved by T (4x4 float32, p_out = R p_in + t) on the
    lattice of voxel size vs -> (coords (m, 3) ascending by key, voxels (m, 4096), dict(blocks, voxels, refused)).  float64 and
    float32 array operations, one per operation of the rule (numpy does not contract), over np_region."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    n = len(coords)
    vox = np.ascontiguousarray(voxels, np.uint8).reshape(n, 4096)
    Rd, tv = motion(T, vs)
    st = dict(blocks=0, voxels=0, refused=0)
    empty = np.zeros((0, 3), np.int64), np.zeros((0, 4096), np.uint8), st
    if n == 0:
        return empty
    keys = np_keys(coords)
    order = np.argsort(keys)
    keys, src = keys[order], vox[order].reshape(n, 512, 8)
    D = np_region(coords, Rd, tv)
    g = (D[:, None, :] * 8 + _OFF[None]).reshape(-1, 3)
    d = g.astype(np.float64) - tv
    u = np.stack([(Rd[0, k] * d[:, 0] + Rd[1, k] * d[:, 1]) + Rd[2, k] * d[:, 2] for k in range(3)], axis=1)
    assert (np.abs(u) < 2.0 ** 30).all()
    b = np.floor(u)
    f = (u - b).astype(np.float32)
    b = b.astype(np.int64)
    a = (np.float32(1.0) - f, f)
    N = len(g)
    started, alls, anys = np.zeros(N, bool), np.ones(N, bool), np.zeros(N, bool)
    acc = np.zeros((N, 4), np.float32)  # sdf, three colour channels
    wmin = np.full(N, 255, np.int64)
    for c in range(8):
        cx, cy, cz = c >> 2, (c >> 1) & 1, c & 1
        w = (a[cx][:, 0] * a[cy][:, 1]) * a[cz][:, 2]
        assert w.dtype == np.float32
        used = w != 0
        p = b + np.array([cx, cy, cz])
        blk = p >> 3
        ok = ((blk >= -B) & (blk < B)).all(1)
        k = np_keys(np.where(ok[:, None], blk, 0))
        at = np.minimum(np.searchsorted(keys, k), n - 1)
        found = ok & (keys[at] == k)
        v8 = src[at, ((p[:, 0] & 7) << 6) | ((p[:, 1] & 7) << 3) | (p[:, 2] & 7)]
        wt = np.where(found, v8[:, 7], 0).astype(np.int64)
        weighted = used & (wt > 0)
        alls &= ~used | (wt > 0)
        anys |= weighted
        val = np.concatenate([np.ascontiguousarray(v8[:, :4]).view(np.float32), v8[:, 4:7].astype(np.float32)], axis=1)
        with np.errstate(all="ignore"):
            term = w[:, None] * val
            summed = acc + term
        assert term.dtype == np.float32 and summed.dtype == np.float32
        acc = np.where((weighted & ~started)[:, None], term, np.where((weighted & started)[:, None], summed, acc))
        started |= weighted
        wmin = np.where(weighted, np.minimum(wmin, wt), wmin)
    out = np.zeros((N, 8), np.uint8)
    wr = alls
    assert not (wr & ~anys).any(), "a voxel without a used corner"
    out[wr, :4] = np.ascontiguousarray(acc[wr, :1]).view(np.uint8)
    out[wr, 4:7] = np.minimum(acc[wr, 1:] + np.float32(0.5), np.float32(255.0)).astype(np.uint8)
    out[wr, 7] = wmin[wr].astype(np.uint8)
    out = out.reshape(len(D), 4096)
    keep = wr.reshape(len(D), 512).any(1)
    st.update(blocks=int(keep.sum()), voxels=int(wr.sum()), refused=int((~alls & anys).sum()))
    return D[keep], out[keep], st


def as_dict(coords, vox):
    return {tuple(int(v) for v in c): vox[i] for i, c in enumerate(coords)}


# ------------------------------------------------------------------ motions and maps
def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def rigid(axis, deg, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = rotation(axis, deg)
    T[:3, 3] = t
    return T


def random_motion(rng, vs, reach=40.0):
    return rigid(rng.normal(size=3), rng.uniform(-180, 180), rng.uniform(-reach, reach, 3) * vs)


def random_blocks(rng, n, finite_scale=(0.08, 1.0, 1e-3)):
    """(n, 4096) blocks: sdf of both signs, random colours, weights 0 (a fifth of the voxels), 1, 255 and anything between."""
    v = np.empty((n * 512, 8), np.uint8)
    scale = rng.choice(np.array(finite_scale, np.float32), n * 512)
    v[:, :4] = (rng.uniform(-1.0, 1.0, n * 512).astype(np.float32) * scale).view(np.uint8).reshape(-1, 4)
    v[:, 4:7] = rng.integers(0, 256, (n * 512, 3), dtype=np.uint8)
    w = rng.integers(1, 256, n * 512)
    pick = rng.integers(0, 10, n * 512)
    w = np.where(pick < 2, 0, np.where(pick == 2, 1, np.where(pick == 3, 255, w)))
    v[:, 7] = w
    return v.reshape(n, 4096)


def cluster(lo, hi):
    r = range(lo, hi + 1)
    return [(x, y, z) for x in r for y in r for z in r]


# ------------------------------------------------------------------ the compiled host half
@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("map_transform") / "libmap_transform_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_transform_check.cpp"), "-o", so])
    h = C.CDLL(so)
    h.mt_pose_fault.argtypes = [f32p]
    h.mt_pose_fault.restype = C.c_int
    h.mt_plan.argtypes = [u64p, C.c_size_t, f32p, C.c_float, u64p, C.c_size_t, C.POINTER(C.c_int)]
    h.mt_plan.restype = C.c_size_t
    h.mt_transform_blocks.argtypes = [u64p, u8p, C.c_size_t, f32p, C.c_float, u64p, u8p, C.c_size_t, u64p]
    h.mt_transform_blocks.restype = C.c_size_t
    return h


def sorted_source(coords, vox):
    keys = np_keys(coords)
    order = np.argsort(keys)
    return np.ascontiguousarray(keys[order]), np.ascontiguousarray(np.asarray(vox, np.uint8).reshape(len(keys), 4096)[order])


def cpp_plan(H, coords, T, vs):
    keys, _ = sorted_source(coords, np.zeros((len(coords), 4096), np.uint8))
    T = np.ascontiguousarray(T, np.float32)
    ok = C.c_int(0)
    n = H.mt_plan(keys.ctypes.data_as(u64p), len(keys), T.ctypes.data_as(f32p), np.float32(vs), None, 0, C.byref(ok))
    out = np.zeros(max(n, 1), np.uint64)
    assert H.mt_plan(keys.ctypes.data_as(u64p), len(keys), T.ctypes.data_as(f32p), np.float32(vs), out.ctypes.data_as(u64p), n, C.byref(ok)) == n
    return out[:n], bool(ok.value)


def cpp_transform(H, coords, vox, T, vs):
    """(keys ascending, voxels, (candidates, voxels written, voxels refused)) of the compiled rule over plan_transform's blocks."""
    keys, src = sorted_source(coords, vox)
    T = np.ascontiguousarray(T, np.float32)
    counts = (C.c_uint64 * 3)()
    args = (keys.ctypes.data_as(u64p), src.ctypes.data_as(u8p), len(keys), T.ctypes.data_as(f32p), np.float32(vs))
    n = H.mt_transform_blocks(*args, None, None, 0, counts)
    ok, ov = np.zeros(max(n, 1), np.uint64), np.zeros((max(n, 1), 4096), np.uint8)
    assert H.mt_transform_blocks(*args, ok.ctypes.data_as(u64p), ov.ctypes.data_as(u8p), n, counts) == n
    return ok[:n], ov[:n], tuple(int(c) for c in counts)


def assert_same_as_restatement(H, coords, vox, T, vs, what):
    wc, wv, st = np_transform_map(coords, vox, T, vs)
    gk, gv, counts = cpp_transform(H, coords, vox, T, vs)
    assert np.array_equal(gk, np_keys(wc)), f"{what}: {len(gk)} blocks against {len(wc)}"
    bad = np.flatnonzero((gv.reshape(-1, 8) != wv.reshape(-1, 8)).any(1))
    assert bad.size == 0, f"{what}: {bad.size} voxels differ, first got {gv.reshape(-1, 8)[bad[0]]} want {wv.reshape(-1, 8)[bad[0]]}"
    assert counts[1:] == (st["voxels"], st["refused"]), what
    return wc, wv, st


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("seed", range(6))
def test_rule_against_the_restatement_on_random_maps(H, seed):
    rng = np.random.default_rng(seed)
    vs = [0.02, 2.0 ** -6, 0.05][seed % 3]
    pool = cluster(-2, 1) + [(9, -4, 3), (-7, -7, 12)]
    coords = [pool[i] for i in rng.choice(len(pool), 7, replace=False)]
    vox = random_blocks(rng, len(coords))
    _, _, st = assert_same_as_restatement(H, coords, vox, random_motion(rng, vs), vs, f"seed {seed}")
    assert st["blocks"] > 0 and st["voxels"] > 0 and st["refused"] > 0


def test_a_fraction_that_rounds_to_one(H):
    """Identity rotation at voxel_size 2^-6 with t = (2^-36, 0, 2^-37): tv = (2^-30, 0, 2^-31), so that along x and z
    u = g - tv has floor g - 1 and a fraction 1 - tiny that rounds to 1.0f: corner 1 carries all the weight (along y f = 0 and
    corner 0 does).  Every weighted voxel stays where it is with its 8 bytes."""
    vs = 2.0 ** -6
    T = rigid((0, 0, 1), 0.0, (2.0 ** -36, 0.0, 2.0 ** -37))
    assert np.array_equal(T[:3, :3], np.eye(3, dtype=np.float32))
    _, tv = motion(T, vs)
    u = -3.0 - tv
    f = (u - np.floor(u)).astype(np.float32)
    assert np.array_equal(np.floor(u), [-4, -3, -4]) and (u - np.floor(u))[0] < 1.0 and np.array_equal(f, np.float32([1, 0, 1]))
    rng = np.random.default_rng(1)
    coords = cluster(-1, 0)
    vox = random_blocks(rng, len(coords))
    wc, wv, st = assert_same_as_restatement(H, coords, vox, T, vs, "f = 1.0f")
    want = lattice_move(coords, vox, np.eye(3), (0, 0, 0))
    got = as_dict(wc, wv)
    assert got.keys() == want.keys() and all(np.array_equal(got[k], want[k]) for k in want)
    assert st["refused"] == 0


def lattice_move(coords, vox, P, shift):
    """The pure integer remapping g' = P g + shift of every weighted voxel: {block coord: 4096 bytes}."""
    out = {}
    P, shift = np.asarray(P, np.int64), np.asarray(shift, np.int64)
    for c, blk in zip(np.asarray(coords, np.int64), np.asarray(vox, np.uint8).reshape(len(coords), 512, 8)):
        g = (c * 8 + _OFF) @ P.T + shift
        for gi, v in zip(g[blk[:, 7] > 0], blk[blk[:, 7] > 0]):
            k = tuple(int(x) for x in gi >> 3)
            out.setdefault(k, np.zeros((512, 8), np.uint8))[((gi[0] & 7) << 6) | ((gi[1] & 7) << 3) | (gi[2] & 7)] = v
    return {k: v.reshape(4096) for k, v in out.items()}


LATTICE = [("identity", np.eye(3), (0, 0, 0)), ("90 degrees about z", [[0, -1, 0], [1, 0, 0], [0, 0, 1]], (25, -5, 2)),
           ("x -> y -> z", [[0, 0, 1], [1, 0, 0], [0, 1, 0]], (0, 0, 0))]


@pytest.mark.parametrize("name,P,shift", LATTICE, ids=[m[0] for m in LATTICE])
def test_lattice_motions_move_voxels_unchanged(H, name, P, shift):
    """u exactly integral: a signed permutation and a whole number of voxels at voxel_size 2^-6; a cluster of negative and
    positive coordinates straddling 0, weight-0 voxels inside weighted blocks."""
    vs = 2.0 ** -6
    rng = np.random.default_rng(5)
    coords = cluster(-1, 0) + [(4, -3, 2)]
    vox = random_blocks(rng, len(coords))
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = P
    T[:3, 3] = np.asarray(shift, np.float64) * vs
    wc, wv, st = assert_same_as_restatement(H, coords, vox, T, vs, name)
    want = lattice_move(coords, vox, P, shift)
    got = as_dict(wc, wv)
    assert got.keys() == want.keys() and all(np.array_equal(got[k], want[k]) for k in want), name
    assert st["refused"] == 0 and st["voxels"] == int((vox.reshape(-1, 8)[:, 7] > 0).sum())


def test_empty_and_weightless_sources(H):
    T = rigid((1, 2, 3), 37.0, (0.313, -1.07, 2.5))
    gk, gv, counts = cpp_transform(H, np.zeros((0, 3), np.int64), np.zeros((0, 4096), np.uint8), T, 0.02)
    assert len(gk) == 0 and counts == (0, 0, 0)
    vox = random_blocks(np.random.default_rng(2), 3)
    vox.reshape(-1, 8)[:, 7] = 0
    gk, gv, counts = cpp_transform(H, [(0, 0, 0), (0, 0, 1), (5, 5, 5)], vox, T, 0.02)
    assert len(gk) == 0 and counts[0] > 0 and counts[1:] == (0, 0)
    assert np_transform_map([(0, 0, 0), (0, 0, 1), (5, 5, 5)], vox, T, 0.02)[2] == dict(blocks=0, voxels=0, refused=0)


# ------------------------------------------------------------------ the planner
def test_plan_is_ascending_unique_and_a_superset(H):
    rng = np.random.default_rng(77)
    vs = 0.02
    coords = cluster(-1, 0) + [(6, 2, -9), (-300, 5, 41)]
    vox = random_blocks(rng, len(coords))
    vox.reshape(-1, 8)[:, 7] = np.maximum(vox.reshape(-1, 8)[:, 7], 1)  # every voxel weighted: every reachable block is non-empty
    for i in range(24):
        T = random_motion(rng, vs, reach=400.0)
        plan, ok = cpp_plan(H, coords, T, vs)
        assert ok and len(plan) > 0
        assert (plan[1:] > plan[:-1]).all(), "ascending and unique"
        wc, _, st = np_transform_map(coords, vox, T, vs)
        assert st["blocks"] >= len(coords)
        missing = set(np_keys(wc).tolist()) - set(plan.tolist())
        assert not missing, f"motion {i}: {len(missing)} non-empty blocks are not among the {len(plan)} candidates"


def test_plan_reports_blocks_outside_the_key_range(H):
    T = rigid((0, 0, 1), 0.0, (0.0, 0.0, 0.0))
    plan, ok = cpp_plan(H, [(B - 1, 0, 0)], T, 0.02)
    assert not ok, "the margin of the last block lies outside the key range"
    plan, ok = cpp_plan(H, [(B - 3, 0, 0), (-B + 2, 3, 3)], T, 0.02)
    assert ok and len(plan) >= 2
    T[0, 3] = 1e30
    assert not cpp_plan(H, [(0, 0, 0)], T, 0.02)[1]


def test_what_a_motion_must_be(H):
    fault = lambda T: H.mt_pose_fault(np.ascontiguousarray(T, np.float32).ctypes.data_as(f32p))  # noqa: E731
    good = rigid((1, 2, 3), 37.0, (0.313, -1.07, 2.5))
    assert fault(good) == 0 and fault(np.eye(4)) == 0
    scaled, nan, inf, row, row2, mirror = (good.copy() for _ in range(6))
    scaled[:3, :3] *= 1.01
    nan[1, 3] = np.nan
    inf[0, 0] = np.inf
    row[3, 3] = 0.5
    row2[3, 0] = 1e-30
    mirror[:3, 0] *= -1
    for T in (scaled, nan, inf, row, row2, mirror):
        assert fault(T) == 1


def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """The same entry points under AddressSanitizer and UBSan: a plain executable, nothing preloaded, nothing loaded into Python."""
    exe = str(tmp_path / "map_transform_san")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_transform_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_transform_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


# ------------------------------------------------------------------ the C ABI
def test_abi_declares_exports_and_types_the_two_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_transform_map", "drf_transform_stats"])
    assert "const float T16[16]" in src and "uint64_t out[6]" in src
    lib = L.lib()
    out = (C.c_uint64 * 6)()
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
    assert lib.drf_transform_map(None, b"a.drfmap", T, b"b.drfmap", 0) == 1 and lib.drf_transform_stats(None, out) == 1
