"""CPU: the host half of the render scope (tandem_amd/csrc/fusion_host.h -- the ray-cast reach, the frustum-cut selection of the
stored blocks a render can read, the union one RenderAsync stages, the capacity decision, the "need not wait for the scan"
predicate) compiled with plain g++ (tests/cpp/render_scope_check.cpp) and held to restatements written here on seeded inputs;
and the C ABI surface (drf_set_render_scope, drf_render_stats).  DESIGN.md §7c "Rendering the whole map"."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from fusion_helpers import abi_module, check_symbols
from test_fusion_streaming import f32, opts, restated_min_radius

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 1 << 20
u64p, f32p, f64p, intp = (C.POINTER(t) for t in (C.c_uint64, C.c_float, C.c_double, C.c_int))

OPTION_SETS = [  # those of tests/test_fusion_host.py::test_min_radius_and_update_reach_equal_the_derived_bounds
    dict(),
    dict(max_sensor_depth=2.5),
    dict(voxel_size=0.02, truncation_distance=0.08, max_sensor_depth=2.0, fx=100.0, fy=100.0, cx=63.5, cy=47.5, height=96, width=128),
    dict(voxel_size=0.005, truncation_distance=0.02, max_sensor_depth=4.0, fx=320.0, fy=330.0, cx=100.0, cy=300.0),
    dict(voxel_size=0.05, truncation_distance=0.0, max_sensor_depth=0.2),
]


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("render_scope") / "librender_scope_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/render_scope_check.cpp"), "-o", so])
    r = C.CDLL(so)
    r.rs_reach.restype = r.rs_margin.restype = C.c_double
    r.rs_min_radius.restype = C.c_float
    r.rs_rigid.argtypes = [f32p]
    r.rs_select.argtypes = [u64p, C.c_int, C.c_void_p, f32p, u64p, C.c_int, intp]
    r.rs_sphere.argtypes = [u64p, C.c_int, C.c_void_p, f32p, u64p, C.c_int]
    r.rs_plan.argtypes = [u64p, C.c_int, C.c_void_p, f32p, C.c_int, C.c_size_t, u64p, C.c_int, intp, intp]
    r.rs_needs_fold.argtypes = [C.c_void_p, f32p, f64p, C.c_double]
    return r


def fusion_options(**kw):
    from tandem_amd._lib import FusionOptions
    o = opts(**kw)
    return FusionOptions(**o), {k: f32(v) if isinstance(v, float) else v for k, v in o.items()}


def pack(c):
    c = np.asarray(c, np.int64) + B
    return ((c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]).astype(np.uint64)


def unpack(k):
    k = np.asarray(k, np.uint64).astype(np.int64)
    return np.stack([((k >> 42) & 0x1fffff) - B, ((k >> 21) & 0x1fffff) - B, (k & 0x1fffff) - B], axis=-1)


def restated_reach(q):
    """D rho + 4.5 s + 8 s + vs, s = sqrt(3) vs (the ray-cast term plus the project's margin)."""
    rho = max(math.sqrt(((u - q["cx"]) / q["fx"]) ** 2 + ((v - q["cy"]) / q["fy"]) ** 2 + 1.0)
              for u in (0, q["width"] - 1) for v in (0, q["height"] - 1))
    s = math.sqrt(3.0) * q["voxel_size"]
    return q["max_sensor_depth"] * rho + 4.5 * s + 8 * s + q["voxel_size"]


def rigid_pose(rng, centre):
    a = rng.normal(size=(3, 3))
    qm, _ = np.linalg.qr(a)
    if np.linalg.det(qm) < 0:
        qm[:, 0] = -qm[:, 0]
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = qm.astype(np.float32)
    T[:3, 3] = np.asarray(centre, np.float32)
    return T


def cloud(rng, q, centre, keep=0.5, extent=None):
    """Random blocks in a cube around `centre` that holds the whole reach sphere."""
    bsz = 8 * q["voxel_size"]
    half = int(math.ceil((extent or restated_reach(q)) / bsz)) + 2
    c0 = np.floor(np.asarray(centre) / bsz).astype(np.int64)
    n = 2 * half + 1
    step = max(1, int(math.ceil(n / 48)))  # at most ~48^3 lattice points, thinned further by `keep`
    ax = np.arange(-half, half + 1, step)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    g = g + rng.integers(0, step, g.shape)
    g = g[rng.random(len(g)) < keep] + c0
    return np.unique(pack(g))


def select(R, keys, fo, pose):
    out = np.empty(max(len(keys), 1), np.uint64)
    rigid = C.c_int()
    pose = np.ascontiguousarray(pose, np.float32).reshape(16)
    n = R.rs_select(keys.ctypes.data_as(u64p), len(keys), C.byref(fo), pose.ctypes.data_as(f32p), out.ctypes.data_as(u64p), len(out), C.byref(rigid))
    assert n <= len(out)
    return out[:n], bool(rigid.value)


def sphere(R, keys, fo, pose):
    out = np.empty(max(len(keys), 1), np.uint64)
    pose = np.ascontiguousarray(pose, np.float32).reshape(16)
    n = R.rs_sphere(keys.ctypes.data_as(u64p), len(keys), C.byref(fo), pose.ctypes.data_as(f32p), out.ctypes.data_as(u64p), len(out))
    return out[:n]


def plan(R, keys, fo, poses, capacity):
    out = np.empty(max(len(keys), 1), np.uint64)
    whole, fits = C.c_int(), C.c_int()
    ps = np.ascontiguousarray(np.stack([np.asarray(p, np.float32).reshape(16) for p in poses]), np.float32)
    n = R.rs_plan(keys.ctypes.data_as(u64p), len(keys), C.byref(fo), ps.ctypes.data_as(f32p), len(poses), capacity, out.ctypes.data_as(u64p), len(out),
                  C.byref(whole), C.byref(fits))
    return out[:n], whole.value, bool(fits.value)


def raycast_blocks(q, pose, rng, n):
    """The blocks n random ray-cast samples read, restated in numpy fp32 from k_raycast2 / interp_voxel2: sample position
    pose * ((u - cx) cur / fx, (v - cy) cur / fy, cur), centre voxel trunc(p / vs + sign(p) / 2), the eight dual-grid
    corners p - vs / 2 + {0, vs} per axis, block = voxel >> 3."""
    F = np.float32
    u = rng.integers(0, q["width"], n).astype(F)
    v = rng.integers(0, q["height"], n).astype(F)
    cur = (rng.random(n) * q["max_sensor_depth"]).astype(F)
    cur = np.minimum(cur, np.nextafter(F(q["max_sensor_depth"]), F(0)))
    cur[: n // 16] = np.nextafter(F(q["max_sensor_depth"]), F(0))  # the far plane and the image corners take part
    u[: n // 32], v[: n // 32] = 0, 0
    u[n // 32: n // 16], v[n // 32: n // 16] = q["width"] - 1, q["height"] - 1
    x = (u - F(q["cx"])) * cur / F(q["fx"])
    y = (v - F(q["cy"])) * cur / F(q["fy"])
    T = np.asarray(pose, F)
    P = [T[i, 0] * x + T[i, 1] * y + T[i, 2] * cur + T[i, 3] * F(1.0) for i in range(3)]
    vs, hv = F(q["voxel_size"]), F(q["voxel_size"]) / F(2.0)

    def voxel(a):
        return np.trunc(a / vs + np.sign(a).astype(F) * F(0.5)).astype(np.int64)
    per_axis = []
    for a in P:
        pd = a - hv
        per_axis.append([voxel(a) >> 3, voxel(pd + F(0.0)) >> 3, voxel(pd + vs) >> 3])
    blocks = [np.stack([per_axis[0][0], per_axis[1][0], per_axis[2][0]], -1)]
    for c in range(8):
        blocks.append(np.stack([per_axis[0][1 + (c & 1)], per_axis[1][1 + ((c >> 1) & 1)], per_axis[2][1 + (c >> 2)]], -1))
    return np.unique(pack(np.concatenate(blocks)))


# ------------------------------------------------------------------ reach
@pytest.mark.parametrize("kw", OPTION_SETS)
def test_render_reach_equals_the_formula_and_stays_below_the_min_radius(R, kw):
    fo, q = fusion_options(**kw)
    reach = R.rs_reach(C.byref(fo))
    assert reach == pytest.approx(restated_reach(q), rel=1e-9, abs=0)
    s = math.sqrt(3.0) * q["voxel_size"]
    assert R.rs_margin(C.byref(fo)) == pytest.approx(12.5 * s + q["voxel_size"], rel=1e-9, abs=0)
    # at the scan pose of a streaming engine no stored block is within it: stored blocks lie beyond the radius
    rmin = restated_min_radius(q)
    assert reach <= rmin - q["truncation_distance"] * (1 - 1e-9)
    # (drf_streaming_min_radius returns the bound rounded to fp32: half an ulp, 2^-24 relative)
    assert R.rs_min_radius(C.byref(fo)) * (1 + 2.0 ** -23) >= reach + q["truncation_distance"]


# ------------------------------------------------------------------ superset, tightness
@pytest.mark.parametrize("seed,kw", [(s, kw) for s, kw in enumerate(OPTION_SETS[1:] + [dict(max_sensor_depth=1.0, voxel_size=0.02)])])
def test_selection_holds_every_stored_block_the_raycast_reads(R, seed, kw):
    rng = np.random.default_rng(100 + seed)
    fo, q = fusion_options(**kw)
    m = R.rs_margin(C.byref(fo))
    hit = total = 0
    for trial in range(4):
        centre = rng.uniform(-3, 3, 3)
        pose = rigid_pose(rng, centre)
        read = raycast_blocks(q, pose, rng, 4000)
        # the store: a random cloud around the camera (thinned where the voxels are small) plus a random 60 % of what the rays read
        keys = np.unique(np.concatenate([cloud(rng, q, centre, keep=0.6), read[rng.random(len(read)) < 0.6]]))
        sel, rigid = select(R, keys, fo, pose)
        assert rigid
        sel_set = set(sel.tolist())
        assert len(sel_set) == len(sel)
        stored_and_read = np.intersect1d(read, keys)
        missing = [k for k in stored_and_read.tolist() if k not in sel_set]
        assert not missing, f"trial {trial}: {len(missing)} stored blocks the ray-cast reads were not selected, e.g. {unpack(missing[:3]).tolist()}"
        hit += len(stored_and_read)
        total += len(read)
        # a subset of the sphere query, and nothing behind the camera beyond the margin
        sph = set(sphere(R, keys, fo, pose).tolist())
        assert sel_set <= sph
        if len(sel):
            cen = (unpack(sel) * 8 + 3.5) * q["voxel_size"] - centre
            z_cam = cen @ np.asarray(pose, np.float64)[:3, 2]
            assert z_cam.min() >= -m * (1 + 1e-9)
    assert hit >= 0.5 * total and hit > 10, "the stores must hold much of what the rays read, or the test shows nothing"


def test_selection_is_strictly_smaller_than_the_sphere_inside_a_uniform_cloud(R):
    rng = np.random.default_rng(7)
    fo, q = fusion_options(max_sensor_depth=2.5)
    centre = np.array([0.3, -0.2, 0.1])
    pose = rigid_pose(rng, centre)
    keys = cloud(rng, q, centre, keep=1.0)
    sel, _ = select(R, keys, fo, pose)
    sph = sphere(R, keys, fo, pose)
    assert 0 < len(sel) < len(sph)
    assert len(sel) < 0.6 * len(sph)  # a 640x480, f = 500 frustum fills well under half of its sphere


@pytest.mark.parametrize("how", ["shear", "scale", "nan", "inf"])
def test_a_pose_that_is_not_rigid_selects_the_whole_store(R, how):
    rng = np.random.default_rng(3)
    fo, q = fusion_options(max_sensor_depth=2.5)
    pose = rigid_pose(rng, (0, 0, 0))
    keys = np.unique(np.concatenate([cloud(rng, q, (0, 0, 0), keep=0.2), pack(np.array([[5000, -7000, 3], [-200000, 0, 1]]))]))
    ok, rigid = select(R, keys, fo, pose)
    assert rigid and 0 < len(ok) < len(keys)
    if how == "shear":
        pose[0, 1] += 0.01
    elif how == "scale":
        pose[:3, :3] *= 1.002
    elif how == "nan":
        pose[1, 3] = np.nan
    else:
        pose[2, 2] = np.inf
    assert R.rs_rigid(np.ascontiguousarray(pose).reshape(16).ctypes.data_as(f32p)) == 0
    sel, rigid = select(R, keys, fo, pose)
    assert not rigid
    assert sorted(sel.tolist()) == keys.tolist()
    got, whole, _ = plan(R, keys, fo, [pose, rigid_pose(rng, (1, 0, 0))], len(keys))
    assert whole == 1 and got.tolist() == keys.tolist()


# ------------------------------------------------------------------ union, capacity
def test_union_over_poses_is_ascending_unique_and_what_the_capacity_counts(R):
    rng = np.random.default_rng(11)
    fo, q = fusion_options(max_sensor_depth=2.5)
    keys = cloud(rng, q, (0, 0, 0), keep=0.5, extent=5.0)
    a = rigid_pose(rng, (0.0, 0.0, 0.0))
    b = a.copy()
    b[:3, 3] += a[:3, :3] @ np.array([0.0, 0.0, 0.3], np.float32)  # a step forward: the two frusta overlap
    c = rigid_pose(rng, (1.5, -0.5, 0.5))
    sa, sb, sc = (set(select(R, keys, fo, p)[0].tolist()) for p in (a, b, c))
    assert sa & sb, "the overlapping poses must share blocks"
    got, whole, fits = plan(R, keys, fo, [a, b, c], 1 << 30)
    want = sorted(sa | sb | sc)
    assert whole == 0 and fits
    assert got.tolist() == want
    assert all(x < y for x, y in zip(got[:-1].tolist(), got[1:].tolist()))
    n_union, n_sum = len(want), len(sa) + len(sb) + len(sc)
    assert n_union < n_sum
    assert plan(R, keys, fo, [a, b, c], n_union)[2] is True          # the union fits exactly
    assert plan(R, keys, fo, [a, b, c], n_union - 1)[2] is False
    assert plan(R, keys, fo, [a, a, a], len(sa))[2] is True          # the same pose three times stages its blocks once
    empty = np.empty(0, np.uint64)
    got, whole, fits = plan(R, empty, fo, [a, b], 0)
    assert len(got) == 0 and whole == 0 and fits                        # an empty store stages nothing, whatever the pose


# ------------------------------------------------------------------ pending evictions
@pytest.mark.parametrize("kw", OPTION_SETS[:4])
def test_a_render_waits_for_the_scan_only_beyond_the_derived_distance(R, kw):
    """Blocks the last scan evicted lie beyond radius + 8 vs of its camera centre p: a render from q needs none of them while
    |q - p| + reach <= radius + 8 vs."""
    rng = np.random.default_rng(5)
    fo, q = fusion_options(**kw)
    reach = restated_reach(q)
    for radius in (restated_min_radius(q), restated_min_radius(q) + 0.7):
        limit = radius + 8 * q["voxel_size"] - reach
        assert limit > 0
        p = rng.uniform(-2, 2, 3)
        for _ in range(20):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            for dist, want in ((0.0, 0), (0.98 * limit, 0), (1.02 * limit + 1e-3, 1), (3 * limit + 1.0, 1)):
                pose = rigid_pose(rng, p + dist * d)
                true_dist = np.linalg.norm(pose[:3, 3].astype(np.float64) - p)
                if abs(true_dist - limit) < 1e-4 * max(1.0, limit):
                    continue  # fp32 rounding of the pose's translation on the boundary itself
                got = R.rs_needs_fold(C.byref(fo), pose.reshape(16).ctypes.data_as(f32p), p.ctypes.data_as(f64p), radius)
                assert got == want, (radius, dist, limit)
    bad = rigid_pose(rng, p)
    bad[0, 0] = np.nan
    assert R.rs_needs_fold(C.byref(fo), bad.reshape(16).ctypes.data_as(f32p), p.ctypes.data_as(f64p), 1e9) == 1


# ------------------------------------------------------------------ C ABI surface
def test_render_scope_symbols_are_declared_exported_typed_and_refuse_null():
    L = abi_module()
    src = check_symbols(L, ("drf_set_render_scope", "drf_render_stats"))
    assert re.search(r"DRF_RENDER_RESIDENT\s*=\s*0\s*,\s*DRF_RENDER_MAP\s*=\s*1", src)
    from tandem_amd import dr_fusion
    assert (dr_fusion.RENDER_RESIDENT, dr_fusion.RENDER_MAP) == (0, 1)
    out = (C.c_uint64 * 4)()
    assert L.lib().drf_set_render_scope(None, 1, 0) == 1
    assert L.lib().drf_render_stats(None, out) == 1
    assert "NULL handle" in L.lib().dr_last_error().decode()
    shim = open(os.path.join(ROOT, "tandem_amd", "libdr", "dr_fusion.h")).read()
    assert re.search(r"void SetRenderScope\(int scope, size_t capacity = 0\)", shim)
