"""CPU: the host half of depth-banded map-scope renders (tandem_amd/csrc/fusion_host.h: plan_render_bands) compiled with plain
g++ (tests/cpp/render_bands_check.cpp) and held to a numpy restatement on seeded block clouds; the superset property of a
band's block list against the restated accesses of the ray-cast; the C ABI surface (drf_set_render_bands,
drf_render_band_stats); and a sanitizer run of a stand-alone program.  DESIGN.md §7c "Rendering beyond the staging"."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from fusion_helpers import abi_module, check_symbols
from test_fusion_render_scope import OPTION_SETS, cloud, fusion_options, pack, rigid_pose, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64p, f32p, intp = (C.POINTER(t) for t in (C.c_uint64, C.c_float, C.c_int))
F = np.float32


def build_check_library(path):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/render_bands_check.cpp"), "-o", path])
    r = C.CDLL(path)
    r.rb_margin.restype = C.c_double
    r.rb_select.argtypes = [u64p, C.c_int, C.c_void_p, f32p, u64p, C.c_int, intp]
    r.rb_union.argtypes = [u64p, C.c_int, C.c_void_p, f32p, C.c_int, u64p, C.c_int]
    r.rb_plan.argtypes = [u64p, C.c_int, C.c_void_p, f32p, C.c_int, C.c_size_t, C.c_int, f32p, intp, u64p, C.c_int, intp]
    return r


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return build_check_library(str(tmp_path_factory.mktemp("render_bands") / "librender_bands_check.so"))


def flat(poses):
    return np.ascontiguousarray(np.stack([np.asarray(p, np.float32).reshape(16) for p in poses]), np.float32)


def select(R, keys, fo, pose):
    out = np.empty(max(len(keys), 1), np.uint64)
    cut = C.c_int()
    n = R.rb_select(keys.ctypes.data_as(u64p), len(keys), C.byref(fo), flat([pose]).ctypes.data_as(f32p), out.ctypes.data_as(u64p), len(out), C.byref(cut))
    return out[:n], bool(cut.value)


def union(R, keys, fo, poses):
    out = np.empty(max(len(keys), 1), np.uint64)
    n = R.rb_union(keys.ctypes.data_as(u64p), len(keys), C.byref(fo), flat(poses).ctypes.data_as(f32p), len(poses), out.ctypes.data_as(u64p), len(out))
    return out[:n]


def plan(R, keys, fo, poses, capacity, max_passes):
    """(z[P + 1], [keys of pass 0, ...]) or None."""
    out = np.empty(64 * max(len(keys), 1), np.uint64)
    z, count, total = np.zeros(65, np.float32), np.zeros(64, np.int32), C.c_int()
    P = R.rb_plan(keys.ctypes.data_as(u64p), len(keys), C.byref(fo), flat(poses).ctypes.data_as(f32p), len(poses), capacity, max_passes,
                  z.ctypes.data_as(f32p), count.ctypes.data_as(intp), out.ctypes.data_as(u64p), len(out), C.byref(total))
    if P < 0:
        return None
    assert total.value <= len(out) and count[:P].sum() == total.value
    ends = np.cumsum(count[:P])
    return z[:P + 1].copy(), [out[e - c:e].copy() for c, e in zip(count[:P], ends)]


def block_depths(q, pose, keys):
    """b_z of fusion_host.h in its order of operations: the third coordinate of R^T (centre - t), in double."""
    T = np.asarray(pose, np.float32).reshape(4, 4).astype(np.float64)
    vs = float(F(q["voxel_size"]))
    w = ((unpack(keys) * 8).astype(np.float64) + 3.5) * vs - T[:3, 3]
    return T[0, 2] * w[:, 0] + T[1, 2] * w[:, 1] + T[2, 2] * w[:, 2]


def slab_items(R, keys, fo, q, poses):
    """Per pose and selected block (key, enter, leave): pass [zs, ze) needs the block iff leave >= zs and enter < ze, with
    enter = b_z - margin - vs and leave = b_z + trunc + margin; a pose without the cut needs its blocks in every pass."""
    m, vs, tr = R.rb_margin(C.byref(fo)), float(F(q["voxel_size"])), float(F(q["truncation_distance"]))
    ks, en, le = [], [], []
    for p in poses:
        sel, cut = select(R, keys, fo, p)
        bz = block_depths(q, p, sel)
        ks.append(sel)
        en.append(bz - m - vs if cut else np.full(len(sel), -np.inf))
        le.append(bz + tr + m if cut else np.full(len(sel), np.inf))
    return np.concatenate(ks), np.concatenate(en), np.concatenate(le)


def float_down(e):
    f = F(e)
    return f if float(f) <= e else np.nextafter(f, F(-np.inf))


def restated_plan(key, enter, leave, D, capacity, max_passes):
    """The greedy sweep: a pass reaches as far as its distinct blocks stay within the capacity and ends where the first block
    that does not fit enters (rounded down to fp32); it fails if that is not past its start, or after max_passes passes."""
    order = np.lexsort((key, enter))
    key, enter, leave = key[order], enter[order], leave[order]
    zs, z, passes = F(0), [F(0)], []
    while True:
        if len(passes) >= max_passes:
            return None
        act = np.flatnonzero(leave >= float(zs))
        _, first = np.unique(key[act], return_index=True)
        first = np.sort(first)
        ze = F(D)
        if len(first) > capacity:
            e = enter[act][first[capacity]]
            if not e > float(zs):
                return None
            ze = float_down(e)
            if not ze > zs:
                return None
        passes.append(np.unique(key[(leave >= float(zs)) & (enter < float(ze))]))
        z.append(ze)
        if ze >= F(D):
            return np.array(z, np.float32), passes
        zs = ze


def capacities(n):
    return sorted({n + 3, n, (3 * n) // 4, n // 2, n // 3, n // 10, 5, 0}, reverse=True)


# ------------------------------------------------------------------ planner against the restatement
@pytest.mark.parametrize("case,kw", list(enumerate(OPTION_SETS)))
def test_plan_equals_the_restated_greedy_sweep(R, case, kw):
    rng = np.random.default_rng(40 + case)
    fo, q = fusion_options(**kw)
    D = q["max_sensor_depth"]
    banded = refused = 0
    for nposes in (1, 2, 3):
        centre = rng.uniform(-1, 1, 3)
        keys = cloud(rng, q, centre, keep=0.6)
        poses = [rigid_pose(rng, centre + rng.uniform(-0.2, 0.2, 3) * (i > 0)) for i in range(nposes)]
        want_union = union(R, keys, fo, poses)
        item = slab_items(R, keys, fo, q, poses)
        assert np.array_equal(np.unique(item[0]), want_union)
        for cap in capacities(len(want_union)):
            for max_passes in (2, 64):
                got, want = plan(R, keys, fo, poses, cap, max_passes), restated_plan(*item, D, cap, max_passes)
                what = f"{nposes} poses, capacity {cap} of {len(want_union)}, max_passes {max_passes}"
                if want is None:
                    assert got is None, what
                    refused += 1
                    continue
                assert got is not None, what
                z, passes = got
                assert z[0] == 0 and z[-1] >= F(D) and np.all(np.diff(z.astype(np.float64)) > 0), what
                assert len(passes) == len(z) - 1 <= max_passes, what
                assert np.array_equal(z, want[0]), what
                for j, (a, b) in enumerate(zip(passes, want[1])):
                    assert len(a) <= cap, (what, j)
                    assert np.array_equal(a, b), (what, j)                  # ascending, unique, the restated slab selection
                assert np.array_equal(np.unique(np.concatenate(passes)), want_union), what
                if cap >= len(want_union):                                  # a plan that fits: one pass, exactly the one-pass keys
                    assert len(passes) == 1 and np.array_equal(passes[0], want_union), what
                banded += len(passes) > 1
    assert refused > 0, "the capacities must reach below the thinnest band"
    if q["truncation_distance"] > 0 and D > 1.0:
        assert banded > 0, "no case was planned in more than one pass"


def test_too_few_passes_fail_where_more_succeed(R):
    rng = np.random.default_rng(9)
    fo, q = fusion_options(**OPTION_SETS[3])
    centre = np.zeros(3)
    keys = cloud(rng, q, centre, keep=0.6)
    pose = rigid_pose(rng, centre)
    n = len(union(R, keys, fo, [pose]))
    full = plan(R, keys, fo, [pose], n // 3, 64)
    assert full is not None and len(full[1]) >= 3
    P = len(full[1])
    assert plan(R, keys, fo, [pose], n // 3, P) is not None
    assert plan(R, keys, fo, [pose], n // 3, P - 1) is None
    assert plan(R, keys, fo, [pose], n // 3, 1) is None and plan(R, keys, fo, [pose], n, 1) is not None


@pytest.mark.parametrize("how", ["shear", "nan"])
def test_a_pose_that_is_not_rigid_puts_the_whole_store_in_every_pass(R, how):
    rng = np.random.default_rng(3)
    fo, q = fusion_options(max_sensor_depth=2.5, voxel_size=0.01, truncation_distance=0.04)
    keys = cloud(rng, q, (0, 0, 0), keep=0.3)
    good, bad = rigid_pose(rng, (0, 0, 0)), rigid_pose(rng, (0.1, 0, 0))
    if how == "shear":
        bad[0, 1] += 0.01
    else:
        bad[1, 3] = np.nan
    sel, cut = select(R, keys, fo, bad)
    assert not cut and len(sel) == len(keys)
    assert plan(R, keys, fo, [good, bad], len(keys) - 1, 64) is None        # every pass would hold the whole store
    z, passes = plan(R, keys, fo, [good, bad], len(keys), 64)
    assert len(passes) == 1 and np.array_equal(passes[0], keys)
    n_good = len(union(R, keys, fo, [good]))
    assert plan(R, keys, fo, [good], n_good // 2, 64) is not None, "the rigid pose alone bands at a capacity the other refuses"


def test_huge_reach_selection_is_not_cut_and_goes_into_every_pass(R):
    """Depth above ~10^4 voxels: select_render_blocks grows the sphere and applies no cut, so the blocks carry no depth."""
    rng = np.random.default_rng(4)
    fo, q = fusion_options(voxel_size=0.001, truncation_distance=0.004, max_sensor_depth=4.0)
    keys = cloud(rng, q, (0, 0, 0), keep=0.5)
    pose = rigid_pose(rng, (0, 0, 0))
    sel, cut = select(R, keys, fo, pose)
    assert not cut and len(sel) > 10
    assert plan(R, keys, fo, [pose], len(sel) - 1, 64) is None
    z, passes = plan(R, keys, fo, [pose], len(sel), 64)
    assert len(passes) == 1 and np.array_equal(passes[0], np.sort(sel))


# ------------------------------------------------------------------ superset
def sample_blocks(q, pose, u, v, cur):
    """The blocks the ray-cast samples (u, v, cur) read: raycast_blocks of tests/test_fusion_render_scope.py (restated in numpy
    fp32 from k_raycast2 / interp_voxel2) with the samples given instead of drawn."""
    u, v, cur = (np.asarray(a, F) for a in (u, v, cur))
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


def band_samples(rng, q, lo, hi, n):
    """n loop samples with lo <= cur < hi (both ends and their neighbours included) and, for each, a final colour sample in
    [cur - trunc, cur + vs): the image corners take part."""
    u = rng.integers(0, q["width"], n).astype(F)
    v = rng.integers(0, q["height"], n).astype(F)
    u[:n // 16], v[:n // 16] = 0, 0
    u[n // 16:n // 8], v[n // 16:n // 8] = q["width"] - 1, q["height"] - 1
    last = np.nextafter(F(hi), F(-np.inf))
    cur = (F(lo) + rng.random(n).astype(F) * (F(hi) - F(lo))).astype(F)
    cur = np.clip(cur, F(lo), last)
    cur[::7] = F(lo)
    cur[1::7] = last
    cur[2::7] = np.minimum(np.nextafter(F(lo), F(np.inf)), last)
    r = rng.random(n)
    r[::5], r[1::5] = 0.0, 1.0
    fin = (cur.astype(np.float64) - q["truncation_distance"] + r * (q["truncation_distance"] + q["voxel_size"])).astype(F)
    fin = np.minimum(fin, np.nextafter(cur + F(q["voxel_size"]), F(-np.inf)))
    fin = np.maximum(fin, cur - F(q["truncation_distance"]))
    return u, v, cur, fin


@pytest.mark.parametrize("seed,kw", list(enumerate(OPTION_SETS[1:4] + [dict(max_sensor_depth=3.0, voxel_size=0.01, truncation_distance=0.04)])))
def test_a_pass_holds_every_stored_block_its_samples_read(R, seed, kw):
    """Every block a loop sample with z_j <= cur < z_j+1 reads, and every block its final colour sample reads, is staged by
    pass j -- whichever of the call's poses the ray belongs to."""
    rng = np.random.default_rng(200 + seed)
    fo, q = fusion_options(**kw)
    D = q["max_sensor_depth"]
    checked = multi = 0
    for trial in range(3):
        centre = rng.uniform(-2, 2, 3)
        poses = [rigid_pose(rng, centre + rng.uniform(-0.3, 0.3, 3) * (i > 0)) for i in range(1 + trial % 2)]
        u, v, cur, _ = band_samples(rng, q, 0.0, D, 3000)
        read_all = np.unique(np.concatenate([sample_blocks(q, p, u, v, cur) for p in poses]))
        keys = np.unique(np.concatenate([cloud(rng, q, centre, keep=0.6), read_all[rng.random(len(read_all)) < 0.6]]))
        n = len(union(R, keys, fo, poses))
        got = next((g for g in (plan(R, keys, fo, poses, c, 64) for c in (n // 4, n // 3, n // 2, (3 * n) // 4, n)) if g is not None), None)
        assert got is not None
        z, passes = got
        multi += len(passes) > 1
        for j, staged in enumerate(passes):
            staged = set(staged.tolist())
            u, v, cur, fin = band_samples(rng, q, z[j], min(z[j + 1], F(D)), 1500)
            assert np.all((cur >= z[j]) & (cur < z[j + 1]))
            for p in poses:
                for what, c in (("loop", cur), ("colour", fin)):
                    need = np.intersect1d(sample_blocks(q, p, u, v, c), keys)
                    missing = [k for k in need.tolist() if k not in staged]
                    assert not missing, f"trial {trial}, pass {j} of {len(passes)}: {len(missing)} stored blocks a {what} sample reads are not staged, e.g. {unpack(missing[:3]).tolist()}"
                    checked += len(need)
    assert checked > 100 and multi > 0, "the stores must hold what the rays read, and some plan must band"


# ------------------------------------------------------------------ C ABI surface
def test_render_band_symbols_are_declared_exported_typed_and_refuse_null():
    L = abi_module()
    check_symbols(L, ("drf_set_render_bands", "drf_render_band_stats"))
    out = (C.c_uint64 * 4)()
    for passes in (-1, 0, 2, 64, 65):
        assert L.lib().drf_set_render_bands(None, passes) == 1
    assert "NULL handle" in L.lib().dr_last_error().decode()
    assert L.lib().drf_render_band_stats(None, out) == 1
    assert L.lib().drf_render_band_stats(None, None) == 1
    from tandem_amd.dr_fusion import DrFusion
    assert callable(DrFusion.set_render_bands) and callable(DrFusion.render_band_stats)
    shim = open(os.path.join(ROOT, "tandem_amd", "libdr", "dr_fusion.h")).read()
    assert re.search(r"void SetRenderBands\(int max_passes\)", shim)


def test_shim_program_compiles_and_links_with_gcc(tmp_path):
    """tests/cpp/render_bands_shim.cpp (run by tests/test_fusion_render_bands_gpu.py) against tandem_amd/libdr/dr_fusion.h, as C++14."""
    abi_module()
    exe = str(tmp_path / "render_bands_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tandem_amd", "libdr"), os.path.join(ROOT, "tests/cpp/render_bands_shim.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x", "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert subprocess.run([exe]).returncode == 2                            # its usage message: it needs a device to do more


# ------------------------------------------------------------------ sanitizer
def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """plan_render_bands under AddressSanitizer and UBSan: a plain executable, nothing preloaded, nothing loaded into Python."""
    exe = str(tmp_path / "render_bands_san")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/render_bands_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "render_bands_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
