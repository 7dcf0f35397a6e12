"""CPU: the host half of DrFusion's map (tandem_amd/csrc/fusion_host.h -- block keys, the host block store, the streaming
reach bounds, the reach balls, the lattice-to-block range, the merged walk and the chunk planner of the map-scope mesh pass)
compiled with plain g++ (tests/cpp/fusion_host_check.cpp) and held to brute-force restatements written here, on seeded inputs."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from test_fusion_streaming import f32, opts, restated_min_radius

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 1 << 20
u64p, i32p, f64p, szp = (C.POINTER(t) for t in (C.c_uint64, C.c_int, C.c_double, C.c_size_t))


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fusion_host") / "libfusion_host_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/fusion_host_check.cpp"), "-o", so])
    h = C.CDLL(so)
    h.fh_cell_key.restype = C.c_uint64
    h.fh_cell_key.argtypes = [C.c_uint64]
    h.fh_unpack.argtypes = [C.c_uint64, i32p]
    for f in (h.fh_min_radius, h.fh_update_reach2, h.fh_max_valid_depth):
        f.restype = C.c_float
    h.fh_max_valid_depth.argtypes = [C.POINTER(C.c_float), C.c_size_t, C.c_float, C.c_float]
    h.fh_f2i.argtypes = [C.c_float]
    for f in (h.fh_store_new, h.fh_balls_new, h.fh_plan):
        f.restype = C.c_void_p
    h.fh_store_size.restype = C.c_size_t
    h.fh_balls_farthest.restype = C.c_double
    for name in ("put", "get", "erase", "contains"):
        getattr(h, "fh_store_" + name).argtypes = [C.c_void_p, C.c_uint64] + ([C.c_void_p] if name in ("put", "get") else [])
    for f in (h.fh_store_free, h.fh_store_size, h.fh_balls_free, h.fh_balls_reset, h.fh_plan_free):
        f.argtypes = [C.c_void_p]
    h.fh_store_sorted_keys.argtypes = [C.c_void_p, u64p]
    h.fh_store_query.argtypes = [C.c_void_p, f64p, C.c_double, C.c_float, u64p, C.c_int]
    h.fh_balls_add.argtypes = [C.c_void_p, f64p, C.c_double]
    h.fh_balls_farthest.argtypes = [C.c_void_p, f64p]
    h.fh_balls_get.argtypes = [C.c_void_p, f64p]
    h.fh_block_range.argtypes = [C.POINTER(C.c_float), i32p, C.c_float, i32p]
    h.fh_merged.argtypes = [u64p, C.c_int, u64p, C.c_int, i32p, u64p, C.c_void_p]
    h.fh_plan.argtypes = [u64p, C.c_int, u64p, C.c_int, i32p, C.c_size_t, C.c_size_t, u64p, C.c_int, szp]
    h.fh_plan_get.argtypes = [C.c_void_p, u64p, u64p, szp, szp]
    return h


def pack(c):
    return ((int(c[0]) + B) << 42) | ((int(c[1]) + B) << 21) | (int(c[2]) + B)


def unpack(k):
    return ((k >> 42) & 0x1fffff) - B, ((k >> 21) & 0x1fffff) - B, (k & 0x1fffff) - B


def arr(v, t=np.uint64):
    return np.ascontiguousarray(v, dtype=t)


def ptr(a, p=u64p):
    return a.ctypes.data_as(p)


def d3(p):
    return (C.c_double * 3)(*p)


# ------------------------------------------------------------------ keys
def test_key_round_trip_at_the_range_ends_and_refusal_outside(H):
    rng = np.random.default_rng(1)
    ends = [-B, -B + 1, -1, 0, 1, B - 2, B - 1]
    cases = [(x, y, z) for x in ends for y in ends for z in ends] + [tuple(c) for c in rng.integers(-B, B, (500, 3))]
    k, c = C.c_uint64(), (C.c_int * 3)()
    for x, y, z in cases:
        assert H.fh_pack(int(x), int(y), int(z), C.byref(k)) == 1
        assert k.value == pack((x, y, z))
        H.fh_unpack(k.value, c)
        assert tuple(c) == (x, y, z)
    for bad in (B, B + 1, -B - 1, 2 ** 31 - 1, -2 ** 31):
        for axis in range(3):
            p = [0, 0, 0]
            p[axis] = bad
            assert H.fh_pack(p[0], p[1], p[2], C.byref(k)) == 0, p
    # ascending key = ascending (x, y, z)
    pts = [tuple(int(v) for v in c) for c in rng.integers(-40, 40, (300, 3))]
    assert sorted(pts) == [unpack(k) for k in sorted(pack(p) for p in pts)]


def test_cell_key_is_floor_division_by_eight(H):
    rng = np.random.default_rng(2)
    for c in [(-1, -8, -9), (-7, 7, 8), (-B, B - 1, 0), (-17, -16, -15)] + [tuple(v) for v in rng.integers(-3000, 3000, (500, 3))]:
        assert H.fh_cell_key(pack(c)) == pack([int(v) // 8 for v in c]), c


def test_f2i_saturates_and_maps_nan_to_zero(H):
    for f, want in ((float("nan"), 0), (3e9, 2 ** 31 - 1), (-3e9, -2 ** 31), (float("inf"), 2 ** 31 - 1), (-2.9, -2), (2.9, 2), (-0.0, 0)):
        assert H.fh_f2i(f) == want, f


# ------------------------------------------------------------------ host store
def test_store_put_get_erase_and_slot_reuse_keep_contents(H):
    rng = np.random.default_rng(3)
    s = H.fh_store_new()
    model = {}
    keys = [pack(c) for c in {tuple(v) for v in rng.integers(-50, 50, (3000, 3))}]  # beyond one 1024-block slab
    buf = np.empty(4096, np.uint8)

    def check():
        assert H.fh_store_size(s) == len(model)
        out = np.empty(len(model) + 1, np.uint64)
        assert H.fh_store_sorted_keys(s, ptr(out)) == len(model)
        assert out[:len(model)].tolist() == sorted(model)
        for k, v in model.items():
            assert H.fh_store_contains(s, k) == 1
            H.fh_store_get(s, k, buf.ctypes.data)
            assert np.array_equal(buf, v), k

    for k in keys[:2000]:
        model[k] = rng.integers(0, 256, 4096, dtype=np.uint8)
        H.fh_store_put(s, k, model[k].ctypes.data)
    check()
    for k in rng.permutation(keys[:2000])[:900].tolist():  # erase frees slots ...
        H.fh_store_erase(s, k)
        del model[k]
        assert H.fh_store_contains(s, k) == 0
    check()
    for k in keys[2000:]:                                  # ... which later puts reuse
        model[k] = rng.integers(0, 256, 4096, dtype=np.uint8)
        H.fh_store_put(s, k, model[k].ctypes.data)
    check()
    H.fh_store_free(s)


@pytest.mark.parametrize("case", ["few occupied cells, large radius", "many cells, small radius"])
def test_query_sphere_equals_a_linear_scan(H, case):
    """The two walks of query_sphere: span of cells in range > occupied cells (walk the occupied ones) and the reverse (walk the range)."""
    rng = np.random.default_rng(4)
    vs = f32(0.01)
    if case.startswith("few"):   # 3 clusters = a handful of cells; a 3 m radius spans thousands of 0.64 m cells
        pts = np.concatenate([c + rng.integers(-6, 6, (150, 3)) for c in ((0, 0, 0), (90, -40, 10), (-200, 30, 5))])
        queries = [((0.1, -0.2, 0.3), 3.0), ((6.0, -2.0, 1.0), 4.5), ((-16.0, 2.0, 0.0), 1.0), ((50.0, 50.0, 50.0), 2.0)]
    else:                        # 24^3 = 13824 cells occupied (a block in each, and more); a 2 m radius spans about 10^3 cells
        g = np.stack(np.meshgrid(*[np.arange(-12, 12)] * 3, indexing="ij"), -1).reshape(-1, 3) * 8
        pts = np.concatenate([g + rng.integers(0, 8, g.shape), rng.integers(-96, 96, (4000, 3))])
        queries = [((0.1, -0.2, 0.3), 2.0), ((-3.0, 2.5, 1.0), 1.5), ((5.5, 5.5, -5.5), 2.5), ((7.9, 0.0, 0.0), 0.7), ((0.0, 0.0, 0.0), 0.0)]
    keys = sorted({pack(p) for p in pts})
    s = H.fh_store_new()
    z = np.zeros(4096, np.uint8)
    for k in keys:
        H.fh_store_put(s, k, z.ctypes.data)
    cells = len({tuple(v // 8 for v in unpack(k)) for k in keys})
    out = np.empty(len(keys), np.uint64)
    hits = []
    for p, r in queries:
        span = 1
        for a in range(3):
            span *= (math.floor((p[a] + r) / (64.0 * vs)) + 1) - (math.floor((p[a] - r) / (64.0 * vs)) - 1) + 1
        assert (span > cells) == case.startswith("few"), (span, cells)
        n = H.fh_store_query(s, d3(p), r, vs, ptr(out), len(keys))
        want = [k for k in keys if sum((((8 * c + 3.5) * vs) - p[a]) ** 2 for a, c in enumerate(unpack(k))) <= r * r]
        assert sorted(out[:n].tolist()) == want
        hits.append(len(want))
    assert max(hits) > 50 and min(hits) < 5
    H.fh_store_free(s)


# ------------------------------------------------------------------ reach bounds
@pytest.mark.parametrize("kw", [
    dict(),
    dict(max_sensor_depth=2.5),
    dict(voxel_size=0.02, truncation_distance=0.08, max_sensor_depth=2.0, fx=100.0, fy=100.0, cx=63.5, cy=47.5, height=96, width=128),
    dict(voxel_size=0.005, truncation_distance=0.02, max_sensor_depth=4.0, fx=320.0, fy=330.0, cx=100.0, cy=300.0),
    dict(voxel_size=0.05, truncation_distance=0.0, max_sensor_depth=0.2),
])
def test_min_radius_and_update_reach_equal_the_derived_bounds(H, kw):
    from tandem_amd._lib import FusionOptions
    o = opts(**kw)
    fo = FusionOptions(**o)
    q = {k: f32(v) if isinstance(v, float) else v for k, v in o.items()}
    assert H.fh_options_ok(C.byref(fo)) == 1
    assert H.fh_min_radius(C.byref(fo)) == pytest.approx(restated_min_radius(q), rel=1e-6, abs=0)
    # the update reach: the voxel-update term at the block origin (7 s) + block diagonal (8 s) + a voxel, squared, 1e-5 of margin
    rho = max(math.sqrt(((u - q["cx"]) / q["fx"]) ** 2 + ((v - q["cy"]) / q["fy"]) ** 2 + 1.0) for u in (0, q["width"] - 1) for v in (0, q["height"] - 1))
    s = math.sqrt(3.0) * q["voxel_size"]
    r = q["max_sensor_depth"] * rho + q["truncation_distance"] + 15 * s + q["voxel_size"]
    assert H.fh_update_reach2(C.byref(fo)) == pytest.approx(r * r * (1 + 1e-5), rel=1e-6, abs=0)


def test_update_reach_is_infinite_for_invalid_options(H):
    from tandem_amd._lib import FusionOptions
    for bad in (dict(voxel_size=0.0), dict(fx=-1.0), dict(fy=0.0), dict(width=0), dict(height=-4), dict(max_sensor_depth=0.0),
                dict(max_sensor_depth=float("nan")), dict(truncation_distance=-0.1), dict(cx=float("inf"))):
        fo = FusionOptions(**opts(**bad))
        assert H.fh_options_ok(C.byref(fo)) == 0, bad
        assert H.fh_update_reach2(C.byref(fo)) == math.inf, bad
    assert H.fh_update_reach2(C.byref(FusionOptions(**opts(max_sensor_depth=3e38)))) == math.inf  # the square overflows fp32


def test_max_valid_depth_is_the_largest_depth_within_the_sensor_range(H):
    rng = np.random.default_rng(5)
    for n in (0, 1, 7, 8, 9, 64 * 48 + 5):
        d = rng.uniform(-1.0, 12.0, n).astype(np.float32)
        d[rng.random(n) < 0.1] = np.nan
        ok = d[(d >= np.float32(0.1)) & (d <= np.float32(10.0))]
        want = float(ok.max()) if ok.size else 0.0
        assert H.fh_max_valid_depth(d.ctypes.data_as(C.POINTER(C.c_float)), n, 0.1, 10.0) == want


# ------------------------------------------------------------------ reach balls
@pytest.mark.parametrize("seed,spread", [(0, 1.0), (1, 30.0), (2, 300.0)])
def test_reach_balls_keep_covering_what_was_added(H, seed, spread):
    """spread 1: new balls swallow old ones; 300: none does, so the list reaches 256 and collapses."""
    rng = np.random.default_rng(seed)
    b = H.fh_balls_new()
    assert H.fh_balls_farthest(b, d3((1, 2, 3))) == 0.0
    witnesses = []  # points inside an added ball
    out = np.empty((257, 4))
    sizes = []
    for step in range(700):
        c, r = rng.normal(0, spread, 3), float(rng.uniform(0.5, 8.0))
        H.fh_balls_add(b, d3(c), r)
        for _ in range(3):
            v = rng.normal(size=3)
            witnesses.append(c + v / np.linalg.norm(v) * r * rng.uniform(0, 0.999))
        n = H.fh_balls_get(b, ptr(out, f64p))
        sizes.append(n)
        assert 1 <= n <= 256
        balls = out[:n].copy()
        if step % 25 == 0 or step > 690:
            w = np.asarray(witnesses)
            dist = np.linalg.norm(w[:, None, :] - balls[None, :, :3], axis=2)
            assert np.all((dist <= balls[None, :, 3] * (1 + 1e-12)).any(axis=1)), step
            p = rng.normal(0, spread, 3)
            far = H.fh_balls_farthest(b, d3(p))
            assert far == pytest.approx(float((np.linalg.norm(balls[:, :3] - p, axis=1) + balls[:, 3]).max()), rel=1e-12)
            assert np.all(np.linalg.norm(w - p, axis=1) <= far * (1 + 1e-12))
    if spread == 1.0:
        assert max(sizes) < 256 and any(b <= a for a, b in zip(sizes, sizes[1:]))  # contained balls were dropped
    if spread == 300.0:
        assert 256 in sizes and 1 in sizes[sizes.index(256):]
    H.fh_balls_reset(b)
    assert H.fh_balls_get(b, ptr(out, f64p)) == 0
    H.fh_balls_free(b)


# ------------------------------------------------------------------ lattice range, merged walk, planner
def test_block_range_holds_every_block_that_owns_a_lattice_cell(H):
    rng = np.random.default_rng(6)
    r6 = (C.c_int * 6)()
    for _ in range(60):
        vs = np.float32(rng.choice([0.005, 0.01, 0.04]))
        lower = rng.uniform(-3, 3, 3).astype(np.float32)
        n = rng.integers(1, 200, 3).astype(np.int32)
        H.fh_block_range(lower.ctypes.data_as(C.POINTER(C.c_float)), ptr(n, i32p), float(vs), r6)
        for a in range(3):
            g = np.arange(n[a], dtype=np.float32) * vs + lower[a]                  # k_mc_axes: cell position, then its voxel
            mc = np.trunc(g / vs + np.sign(g).astype(np.float32) * np.float32(0.5)).astype(np.int64)
            blocks = np.floor_divide(mc, 8)
            assert r6[a] == blocks.min() - 1 and r6[3 + a] == blocks.max() + 1


def restated_merge(res, sto, r6):
    """ascending key over both lists, restricted to the block range; (key, stored)"""
    inside = lambda k: all(r6[a] <= c <= r6[3 + a] for a, c in enumerate(unpack(k)))
    return sorted([(k, False) for k in res if inside(k)] + [(k, True) for k in sto if inside(k)])


def restated_plan(seq, stored, own_cap, stage_cap):
    """The greedy rule, directly: a block joins the open chunk unless the chunk owns own_cap blocks already or the stored blocks
    among its 27 neighbours (itself included, if stored) would take the chunk's staged set beyond stage_cap."""
    chunks, own, stg = [], [], set()
    for k in seq:
        c = unpack(k)
        need = {q for q in (pack((c[0] + dx, c[1] + dy, c[2] + dz)) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)) if q in stored}
        if len(own) == own_cap or len(stg | need) > stage_cap:
            chunks.append((own, sorted(stg)))
            own, stg = [], set()
        own.append(k)
        stg |= need
    if own:
        chunks.append((own, sorted(stg)))
    return chunks


def make_map(kind, rng):
    if kind == "interleaved":   # resident and stored blocks mixed at random in one cloud
        pts = list({tuple(v) for v in rng.integers(-9, 9, (2500, 3))})
        stored = rng.random(len(pts)) < 0.5
        res, sto = [p for p, s in zip(pts, stored) if not s], [p for p, s in zip(pts, stored) if s]
    elif kind == "slabs":       # a stored slab next to a resident slab: the staged sets are the boundary layer
        res = [(x, y, z) for x in range(0, 6) for y in range(-8, 8) for z in range(-8, 8)]
        sto = [(x, y, z) for x in range(-6, 0) for y in range(-8, 8) for z in range(-8, 8)]
    else:                       # sparse: most neighbourhoods hold no stored block
        pts = list({tuple(v) for v in rng.integers(-40, 40, (1500, 3))})
        res, sto = pts[::2], pts[1::2]
    return sorted(pack(p) for p in res), sorted(pack(p) for p in sto)


@pytest.mark.parametrize("kind", ["interleaved", "slabs", "sparse"])
@pytest.mark.parametrize("own_cap,stage_cap", [(8192, 8192), (64, 64), (5, 27), (1000, 40)])
@pytest.mark.parametrize("form", ["all", "picked"])
def test_planner_equals_the_restated_greedy_rule(H, kind, own_cap, stage_cap, form):
    rng = np.random.default_rng(["interleaved", "slabs", "sparse"].index(kind) * 10000 + own_cap)
    res, sto = make_map(kind, rng)
    r6v = [-7, -6, -8, 5, 8, 7] if kind != "sparse" else [-30, -40, -40, 40, 25, 40]   # cuts the map on some sides
    r6 = (C.c_int * 6)(*r6v)
    ra, sa = arr(res), arr(sto)
    # the merged walk
    out, flags = np.empty(len(res) + len(sto), np.uint64), np.empty(len(res) + len(sto), np.uint8)
    m = H.fh_merged(ptr(ra), len(res), ptr(sa), len(sto), r6, ptr(out), flags.ctypes.data)
    merged = restated_merge(res, sto, r6v)
    assert 0 < m < len(res) + len(sto)
    assert list(zip(out[:m].tolist(), flags[:m].astype(bool).tolist())) == merged
    seq = [k for k, _ in merged]
    if form == "picked":
        seq = [k for k in seq if rng.random() < 0.3]
    pa = arr(seq)
    sizes = (C.c_size_t * 3)()
    h = H.fh_plan(ptr(ra), len(res), ptr(sa), len(sto), r6, own_cap, stage_cap, ptr(pa) if form == "picked" else None,
                  len(seq) if form == "picked" else -1, sizes)
    n_own, n_stg, n_ch = sizes
    own, stg = np.empty(n_own, np.uint64), np.empty(n_stg, np.uint64)
    ob, sb = np.empty(n_ch + 1, np.uintp), np.empty(n_ch + 1, np.uintp)
    H.fh_plan_get(h, ptr(own), ptr(stg), ptr(ob, szp), ptr(sb, szp))
    H.fh_plan_free(h)
    own, stg, ob, sb = own.tolist(), stg.tolist(), ob.tolist(), sb.tolist()
    # own = the merged in-range list (or the selection), ascending
    assert own == seq and own == sorted(own)
    assert ob[0] == 0 and sb[0] == 0 and ob[-1] == n_own and sb[-1] == n_stg
    stored = set(sto)
    for c in range(n_ch):
        mine, staged = own[ob[c]:ob[c + 1]], stg[sb[c]:sb[c + 1]]
        assert 0 < len(mine) <= own_cap and len(staged) <= stage_cap
        assert staged == sorted(set(staged))
        want = set()
        for k in mine:
            x, y, z = unpack(k)
            want |= {q for q in (pack((x + dx, y + dy, z + dz)) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)) if q in stored}
        assert set(staged) == want
    # chunk boundaries (hence drf_mesh_stats' chunks and uploads) = the direct restatement's
    ref = restated_plan(seq, stored, own_cap, stage_cap)
    assert [ob[c + 1] - ob[c] for c in range(n_ch)] == [len(o) for o, _ in ref]
    assert [stg[sb[c]:sb[c + 1]] for c in range(n_ch)] == [s for _, s in ref]
    if (own_cap, stage_cap) != (8192, 8192):
        assert n_ch > 3


def test_planner_with_nothing_in_range_or_nothing_picked_plans_no_chunk(H):
    res, sto = make_map("slabs", np.random.default_rng(0))
    ra, sa, sizes = arr(res), arr(sto), (C.c_size_t * 3)()
    far = (C.c_int * 6)(100, 100, 100, 120, 120, 120)
    H.fh_plan_free(H.fh_plan(ptr(ra), len(res), ptr(sa), len(sto), far, 64, 64, None, -1, sizes))
    assert list(sizes) == [0, 0, 0]
    near = (C.c_int * 6)(-9, -9, -9, 9, 9, 9)
    H.fh_plan_free(H.fh_plan(ptr(ra), len(res), ptr(sa), len(sto), near, 64, 64, ptr(arr([])), 0, sizes))
    assert list(sizes) == [0, 0, 0]
