"""CPU: the host half of drf_align_system / drf_align_map (include/dr_mi355x.h "map files", DESIGN.md §7c "Registering two maps").
align_voxel, align_block, align_system_host, align_step and align_maps_host of tandem_amd/csrc/fusion_host.h compiled with plain
g++ (tests/cpp/map_align_check.cpp) and held, bit for bit, to np_align_system / np_align_maps, numpy restatements of the rule
written here from the header's statement -- the reference of tests/test_fusion_map_align_gpu.py too; the recovery of a known pose
on three planes, against the truth; the status paths; the same under AddressSanitizer and UBSan as a stand-alone program
(tests/cpp/map_align_san.cpp); the three new names of the C ABI."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import abi_module, check_symbols
from test_map_transform import B, _OFF, cluster, motion, np_keys, random_blocks, rigid, rotation, sorted_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p, u64p, f32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_double)
CONVERGED, MAX_ITERS, DEGENERATE, LOST = 0, 1, 2, 3
_LANES = np.arange(64)
# lane l adds voxels 2 (l + 64 k) and the next for k = 0..3: the 8 voxel indices of each lane, in order
_SEQ = np.stack([2 * (_LANES + 64 * k) + t for k in range(4) for t in range(2)], axis=1)


# ------------------------------------------------------------------ the rule, restated
def np_options(vs, **opt):
    """drf_align_options_t with its defaults: a zero (or missing) field is its default."""
    o = dict(max_iters=30, min_weight=1, band=np.float32(2.0) * np.float32(vs), huber=np.float32(1.0), eps_rot=1e-7, eps_trans=1e-5, min_valid=0.25)
    for k, v in opt.items():
        assert k in o, k
        if v:
            o[k] = np.float32(v) if k in ("band", "huber") else (int(v) if k in ("max_iters", "min_weight") else float(v))
    return o


def butterfly(x):
    """x = x + x[lane ^ off] for off = 32, 16, 8, 4, 2, 1 along axis -2 (64 lanes)."""
    for off in (32, 16, 8, 4, 2, 1):
        x = x + np.take(x, _LANES ^ off, axis=-2)
    return x


def centre_src(coords):
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    if len(coords) == 0:
        return np.zeros(3, np.float64)
    return (4 * (coords.min(0) + coords.max(0) + 1)).astype(np.float64)


def np_partials(sc, sv, rk, rv, R, tv, c, vs, o):
    """The per-block half of one evaluation: source blocks sc (n, 3) with voxels sv (n, 4096), ascending by key (any run of the
    source's blocks: the blocks do not depend on each other), against the reference's ascending keys rk and voxels rv, at the pose
    (R, tv) with the centre c -> (partial (n, 28) float64, sample (n, 512) bool, valid (n, 512) bool, q (n, 512, 3))."""
    n, nr = len(sc), len(rk)
    vs64 = np.float64(np.float32(vs))
    v8 = sv.reshape(n, 512, 8)
    s_src = np.ascontiguousarray(v8[:, :, :4]).view(np.float32)[:, :, 0]
    with np.errstate(all="ignore"):
        sample = (v8[:, :, 7].astype(np.int64) >= o["min_weight"]) & (np.abs(s_src) <= o["band"])
    g = (sc[:, None, :] * 8 + _OFF[None]).astype(np.float64)
    q = np.stack([((R[k, 0] * g[..., 0] + R[k, 1] * g[..., 1]) + R[k, 2] * g[..., 2]) + tv[k] for k in range(3)], axis=-1)
    inr = ((q > -2.0 ** 30) & (q < 2.0 ** 30)).all(-1)
    q = np.where(inr[..., None], q, 0.0)
    b = np.floor(q)
    f = (q - b).astype(np.float32)
    bi = b.astype(np.int64)
    valid = sample & inr
    refv = rv.reshape(nr, 512, 8)
    s = np.zeros((2, 2, 2) + q.shape[:2], np.float32)
    for cx in range(2):
        for cy in range(2):
            for cz in range(2):
                p = bi + np.array([cx, cy, cz])
                blk = p >> 3
                ok = ((blk >= -B) & (blk < B)).all(-1)
                if nr == 0:
                    valid &= False
                    continue
                k = np_keys(np.where(ok[..., None], blk, 0).reshape(-1, 3)).reshape(ok.shape)
                at = np.minimum(np.searchsorted(rk, k), nr - 1)
                found = ok & (rk[at] == k)
                vx = refv[at, ((p[..., 0] & 7) << 6) | ((p[..., 1] & 7) << 3) | (p[..., 2] & 7)]
                valid &= found & (vx[..., 7].astype(np.int64) >= o["min_weight"])
                s[cx, cy, cz] = np.ascontiguousarray(vx[..., :4]).view(np.float32)[..., 0]
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    with np.errstate(all="ignore"):
        h = s[:, :, 1] - s[:, :, 0]                      # [cx][cy]
        e = s[:, :, 0] + fz * h
        dy = e[:, 1] - e[:, 0]                           # [cx]
        d = e[:, 0] + fy * dy
        hy = h[:, 0] + fy * (h[:, 1] - h[:, 0])
        gx = d[1] - d[0]
        phi = d[0] + fx * (d[1] - d[0])
        gy = dy[0] + fx * (dy[1] - dy[0])
        gz = hy[0] + fx * (hy[1] - hy[0])
        assert all(a.dtype == np.float32 for a in (h, e, dy, d, hy, gx, phi, gy, gz))
        r = (phi.astype(np.float64) - s_src.astype(np.float64)) / vs64
        nn = [gx.astype(np.float64) / vs64, gy.astype(np.float64) / vs64, gz.astype(np.float64) / vs64]
        x = [q[..., k] - c[k] for k in range(3)]
        J = [x[1] * nn[2] - x[2] * nn[1], x[2] * nn[0] - x[0] * nn[2], x[0] * nn[1] - x[1] * nn[0], nn[0], nn[1], nn[2]]
        a = np.abs(r)
        hub = np.float64(o["huber"])
        w = np.where(a <= hub, 1.0, hub / a)
        terms = []
        for i in range(6):
            wj = w * J[i]
            terms += [wj * J[j] for j in range(i, 6)]
        terms = terms[:21] + [(w * J[i]) * r for i in range(6)] + [(w * r) * r]
        t = np.where(valid[..., None], np.stack(terms, axis=-1), 0.0)   # (n, 512, 28); a sample that is not valid adds nothing
    assert t.dtype == np.float64
    acc = np.zeros((n, 64, 28), np.float64)
    for step in range(8):                                              # sequential, in the lane's order
        acc = acc + t[:, _SEQ[:, step], :]
    return butterfly(acc)[:, 0, :], sample, valid, q                   # (n, 28): every lane holds the block's sums


def np_fold(partial):
    """The fold over blocks: per component lane l adds partial[l], partial[l + 64], ... from +0.0, then the butterfly."""
    n = len(partial)
    pad = np.zeros((-n % 64, 28), np.float64)
    rows = np.concatenate([partial, pad]).reshape(-1, 64, 28)          # rows[j][l] = partial[l + 64 j]
    lane = np.zeros((64, 28), np.float64)
    for j in range(len(rows)):
        lane = lane + rows[j]
    return butterfly(lane)[0]


def np_centre(sc, R, tv):
    """c = R c_src + tv in the rule's order, from the source's block coordinates."""
    cs = centre_src(sc)
    return np.array([((R[k, 0] * cs[0] + R[k, 1] * cs[1]) + R[k, 2] * cs[2]) + tv[k] for k in range(3)], np.float64)


def np_system(src, ref, R, tv, vs, o, detail=False):
    """One evaluation at the pose (R (3, 3), tv (3,)) in float64: (sums (28,) float64, (samples, valid, invalid)).  src and ref are
    (block coordinates (n, 3), voxels (n, 4096) uint8).  float64 and float32 array operations, one per operation of the rule."""
    sk, sv = sorted_source(*src)
    rk, rv = sorted_source(*ref)
    n = len(sk)
    sc = np.asarray(src[0], np.int64).reshape(-1, 3)[np.argsort(np_keys(src[0]))] if n else np.zeros((0, 3), np.int64)
    c = np_centre(sc, R, tv)
    if n == 0:
        return (np.zeros(28), (0, 0, 0)) + ((dict(valid=np.zeros((0, 512), bool), q=np.zeros((0, 512, 3)), c=c, coords=sc),) if detail else ())
    partial, sample, valid, q = np_partials(sc, sv, rk, rv, R, tv, c, vs, o)
    sums = np_fold(partial)
    counts = (int(sample.sum()), int(valid.sum()), int((sample & ~valid).sum()))
    return (sums, counts) + ((dict(valid=valid, q=q, c=c, coords=sc),) if detail else ())


def np_align_system(src, ref, T, vs, **opt):
    R, tv = motion(T, vs)
    return np_system(src, ref, R, tv, vs, np_options(vs, **opt))


def np_step(sums, c, R, tv, eps_rot, eps_trans):
    """align_step in Python floats (IEEE doubles; math.sqrt is correctly rounded): (status or -1, R, tv)."""
    S = [float(v) for v in sums]
    H = [[0.0] * 6 for _ in range(6)]
    idx = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = H[j][i] = S[idx]
            idx += 1
    top = H[0][0]
    for j in range(1, 6):
        top = H[j][j] if H[j][j] > top else top
    if not top > 0.0:
        return DEGENERATE, R, tv
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        p = H[j][j]
        for k in range(j):
            p = p - L[j][k] * L[j][k]
        if not p > 1e-12 * top:
            return DEGENERATE, R, tv
        L[j][j] = math.sqrt(p)
        for i in range(j + 1, 6):
            t = H[i][j]
            for k in range(j):
                t = t - L[i][k] * L[j][k]
            L[i][j] = t / L[j][j]
    y, d = [0.0] * 6, [0.0] * 6
    for i in range(6):
        t = -S[21 + i]
        for k in range(i):
            t = t - L[i][k] * y[k]
        y[i] = t / L[i][i]
    for i in range(5, -1, -1):
        t = y[i]
        for k in range(i + 1, 6):
            t = t - L[k][i] * d[k]
        d[i] = t / L[i][i]
    oo = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    vv = (d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]
    if oo != oo or vv != vv:
        return DEGENERATE, R, tv
    if math.sqrt(oo) < eps_rot and math.sqrt(vv) < eps_trans:
        return CONVERGED, R, tv
    a = 1.0 / math.sqrt(1.0 + oo / 4.0)
    qw, qx, qy, qz = a, (a * d[0]) / 2.0, (a * d[1]) / 2.0, (a * d[2]) / 2.0
    Rq = [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
          [2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)],
          [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]]
    Rl, tl, cl = [[float(v) for v in row] for row in R], [float(v) for v in tv], [float(v) for v in c]
    e = [tl[k] - cl[k] for k in range(3)]
    R2 = np.array([[(Rq[i][0] * Rl[0][j] + Rq[i][1] * Rl[1][j]) + Rq[i][2] * Rl[2][j] for j in range(3)] for i in range(3)], np.float64)
    t2 = np.array([(cl[i] + ((Rq[i][0] * e[0] + Rq[i][1] * e[1]) + Rq[i][2] * e[2])) + d[3 + i] for i in range(3)], np.float64)
    return -1, R2, t2


def np_align_maps(src, ref, T_init, vs, **opt):
    """The loop of drf_align_map: dict(T (4, 4) float64, sums, samples, valid0, valid, cost0, cost, iterations, status, trace)."""
    o = np_options(vs, **opt)
    R, tv = motion(T_init, vs)
    good = (R, tv)
    res = dict(status=MAX_ITERS, iterations=0, sums=np.zeros(28), samples=0, valid0=0, valid=0, cost0=0.0, cost=0.0, trace=[])
    for it in range(o["max_iters"]):
        sums, counts, det = np_system(src, ref, R, tv, vs, o, detail=True)
        res["trace"].append(sums)
        cost = float(sums[27]) / float(counts[1]) if counts[1] else 0.0
        res.update(iterations=it + 1, sums=sums, samples=counts[0], valid=counts[1], cost=cost)
        if it == 0:
            res.update(valid0=counts[1], cost0=cost)
        if float(counts[1]) < o["min_valid"] * float(counts[0]) or counts[1] < 6:
            res["status"] = LOST
            R, tv = good
            break
        good = (R, tv)
        s, R, tv = np_step(sums, det["c"], R, tv, o["eps_rot"], o["eps_trans"])
        if s >= 0:
            res["status"] = s
            break
    T = np.zeros((4, 4), np.float64)
    T[:3, :3] = R
    T[:3, 3] = tv * np.float64(np.float32(vs))
    T[3, 3] = 1.0
    res["T"] = T
    return res


# ------------------------------------------------------------------ the compiled host half
class Options(C.Structure):
    _fields_ = [("max_iters", C.c_int), ("min_weight", C.c_int), ("band", C.c_float), ("huber", C.c_float),
                ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("min_valid", C.c_double)]


class Result(C.Structure):
    _fields_ = [("T", C.c_double * 16), ("sums", C.c_double * 28), ("samples", C.c_uint64), ("valid0", C.c_uint64), ("valid", C.c_uint64),
                ("cost0", C.c_double), ("cost", C.c_double), ("iterations", C.c_int), ("status", C.c_int)]


def build_check(directory):
    so = os.path.join(str(directory), "libmap_align_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_align_check.cpp"), "-o", so])
    h = C.CDLL(so)
    maps = [u64p, u8p, C.c_size_t, u64p, u8p, C.c_size_t, f32p, C.c_float, C.POINTER(Options)]
    h.ma_options.argtypes = [C.POINTER(Options), C.c_float, f64p]
    h.ma_system.argtypes = maps + [f64p, u64p]
    h.ma_align.argtypes = maps + [C.POINTER(Result), f64p, C.c_size_t]
    return h


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("map_align"))


def _maps(src, ref, T, vs, opt):
    sk, sv = sorted_source(*src)
    rk, rv = sorted_source(*ref)
    T = np.ascontiguousarray(T, np.float32)
    o = Options(**opt)
    keep = (sk, sv, rk, rv, T, o)
    return keep, (sk.ctypes.data_as(u64p), sv.ctypes.data_as(u8p), len(sk), rk.ctypes.data_as(u64p), rv.ctypes.data_as(u8p), len(rk),
                  T.ctypes.data_as(f32p), np.float32(vs), C.byref(o))


def cpp_system(H, src, ref, T, vs, **opt):
    keep, args = _maps(src, ref, T, vs, opt)
    sums, counts = np.zeros(28, np.float64), np.zeros(3, np.uint64)
    assert H.ma_system(*args, sums.ctypes.data_as(f64p), counts.ctypes.data_as(u64p)) == 0
    return sums, tuple(int(v) for v in counts)


def cpp_align(H, src, ref, T, vs, **opt):
    """align_maps_host as a dict shaped like np_align_maps' (trace: the sums of every evaluation)."""
    keep, args = _maps(src, ref, T, vs, opt)
    r = Result()
    cap = int(opt.get("max_iters", 0) or 30)
    trace = np.zeros((cap, 28), np.float64)
    assert H.ma_align(*args, C.byref(r), trace.ctypes.data_as(f64p), cap) == 0
    return dict(T=np.array(r.T, np.float64).reshape(4, 4), sums=np.array(r.sums, np.float64), samples=int(r.samples), valid0=int(r.valid0),
                valid=int(r.valid), cost0=float(r.cost0), cost=float(r.cost), iterations=int(r.iterations), status=int(r.status),
                trace=[trace[i] for i in range(int(r.iterations))])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same_system(got, want, what):
    assert got[1] == want[1], f"{what}: counts {got[1]} against {want[1]}"
    bad = np.flatnonzero(bits(got[0]) != bits(want[0]))
    assert bad.size == 0, f"{what}: sums differ at {bad.tolist()}: got {got[0][bad[:3]]} want {want[0][bad[:3]]}"


def assert_same_result(got, want, what):
    """Two results of the registration (dicts shaped like np_align_maps'), bit for bit."""
    assert (got["status"], got["iterations"]) == (want["status"], want["iterations"]), f"{what}: {got['status'], got['iterations']} against {want['status'], want['iterations']}"
    assert (got["samples"], got["valid0"], got["valid"]) == (want["samples"], want["valid0"], want["valid"]), what
    for k in ("T", "sums", "cost0", "cost"):
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{what}: {k} differs: {got[k]} against {want[k]}"
    if "trace" in got and "trace" in want:
        for i, (a, b) in enumerate(zip(got["trace"], want["trace"])):
            assert np.array_equal(bits(a), bits(b)), f"{what}: the sums of evaluation {i} differ"


# ------------------------------------------------------------------ maps
VS = 0.02
T37 = rigid((1, 2, 3), 37.0, (0.05, -0.03, 0.04))  # the rotation of the transform tests; the translation keeps the maps overlapping
SMALL = rigid((3, -1, 2), 1.5, (0.011, -0.017, 0.009))


def band_blocks(rng, n, weights=(0, 1, 2, 3, 255), vs=VS):
    """(n, 4096) blocks whose sdf lies within +-3 voxels (most of them samples at the default band of 2), weights drawn from
    `weights` and anything between."""
    v = random_blocks(rng, n)
    r = v.reshape(-1, 8)
    r[:, :4] = (rng.uniform(-3.0, 3.0, len(r)).astype(np.float32) * np.float32(vs)).view(np.uint8).reshape(-1, 4)
    pick = rng.integers(0, 2 * len(weights), len(r))
    w = rng.integers(1, 256, len(r))
    for i, wt in enumerate(weights):
        w = np.where(pick == i, wt, w)
    r[:, 7] = w
    return v


def random_pair(seed, n_src=40, vs=VS):
    """A source of n_src blocks in a cluster (negative and positive coordinates) plus outliers, and a reference that covers the
    cluster's surroundings with every fourth block missing."""
    rng = np.random.default_rng(seed)
    pool = cluster(-2, 2)
    rng.shuffle(pool)
    sc = (pool + [(x, 3, 3) for x in range(-40, 40)])[:n_src]
    src = (np.array(sc, np.int64).reshape(-1, 3), band_blocks(rng, len(sc), vs=vs))
    rc = [c for i, c in enumerate(cluster(-3, 3)) if i % 4 != 1]
    ref = (np.array(rc, np.int64), band_blocks(rng, len(rc), vs=vs))
    return src, ref


def planes_case(vs=VS, only=None, shift_ref=0):
    """Three planar patches (`only`: one of them) with unit normals n_i.  Patch i lies around lattice point 8 o_i, o_i = 25 n_i
    blocks: its plane goes through 8 o_i.  The reference holds n_i.p - d_i (float64, rounded once) at every lattice point of its
    4x4x4 blocks o_i + [-2, 1], weight 5.  The source holds n_i.(R p + t) - d_i for T_true = (R, t) on 3x3x3 blocks inside them, the
    ones around the source lattice point g_i that T_true takes to 8 o_i.
    Where the patches lie and which source voxels carry weight follows from the condition sigma_min(J) > 0.1 sigma_max(J): the
    rotation columns of J are x cross n in VOXELS, the translation columns are the unit normals, whose smallest singular value over
    these three normals is 0.29 sqrt(N) at best -- so the lever arms x cross n must stay below about 3 voxels rms.  Hence (a) the
    patches sit along their own normals from the centre c (a displacement along n does not enter x cross n: only the in-plane
    extent does), 25 blocks out because 25 n_i is integral; (b) only the source voxels within 3 voxels (per axis) of g_i carry
    weight 5, the rest of the 3x3x3 blocks weight 0; (c) one more source block without a weighted voxel makes the source's block
    bounds symmetric, so that c_src = 0 and c is the point the normals meet in.  Patches of the full 24 voxels give a ratio of 0.05.
    shift_ref moves the reference's blocks along z (blocks)."""
    vs64 = np.float64(np.float32(vs))
    normals = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [0.36, -0.48, 0.8]])
    origins = np.array([[25, 0, 0], [15, 20, 0], [9, -12, 20]], np.int64)
    assert np.array_equal(origins, 25 * normals)
    T_true = np.eye(4)
    T_true[:3, :3] = rotation((1, 2, 3), 2.0)
    T_true[:3, 3] = np.array([0.7, -0.4, 0.5]) * vs64
    rc, rvox, sc, svox = [], [], [], []
    for i in ([only] if only is not None else range(3)):
        n, o = normals[i], origins[i]
        d = n @ (o * 8 * vs64)
        gi = np.rint(T_true[:3, :3].T @ (o * 8 - np.array([0.7, -0.4, 0.5]))).astype(np.int64)
        for lo, hi, at, coords, vox, pull in ((-2, 1, o, rc, rvox, False), (-1, 1, gi >> 3, sc, svox, True)):
            c = np.array(cluster(lo, hi), np.int64) + at
            g = c[:, None, :] * 8 + _OFF[None]
            p = g.astype(np.float64) * vs64
            if pull:
                p = p @ T_true[:3, :3].T + T_true[:3, 3]
            v = np.zeros((len(c), 512, 8), np.uint8)
            v[:, :, :4] = np.ascontiguousarray((p @ n - d).astype(np.float32)).view(np.uint8).reshape(len(c), 512, 4)
            v[:, :, 4:7] = (40, 130, 220)
            v[:, :, 7] = np.where((np.abs(g - gi) <= 3).all(-1), 5, 0) if pull else 5
            coords.append(c)
            vox.append(v.reshape(len(c), 4096))
            if pull:
                assert (c >= o - 2).all() and (c <= o + 1).all(), "the source's blocks lie inside the reference's"
    rc, sc = np.concatenate(rc), np.concatenate(sc)
    rc[:, 2] += shift_ref
    lo, hi = sc.min(0), sc.max(0)
    extra = np.unique(np.stack([np.minimum(lo, -(hi + 1)), np.maximum(hi, -(lo + 1))]), axis=0)   # (c): weight 0 throughout
    have = set(map(tuple, sc.tolist()))
    extra = np.array([e for e in extra.tolist() if tuple(e) not in have], np.int64).reshape(-1, 3)
    sc = np.concatenate([sc, extra])
    assert not centre_src(sc).any()
    svox.append(np.zeros((len(extra), 4096), np.uint8))
    use = [only] if only is not None else [0, 1, 2]
    return dict(vs=vs, ref=(rc, np.concatenate(rvox)), src=(sc, np.concatenate(svox)), T_true=T_true, origins=origins[use].astype(np.float64),
                patch_normals=normals[use])


def twist_between(T_got, T_true, coords, vs):
    """The rule's step d = (omega, v) that takes the pose T_true to T_got: Rq = R_got R_true^T as the unit quaternion
    normalize(1, omega / 2), and v = tv_got - (c + Rq (tv_true - c)) with c = R_true c_src + tv_true, in voxels."""
    vs64 = np.float64(np.float32(vs))
    Rg, Rt = T_got[:3, :3], T_true[:3, :3]
    tg, tt = T_got[:3, 3] / vs64, T_true[:3, 3] / vs64
    Rq = Rg @ Rt.T
    qw = math.sqrt(max(1.0 + np.trace(Rq), 0.0)) / 2.0
    qv = np.array([Rq[2, 1] - Rq[1, 2], Rq[0, 2] - Rq[2, 0], Rq[1, 0] - Rq[0, 1]]) / (4.0 * qw)
    c = Rt @ centre_src(coords) + tt
    return np.concatenate([2.0 * qv / qw, tg - (c + Rq @ (tt - c))])


def plane_bound(case, src=None, T_truth=None, eps_scale=1.0):
    """(bound on |d|, N, sigma_min, sigma_max, counts at the truth) for the source `src` (default: the case's) whose true pose is
    T_truth (default: the case's T_true).  eps = 1e-5 max|sdf| / voxel_size voxels of rounding per sample (the bound of
    tests/test_fusion_map_transform_gpu.py for an interpolated plane), J the float64 Jacobian at the truth from the analytic normals
    (a sample belongs to the patch whose middle its image is nearest to) over the samples valid there; a least-squares solve turns
    residual noise e into a pose error of at most |e| / sigma_min(J) <= eps sqrt(N) / sigma_min; ten times that is allowed."""
    vs = case["vs"]
    vs64 = np.float64(np.float32(vs))
    src = case["src"] if src is None else src
    Tt = case["T_true"] if T_truth is None else T_truth
    _, counts, det = np_system(src, case["ref"], Tt[:3, :3], Tt[:3, 3] / vs64, vs, np_options(vs), detail=True)
    q = det["q"][det["valid"]]
    nearest = np.argmin(np.linalg.norm(q[:, None, :] - 8.0 * case["origins"][None], axis=-1), axis=1)
    nrm = case["patch_normals"][nearest]
    x = q - det["c"]
    J = np.concatenate([np.cross(x, nrm), nrm], axis=1)
    sv = np.linalg.svd(J, compute_uv=False)
    sdf = [np.ascontiguousarray(m[1].reshape(-1, 8)[:, :4]).view(np.float32) for m in (src, case["ref"])]
    eps = eps_scale * 1e-5 * max(float(np.abs(v).max()) for v in sdf) / vs
    N = len(J)
    return 10.0 * eps * math.sqrt(N) / sv[-1], N, sv[-1], sv[0], counts


@pytest.fixture(scope="module")
def planes():
    return planes_case()


# ------------------------------------------------------------------ the system against the restatement
SYSTEM_CASES = [("T37", T37, {}), ("small", SMALL, {}), ("identity", np.eye(4, dtype=np.float32), {}), ("min_weight 3", SMALL, dict(min_weight=3)),
                ("wide band, tight huber", SMALL, dict(band=0.05, huber=0.25))]


@pytest.mark.parametrize("name,T,opt", SYSTEM_CASES, ids=[c[0] for c in SYSTEM_CASES])
def test_system_against_the_restatement_on_random_maps(H, name, T, opt):
    """About 40 source blocks with negative coordinates, reference blocks missing inside the 27, weights 0, 1, 2, 3, 255."""
    src, ref = random_pair(3)
    w = src[1].reshape(-1, 8)[:, 7]
    assert all((w == k).any() for k in (0, 1, 2, 3, 255))
    want = np_align_system(src, ref, T, VS, **opt)
    assert_same_system(cpp_system(H, src, ref, T, VS, **opt), want, name)
    assert want[1][0] > 5000 and want[1][1] > 0 and want[1][2] > 0, want[1]
    if name == "min_weight 3":
        assert want[1] != np_align_system(src, ref, T, VS)[1]


def test_lattice_motion_gives_the_difference_of_the_fields(H):
    """voxel_size 2^-6, a signed permutation and whole voxels: f = 0 everywhere, phi is the reference's voxel itself and every valid
    sample's residual is (s_ref - s_src) / voxel_size exactly; [27] is recomputed from that alone."""
    vs = 2.0 ** -6
    src, ref = random_pair(5, vs=vs)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = np.array([3, -5, 2]) * vs
    o = np_options(vs)
    sums, counts, det = np_system(src, ref, *motion(T, vs), vs, o, detail=True)
    assert_same_system(cpp_system(H, src, ref, T, vs), (sums, counts), "lattice")
    assert counts[1] > 100
    ref_at = {tuple(int(v) for v in c): b.reshape(512, 8) for c, b in zip(*ref)}
    sk, sv = sorted_source(*src)
    v8 = sv.reshape(-1, 512, 8)
    r = []
    for i, j in zip(*np.nonzero(det["valid"])):
        p = det["q"][i, j].astype(np.int64)
        assert np.array_equal(p.astype(np.float64), det["q"][i, j])
        s_ref = ref_at[tuple(int(v) for v in p >> 3)][((p[0] & 7) << 6) | ((p[1] & 7) << 3) | (p[2] & 7), :4].copy().view(np.float32)[0]
        r.append((np.float64(s_ref) - np.float64(v8[i, j, :4].copy().view(np.float32)[0])) / np.float64(vs))
    r = np.array(r)
    w = np.where(np.abs(r) <= 1.0, 1.0, 1.0 / np.abs(r))
    assert abs(float(((w * r) * r).sum()) - sums[27]) <= 1e-9 * sums[27]


def test_positions_next_to_whole_numbers(H):
    """q within 1e-12 of whole numbers: identity rotation, tv = (2^-40, -2^-40, 0) at voxel_size 2^-6 -- floor goes one down on y,
    where f rounds to 1.0f."""
    vs = 2.0 ** -6
    src, ref = random_pair(6, vs=vs)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [2.0 ** -46, -2.0 ** -46, 0.0]
    _, tv = motion(T, vs)
    assert np.array_equal(tv, [2.0 ** -40, -2.0 ** -40, 0.0])
    q = 5.0 + tv
    assert np.array_equal(np.floor(q), [5, 4, 5]) and (q - np.floor(q)).astype(np.float32)[1] == 1.0
    want = np_align_system(src, ref, T, vs)
    assert_same_system(cpp_system(H, src, ref, T, vs), want, "whole numbers")
    assert want[1][1] > 0


def test_a_block_near_the_edge_of_the_key_range(H):
    rng = np.random.default_rng(8)
    sc = np.array([(B - 1, 0, 0), (B - 2, 0, 0), (-B, -B, -B), (0, 0, 0)], np.int64)
    src = (sc, band_blocks(rng, len(sc)))
    ref = (sc, band_blocks(rng, len(sc)))
    for name, T in (("identity", np.eye(4, dtype=np.float32)), ("pushed out", rigid((0, 0, 1), 0.0, (3 * VS, 0, 0)))):
        want = np_align_system(src, ref, T, VS)
        assert_same_system(cpp_system(H, src, ref, T, VS), want, name)
        assert want[1][1] > 0 and want[1][2] > 0


@pytest.mark.parametrize("n_src", [1, 3, 63, 64, 65, 130])
def test_block_counts_around_the_grid_and_fold_tails(H, n_src):
    src, ref = random_pair(10 + n_src, n_src=n_src)
    assert len(src[0]) == n_src
    want = np_align_system(src, ref, SMALL, VS)
    assert_same_system(cpp_system(H, src, ref, SMALL, VS), want, f"{n_src} blocks")
    assert want[1][1] > 0


def test_empty_maps(H):
    src, ref = random_pair(4)
    none = (np.zeros((0, 3), np.int64), np.zeros((0, 4096), np.uint8))
    for name, s, r in (("empty source", none, ref), ("empty reference", src, none), ("both empty", none, none)):
        want = np_align_system(s, r, SMALL, VS)
        got = cpp_system(H, s, r, SMALL, VS)
        assert_same_system(got, want, name)
        assert not got[0].any() and got[1][1] == 0
        res = cpp_align(H, s, r, SMALL, VS)
        assert_same_result(res, np_align_maps(s, r, SMALL, VS), name)
        assert res["status"] == LOST and res["iterations"] == 1
        assert np.array_equal(res["T"][:3, :3], SMALL[:3, :3].astype(np.float64))


def test_options_and_their_defaults(H):
    out = np.zeros(7, np.float64)
    assert H.ma_options(None, np.float32(VS), out.ctypes.data_as(f64p)) == 0
    o = np_options(VS)
    assert out.tolist() == [30, 1, float(o["band"]), 1.0, 1e-7, 1e-5, 0.25]
    assert H.ma_options(C.byref(Options(max_iters=7, min_weight=3, band=0.5, huber=2.0, eps_rot=1e-3, eps_trans=1e-2, min_valid=0.5)), np.float32(VS), out.ctypes.data_as(f64p)) == 0
    assert out.tolist() == [7, 3, 0.5, 2.0, 1e-3, 1e-2, 0.5]
    for bad in (dict(max_iters=-1), dict(min_weight=-2), dict(band=-1.0), dict(huber=float("nan")), dict(eps_rot=-1.0), dict(eps_trans=float("inf")), dict(min_valid=-0.1)):
        assert H.ma_options(C.byref(Options(**bad)), np.float32(VS), out.ctypes.data_as(f64p)) == 1, bad


# ------------------------------------------------------------------ the registration against the restatement
def test_registration_against_the_restatement_on_random_maps(H):
    """Noise has no pose: whatever status this ends in, every evaluation and the final pose agree bit for bit."""
    src, ref = random_pair(3)
    for name, opt in (("few iterations", dict(max_iters=6, min_valid=0.01)), ("min_weight 3", dict(max_iters=4, min_weight=3, huber=0.5, min_valid=0.01))):
        got, want = cpp_align(H, src, ref, SMALL, VS, **opt), np_align_maps(src, ref, SMALL, VS, **opt)
        assert_same_result(got, want, name)
        assert got["iterations"] >= 2


def test_registration_against_the_restatement_on_planes(H, planes):
    got = cpp_align(H, planes["src"], planes["ref"], np.eye(4, dtype=np.float32), VS)
    assert_same_result(got, np_align_maps(planes["src"], planes["ref"], np.eye(4, dtype=np.float32), VS), "planes")
    assert got["status"] == CONVERGED


# ------------------------------------------------------------------ meaning
def test_planes_recover_the_known_pose(H, planes):
    """From the identity to T_true (2 degrees about (1, 2, 3), (0.7, -0.4, 0.5) voxels), compared with the truth itself."""
    bound, N, smin, smax, at_truth = plane_bound(planes)
    at_init = np_align_system(planes["src"], planes["ref"], np.eye(4, dtype=np.float32), VS)[1]
    print("planes: %d samples, valid %d at the identity, %d at the truth; sigma %.3g .. %.3g" % (at_init[0], at_init[1], at_truth[1], smin, smax))
    assert at_init[1] >= 0.5 * at_init[0] and at_truth[1] >= 0.9 * at_truth[0]
    assert smin > 0.1 * smax
    res = cpp_align(H, planes["src"], planes["ref"], np.eye(4, dtype=np.float32), VS)
    assert res["status"] == CONVERGED and res["iterations"] <= 20, (res["status"], res["iterations"])
    d = twist_between(res["T"], planes["T_true"], planes["src"][0], VS)
    print("planes: %d evaluations, cost %.3g -> %.3g, |d| %.3g, bound %.3g" % (res["iterations"], res["cost0"], res["cost"], np.linalg.norm(d), bound))
    assert np.linalg.norm(d) <= bound
    assert res["cost"] < 1e-6 * res["cost0"]


# ------------------------------------------------------------------ status paths
def test_one_plane_is_degenerate(H):
    one = planes_case(only=2)
    res = cpp_align(H, one["src"], one["ref"], np.eye(4, dtype=np.float32), VS)
    assert res["status"] == DEGENERATE and res["iterations"] == 1 and res["valid"] > 100
    assert np.array_equal(res["T"], np.eye(4))


def test_a_reference_far_away_is_lost(H):
    far = planes_case(shift_ref=5)                                     # 40 voxels along z
    res = cpp_align(H, far["src"], far["ref"], np.eye(4, dtype=np.float32), VS)
    assert res["status"] == LOST and res["iterations"] == 1 and res["valid"] < 0.25 * res["samples"]
    assert np.array_equal(res["T"], np.eye(4))


def test_max_iters_moves_the_pose(H, planes):
    res = cpp_align(H, planes["src"], planes["ref"], np.eye(4, dtype=np.float32), VS, max_iters=1)
    assert res["status"] == MAX_ITERS and res["iterations"] == 1
    d0 = np.linalg.norm(twist_between(np.eye(4), planes["T_true"], planes["src"][0], VS))
    d1 = np.linalg.norm(twist_between(res["T"], planes["T_true"], planes["src"][0], VS))
    print("one step: |d| %.3g -> %.3g" % (d0, d1))
    assert d1 < 0.5 * d0


def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """align_maps_host, the empty maps and the refused motions under AddressSanitizer and UBSan: a plain executable, nothing
    preloaded, nothing loaded into Python."""
    exe = str(tmp_path / "map_align_san")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_align_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_align_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


# ------------------------------------------------------------------ the C ABI
def test_abi_declares_exports_and_types_the_three_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_align_system", "drf_align_map", "drf_align_stats"])
    assert "drf_align_options_t" in src and "drf_align_result_t" in src and "double sums[28]" in src
    assert C.sizeof(L.AlignOptions) == C.sizeof(Options) == 40 and C.sizeof(L.AlignResultStruct) == C.sizeof(Result) == 400
    lib = L.lib()
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
    sums, counts, out = (C.c_double * 28)(), (C.c_uint64 * 3)(), (C.c_uint64 * 6)()
    assert lib.drf_align_system(None, b"a.drfmap", b"b.drfmap", T, None, sums, counts) == 1
    assert lib.drf_align_map(None, b"a.drfmap", b"b.drfmap", T, None, T, None) == 1
    assert lib.drf_align_stats(None, out) == 1
