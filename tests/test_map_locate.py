"""CPU: the host half of drf_locate_system / drf_locate_frame (include/dr_mi355x.h "map files", DESIGN.md §7c "Locating a depth
frame in the map").  locate_pixel, locate_group, locate_system_host and locate_frame_host of tandem_amd/csrc/fusion_host.h compiled
with plain g++ (tests/cpp/map_locate_check.cpp) and held, bit for bit, to np_locate_system / np_locate_frame, numpy restatements of
the rule written here from the header's statement -- the reference of tests/test_fusion_map_locate_gpu.py too; the recovery of a
known pose on three analytic planes and on a map integrated by the CPU oracle, against the truth; the status paths; the same under
AddressSanitizer and UBSan as a stand-alone program (tests/cpp/map_locate_san.cpp); the five new names of the C ABI.
np_fold, np_step, butterfly, the keys and the motion come from tests/test_map_align.py and tests/test_map_transform.py by import;
the field arithmetic there is written inside np_partials over source blocks, so its nine lines are restated here over points."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import abi_module, check_symbols
from test_map_align import (CONVERGED, DEGENERATE, LOST, MAX_ITERS, Result, assert_same_result, assert_same_system, band_blocks, butterfly, np_fold, np_step)
from test_map_transform import B, _OFF, cluster, motion, np_keys, rigid, rotation, sorted_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p, u64p, f32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_double)
VS, H, W = 0.02, 96, 128


def camera(vs=VS, height=H, width=W, **kw):
    """The engine options of the locate tests (those of tests/test_fusion_map_transform_gpu.py): what the rule reads of them is
    width, height, fx, fy, cx, cy, voxel_size, truncation_distance and the sensor's depth range."""
    d = dict(voxel_size=vs, num_buckets=4000, bucket_size=10, num_blocks=4000, block_size=8, max_sdf_weight=64, truncation_distance=4 * vs,
             max_sensor_depth=10.0, min_sensor_depth=0.1, num_render_streams=1, fx=110.0, fy=110.0, cx=63.5, cy=47.5, height=height, width=width)
    d.update(kw)
    return d


# ------------------------------------------------------------------ the rule, restated
def np_options(cam, **opt):
    """drf_locate_options_t with its defaults: a zero (or missing) field is its default."""
    o = dict(max_iters=30, min_weight=1, step=1, band=np.float32(cam["truncation_distance"]), huber=np.float32(1.0), centre_depth=np.float32(0.0),
             eps_rot=1e-7, eps_trans=1e-5, min_valid=0.25)
    for k, v in opt.items():
        assert k in o, k
        if v:
            o[k] = np.float32(v) if k in ("band", "huber", "centre_depth") else (int(v) if k in ("max_iters", "min_weight", "step") else float(v))
    return o


def np_centre(R, tv, cam, o):
    """c = Rd c_src + tv with c_src = (0, 0, (double)centre_depth / vs), in the rule's order."""
    cs = [0.0, 0.0, float(np.float64(o["centre_depth"]) / np.float64(np.float32(cam["voxel_size"])))]
    return np.array([((R[k, 0] * cs[0] + R[k, 1] * cs[1]) + R[k, 2] * cs[2]) + tv[k] for k in range(3)], np.float64)


def np_system(blocks, cam, depth, R, tv, o, detail=False):
    """One evaluation at the pose (R (3, 3), tv (3,)) in float64: (sums (28,) float64, (samples, valid, unobserved, outside)).
    blocks is (block coordinates (n, 3), voxels (n, 4096) uint8), depth (H, W) float32.  float64 and float32 array operations,
    one per operation of the rule, over all grid positions at once."""
    f32, f64 = np.float32, np.float64
    rk, rv = sorted_source(*blocks)
    nr = len(rk)
    Wd, Hd, step = int(cam["width"]), int(cam["height"]), int(o["step"])
    Wg, Hg = -(-Wd // step), -(-Hd // step)
    total = Wg * Hg
    groups = -(-total // 512)
    depth = np.ascontiguousarray(depth, f32).reshape(Hd, Wd)
    n = np.arange(groups * 512)
    inside = n < total
    j, i = np.where(inside, n // Wg, 0), np.where(inside, n % Wg, 0)
    u, v = step * i, step * j
    dep = depth[v, u]
    with np.errstate(all="ignore"):
        sample = inside & (dep > f32(0)) & (dep >= f32(cam["min_sensor_depth"])) & (dep <= f32(cam["max_sensor_depth"]))
    vs64 = f64(f32(cam["voxel_size"]))
    z = np.where(sample, dep, f32(1)).astype(f64)
    g = [(((u.astype(f64) - f64(f32(cam["cx"]))) / f64(f32(cam["fx"]))) * z) / vs64, (((v.astype(f64) - f64(f32(cam["cy"]))) / f64(f32(cam["fy"]))) * z) / vs64,
         z / vs64]
    q = np.stack([((R[k, 0] * g[0] + R[k, 1] * g[1]) + R[k, 2] * g[2]) + tv[k] for k in range(3)], axis=-1)
    c = np_centre(R, tv, cam, o)
    inr = ((q > -2.0 ** 30) & (q < 2.0 ** 30)).all(-1)
    q = np.where(inr[..., None], q, 0.0)
    b = np.floor(q)
    f = (q - b).astype(f32)
    bi = b.astype(np.int64)
    observed = sample & inr
    refv = rv.reshape(nr, 512, 8)
    s = np.zeros((2, 2, 2, len(n)), f32)
    for cx in range(2):
        for cy in range(2):
            for cz in range(2):
                p = bi + np.array([cx, cy, cz])
                blk = p >> 3
                ok = ((blk >= -B) & (blk < B)).all(-1)
                if nr == 0:
                    observed &= False
                    continue
                k = np_keys(np.where(ok[..., None], blk, 0).reshape(-1, 3)).reshape(ok.shape)
                at = np.minimum(np.searchsorted(rk, k), nr - 1)
                found = ok & (rk[at] == k)
                vx = refv[at, ((p[..., 0] & 7) << 6) | ((p[..., 1] & 7) << 3) | (p[..., 2] & 7)]
                observed &= found & (vx[..., 7].astype(np.int64) >= o["min_weight"])
                s[cx, cy, cz] = np.ascontiguousarray(vx[..., :4]).view(f32)[..., 0]
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
        assert all(a.dtype == f32 for a in (h, e, dy, d, hy, gx, phi, gy, gz))
        near = np.abs(phi) < o["band"]                   # fp32 compare; a NaN is outside
        valid, outside = observed & near, observed & ~near
        r = phi.astype(f64) / vs64                       # s_src = 0: (double)phi - 0.0 is (double)phi
        nn = [gx.astype(f64) / vs64, gy.astype(f64) / vs64, gz.astype(f64) / vs64]
        x = [q[..., k] - c[k] for k in range(3)]
        J = [x[1] * nn[2] - x[2] * nn[1], x[2] * nn[0] - x[0] * nn[2], x[0] * nn[1] - x[1] * nn[0], nn[0], nn[1], nn[2]]
        a = np.abs(r)
        hub = f64(o["huber"])
        w = np.where(a <= hub, 1.0, hub / a)
        terms = []
        for ii in range(6):
            wj = w * J[ii]
            terms += [wj * J[jj] for jj in range(ii, 6)]
        terms = terms[:21] + [(w * J[ii]) * r for ii in range(6)] + [(w * r) * r]
        t = np.where(valid[..., None], np.stack(terms, axis=-1), 0.0)   # a sample that is not valid adds nothing
    assert t.dtype == f64
    t = t.reshape(groups, 8, 64, 28)                                    # position 512 i + l + 64 k -> [i][k][l]
    acc = np.zeros((groups, 64, 28), f64)
    for k in range(8):                                                  # sequential, in the lane's order
        acc = acc + t[:, k]
    partial = butterfly(acc)[:, 0, :]
    sums = np_fold(partial) if groups else np.zeros(28)
    counts = (int(sample.sum()), int(valid.sum()), int((sample & ~observed).sum()), int(outside.sum()))
    assert counts[0] == counts[1] + counts[2] + counts[3]
    return (sums, counts) + ((dict(valid=valid, q=q, c=c, partial=partial, u=u, v=v, phi=phi),) if detail else ())


def np_locate_system(blocks, cam, depth, pose, **opt):
    R, tv = motion(pose, cam["voxel_size"])
    return np_system(blocks, cam, depth, R, tv, np_options(cam, **opt))


def np_locate_frame(blocks, cam, depth, pose_init, **opt):
    """The loop of drf_locate_frame: a dict shaped like test_map_align.np_align_maps' (T: camera-to-world), plus counts4, the four
    counters of the last evaluation."""
    o = np_options(cam, **opt)
    R, tv = motion(pose_init, cam["voxel_size"])
    good = (R, tv)
    res = dict(status=MAX_ITERS, iterations=0, sums=np.zeros(28), samples=0, valid0=0, valid=0, cost0=0.0, cost=0.0, trace=[], counts4=(0, 0, 0, 0))
    for it in range(o["max_iters"]):
        sums, c4, det = np_system(blocks, cam, depth, R, tv, o, detail=True)
        counts = (c4[0], c4[1], c4[2] + c4[3])
        res["trace"].append(sums)
        cost = float(sums[27]) / float(counts[1]) if counts[1] else 0.0
        res.update(iterations=it + 1, sums=sums, samples=counts[0], valid=counts[1], cost=cost, counts4=c4)
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
    T[:3, 3] = tv * np.float64(np.float32(cam["voxel_size"]))
    T[3, 3] = 1.0
    res["T"] = T
    return res


# ------------------------------------------------------------------ the compiled host half
class Options(C.Structure):
    _fields_ = [("max_iters", C.c_int), ("min_weight", C.c_int), ("step", C.c_int), ("band", C.c_float), ("huber", C.c_float), ("centre_depth", C.c_float),
                ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("min_valid", C.c_double)]


class Camera(C.Structure):
    """drf_options_t"""
    _fields_ = [("voxel_size", C.c_float), ("num_buckets", C.c_int), ("bucket_size", C.c_int), ("num_blocks", C.c_int), ("block_size", C.c_int),
                ("max_sdf_weight", C.c_int), ("truncation_distance", C.c_float), ("max_sensor_depth", C.c_float), ("min_sensor_depth", C.c_float),
                ("num_render_streams", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("height", C.c_int), ("width", C.c_int)]


def build_check(directory):
    so = os.path.join(str(directory), "libmap_locate_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_locate_check.cpp"), "-o", so])
    h = C.CDLL(so)
    args = [u64p, u8p, C.c_size_t, C.POINTER(Camera), f32p, f32p, C.POINTER(Options)]
    h.ml_options.argtypes = [C.POINTER(Options), C.c_float, f64p, C.c_char_p]
    h.ml_system.argtypes = args + [f64p, u64p]
    h.ml_frame.argtypes = args + [C.POINTER(Result), f64p, C.c_size_t]
    return h


@pytest.fixture(scope="module")
def HL(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("map_locate"))


def _args(blocks, cam, depth, pose, opt):
    rk, rv = sorted_source(*blocks)
    pose = np.ascontiguousarray(pose, np.float32).reshape(16)
    depth = np.ascontiguousarray(depth, np.float32)
    assert depth.size == cam["height"] * cam["width"]
    o, cm = Options(**opt), Camera(**cam)
    keep = (rk, rv, pose, depth, o, cm)
    return keep, (rk.ctypes.data_as(u64p), rv.ctypes.data_as(u8p), len(rk), C.byref(cm), depth.ctypes.data_as(f32p), pose.ctypes.data_as(f32p), C.byref(o))


def cpp_system(HL, blocks, cam, depth, pose, **opt):
    keep, args = _args(blocks, cam, depth, pose, opt)
    sums, counts = np.zeros(28, np.float64), np.zeros(4, np.uint64)
    assert HL.ml_system(*args, sums.ctypes.data_as(f64p), counts.ctypes.data_as(u64p)) == 0
    return sums, tuple(int(v) for v in counts)


def cpp_frame(HL, blocks, cam, depth, pose, **opt):
    """locate_frame_host as a dict shaped like np_locate_frame's (trace: the sums of every evaluation)."""
    keep, args = _args(blocks, cam, depth, pose, opt)
    r = Result()
    cap = int(opt.get("max_iters", 0) or 30)
    trace = np.zeros((cap, 28), np.float64)
    assert HL.ml_frame(*args, C.byref(r), trace.ctypes.data_as(f64p), cap) == 0
    return dict(T=np.array(r.T, np.float64).reshape(4, 4), sums=np.array(r.sums, np.float64), samples=int(r.samples), valid0=int(r.valid0),
                valid=int(r.valid), cost0=float(r.cost0), cost=float(r.cost), iterations=int(r.iterations), status=int(r.status),
                trace=[trace[i] for i in range(int(r.iterations))])


# ------------------------------------------------------------------ maps, images and poses
NONE = (np.zeros((0, 3), np.int64), np.zeros((0, 4096), np.uint8))
# the camera a metre in front of the random map, turned a little: its points fall among the blocks and past their edge
POSE_RND = rigid((2, -1, 3), 4.0, (0.07, 0.03, -0.93))


def random_case(seed, height=H, width=W, shift=(0, 0, 0)):
    """A map of band-limited noise (test_map_align.band_blocks: sdf within +-3 voxels, weights 0, 1, 2, 3, 255 and anything between)
    on the blocks [-3, 3]^3 with every fourth one missing, and a depth image whose points at POSE_RND fall among them, with whole,
    zero, NaN, negative and out-of-range depths.  shift (blocks) moves map and camera together."""
    rng = np.random.default_rng(seed)
    rc = np.array([c for i, c in enumerate(cluster(-3, 3)) if i % 4 != 1], np.int64)
    blocks = (rc + np.array(shift, np.int64), band_blocks(rng, len(rc)))
    depth = rng.uniform(0.45, 1.6, (height, width)).astype(np.float32)
    pick = rng.integers(0, 40, (height, width))
    for k, val in enumerate((0.0, np.nan, -0.7, 0.05, 11.0, 1.0, np.inf, 0.1, 10.0)):
        depth[pick == k] = val
    depth[: height // 8] = 0.0                                           # whole groups without a sample (96x128, step 1: 3 groups of 4 rows)
    pose = POSE_RND.copy()
    pose[:3, 3] += (np.array(shift, np.float64) * 8 * np.float64(np.float32(VS))).astype(np.float32)
    return dict(blocks=blocks, depth=depth, pose=pose, cam=camera(height=height, width=width))


def planes_case(vs=VS, only=None, far=0):
    """Three planar patches with non-parallel unit normals n_i, seen by a camera whose true pose T_true is a turn of 2 degrees about
    (1, 2, 3) and (0.7, -0.4, 0.5) voxels away from the world's origin, looking along +z.  c = T_true (0, 0, CD) is the centre of
    rotation (centre_depth = CD = 1.04 m); patch i has its middle at P_i = c + 0.6 m * n_i and its plane through P_i with normal n_i.
    The map holds n_i.p - d_i exactly (float64, rounded once) with weight 5 at every lattice point of the 3x3x3 blocks around P_i, i
    the patch whose middle is nearest to the voxel.  The depth image is the analytic intersection of each pixel's ray at T_true with
    plane i, for the pixels whose intersection lies within EXT voxels of P_i, and 0 elsewhere.
    Where the patches lie follows from the condition sigma_min(J) > 0.1 sigma_max(J), as in test_map_align.planes_case: the rotation
    columns of J are x cross n in voxels, x = q - c, the translation columns the unit normals, whose smallest singular value over
    these normals is 0.27 sqrt(N); so the patches sit along their own normals from c (a displacement along n does not enter
    x cross n: only the in-plane extent does) and EXT = 4 voxels keeps the lever arms at about 2 voxels rms.
    only: one of the patches; far (blocks): the map moved along x."""
    vs64 = np.float64(np.float32(vs))
    CD, RHO, EXT = 1.04, 0.6, 4.0
    normals = np.array([[0.6, 0.0, 0.8], [-0.6, 0.0, 0.8], [0.0, 0.8, 0.6]])
    T_true = np.eye(4)
    T_true[:3, :3] = rotation((1, 2, 3), 2.0)
    T_true[:3, 3] = np.array([0.7, -0.4, 0.5]) * vs64
    cam = camera(vs)
    c = T_true[:3, :3] @ np.array([0.0, 0.0, np.float64(np.float32(CD))]) + T_true[:3, 3]
    use = [only] if only is not None else [0, 1, 2]
    P = c + RHO * normals[use]
    d = np.einsum("ik,ik->i", normals[use], P)
    coords = np.unique(np.concatenate([np.floor(p / (8 * vs64)).astype(np.int64) + np.array(cluster(-1, 1), np.int64) for p in P]), axis=0)
    pts = (coords[:, None, :] * 8 + _OFF[None]).astype(np.float64) * vs64
    nearest = np.argmin(np.linalg.norm(pts[:, :, None, :] - P[None, None], axis=-1), axis=-1)
    sdf = (np.einsum("bvk,bvk->bv", pts, normals[use][nearest]) - d[nearest]).astype(np.float32)
    vox = np.zeros((len(coords), 512, 8), np.uint8)
    vox[:, :, :4] = np.ascontiguousarray(sdf).view(np.uint8).reshape(len(coords), 512, 4)
    vox[:, :, 4:7] = (40, 130, 220)
    vox[:, :, 7] = 5
    uu, vv = np.meshgrid(np.arange(cam["width"], dtype=np.float64), np.arange(cam["height"], dtype=np.float64))
    ray = np.stack([(uu - np.float64(np.float32(cam["cx"]))) / np.float64(np.float32(cam["fx"])),
                    (vv - np.float64(np.float32(cam["cy"]))) / np.float64(np.float32(cam["fy"])), np.ones_like(uu)], axis=-1)
    wdir = ray @ T_true[:3, :3].T
    depth = np.zeros((cam["height"], cam["width"]), np.float32)
    for i in range(len(use)):
        z = (d[i] - normals[use][i] @ T_true[:3, 3]) / (wdir @ normals[use][i])
        hit = T_true[:3, 3] + z[..., None] * wdir
        take = (np.linalg.norm(hit - P[i], axis=-1) <= EXT * vs64) & (z > 0)
        assert not (depth[take] != 0).any(), "the patches' pixels are disjoint"
        depth[take] = z[take].astype(np.float32)
    coords = coords + np.array([far, 0, 0], np.int64)
    return dict(vs=vs, cam=cam, blocks=(coords, vox.reshape(len(coords), 4096)), depth=depth, T_true=T_true, normals=normals[use], middles=P, centre_depth=CD,
                max_ray=float(np.linalg.norm(ray, axis=-1).max()))


def start_near(T_true, axis, deg, voxels, vs=VS):
    """A start off the truth: the camera turned by deg about axis (through its own centre) and moved by `voxels`, as float32."""
    T = np.array(T_true, np.float64)
    T[:3, :3] = rotation(axis, deg) @ T[:3, :3]
    T[:3, 3] += np.asarray(voxels, np.float64) * np.float64(np.float32(vs))
    return T.astype(np.float32)


def twist_between(T_got, T_true, centre_depth, vs):
    """The rule's step d = (omega, v) that takes the pose T_true to T_got: Rq = R_got R_true^T as the unit quaternion
    normalize(1, omega / 2), and v = tv_got - (c + Rq (tv_true - c)) with c = R_true c_src + tv_true, in voxels."""
    vs64 = np.float64(np.float32(vs))
    Rg, Rt = T_got[:3, :3], T_true[:3, :3]
    tg, tt = T_got[:3, 3] / vs64, T_true[:3, 3] / vs64
    Rq = Rg @ Rt.T
    qw = math.sqrt(max(1.0 + np.trace(Rq), 0.0)) / 2.0
    qv = np.array([Rq[2, 1] - Rq[1, 2], Rq[0, 2] - Rq[2, 0], Rq[1, 0] - Rq[0, 1]]) / (4.0 * qw)
    c = Rt @ np.array([0.0, 0.0, np.float64(np.float32(centre_depth)) / vs64]) + tt
    return np.concatenate([2.0 * qv / qw, tg - (c + Rq @ (tt - c))])


def plane_bound(case):
    """(bound on |d|, N, sigma_min, sigma_max, counts at the truth), derived as test_map_align.plane_bound derives its own.  The noise
    of a sample's residual, in voxels: the fp32 rounding of dep moves the point along its ray by at most 2^-24 dep |ray|, |ray| <=
    max_ray the length of (x, y, 1), hence the residual by at most that (|n| = 1); plus 1e-5 max|sdf| / voxel_size for the
    interpolated plane's own rounding (the bound of tests/test_fusion_map_transform_gpu.py).  J is the float64 Jacobian at the truth
    from the analytic normals (a sample belongs to the patch whose middle its point is nearest to) over the samples valid there; a
    least-squares solve turns residual noise e into a pose error of at most |e| / sigma_min(J) <= eps sqrt(N) / sigma_min; ten times
    that is allowed."""
    vs64 = np.float64(np.float32(case["vs"]))
    Tt = case["T_true"]
    o = np_options(case["cam"], centre_depth=case["centre_depth"])
    _, counts, det = np_system(case["blocks"], case["cam"], case["depth"], Tt[:3, :3], Tt[:3, 3] / vs64, o, detail=True)
    q = det["q"][det["valid"]]
    nearest = np.argmin(np.linalg.norm(q[:, None, :] - case["middles"][None] / vs64, axis=-1), axis=1)
    nrm = case["normals"][nearest]
    x = q - det["c"]
    J = np.concatenate([np.cross(x, nrm), nrm], axis=1)
    sv = np.linalg.svd(J, compute_uv=False)
    sdf = np.ascontiguousarray(case["blocks"][1].reshape(-1, 8)[:, :4]).view(np.float32)
    eps = (2.0 ** -24 * float(case["depth"].max()) * case["max_ray"] + 1e-5 * float(np.abs(sdf).max())) / case["vs"]
    N = len(J)
    return 10.0 * eps * math.sqrt(N) / sv[-1], N, sv[-1], sv[0], counts


@pytest.fixture(scope="module")
def planes():
    return planes_case()


PLANES_STARTS = [("turned", (3, -1, 2), 1.5, (1.2, -0.8, 1.0)), ("moved", (0, 1, 0), -1.0, (-1.5, 1.0, 2.0))]


def scene_case():
    """synth.scene.make_scans at 96x128, the first scan integrated by the CPU oracle: the map, the scan's depth image, its pose and
    a start 1.5 voxels and 1 degree off it."""
    from oracle.tsdf_oracle import TsdfOracle
    from synth import scene
    sc = scene.make_scans(1, H, W, seed=11)
    cam = camera(fx=sc["fx"], fy=sc["fy"], cx=sc["cx"], cy=sc["cy"], num_blocks=40000, num_buckets=40000)
    orc = TsdfOracle(**cam)
    bgr, depth, pose = sc["scans"][0]
    orc.integrate(bgr, depth, pose)
    blk = orc.export_blocks()
    coords = np.array(sorted(blk), np.int64).reshape(-1, 3)
    vox = np.stack([blk[tuple(c)] for c in coords.tolist()])
    off = np.array([1.0, -0.5, 1.0])
    start = start_near(pose.astype(np.float64), (1, 1, -1), 1.0, 1.5 * off / np.linalg.norm(off))
    return dict(cam=cam, blocks=(coords, vox), depth=depth, bgr=bgr, pose=pose, start=start, centre_depth=float(np.median(depth[depth > 0])))


@pytest.fixture(scope="module")
def scene_map():
    return scene_case()


# ------------------------------------------------------------------ the system against the restatement
SYSTEM_CASES = [("defaults", {}), ("step 2", dict(step=2)), ("step 3", dict(step=3)), ("min_weight 3", dict(min_weight=3)),
                ("tight huber, narrow band", dict(huber=0.25, band=0.03)), ("centre 1.0", dict(centre_depth=1.0)),
                ("step 3, centre 1.0, min_weight 3", dict(step=3, centre_depth=1.0, min_weight=3))]


@pytest.mark.parametrize("name,opt", SYSTEM_CASES, ids=[c[0] for c in SYSTEM_CASES])
def test_system_against_the_restatement_on_random_maps(HL, name, opt):
    case = random_case(3)
    d = case["depth"]
    assert (d == 0).any() and np.isnan(d).any() and (d < 0).any() and (d == 1.0).any() and (d > 10).any() and ((d > 0) & (d < 0.1)).any()
    want = np_locate_system(case["blocks"], case["cam"], d, case["pose"], **opt)
    assert_same_system(cpp_system(HL, case["blocks"], case["cam"], d, case["pose"], **opt), want, name)
    assert want[1][0] > 1000 and want[1][1] > 30 and want[1][2] > 0, want[1]
    if "band" in opt:
        assert want[1][3] > 100, want[1]
    if name == "min_weight 3":
        assert want[1] != np_locate_system(case["blocks"], case["cam"], d, case["pose"])[1]


def test_images_without_a_sample_and_an_empty_map(HL):
    case = random_case(4)
    for name, blocks, depth in (("no samples", case["blocks"], np.zeros((H, W), np.float32)), ("NaN only", case["blocks"], np.full((H, W), np.nan, np.float32)),
                                ("empty map", NONE, case["depth"])):
        want = np_locate_system(blocks, case["cam"], depth, case["pose"])
        got = cpp_system(HL, blocks, case["cam"], depth, case["pose"])
        assert_same_system(got, want, name)
        assert not got[0].any() and got[1][1] == 0
        res = cpp_frame(HL, blocks, case["cam"], depth, case["pose"])
        assert_same_result(res, np_locate_frame(blocks, case["cam"], depth, case["pose"]), name)
        assert res["status"] == LOST and res["iterations"] == 1
        assert np.array_equal(res["T"][:3, :3], case["pose"][:3, :3].astype(np.float64))
    assert got[1][0] > 1000 and got[1][2] == got[1][0]


@pytest.mark.parametrize("height,width,step", [(96, 128, 3), (168, 200, 1), (5, 7, 1), (8, 64, 1), (9, 64, 1)])
def test_grids_with_tails(HL, height, width, step):
    """96x128 at step 3: 1 376 positions, the last group 352 wide; 168x200: 66 groups, the last 320 wide, so the fold crosses its
    64-lane stride with a tail; 35 positions; exactly one group; one group and 64 positions."""
    case = random_case(20 + height, height, width)
    case["cam"].update(cx=(width - 1) / 2.0, cy=(height - 1) / 2.0)
    want = np_locate_system(case["blocks"], case["cam"], case["depth"], case["pose"], step=step)
    assert_same_system(cpp_system(HL, case["blocks"], case["cam"], case["depth"], case["pose"], step=step), want, f"{height}x{width}/{step}")
    assert want[1][1] > 0


def test_far_blocks(HL):
    case = random_case(3, shift=(300, -270, 5))
    want = np_locate_system(case["blocks"], case["cam"], case["depth"], case["pose"])
    assert_same_system(cpp_system(HL, case["blocks"], case["cam"], case["depth"], case["pose"]), want, "far")
    assert want[1][1] > 100


def test_options_and_their_defaults(HL):
    out, name = np.zeros(9, np.float64), C.create_string_buffer(32)
    tr = np.float32(0.08)
    assert HL.ml_options(None, tr, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [30, 1, 1, float(tr), 1.0, 0.0, 1e-7, 1e-5, 0.25]
    full = dict(max_iters=7, min_weight=3, step=2, band=0.5, huber=2.0, centre_depth=1.5, eps_rot=1e-3, eps_trans=1e-2, min_valid=0.5)
    assert HL.ml_options(C.byref(Options(**full)), tr, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [7, 3, 2, 0.5, 2.0, 1.5, 1e-3, 1e-2, 0.5]
    for bad in (dict(max_iters=-1), dict(min_weight=-2), dict(step=-1), dict(band=-1.0), dict(huber=float("nan")), dict(centre_depth=-0.5),
                dict(centre_depth=float("inf")), dict(eps_rot=-1.0), dict(eps_trans=float("inf")), dict(min_valid=-0.1)):
        assert HL.ml_options(C.byref(Options(**bad)), tr, out.ctypes.data_as(f64p), name) == 1, bad
        assert name.value.decode() == list(bad)[0]


# ------------------------------------------------------------------ the refinement against the restatement
def test_refinement_against_the_restatement_on_random_maps(HL):
    """Noise has no pose: whatever status this ends in, every evaluation and the final pose agree bit for bit."""
    case = random_case(3)
    for name, opt in (("few iterations", dict(max_iters=6, min_valid=0.01)), ("step 2, min_weight 3", dict(max_iters=4, step=2, min_weight=3, huber=0.5, min_valid=0.01, centre_depth=1.0))):
        got = cpp_frame(HL, case["blocks"], case["cam"], case["depth"], case["pose"], **opt)
        assert_same_result(got, np_locate_frame(case["blocks"], case["cam"], case["depth"], case["pose"], **opt), name)
        assert got["iterations"] >= 2


def test_refinement_against_the_restatement_on_planes(HL, planes):
    start = start_near(planes["T_true"], *PLANES_STARTS[0][1:])
    got = cpp_frame(HL, planes["blocks"], planes["cam"], planes["depth"], start, centre_depth=planes["centre_depth"])
    assert_same_result(got, np_locate_frame(planes["blocks"], planes["cam"], planes["depth"], start, centre_depth=planes["centre_depth"]), "planes")
    assert got["status"] == CONVERGED


# ------------------------------------------------------------------ meaning
@pytest.mark.parametrize("name,axis,deg,voxels", PLANES_STARTS, ids=[s[0] for s in PLANES_STARTS])
def test_planes_recover_the_known_pose(HL, planes, name, axis, deg, voxels):
    """From starts a few voxels and degrees off to T_true, compared with the truth itself: the restatement alone, and the host."""
    bound, N, smin, smax, at_truth = plane_bound(planes)
    print("planes: %d samples, %d valid at the truth; sigma %.3g .. %.3g" % (at_truth[0], at_truth[1], smin, smax))
    assert at_truth[1] >= 0.9 * at_truth[0] and at_truth[1] > 200
    assert smin > 0.1 * smax
    start = start_near(planes["T_true"], axis, deg, voxels)
    want = np_locate_frame(planes["blocks"], planes["cam"], planes["depth"], start, centre_depth=planes["centre_depth"])
    res = cpp_frame(HL, planes["blocks"], planes["cam"], planes["depth"], start, centre_depth=planes["centre_depth"])
    for who, r in (("restatement", want), ("host", res)):
        assert r["status"] == CONVERGED and r["iterations"] <= 20, (who, r["status"], r["iterations"])
        d0 = np.linalg.norm(twist_between(start.astype(np.float64), planes["T_true"], planes["centre_depth"], VS))
        d = np.linalg.norm(twist_between(r["T"], planes["T_true"], planes["centre_depth"], VS))
        print("%s, %s: %d evaluations, cost %.3g -> %.3g, |d| %.3g -> %.3g, bound %.3g" % (name, who, r["iterations"], r["cost0"], r["cost"], d0, d, bound))
        assert d <= bound
        assert r["cost"] < 1e-6 * r["cost0"]


def scene_errors(T, pose, vs=VS):
    """(rotation error in degrees, translation error in voxels) of T against the scan's pose."""
    pose = np.asarray(pose, np.float64)
    Rq = T[:3, :3] @ pose[:3, :3].T
    ang = math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(Rq) - 1.0) / 2.0))))
    return ang, float(np.linalg.norm(T[:3, 3] - pose[:3, 3]) / vs)


def test_integrated_scene_recovers_the_scan_pose(HL, scene_map):
    """The first scan of synth.scene (seed 11, 96x128) integrated by the CPU oracle, the same depth image located from a start 1.5
    voxels and 1 degree off.  This fixes the lattice convention -- the map's lattice point g sits at world g * voxel_size, no
    half-voxel offset: a convention off by half a voxel would show as a translation error near 0.5 voxels.
    MEASURED on the restatement (SCENE_MEASURED below): 0.0515 degrees and 0.199 voxels -- (-0.117, -0.157, 0.033) voxels in the
    camera's frame, the lateral part being what 0.05 degrees move a scene 2.3 m away -- after 20 evaluations from the start and
    the same from the scan's pose itself: it is the minimum of this map (one scan's projective distances, trilinear), not where the
    iteration stopped.  Along the optical axis, where a half-voxel offset of the lattice would show in full, it is 0.03 voxels.
    Asserted with a factor of 2, room for another libm only (the computation is deterministic)."""
    s = scene_map
    opt = dict(centre_depth=s["centre_depth"])
    want = np_locate_frame(s["blocks"], s["cam"], s["depth"], s["start"], **opt)
    a0, t0 = scene_errors(s["start"].astype(np.float64), s["pose"])
    a, t = scene_errors(want["T"], s["pose"])
    print("scene: %d blocks, %d samples, %d valid; start %.3f deg %.3f voxels -> %.5f deg %.5f voxels after %d evaluations (status %d), cost %.3g -> %.3g" %
          (len(s["blocks"][0]), want["samples"], want["valid"], a0, t0, a, t, want["iterations"], want["status"], want["cost0"], want["cost"]))
    assert abs(a0 - 1.0) < 0.01 and abs(t0 - 1.5) < 0.01
    assert want["status"] == CONVERGED
    assert a <= 2 * SCENE_MEASURED[0] and t <= 2 * SCENE_MEASURED[1]
    assert t < 0.25, "a translation error near half a voxel means the lattice convention is wrong"
    got = cpp_frame(HL, s["blocks"], s["cam"], s["depth"], s["start"], **opt)
    assert_same_result(got, want, "scene")


# measured on the restatement (degrees, voxels); the docstring above and DESIGN.md §7c quote them
SCENE_MEASURED = (0.0515, 0.1987)


# ------------------------------------------------------------------ status paths
def test_one_plane_is_degenerate(HL):
    one = planes_case(only=2)
    res = cpp_frame(HL, one["blocks"], one["cam"], one["depth"], one["T_true"].astype(np.float32), centre_depth=one["centre_depth"])
    assert res["status"] == DEGENERATE and res["iterations"] == 1 and res["valid"] > 50
    assert np.array_equal(res["T"][:3, :3], one["T_true"].astype(np.float32)[:3, :3].astype(np.float64))


def test_a_map_far_away_is_lost(HL, planes):
    far = planes_case(far=50)
    start = start_near(far["T_true"], *PLANES_STARTS[0][1:])
    res = cpp_frame(HL, far["blocks"], far["cam"], far["depth"], start)
    assert res["status"] == LOST and res["iterations"] == 1 and res["valid"] == 0 and res["samples"] > 200
    assert np.array_equal(res["T"][:3, :3], start[:3, :3].astype(np.float64))
    assert np.array_equal(res["T"][:3, 3], start[:3, 3].astype(np.float64) / np.float64(np.float32(VS)) * np.float64(np.float32(VS)))


def test_max_iters_applies_its_step(HL, planes):
    start = start_near(planes["T_true"], *PLANES_STARTS[0][1:])
    res = cpp_frame(HL, planes["blocks"], planes["cam"], planes["depth"], start, max_iters=1, centre_depth=planes["centre_depth"])
    assert res["status"] == MAX_ITERS and res["iterations"] == 1
    d0 = np.linalg.norm(twist_between(start.astype(np.float64), planes["T_true"], planes["centre_depth"], VS))
    d1 = np.linalg.norm(twist_between(res["T"], planes["T_true"], planes["centre_depth"], VS))
    print("one step: |d| %.3g -> %.3g" % (d0, d1))
    assert d1 < 0.5 * d0


def test_a_pose_that_is_no_rigid_motion_is_refused(HL, planes):
    keep, args = _args(planes["blocks"], planes["cam"], planes["depth"], np.eye(4, dtype=np.float32), {})
    sums, counts = np.zeros(28, np.float64), np.zeros(4, np.uint64)
    scaled, nan, row, mirror = (np.eye(4, dtype=np.float32) for _ in range(4))
    scaled[:3, :3] *= 1.01
    nan[2, 3] = np.nan
    row[3, 3] = 1.0 + 2.0 ** -20
    mirror[1, 1] = -1
    for bad in (scaled, nan, row, mirror):
        a = list(args)
        a[5] = np.ascontiguousarray(bad).ctypes.data_as(f32p)
        assert HL.ml_system(*a, sums.ctypes.data_as(f64p), counts.ctypes.data_as(u64p)) == 2


def test_sanitizer_run_of_the_stand_alone_program(tmp_path, planes):
    """locate_system_host and locate_frame_host under AddressSanitizer and UBSan: a plain executable, nothing preloaded, nothing
    loaded into Python.  It reads a small case from a file (the planes, and noise with the depths that are no samples) and prints
    the sums, which are the restatement's bit for bit."""
    exe, data = str(tmp_path / "map_locate_san"), str(tmp_path / "case.bin")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_locate_san.cpp"), "-o", exe])
    start = start_near(planes["T_true"], *PLANES_STARTS[0][1:])
    rk, rv = sorted_source(*planes["blocks"])
    opt = Options(centre_depth=planes["centre_depth"])
    with open(data, "wb") as fh:
        fh.write(np.uint64(len(rk)).tobytes() + rk.tobytes() + rv.tobytes() + bytes(Camera(**planes["cam"])) + bytes(opt))
        fh.write(np.ascontiguousarray(planes["depth"], np.float32).tobytes() + np.ascontiguousarray(start, np.float32).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_locate_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith(("system", "frame"))}
    want_sys = np_locate_system(planes["blocks"], planes["cam"], planes["depth"], start, centre_depth=planes["centre_depth"])
    want = np_locate_frame(planes["blocks"], planes["cam"], planes["depth"], start, centre_depth=planes["centre_depth"])
    got = np.array([int(x, 16) for x in lines["system"][:28]], np.uint64)
    assert np.array_equal(got, np.ascontiguousarray(want_sys[0]).view(np.uint64)) and tuple(int(x) for x in lines["system"][28:]) == want_sys[1]
    got = np.array([int(x, 16) for x in lines["frame"][:28]], np.uint64)
    assert np.array_equal(got, np.ascontiguousarray(want["sums"]).view(np.uint64))
    assert [int(x) for x in lines["frame"][28:]] == [want["status"], want["iterations"], want["samples"], want["valid"]]


# ------------------------------------------------------------------ the C ABI and the shim
def test_abi_declares_exports_and_types_the_five_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_locate_system", "drf_locate_frame", "drf_locate_system_device", "drf_locate_frame_device", "drf_locate_stats"])
    assert "drf_locate_options_t" in src and "uint64_t counts[4]" in src
    assert C.sizeof(L.LocateOptions) == C.sizeof(Options) == 48
    assert [(n, t) for n, t in L.LocateOptions._fields_] == [(n, t) for n, t in Options._fields_]
    for name, off in (("max_iters", 0), ("min_weight", 4), ("step", 8), ("band", 12), ("huber", 16), ("centre_depth", 20), ("eps_rot", 24), ("eps_trans", 32), ("min_valid", 40)):
        assert getattr(L.LocateOptions, name).offset == off, name
    lib = L.lib()
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
    depth = (C.c_float * 4)()
    sums, counts, out = (C.c_double * 28)(), (C.c_uint64 * 4)(), (C.c_uint64 * 6)()
    assert lib.drf_locate_system(None, depth, T, None, sums, counts) == 1
    assert lib.drf_locate_frame(None, depth, T, None, T, None) == 1
    assert lib.drf_locate_system_device(None, None, T, None, sums, counts) == 1
    assert lib.drf_locate_frame_device(None, None, T, None, T, None) == 1
    assert lib.drf_locate_stats(None, out) == 1


def test_shim_compiles(tmp_path):
    """tandem_amd/libdr/dr_fusion.h LocateDepthFrame as a TANDEM translation unit would call it (tests/cpp/map_locate_shim.cpp): it
    compiles and links against the library; tests/test_fusion_map_locate_gpu.py runs it."""
    abi_module()
    exe = str(tmp_path / "map_locate_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_locate_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert os.path.isfile(exe)
