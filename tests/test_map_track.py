"""CPU: the host half of drf_track_system / drf_track_frame (include/dr_mi355x.h "Tracks a depth frame against the ray-cast model",
DESIGN.md §7c "Tracking a depth frame against the ray-cast model").  track_normal, track_point, track_system_host and track_loop of
tandem_amd/csrc/fusion_host.h compiled with plain g++ (tests/cpp/map_track_check.cpp) and held, bit for bit, to np_track_model /
np_track_system / np_track_frame, numpy restatements of the rule written here from the header's statement -- the reference of
tests/test_fusion_map_track_gpu.py too; the basin on a map integrated by the CPU oracle (whose ray-cast is the model's renderer);
the status paths; the same under AddressSanitizer and UBSan as a stand-alone program (tests/cpp/map_track_san.cpp); the five new
names of the C ABI.  np_fold, np_step, butterfly and the motion come from tests/test_map_align.py and tests/test_map_transform.py by
import, the sample grid's few lines are restated from tests/test_map_locate.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import abi_module, check_symbols
from test_map_align import CONVERGED, DEGENERATE, LOST, MAX_ITERS, Result, assert_same_result, assert_same_system, bits, butterfly, np_fold, np_step
from test_map_locate import SCENE_MEASURED, Camera, camera, np_locate_frame, scene_errors, start_near
from test_map_transform import motion, rigid, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p, u64p, f32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_double)
VS, H, W = 0.02, 96, 128
f32, f64 = np.float32, np.float64
MISS = f32(0.0)   # what k_raycast2 / k_raycast_fix write for a ray that found no surface


# ------------------------------------------------------------------ the rule, restated
def np_options(cam, **opt):
    """drf_track_options_t with its defaults: a zero (or missing) field is its default."""
    vs = f32(cam["voxel_size"])
    o = dict(max_renders=10, inner_iters=4, step=1, dist_max=f32(25.0) * vs, max_jump=f32(5.0) * vs, huber=f32(1.0), centre_depth=f32(0.0),
             eps_rot=1e-7, eps_trans=1e-5, min_valid=0.25)
    for k, v in opt.items():
        assert k in o, k
        if v:
            o[k] = f32(v) if k in ("dist_max", "max_jump", "huber", "centre_depth") else (int(v) if k in ("max_renders", "inner_iters", "step") else float(v))
    return o


def np_track_model(cam, Dm, max_jump):
    """The model map of the model depth image Dm: (H, W, 4) float32 (nx, ny, nz, z), zeros where the pixel is invalid.  Every
    operation is an fp32 array operation, one per operation of the rule."""
    Hd, Wd = int(cam["height"]), int(cam["width"])
    Dm = np.ascontiguousarray(Dm, f32).reshape(Hd, Wd)
    fx, fy, cx, cy, mj = f32(cam["fx"]), f32(cam["fy"]), f32(cam["cx"]), f32(cam["cy"]), f32(max_jump)
    out = np.zeros((Hd, Wd, 4), f32)
    if Hd < 3 or Wd < 3:
        return out
    z = Dm[1:-1, 1:-1]
    zl, zr, zu, zd = Dm[1:-1, :-2], Dm[1:-1, 2:], Dm[:-2, 1:-1], Dm[2:, 1:-1]
    with np.errstate(all="ignore"):
        ok = (z > MISS) & (zl > MISS) & (zr > MISS) & (zu > MISS) & (zd > MISS)
        for zn in (zl, zr, zu, zd):
            ok &= ~(np.abs(zn - z) > mj)
        v, u = np.meshgrid(np.arange(1, Hd - 1), np.arange(1, Wd - 1), indexing="ij")
        rx, ry = (u.astype(f32) - cx) / fx, (v.astype(f32) - cy) / fy
        rxl, rxr = ((u - 1).astype(f32) - cx) / fx, ((u + 1).astype(f32) - cx) / fx
        ryu, ryd = ((v - 1).astype(f32) - cy) / fy, ((v + 1).astype(f32) - cy) / fy
        a0, a1, a2 = rxr * zr - rxl * zl, ry * zr - ry * zl, zr - zl
        b0, b1, b2 = rx * zd - rx * zu, ryd * zd - ryu * zu, zd - zu
        n0, n1, n2 = a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0
        l2 = (n0 * n0 + n1 * n1) + n2 * n2
        ok &= l2 > f32(0)
        ln = np.sqrt(np.where(ok, l2, f32(1)))
        n0, n1, n2 = n0 / ln, n1 / ln, n2 / ln
        s = (n0 * (rx * z) + n1 * (ry * z)) + n2 * z
        flip = s > f32(0)
        n0, n1, n2 = np.where(flip, -n0, n0), np.where(flip, -n1, n1), np.where(flip, -n2, n2)
        assert all(a.dtype == f32 for a in (a0, a1, a2, b0, b1, b2, n0, n1, n2, l2, ln, s))
    inner = np.stack([n0, n1, n2, z], axis=-1)
    out[1:-1, 1:-1] = np.where(ok[..., None], inner, f32(0))
    return out


def np_centre(R, tv, cam, o):
    cs = [0.0, 0.0, float(f64(o["centre_depth"]) / f64(f32(cam["voxel_size"])))]
    return np.array([((R[k, 0] * cs[0] + R[k, 1] * cs[1]) + R[k, 2] * cs[2]) + tv[k] for k in range(3)], f64)


def np_system(cam, depth, model, model_pose, R, tv, o, detail=False):
    """One evaluation at the pose (R (3, 3), tv (3,)) in float64 against the model map `model` (np_track_model's) of a ray-cast at
    model_pose: (sums (28,) float64, (samples, valid, unassociated, rejected))."""
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
    fx, fy, cx, cy = (f64(f32(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    z = np.where(sample, dep, f32(1)).astype(f64)
    g = [(((u.astype(f64) - cx) / fx) * z) / vs64, (((v.astype(f64) - cy) / fy) * z) / vs64, z / vs64]
    q = [((R[k, 0] * g[0] + R[k, 1] * g[1]) + R[k, 2] * g[2]) + tv[k] for k in range(3)]
    c = np_centre(R, tv, cam, o)
    Rm, tvm = motion(model_pose, cam["voxel_size"])
    with np.errstate(all="ignore"):
        s = [q[k] - tvm[k] for k in range(3)]
        m = [(Rm[0, k] * s[0] + Rm[1, k] * s[1]) + Rm[2, k] * s[2] for k in range(3)]
        front = m[2] > 0.0
        m2 = np.where(front, m[2], 1.0)
        up, vp = fx * (m[0] / m2) + cx, fy * (m[1] / m2) + cy
        pu, pv = np.floor(up + 0.5), np.floor(vp + 0.5)
        inimg = front & (pu >= 0.0) & (pu <= float(Wd - 1)) & (pv >= 0.0) & (pv <= float(Hd - 1))
        iu, iv = np.where(inimg, pu, 0.0).astype(np.int64), np.where(inimg, pv, 0.0).astype(np.int64)
        px = model.reshape(Hd, Wd, 4)[iv, iu]
        assoc = sample & inimg & (px[:, 3] > f32(0))
        zm = px[:, 3].astype(f64)
        d = [m[0] - (((pu - cx) / fx) * zm) / vs64, m[1] - (((pv - cy) / fy) * zm) / vs64, m[2] - zm / vs64]
        dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        lim = f64(o["dist_max"]) / vs64
        near = dd <= lim * lim
        valid, rejected = assoc & near, assoc & ~near
        nn = [px[:, k].astype(f64) for k in range(3)]
        r = (nn[0] * d[0] + nn[1] * d[1]) + nn[2] * d[2]
        nw = [(Rm[k, 0] * nn[0] + Rm[k, 1] * nn[1]) + Rm[k, 2] * nn[2] for k in range(3)]
        x = [q[k] - c[k] for k in range(3)]
        J = [x[1] * nw[2] - x[2] * nw[1], x[2] * nw[0] - x[0] * nw[2], x[0] * nw[1] - x[1] * nw[0], nw[0], nw[1], nw[2]]
        a = np.abs(r)
        hub = f64(o["huber"])
        w = np.where(a <= hub, 1.0, hub / a)
        terms = []
        for ii in range(6):
            wj = w * J[ii]
            terms += [wj * J[jj] for jj in range(ii, 6)]
        terms = terms[:21] + [(w * J[ii]) * r for ii in range(6)] + [(w * r) * r]
        t = np.where(valid[..., None], np.stack(terms, axis=-1), 0.0)
    assert t.dtype == f64
    t = t.reshape(groups, 8, 64, 28)
    acc = np.zeros((groups, 64, 28), f64)
    for k in range(8):
        acc = acc + t[:, k]
    partial = butterfly(acc)[:, 0, :]
    sums = np_fold(partial) if groups else np.zeros(28)
    counts = (int(sample.sum()), int(valid.sum()), int((sample & ~assoc).sum()), int(rejected.sum()))
    assert counts[0] == counts[1] + counts[2] + counts[3]
    return (sums, counts) + ((dict(c=c, up=up, vp=vp, pu=pu, pv=pv, sample=sample, front=front, inimg=inimg, valid=valid, r=r),) if detail else ())


def np_track_system(cam, depth, model_depth, model_pose, pose, detail=False, **opt):
    o = np_options(cam, **opt)
    R, tv = motion(pose, cam["voxel_size"])
    return np_system(cam, depth, np_track_model(cam, model_depth, o["max_jump"]), model_pose, R, tv, o, detail=detail)


def np_round(cam, depth, model, p16, o):
    """One round of the outer loop: drf_align_map's loop from the pose p16 (float32) against the model rendered at p16."""
    R, tv = motion(p16, cam["voxel_size"])
    good = (R, tv)
    res = dict(status=MAX_ITERS, iterations=0, sums=np.zeros(28), samples=0, valid0=0, valid=0, cost0=0.0, cost=0.0, trace=[], counts4=(0, 0, 0, 0))
    for it in range(o["inner_iters"]):
        sums, c4, det = np_system(cam, depth, model, p16, R, tv, o, detail=True)
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
    T = np.zeros((4, 4), f64)
    T[:3, :3] = R
    T[:3, 3] = tv * f64(f32(cam["voxel_size"]))
    T[3, 3] = 1.0
    res["T"] = T
    return res


def np_track_frame(render, cam, depth, pose_init, **opt):
    """The outer loop of drf_track_frame over render(pose (4, 4) float32) -> (H, W) float32 model depth: a dict shaped like
    np_locate_frame's, plus renders and poses (the float32 pose of every round)."""
    o = np_options(cam, **opt)
    p16 = np.ascontiguousarray(pose_init, f32).reshape(4, 4).copy()
    out = dict(status=MAX_ITERS, iterations=0, sums=np.zeros(28), samples=0, valid0=0, valid=0, cost0=0.0, cost=0.0, trace=[], counts4=(0, 0, 0, 0),
               T=p16.astype(f64), renders=0, poses=[])
    for r in range(o["max_renders"]):
        model = np_track_model(cam, render(p16), o["max_jump"])
        out["poses"].append(p16.copy())
        rd = np_round(cam, depth, model, p16, o)
        first = (out["valid0"], out["cost0"]) if r else (rd["valid0"], rd["cost0"])
        out.update(T=rd["T"], sums=rd["sums"], samples=rd["samples"], valid=rd["valid"], cost=rd["cost"], counts4=rd["counts4"], valid0=first[0], cost0=first[1],
                   iterations=out["iterations"] + rd["iterations"], trace=out["trace"] + rd["trace"], renders=r + 1)
        if rd["status"] in (LOST, DEGENERATE) or (rd["status"] == CONVERGED and rd["iterations"] == 1):
            out["status"] = rd["status"]
            return out
        out["status"] = MAX_ITERS
        p16 = rd["T"].astype(f32)
    return out


# ------------------------------------------------------------------ the compiled host half
class Options(C.Structure):
    """drf_track_options_t"""
    _fields_ = [("max_renders", C.c_int), ("inner_iters", C.c_int), ("step", C.c_int), ("dist_max", C.c_float), ("max_jump", C.c_float), ("huber", C.c_float),
                ("centre_depth", C.c_float), ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("min_valid", C.c_double)]


RENDER_FN = C.CFUNCTYPE(None, f32p, f32p, C.c_void_p)


def build_check(directory):
    so = os.path.join(str(directory), "libmap_track_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_track_check.cpp"), "-o", so])
    h = C.CDLL(so)
    h.mt_options.argtypes = [C.POINTER(Options), C.c_float, f64p, C.c_char_p]
    h.mt_model.argtypes = [C.POINTER(Camera), f32p, C.c_float, f32p]
    h.mt_system.argtypes = [C.POINTER(Camera), f32p, f32p, f32p, f32p, C.POINTER(Options), f64p, u64p]
    h.mt_frame.argtypes = [C.POINTER(Camera), f32p, RENDER_FN, C.c_void_p, f32p, C.POINTER(Options), C.POINTER(Result), f64p, C.c_size_t, u64p]
    return h


@pytest.fixture(scope="module")
def HT(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("map_track"))


def _f32(a):
    return np.ascontiguousarray(a, f32)


def cpp_model(HT, cam, Dm, max_jump):
    Dm, out = _f32(Dm), np.zeros((cam["height"], cam["width"], 4), f32)
    assert HT.mt_model(C.byref(Camera(**cam)), Dm.ctypes.data_as(f32p), f32(max_jump), out.ctypes.data_as(f32p)) == 0
    return out


def cpp_system(HT, cam, depth, model_depth, model_pose, pose, **opt):
    depth, model_depth, model_pose, pose = _f32(depth), _f32(model_depth), _f32(model_pose).reshape(16), _f32(pose).reshape(16)
    sums, counts = np.zeros(28, f64), np.zeros(4, np.uint64)
    assert HT.mt_system(C.byref(Camera(**cam)), depth.ctypes.data_as(f32p), model_depth.ctypes.data_as(f32p), model_pose.ctypes.data_as(f32p),
                        pose.ctypes.data_as(f32p), C.byref(Options(**opt)), sums.ctypes.data_as(f64p), counts.ctypes.data_as(u64p)) == 0
    return sums, tuple(int(v) for v in counts)


def cpp_frame(HT, render, cam, depth, pose, **opt):
    """track_frame_host over the Python renderer as a dict shaped like np_track_frame's."""
    depth, pose = _f32(depth), _f32(pose).reshape(16)
    npix = cam["height"] * cam["width"]

    def call(p16, out, user):
        d = _f32(render(np.ctypeslib.as_array(p16, (16,)).reshape(4, 4).copy()))
        C.memmove(out, d.ctypes.data, npix * 4)

    r = Result()
    cap = int(opt.get("max_renders", 0) or 10) * int(opt.get("inner_iters", 0) or 4)
    trace, stats = np.zeros((cap, 28), f64), np.zeros(6, np.uint64)
    assert HT.mt_frame(C.byref(Camera(**cam)), depth.ctypes.data_as(f32p), RENDER_FN(call), None, pose.ctypes.data_as(f32p), C.byref(Options(**opt)), C.byref(r),
                       trace.ctypes.data_as(f64p), cap, stats.ctypes.data_as(u64p)) == 0
    assert int(stats[4]) == int(r.iterations)
    return dict(T=np.array(r.T, f64).reshape(4, 4), sums=np.array(r.sums, f64), samples=int(r.samples), valid0=int(r.valid0), valid=int(r.valid),
                cost0=float(r.cost0), cost=float(r.cost), iterations=int(r.iterations), status=int(r.status), trace=[trace[i] for i in range(int(r.iterations))],
                counts4=tuple(int(v) for v in stats[:4]), renders=int(stats[5]))


# ------------------------------------------------------------------ synthetic image pairs (no map)
PM = rigid((2, -1, 3), 4.0, (0.07, 0.03, -0.93))     # the model's pose


def pair_case(seed, height, width, vs=VS):
    """A model depth image of three analytic planes as the camera at PM sees them -- one tilted about y over the left two fifths, one
    tilted about x over the upper right, one fronto-parallel at 1.2 m over the lower right, so that the seams are depth steps far
    above max_jump -- with misses (0: a rectangle and a twentieth of the pixels), and a frame depth image of the same planes with
    +-1.5 voxels of noise and a tenth of the pixels zero, negative or out of the sensor's range.  No NaN."""
    rng = np.random.default_rng(seed)
    cam = camera(vs, height, width, fx=0.86 * width, fy=0.86 * width, cx=(width - 1) / 2.0, cy=(height - 1) / 2.0)
    v, u = np.meshgrid(np.arange(height, dtype=f64), np.arange(width, dtype=f64), indexing="ij")
    x, y = (u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"]
    za, zb, zc = 1.5 / (1.0 - 0.3 * x), 2.0 / (1.0 + 0.2 * y), np.full_like(x, 1.2)
    surf = np.where(u < 0.4 * width, za, np.where(v < 0.6 * height, zb, zc))
    model = surf.astype(f32)
    model[rng.integers(0, 20, model.shape) == 0] = MISS
    if height >= 16:
        model[height // 2: height // 2 + 3, width // 8: width // 4] = MISS
    depth = (surf + rng.uniform(-1.5, 1.5, surf.shape) * vs).astype(f32)
    pick = rng.integers(0, 40, depth.shape)
    for k, val in enumerate((0.0, -0.7, 0.05, 11.0)):
        depth[pick == k] = val
    if height >= 16:
        depth[: height // 8] = 0.0                      # whole groups without a sample at 96x128
    return dict(cam=cam, model=model, depth=depth)


def pose_near(deg=1.0, voxels=(1.5, -1.0, 0.8), axis=(1, 2, 3), vs=VS):
    return start_near(PM.astype(f64), axis, deg, voxels, vs)


def pose_camera_shift(dx_m, dy_m=0.0, dz_m=0.0):
    """PM moved along its own camera axes."""
    T = PM.astype(f64).copy()
    T[:3, 3] += T[:3, :3] @ np.array([dx_m, dy_m, dz_m])
    return T.astype(f32)


def pose_turned(axis, deg):
    """PM turned about its own camera centre, the axis in camera coordinates."""
    T = PM.astype(f64).copy()
    T[:3, :3] = T[:3, :3] @ rotation(axis, deg)
    return T.astype(f32)


GRIDS = [(5, 7), (16, 32), (18, 32), (24, 32), (96, 128)]           # 35, 512, 576, 768 and 12 288 positions


def pair_poses(cam):
    """(name, pose): a small motion; half a pixel sideways at the fronto-parallel plane (u' + 0.5 next to a whole number); a few
    pixels sideways and down (samples on the border column and row, and outside); turned away (outside); turned round (behind)."""
    half = 0.5 * 1.2 / cam["fx"]
    return [("near", pose_near()), ("half a pixel", pose_camera_shift(half)), ("shifted", pose_camera_shift(-2.0 * 1.2 / cam["fx"], 1.0 * 1.2 / cam["fy"])),
            ("turned away", pose_turned((0, 1, 0), 25.0)), ("behind", pose_turned((0, 1, 0), 180.0)), ("the model's pose", PM.copy())]


# ------------------------------------------------------------------ the model map and the system against the restatement
@pytest.mark.parametrize("height,width", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_model_map_against_the_restatement(HT, height, width):
    """Misses, the border, a miss among the neighbours, the seams between the planes (steps of 0.3 m and more against max_jump =
    0.1 m), and a max_jump so small that the tilted planes' own slope is a step."""
    case = pair_case(7 + height, height, width)
    Dm = case["model"].copy()
    if height >= 16:
        Dm[3, 5], Dm[4, 9], Dm[6, 3] = np.nan, -1.0, np.inf            # no ray-cast writes these; the rule's test covers them
    for mj in (0.1, 0.004):
        want = np_track_model(case["cam"], Dm, mj)
        got = cpp_model(HT, case["cam"], Dm, mj)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (height, width, mj)
        valid = want[..., 3] > 0
        assert not valid[0].any() and not valid[-1].any() and not valid[:, 0].any() and not valid[:, -1].any()
        assert not want[~valid].any(), "an invalid pixel is four zeros"
        assert valid.any() or (height < 16 and mj < 0.1)
        nrm = np.linalg.norm(want[valid][:, :3].astype(f64), axis=1)
        assert (np.abs(nrm - 1.0) < 1e-6).all()
        assert (want[valid][:, 2] < 0).all(), "the normals look at the camera (-z)"
    wide, tight = np_track_model(case["cam"], Dm, 0.1)[..., 3] > 0, np_track_model(case["cam"], Dm, 0.004)[..., 3] > 0
    assert tight.sum() < wide.sum()
    if height >= 16:
        seam = int(math.ceil(0.4 * width))                            # the first column of the second plane
        assert not wide[2:-2, seam - 1: seam + 1].any(), "the pixels on both sides of a depth step are invalid"
        miss = np.argwhere(Dm[1:-1, 1:-1] == 0)[0] + 1
        assert not wide[miss[0], miss[1]] and not wide[miss[0], miss[1] - 1] and not wide[miss[0] - 1, miss[1]]
        assert not wide[3, 5] and not wide[3, 4] and not wide[4, 9] and not wide[6, 3] and not wide[6, 4]


SYSTEM_OPTS = [("defaults", {}), ("step 2, centre 1.5", dict(step=2, centre_depth=1.5)), ("step 3, tight huber", dict(step=3, huber=0.25)),
               ("dist_max 0.016", dict(dist_max=0.016)), ("step 2, dist_max 0.016, max_jump 0.03, centre 1.5", dict(step=2, dist_max=0.016, max_jump=0.03, centre_depth=1.5))]


@pytest.mark.parametrize("height,width", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_system_against_the_restatement(HT, height, width):
    """Every pose of pair_poses under every option set, bit for bit; over them every count class occurs, samples project on the
    border row and column, behind the model camera and outside the image, and u' + 0.5 comes next to a whole number."""
    case = pair_case(7 + height, height, width)
    cam, d = case["cam"], case["depth"]
    assert not np.isnan(d).any()
    if height >= 16:
        assert (d == 0).any() and (d < 0).any() and (d > 10).any() and ((d > 0) & (d < 0.1)).any()
    seen = np.zeros(4, np.int64)
    for pname, pose in pair_poses(cam):
        for oname, opt in SYSTEM_OPTS:
            want = np_track_system(cam, d, case["model"], PM, pose, detail=True, **opt)
            assert_same_system(cpp_system(HT, cam, d, case["model"], PM, pose, **opt), want[:2], "%s, %s" % (pname, oname))
            seen += np.array(want[1]) > 0
            det = want[2]
            if oname == "defaults" and height >= 16:
                s = det["sample"]
                if pname == "behind":
                    assert not det["front"][s].any() and want[1][2] == want[1][0]
                if pname == "turned away":
                    assert (det["front"] & ~det["inimg"])[s].any(), "samples outside the image"
                if pname == "shifted":
                    on = s & det["inimg"]
                    assert (det["pu"][on] == 0).any() and (det["pv"][on] == height - 1).any(), "samples on the border column and row"
            if "dist_max" in opt and pname == "near" and height == 96:
                share = want[1][3] / float(want[1][1] + want[1][3])
                assert 0.3 < share < 0.7, "dist_max rejects about half: %s" % (want[1],)
    assert (seen > 0).all(), seen


def test_projections_next_to_a_whole_number(HT):
    """Frame and model both the plane z = 1.2 m seen head-on, the camera moved sideways by half a pixel's width at that depth and,
    a second time, up by half a pixel's height: u' + 0.5 (then v' + 0.5) lies within 1e-6 of a whole number for every sample, where
    the floor turns on the last bits of the projection."""
    case = pair_case(5, 24, 32)
    cam = case["cam"]
    flat = np.full((24, 32), 1.2, f32)
    for name, pose, key in (("u", pose_camera_shift(0.5 * 1.2 / cam["fx"]), "up"), ("v", pose_camera_shift(0.0, -0.5 * 1.2 / cam["fy"]), "vp")):
        want = np_track_system(cam, flat, flat, PM, pose, detail=True)
        t = (want[2][key] + 0.5)[want[2]["sample"]]
        assert (np.abs(t - np.round(t)) < 1e-6).all(), name
        assert_same_system(cpp_system(HT, cam, flat, flat, PM, pose), want[:2], name)
        assert want[1][1] > 300


def test_images_without_a_sample_and_a_model_without_a_hit(HT):
    case = pair_case(5, 24, 32)
    cam = case["cam"]
    for name, depth, model in (("no samples", np.zeros((24, 32), f32), case["model"]), ("no hit", case["depth"], np.zeros((24, 32), f32))):
        want = np_track_system(cam, depth, model, PM, pose_near())
        got = cpp_system(HT, cam, depth, model, PM, pose_near())
        assert_same_system(got, want, name)
        assert not got[0].any() and got[1][1] == 0 and got[1][3] == 0
    assert got[1][0] > 300 and got[1][2] == got[1][0]


def test_options_and_their_defaults(HT):
    out, name = np.zeros(10, f64), C.create_string_buffer(32)
    vs = f32(0.02)
    assert HT.mt_options(None, vs, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [10, 4, 1, float(f32(25.0) * vs), float(f32(5.0) * vs), 1.0, 0.0, 1e-7, 1e-5, 0.25]
    full = dict(max_renders=3, inner_iters=7, step=2, dist_max=0.5, max_jump=0.25, huber=2.0, centre_depth=1.5, eps_rot=1e-3, eps_trans=1e-2, min_valid=0.5)
    assert HT.mt_options(C.byref(Options(**full)), vs, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [3, 7, 2, 0.5, 0.25, 2.0, 1.5, 1e-3, 1e-2, 0.5]
    for bad in (dict(max_renders=-1), dict(inner_iters=-2), dict(step=-1), dict(dist_max=-1.0), dict(max_jump=float("nan")), dict(huber=float("inf")),
                dict(centre_depth=-0.5), dict(eps_rot=-1.0), dict(eps_trans=float("inf")), dict(min_valid=-0.1)):
        assert HT.mt_options(C.byref(Options(**bad)), vs, out.ctypes.data_as(f64p), name) == 1, bad
        assert name.value.decode() == list(bad)[0]
    assert C.sizeof(Options) == 56


def test_a_pose_that_is_no_rigid_motion_is_refused(HT):
    case = pair_case(5, 24, 32)
    scaled, nan = np.eye(4, dtype=f32), np.eye(4, dtype=f32)
    scaled[:3, :3] *= 1.01
    nan[2, 3] = np.nan
    cm, d, m, pm = Camera(**case["cam"]), _f32(case["depth"]), _f32(case["model"]), _f32(PM).reshape(16)
    sums, counts = np.zeros(28, f64), np.zeros(4, np.uint64)
    for bad in (scaled, nan):
        b = _f32(bad).reshape(16)
        for mp, p in ((pm, b), (b, pm)):
            assert HT.mt_system(C.byref(cm), d.ctypes.data_as(f32p), m.ctypes.data_as(f32p), mp.ctypes.data_as(f32p), p.ctypes.data_as(f32p), None,
                                sums.ctypes.data_as(f64p), counts.ctypes.data_as(u64p)) == 2


# ------------------------------------------------------------------ the loop on a map: the oracle's ray-cast is the renderer
def track_scene():
    """The map of tests/test_map_locate.py's scene_case, rebuilt here with its oracle kept: synth.scene.make_scans at 96x128, seed
    11, the first scan integrated by the CPU oracle, whose render(pose) is bit for bit the engine's ray-cast."""
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
    return dict(cam=cam, blocks=(coords, vox), depth=depth, bgr=bgr, pose=pose, oracle=orc, render=lambda p: orc.render(p)[1],
                centre_depth=float(np.median(depth[depth > 0])))


# The starts of the basin test: (voxels, degrees) off the scan's pose, the turn about (1, 2, 3), the move along (1.5, -1.0, 0.8).
BASIN_STARTS = [(8.0, 4.0), (12.0, 6.0), (20.0, 10.0)]
# The thresholds the tracking is run with on the scene.  A model that is rendered again moves the fixed point by far more than
# drf_locate_frame's 1e-7 rad and 1e-5 voxels, so a tracking says for itself what "no longer moving" means: a step that turns by
# less than 1e-3 rad -- a tenth of a voxel at the scene's 115 voxels of depth -- and moves by less than 0.02 voxels is two orders of
# magnitude inside the 4-voxel band that drf_locate_frame needs.  Everything else is the default.
TRACK_EPS = dict(eps_rot=1e-3, eps_trans=0.02)
# measured on the restatement: the largest start that ends CONVERGED, and the error after the tracking alone (degrees, voxels)
BASIN_USED = 0
BASIN_TRACK_ERROR = (0.6672, 0.5076)


def basin_start(s, k):
    vox, deg = BASIN_STARTS[k]
    along = np.array([1.5, -1.0, 0.8])
    return start_near(s["pose"].astype(f64), (1, 2, 3), deg, vox * along / np.linalg.norm(along))


def track_opts(s, **kw):
    return dict(dict(centre_depth=s["centre_depth"], **TRACK_EPS), **kw)


@pytest.fixture(scope="module")
def scene_map():
    return track_scene()


def test_loop_against_the_restatement_on_every_evaluation(HT, scene_map):
    """track_loop over the oracle's renders from the first basin start: the sums of every evaluation, the counters, the number of
    renders and the pose, bit for bit; and a second run that ends by max_renders, with a stride."""
    s = scene_map
    for name, opt in (("first start", track_opts(s)), ("two renders of three evaluations, step 2", track_opts(s, max_renders=2, inner_iters=3, step=2))):
        start = basin_start(s, 0)
        want = np_track_frame(s["render"], s["cam"], s["depth"], start, **opt)
        got = cpp_frame(HT, s["render"], s["cam"], s["depth"], start, **opt)
        assert_same_result(got, want, name)
        assert got["counts4"] == want["counts4"] and got["renders"] == want["renders"] and len(got["trace"]) == want["iterations"]
        print("%s: status %d, %d renders, %d evaluations, counts %s" % (name, want["status"], want["renders"], want["iterations"], want["counts4"]))
    assert want["status"] == MAX_ITERS and want["renders"] == 2 and want["iterations"] == 6


def test_the_basin(HT, scene_map):
    """The point of the call.  From each of BASIN_STARTS the restatement tracks the scan's own depth image against the one-scan map.
    MEASURED on the restatement (TRACK_EPS, every other option its default): (8 voxels, 4 degrees) ends CONVERGED after 6 renders and
    13 evaluations, 0.6672 degrees and 0.5076 voxels from the scan's pose; (12, 6) ends MAX_ITERS after 10 renders, 1.217 degrees and
    0.598 voxels off and still creeping; (20, 10) ends LOST at its first evaluation (2 644 of 11 973 samples valid, below min_valid).
    So the start used is the first.  What remains after the tracking is a turn about the optical axis with the sideways move that
    goes with it: the scene is a tilted wall and a slab parallel to the image plane, two normals 11 degrees apart, and planes alone
    do not hold that motion -- the slab's edges do, which only the SDF sees.  drf_locate_frame alone from that start is LOST (its
    points are 8 voxels outside a band of 4); from the tracked pose it ends CONVERGED at 0.055 degrees and 0.1986 voxels, the
    minimum of this map that tests/test_map_locate.py measured (SCENE_MEASURED, asserted with its factor of 2)."""
    s = scene_map
    runs = [np_track_frame(s["render"], s["cam"], s["depth"], basin_start(s, k), **track_opts(s)) for k in range(len(BASIN_STARTS))]
    for k, r in enumerate(runs):
        a, t = scene_errors(r["T"], s["pose"])
        print("start %s: status %d after %d renders and %d evaluations, %d of %d valid, %.4f degrees %.4f voxels off" %
              (BASIN_STARTS[k], r["status"], r["renders"], r["iterations"], r["valid"], r["samples"], a, t))
    converged = [k for k, r in enumerate(runs) if r["status"] == CONVERGED]
    assert converged, "not even the first start converges: the rule is wrong"
    used = max(converged)
    assert used == BASIN_USED
    start, tracked = basin_start(s, used), runs[used]
    a, t = scene_errors(tracked["T"], s["pose"])
    assert abs(a - BASIN_TRACK_ERROR[0]) < 1e-3 and abs(t - BASIN_TRACK_ERROR[1]) < 1e-3, (a, t)
    alone = np_locate_frame(s["blocks"], s["cam"], s["depth"], start, centre_depth=s["centre_depth"])
    a0, t0 = scene_errors(alone["T"], s["pose"])
    print("locate alone: status %d, %.4f degrees %.4f voxels off" % (alone["status"], a0, t0))
    assert alone["status"] == LOST or t0 > 1.0
    both = np_locate_frame(s["blocks"], s["cam"], s["depth"], tracked["T"].astype(f32), centre_depth=s["centre_depth"])
    a1, t1 = scene_errors(both["T"], s["pose"])
    print("track, then locate: status %d after %d evaluations, %.5f degrees %.5f voxels off" % (both["status"], both["iterations"], a1, t1))
    assert both["status"] == CONVERGED
    assert a1 <= 2 * SCENE_MEASURED[0] and t1 <= 2 * SCENE_MEASURED[1]
    got = cpp_frame(HT, s["render"], s["cam"], s["depth"], start, **track_opts(s))
    assert_same_result(got, tracked, "the basin start on the host")


# ------------------------------------------------------------------ status paths
def plane_renderer(cam, normal, offset):
    """render(pose): the analytic ray-cast of the world plane normal . X = offset."""
    v, u = np.meshgrid(np.arange(cam["height"], dtype=f64), np.arange(cam["width"], dtype=f64), indexing="ij")
    ray = np.stack([(u - f64(f32(cam["cx"]))) / f64(f32(cam["fx"])), (v - f64(f32(cam["cy"]))) / f64(f32(cam["fy"])), np.ones_like(u)], axis=-1)
    n = np.asarray(normal, f64)

    def render(pose):
        T = np.asarray(pose, f64).reshape(4, 4)
        z = (offset - n @ T[:3, 3]) / ((ray @ T[:3, :3].T) @ n)
        return np.where(z > 0, z, 0.0).astype(f32)
    return render


def test_one_plane_is_degenerate(HT):
    cam = camera(height=24, width=32, fx=28.0, fy=28.0, cx=15.5, cy=11.5)
    render = plane_renderer(cam, (0.0, 0.0, 1.0), 1.5)
    pose = np.eye(4, dtype=f32)
    res = cpp_frame(HT, render, cam, render(pose), pose)
    assert_same_result(res, np_track_frame(render, cam, render(pose), pose), "one plane")
    assert res["status"] == DEGENERATE and res["iterations"] == 1 and res["renders"] == 1 and res["valid"] > 300
    assert np.array_equal(res["T"], pose.astype(f64))


def test_a_map_far_away_is_lost(HT, scene_map):
    s = scene_map
    gone = basin_start(s, 0)
    gone[0, 3] += 50 * 8 * VS                                           # the map is 50 blocks away
    res = cpp_frame(HT, s["render"], s["cam"], s["depth"], gone, **track_opts(s))
    assert_same_result(res, np_track_frame(s["render"], s["cam"], s["depth"], gone, **track_opts(s)), "far away")
    assert res["status"] == LOST and res["iterations"] == 1 and res["renders"] == 1 and res["valid"] == 0 and res["samples"] > 10000
    assert np.array_equal(res["T"][:3, :3], gone[:3, :3].astype(f64))


def test_max_renders_one_is_max_iters(HT, scene_map):
    s = scene_map
    start = basin_start(s, 0)
    res = cpp_frame(HT, s["render"], s["cam"], s["depth"], start, **track_opts(s, max_renders=1))
    assert res["status"] == MAX_ITERS and res["renders"] == 1 and res["iterations"] == 4
    a0, t0 = scene_errors(start.astype(f64), s["pose"])
    a, t = scene_errors(res["T"], s["pose"])
    print("one render: %.3f degrees %.3f voxels -> %.3f degrees %.3f voxels" % (a0, t0, a, t))
    assert t < 0.25 * t0 and a < a0


# ------------------------------------------------------------------ sanitizers, the C ABI and the shim
def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """track_model_host, track_system_host and track_loop under AddressSanitizer and UBSan: a plain executable, nothing preloaded,
    nothing loaded into Python.  It reads one synthetic pair from a file and prints the sums, which are the restatement's bit for
    bit; then cases of its own."""
    exe, data = str(tmp_path / "map_track_san"), str(tmp_path / "case.bin")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_track_san.cpp"), "-o", exe])
    case = pair_case(31, 24, 32)
    opt = dict(step=2, centre_depth=1.5, dist_max=0.04)
    pose = pose_near()
    with open(data, "wb") as fh:
        fh.write(bytes(Camera(**case["cam"])) + bytes(Options(**opt)) + _f32(case["depth"]).tobytes() + _f32(case["model"]).tobytes() + _f32(PM).tobytes() +
                 _f32(pose).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_track_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    line = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("system")][0]
    want = np_track_system(case["cam"], case["depth"], case["model"], PM, pose, **opt)
    assert np.array_equal(np.array([int(x, 16) for x in line[:28]], np.uint64), bits(want[0])) and tuple(int(x) for x in line[28:]) == want[1]
    assert want[1][1] > 20


def test_abi_declares_exports_and_types_the_five_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_track_system", "drf_track_frame", "drf_track_system_device", "drf_track_frame_device", "drf_track_stats"])
    assert "drf_track_options_t" in src
    assert C.sizeof(L.TrackOptions) == C.sizeof(Options) == 56
    assert [(n, t) for n, t in L.TrackOptions._fields_] == [(n, t) for n, t in Options._fields_]
    for name, off in (("max_renders", 0), ("inner_iters", 4), ("step", 8), ("dist_max", 12), ("max_jump", 16), ("huber", 20), ("centre_depth", 24), ("eps_rot", 32),
                      ("eps_trans", 40), ("min_valid", 48)):
        assert getattr(L.TrackOptions, name).offset == off, name
    lib = L.lib()
    T = (C.c_float * 16)(*np.eye(4, dtype=f32).reshape(16))
    depth = (C.c_float * 4)()
    sums, counts, out = (C.c_double * 28)(), (C.c_uint64 * 4)(), (C.c_uint64 * 6)()
    assert lib.drf_track_system(None, depth, depth, T, T, None, sums, counts) == 1
    assert lib.drf_track_frame(None, depth, T, None, T, None) == 1
    assert lib.drf_track_system_device(None, None, None, T, T, None, sums, counts) == 1
    assert lib.drf_track_frame_device(None, None, T, None, T, None) == 1
    assert lib.drf_track_stats(None, out) == 1
    import tandem_amd.dr_fusion as F
    for name in ("track_system", "track_frame", "track_stats"):
        assert callable(getattr(F.DrFusion, name))


def test_shim_compiles(tmp_path):
    """tandem_amd/libdr/dr_fusion.h TrackDepthFrame as a TANDEM translation unit would call it (tests/cpp/map_track_shim.cpp): it
    compiles and links against the library; tests/test_fusion_map_track_gpu.py runs it."""
    abi_module()
    exe = str(tmp_path / "map_track_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_track_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert os.path.isfile(exe)
