"""CPU: the host half of drf_track_colour_system / drf_track_colour_frame (include/dr_mi355x.h "Tracks a depth frame AND its colour
image against the ray-cast model", DESIGN.md §7c "Tracking with colour").  track_model_colour_host, track_photo_term,
track_colour_system_host and track_colour_frame_host of tandem_amd/csrc/fusion_host.h compiled with plain g++
(tests/cpp/map_track_colour_check.cpp) and held, bit for bit, to np_colour_model / np_colour_term / np_colour_eval /
np_track_colour_frame, numpy restatements of the rule written here from the header's statement -- the reference of
tests/test_fusion_track_colour_gpu.py too; the uniform-colour case against the geometric rule; one textured plane, where geometry
alone is degenerate; the loop on the oracle's map; options and refusals; the same under AddressSanitizer and UBSan as a stand-alone
program (tests/cpp/map_track_colour_san.cpp); the five new names of the C ABI.  The geometric restatement, the synthetic pairs
and the scene come from tests/test_map_track.py by import."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import test_map_track as MT
from fusion_helpers import abi_module, check_symbols
from test_map_align import CONVERGED, DEGENERATE, LOST, MAX_ITERS, Result, assert_same_result, assert_same_system, bits, butterfly, np_fold, np_step
from test_map_locate import Camera, camera, scene_errors, start_near
from test_map_track import GRIDS, PM, TRACK_EPS, basin_start, np_centre, np_track_model, pair_case, pair_poses, track_opts, track_scene
from test_map_transform import motion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p, u32p, u64p, f32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_double)
VS = MT.VS
f32, f64 = np.float32, np.float64
DEFAULT_WEIGHT = f32(1.0 / 27.0)       # (float)(1.0 / 27.0)


# ------------------------------------------------------------------ the rule, restated
def np_colour_options(cam, photo_weight=0.0, **opt):
    """drf_track_colour_options_t with its defaults: (drf_track_options_t's dict, photo_weight as float32)."""
    o = MT.np_options(cam, **opt)
    w = f32(photo_weight) if photo_weight else DEFAULT_WEIGHT * f32(o["huber"])
    assert w.dtype == f32
    return o, w


def np_intensity(bgr):
    """y = ((float)b + (float)g) + (float)r per pixel, float32."""
    c = np.ascontiguousarray(bgr, np.uint8).astype(f32)
    return (c[..., 0] + c[..., 1]) + c[..., 2]


def np_colour_model(cam, Cm, Dm, max_jump):
    """(model map, Ym): Ym is the intensity of Cm where the model map's z > 0 and -1 elsewhere."""
    Hd, Wd = int(cam["height"]), int(cam["width"])
    model = np_track_model(cam, Dm, max_jump)
    Ym = np.where(model[..., 3] > f32(0), np_intensity(np.asarray(Cm).reshape(Hd, Wd, 3)), f32(-1.0)).astype(f32)
    return model, Ym


def np_colour_term(cam, Ym, Rm, m, up, vp, yf, lam):
    """The photometric term for arrays of samples: (exists, r, [n0, n1, n2], detail).  m: three float64 arrays (m2 > 0 where the
    result is used), up, vp float64, yf float32, lam float32."""
    Hd, Wd = int(cam["height"]), int(cam["width"])
    fx, fy = f64(f32(cam["fx"])), f64(f32(cam["fy"]))
    lam = f64(f32(lam))
    with np.errstate(all="ignore"):
        fu, fv = np.floor(up), np.floor(vp)
        inside = (fu >= 0.0) & (fu + 1.0 <= float(Wd - 1)) & (fv >= 0.0) & (fv + 1.0 <= float(Hd - 1))
        iu, iv = np.where(inside, fu, 0.0).astype(np.int64), np.where(inside, fv, 0.0).astype(np.int64)
        if Wd < 2 or Hd < 2:
            zero = np.zeros(np.shape(up), f64)
            return np.zeros(np.shape(up), bool), zero, [zero, zero, zero], dict(inside=inside, corners=inside, a=zero, b=zero, I=zero)
        Y = np.ascontiguousarray(Ym, f32).reshape(Hd, Wd)
        c00, c10, c01, c11 = Y[iv, iu], Y[iv, iu + 1], Y[iv + 1, iu], Y[iv + 1, iu + 1]
        corners = (c00 >= f32(0)) & (c10 >= f32(0)) & (c01 >= f32(0)) & (c11 >= f32(0))
        y00, y10, y01, y11 = c00.astype(f64), c10.astype(f64), c01.astype(f64), c11.astype(f64)
        a, b = up - fu, vp - fv
        oa, ob = 1.0 - a, 1.0 - b
        I = ob * (oa * y00 + a * y10) + b * (oa * y01 + a * y11)
        Iu = ob * (y10 - y00) + b * (y11 - y01)
        Iv = oa * (y01 - y00) + a * (y11 - y10)
        gm0, gm1 = (Iu * fx) / m[2], (Iv * fy) / m[2]
        gm2 = -((gm0 * m[0] + gm1 * m[1]) / m[2])
        r = lam * (I - np.asarray(yf, f32).astype(f64))
        n = [lam * ((Rm[k, 0] * gm0 + Rm[k, 1] * gm1) + Rm[k, 2] * gm2) for k in range(3)]
    return inside & corners, r, n, dict(inside=inside, corners=corners, a=a, b=b, I=I)


def _terms(w, J, r):
    t = []
    for ii in range(6):
        wj = w * J[ii]
        t += [wj * J[jj] for jj in range(ii, 6)]
    return t[:21] + [(w * J[ii]) * r for ii in range(6)] + [(w * r) * r]


def np_colour_eval(cam, bgr, depth, model, Ym, model_pose, R, tv, o, lam, detail=False):
    """One evaluation at the pose (R, tv) in float64: (sums (28,), (samples, valid, unassociated, rejected, photometric))."""
    Wd, Hd, step = int(cam["width"]), int(cam["height"]), int(o["step"])
    Wg, Hg = -(-Wd // step), -(-Hd // step)
    total = Wg * Hg
    groups = -(-total // 512)
    depth = np.ascontiguousarray(depth, f32).reshape(Hd, Wd)
    yimg = np_intensity(np.asarray(bgr).reshape(Hd, Wd, 3))
    n = np.arange(groups * 512)
    inside = n < total
    j, i = np.where(inside, n // Wg, 0), np.where(inside, n % Wg, 0)
    u, v = step * i, step * j
    dep, yf = depth[v, u], yimg[v, u]
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
        m = [m[0], m[1], np.where(front, m[2], 1.0)]
        up, vp = fx * (m[0] / m[2]) + cx, fy * (m[1] / m[2]) + cy
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
        rg = (nn[0] * d[0] + nn[1] * d[1]) + nn[2] * d[2]
        nw = [(Rm[k, 0] * nn[0] + Rm[k, 1] * nn[1]) + Rm[k, 2] * nn[2] for k in range(3)]
        x = [q[k] - c[k] for k in range(3)]
        hub = f64(o["huber"])

        def term(r, nv):
            J = [x[1] * nv[2] - x[2] * nv[1], x[2] * nv[0] - x[0] * nv[2], x[0] * nv[1] - x[1] * nv[0], nv[0], nv[1], nv[2]]
            a = np.abs(r)
            return np.stack(_terms(np.where(a <= hub, 1.0, hub / a), J, r), axis=-1)

        exists, rp, npv, det = np_colour_term(cam, Ym, Rm, m, np.where(inimg, up, 0.0), np.where(inimg, vp, 0.0), yf, lam)
        photo = valid & exists
        tg = np.where(valid[..., None], term(rg, nw), 0.0).reshape(groups, 8, 64, 28)
        tp = np.where(photo[..., None], term(rp, npv), 0.0).reshape(groups, 8, 64, 28)
    assert tg.dtype == f64 and tp.dtype == f64
    acc = np.zeros((groups, 64, 28), f64)
    for k in range(8):
        acc = acc + tg[:, k]
        acc = acc + tp[:, k]
    sums = np_fold(butterfly(acc)[:, 0, :]) if groups else np.zeros(28)
    counts = (int(sample.sum()), int(valid.sum()), int((sample & ~assoc).sum()), int(rejected.sum()), int(photo.sum()))
    assert counts[0] == counts[1] + counts[2] + counts[3]
    if not detail:
        return sums, counts
    return sums, counts, dict(c=c, valid=valid, photo=photo, bounds=valid & ~det["inside"], corner=valid & det["inside"] & ~det["corners"], a=det["a"], b=det["b"],
                              rp=rp, yf=yf, up=up, vp=vp)


def np_track_colour_system(cam, bgr, depth, model_bgr, model_depth, model_pose, pose, detail=False, photo_weight=0.0, **opt):
    o, lam = np_colour_options(cam, photo_weight, **opt)
    R, tv = motion(pose, cam["voxel_size"])
    model, Ym = np_colour_model(cam, model_bgr, model_depth, o["max_jump"])
    return np_colour_eval(cam, bgr, depth, model, Ym, model_pose, R, tv, o, lam, detail=detail)


def np_loop(system, cam, pose_init, o):
    """drf_track_frame's outer loop over system(p16, R, tv) -> (sums, counts, c), which renders when p16 is new: the loop of
    tests/test_map_track.py's np_round and np_track_frame for any evaluator."""
    p16 = np.ascontiguousarray(pose_init, f32).reshape(4, 4).copy()
    out = dict(status=MAX_ITERS, iterations=0, sums=np.zeros(28), samples=0, valid0=0, valid=0, cost0=0.0, cost=0.0, trace=[], counts=(), T=p16.astype(f64), renders=0)
    for rnd in range(o["max_renders"]):
        R, tv = motion(p16, cam["voxel_size"])
        good, status, its = (R, tv), MAX_ITERS, 0
        for it in range(o["inner_iters"]):
            sums, cnt, c = system(p16, R, tv)
            valid = cnt[1]
            cost = float(sums[27]) / float(valid) if valid else 0.0
            out["trace"].append(sums)
            out.update(sums=sums, samples=cnt[0], valid=valid, cost=cost, counts=cnt, iterations=out["iterations"] + 1)
            its = it + 1
            if rnd == 0 and it == 0:
                out.update(valid0=valid, cost0=cost)
            if float(valid) < o["min_valid"] * float(cnt[0]) or valid < 6:
                status = LOST
                R, tv = good
                break
            good = (R, tv)
            s, R, tv = np_step(sums, c, R, tv, o["eps_rot"], o["eps_trans"])
            if s >= 0:
                status = s
                break
        T = np.zeros((4, 4), f64)
        T[:3, :3], T[:3, 3], T[3, 3] = R, tv * f64(f32(cam["voxel_size"])), 1.0
        out.update(T=T, renders=rnd + 1)
        if status in (LOST, DEGENERATE) or (status == CONVERGED and its == 1):
            out["status"] = status
            return out
        out["status"] = MAX_ITERS
        p16 = T.astype(f32)
    return out


def np_track_colour_frame(render, cam, bgr, depth, pose_init, photo_weight=0.0, colour=True, **opt):
    """drf_track_colour_frame over render(pose (4, 4) float32) -> (bgr (H, W, 3) uint8, depth (H, W) float32); colour=False is
    drf_track_frame over the same renderer."""
    o, lam = np_colour_options(cam, photo_weight, **opt)
    state = {}

    def system(p16, R, tv):
        if state.get("at") is None or not np.array_equal(state["at"], p16):
            Cm, Dm = render(p16)
            state["model"], state["Ym"] = np_colour_model(cam, Cm, Dm, o["max_jump"])
            state["at"] = p16.copy()
        if colour:
            sums, cnt, det = np_colour_eval(cam, bgr, depth, state["model"], state["Ym"], p16, R, tv, o, lam, detail=True)
        else:
            sums, cnt, det = MT.np_system(cam, depth, state["model"], p16, R, tv, o, detail=True)
        return sums, cnt, det["c"]
    return np_loop(system, cam, pose_init, o)


# ------------------------------------------------------------------ the compiled host half
class ColourOptions(C.Structure):
    """drf_track_colour_options_t"""
    _fields_ = [("track", MT.Options), ("photo_weight", C.c_float)]


def colour_options(photo_weight=0.0, **opt):
    return ColourOptions(MT.Options(**opt), photo_weight)


RENDER_FN = C.CFUNCTYPE(None, f32p, u8p, f32p, C.c_void_p)


def build_check(directory):
    so = os.path.join(str(directory), "libmap_track_colour_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_track_colour_check.cpp"), "-o", so])
    h = C.CDLL(so)
    cam = C.POINTER(Camera)
    h.mtc_options.argtypes = [C.POINTER(ColourOptions), C.c_float, f64p, u32p, C.c_char_p]
    h.mtc_model.argtypes = [cam, u8p, f32p, C.c_float, f32p, f32p]
    h.mtc_term.argtypes = [cam, f32p, f32p, f64p, C.c_double, C.c_double, C.c_float, C.c_float, f64p]
    h.mtc_system.argtypes = [cam, u8p, f32p, u8p, f32p, f32p, f32p, C.POINTER(ColourOptions), f64p, u64p]
    h.mtc_geometric.argtypes = [cam, f32p, f32p, f32p, f32p, C.POINTER(MT.Options), f64p, u64p]
    h.mtc_frame.argtypes = [cam, u8p, f32p, RENDER_FN, C.c_void_p, f32p, C.POINTER(ColourOptions), C.c_int, C.POINTER(Result), f64p, C.c_size_t, u64p]
    return h


@pytest.fixture(scope="module")
def HC(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("map_track_colour"))


def _f32(a):
    return np.ascontiguousarray(a, f32)


def _u8(a):
    return np.ascontiguousarray(a, np.uint8)


def cpp_system(HC, cam, bgr, depth, model_bgr, model_depth, model_pose, pose, photo_weight=0.0, **opt):
    bgr, depth, model_bgr, model_depth = _u8(bgr), _f32(depth), _u8(model_bgr), _f32(model_depth)
    model_pose, pose = _f32(model_pose).reshape(16), _f32(pose).reshape(16)
    sums, counts = np.zeros(28, f64), np.zeros(5, np.uint64)
    assert HC.mtc_system(C.byref(Camera(**cam)), bgr.ctypes.data_as(u8p), depth.ctypes.data_as(f32p), model_bgr.ctypes.data_as(u8p), model_depth.ctypes.data_as(f32p),
                         model_pose.ctypes.data_as(f32p), pose.ctypes.data_as(f32p), C.byref(colour_options(photo_weight, **opt)), sums.ctypes.data_as(f64p),
                         counts.ctypes.data_as(u64p)) == 0
    return sums, tuple(int(v) for v in counts)


def cpp_frame(HC, render, cam, bgr, depth, pose, photo_weight=0.0, colour=True, **opt):
    """track_colour_frame_host (colour=False: track_frame_host) over the Python renderer as a dict shaped like np_loop's."""
    bgr, depth, pose = _u8(bgr), _f32(depth), _f32(pose).reshape(16)
    npix = cam["height"] * cam["width"]

    def call(p16, cout, dout, user):
        c, d = render(np.ctypeslib.as_array(p16, (16,)).reshape(4, 4).copy())
        c, d = _u8(c), _f32(d)
        C.memmove(cout, c.ctypes.data, npix * 3)
        C.memmove(dout, d.ctypes.data, npix * 4)

    r = Result()
    cap = int(opt.get("max_renders", 0) or 10) * int(opt.get("inner_iters", 0) or 4)
    trace, stats = np.zeros((cap, 28), f64), np.zeros(7, np.uint64)
    assert HC.mtc_frame(C.byref(Camera(**cam)), bgr.ctypes.data_as(u8p), depth.ctypes.data_as(f32p), RENDER_FN(call), None, pose.ctypes.data_as(f32p),
                        C.byref(colour_options(photo_weight, **opt)), 1 if colour else 0, C.byref(r), trace.ctypes.data_as(f64p), cap, stats.ctypes.data_as(u64p)) == 0
    assert int(stats[5]) == int(r.iterations)
    return dict(T=np.array(r.T, f64).reshape(4, 4), sums=np.array(r.sums, f64), samples=int(r.samples), valid0=int(r.valid0), valid=int(r.valid),
                cost0=float(r.cost0), cost=float(r.cost), iterations=int(r.iterations), status=int(r.status), trace=[trace[i] for i in range(int(r.iterations))],
                counts=tuple(int(v) for v in stats[:5 if colour else 4]), renders=int(stats[6]))


# ------------------------------------------------------------------ synthetic image pairs with colour
def texture(height, width, phase=0.0):
    """An analytic texture over the pixels, quantised to uint8: three channels of different frequencies, (H, W, 3)."""
    v, u = np.meshgrid(np.arange(height, dtype=f64), np.arange(width, dtype=f64), indexing="ij")
    ch = [127.5 + 110.0 * np.sin(0.35 * (k + 1) * u + 0.23 * (3 - k) * v + k + phase) for k in range(3)]
    return np.floor(np.stack(ch, axis=-1) + 0.5).clip(0, 255).astype(np.uint8)


def colour_pair(seed, height, width):
    """pair_case with colour: the model's colour image is the texture; the frame's is the same texture with +-6 levels of noise, a
    fortieth of its pixels black (intensity 0) and a fortieth white (765)."""
    case = pair_case(seed, height, width)
    rng = np.random.default_rng(1000 + seed)
    case["model_bgr"] = texture(height, width)
    frame = case["model_bgr"].astype(np.int64) + rng.integers(-6, 7, (height, width, 3))
    frame = frame.clip(0, 255).astype(np.uint8)
    pick = rng.integers(0, 40, (height, width))
    frame[pick == 0] = 0
    frame[pick == 1] = 255
    case["bgr"] = frame
    return case


COLOUR_OPTS = [("defaults", {}), ("step 2, centre 1.5, weight 0.1", dict(step=2, centre_depth=1.5, photo_weight=0.1)),
               ("step 3, tight huber", dict(step=3, huber=0.25)), ("step 2, dist_max 0.016, max_jump 0.03", dict(step=2, dist_max=0.016, max_jump=0.03))]


# ------------------------------------------------------------------ the model map, the term and the system against the restatement
@pytest.mark.parametrize("height,width", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_model_and_intensity_map_against_the_restatement(HC, height, width):
    case = colour_pair(7 + height, height, width)
    cam = case["cam"]
    for mj in (0.1, 0.004):
        want_map, want_y = np_colour_model(cam, case["model_bgr"], case["model"], mj)
        got_map, got_y = np.zeros((height, width, 4), f32), np.zeros((height, width), f32)
        assert HC.mtc_model(C.byref(Camera(**cam)), _u8(case["model_bgr"]).ctypes.data_as(u8p), _f32(case["model"]).ctypes.data_as(f32p), f32(mj),
                            got_map.ctypes.data_as(f32p), got_y.ctypes.data_as(f32p)) == 0
        assert np.array_equal(got_map.view(np.uint32), want_map.view(np.uint32))
        assert np.array_equal(got_y.view(np.uint32), want_y.view(np.uint32))
        valid = want_map[..., 3] > 0
        assert (want_y[~valid] == -1).all() and (want_y[valid] >= 0).all() and (want_y[valid] == np.floor(want_y[valid])).all()
        assert (want_y[0] == -1).all() and (want_y[:, -1] == -1).all(), "the border carries no colour"
    if height >= 16:
        assert valid.any() and (want_y[valid] > 600).any() and (want_y[valid] < 160).any()


def test_the_term_alone_in_every_class(HC):
    """track_photo_term on an intensity map whose border carries colour -- which no model map's does: in the system a sample that
    projects into the last column or above the first row lands on a border pixel of the model map, is unassociated, and never
    reaches the term, so the two bounds of the rule are exercised here, on the function.  Classes: u0 + 1 = width; v0 < 0; one
    corner -1; a and b within 1e-6 of 0 and of 1; yf 0 and 765; and every one that exists bit for bit."""
    height, width = 12, 16
    cam = camera(VS, height, width, fx=14.0, fy=14.0, cx=7.5, cy=5.5)
    Ym = np_intensity(texture(height, width))
    Ym[5, 9] = -1.0
    Rm, _ = motion(PM, VS)
    rng = np.random.default_rng(3)
    ups = np.concatenate([rng.uniform(-0.5, width - 0.5, 400), [width - 1.0, width - 0.75, 3.0 + 1e-7, 4.0 - 1e-7, 8.6, 9.4, 2.5, 6.0]])
    vps = np.concatenate([rng.uniform(-0.5, height - 0.5, 400), [3.3, 4.1, 2.0 - 1e-7, 6.0 + 1e-7, 4.5, 5.2, -0.25, -1e-9]])
    yfs = np.concatenate([rng.integers(0, 766, 400), [0, 765, 0, 765, 300, 300, 100, 100]]).astype(f32)
    m2 = rng.uniform(40.0, 120.0, ups.size)
    m = [rng.uniform(-30, 30, ups.size), rng.uniform(-30, 30, ups.size), m2]
    exists, r, n, det = np_colour_term(cam, Ym, Rm, m, ups, vps, yfs, DEFAULT_WEIGHT)
    seen = dict(right=0, above=0, corner=0, a0=0, a1=0, b0=0, b1=0, black=0, white=0, added=0)
    for k in range(ups.size):
        out, mk = np.zeros(4, f64), np.array([m[0][k], m[1][k], m[2][k]], f64)
        got = HC.mtc_term(C.byref(Camera(**cam)), Ym.ctypes.data_as(f32p), _f32(PM).reshape(16).ctypes.data_as(f32p), mk.ctypes.data_as(f64p), ups[k], vps[k], yfs[k],
                          DEFAULT_WEIGHT, out.ctypes.data_as(f64p))
        assert got == int(exists[k]), k
        if got:
            assert np.array_equal(bits(out), bits(np.array([r[k], n[0][k], n[1][k], n[2][k]]))), k
            seen["added"] += 1
            seen["a0"] += det["a"][k] < 1e-6
            seen["a1"] += det["a"][k] > 1 - 1e-6
            seen["b0"] += det["b"][k] < 1e-6
            seen["b1"] += det["b"][k] > 1 - 1e-6
            seen["black"] += yfs[k] == 0
            seen["white"] += yfs[k] == 765
        else:
            seen["right"] += math.floor(ups[k]) + 1 == width
            seen["above"] += math.floor(vps[k]) < 0
            seen["corner"] += bool(det["inside"][k] and not det["corners"][k])
    print("classes of the term:", seen)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("height,width", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_system_against_the_restatement(HC, height, width):
    """Every pose of pair_poses under every option set, bit for bit, the five counts printed.  Over them: a term skipped for one
    corner of -1 (next to a depth step or a miss); a or b within 1e-6 of 0 and of 1 (the model's own pose); frame pixels of 0 and
    765 with a term; and, on the largest grid, a photo_weight that puts half the colour residuals above Huber's threshold.  A term
    skipped by the image bounds cannot occur here (the model map's border is invalid: test_the_term_alone_in_every_class), which
    is asserted as well."""
    case = colour_pair(7 + height, height, width)
    cam, d, bgr, mb, md = case["cam"], case["depth"], case["bgr"], case["model_bgr"], case["model"]
    seen = dict(photo=0, corner=0, near0=0, near1=0, black=0, white=0, geometric_only=0)
    for pname, pose in pair_poses(cam):
        for oname, opt in COLOUR_OPTS:
            want = np_track_colour_system(cam, bgr, d, mb, md, PM, pose, detail=True, **opt)
            assert_same_system(cpp_system(HC, cam, bgr, d, mb, md, PM, pose, **opt), want[:2], "%s, %s" % (pname, oname))
            print("%dx%d %s, %s: counts %s" % (height, width, pname, oname, want[1]))
            det = want[2]
            assert not det["bounds"].any(), "a valid sample never projects outside the interpolation's bounds"
            ph = det["photo"]
            seen["photo"] += int(ph.sum())
            seen["corner"] += int(det["corner"].sum())
            seen["geometric_only"] += want[1][1] - want[1][4]
            seen["near0"] += int(((det["a"] < 1e-6) | (det["b"] < 1e-6))[ph].sum())
            seen["near1"] += int(((det["a"] > 1 - 1e-6) | (det["b"] > 1 - 1e-6))[ph].sum())
            seen["black"] += int((det["yf"] == 0)[ph].sum())
            seen["white"] += int((det["yf"] == 765)[ph].sum())
    print("%dx%d classes: %s" % (height, width, seen))
    if height >= 16:
        assert all(v > 0 for v in seen.values()), seen
    else:
        assert seen["photo"] > 0 or height < 16
    if height == 96:
        pose = MT.pose_near()
        base = np_track_colour_system(cam, bgr, d, mb, md, PM, pose, detail=True)
        ph = base[2]["photo"]
        med = float(np.median(np.abs(base[2]["rp"][ph]))) / float(DEFAULT_WEIGHT)     # the median colour residual in intensity units
        weight = 1.0 / med                                                              # huber = 1: half of them above it
        want = np_track_colour_system(cam, bgr, d, mb, md, PM, pose, detail=True, photo_weight=weight)
        share = float((np.abs(want[2]["rp"][want[2]["photo"]]) > 1.0).mean())
        print("photo_weight %.5f: %.3f of %d colour residuals above Huber's threshold" % (weight, share, int(ph.sum())))
        assert 0.4 < share < 0.6
        assert_same_system(cpp_system(HC, cam, bgr, d, mb, md, PM, pose, photo_weight=weight), want[:2], "half above Huber")


@pytest.mark.parametrize("height,width", [(18, 32), (96, 128)], ids=["18x32", "96x128"])
def test_uniform_colour_reduces_to_the_geometric_call(HC, height, width):
    """Frame and model one constant grey: every colour residual and gradient is zero, the photometric terms add zeros, and sums
    and the first four counts are drf_track_system's host rule bit for bit -- while counts[4] > 0 says the terms were there."""
    case = pair_case(7 + height, height, width)
    cam = case["cam"]
    grey = np.full((height, width, 3), 93, np.uint8)
    for pname, pose in pair_poses(cam)[:3]:
        for oname, opt in MT.SYSTEM_OPTS:
            got = cpp_system(HC, cam, grey, case["depth"], grey, case["model"], PM, pose, **opt)
            sums, counts = np.zeros(28, f64), np.zeros(4, np.uint64)
            assert HC.mtc_geometric(C.byref(Camera(**cam)), _f32(case["depth"]).ctypes.data_as(f32p), _f32(case["model"]).ctypes.data_as(f32p),
                                    _f32(PM).reshape(16).ctypes.data_as(f32p), _f32(pose).reshape(16).ctypes.data_as(f32p), C.byref(MT.Options(**opt)),
                                    sums.ctypes.data_as(f64p), counts.ctypes.data_as(u64p)) == 0
            assert np.array_equal(bits(got[0]), bits(sums)), (pname, oname)
            assert got[1][:4] == tuple(int(v) for v in counts), (pname, oname)
            assert_same_system((sums, tuple(int(v) for v in counts)), MT.np_track_system(cam, case["depth"], case["model"], PM, pose, **opt), "geometric")
            if got[1][1] > 50:
                assert got[1][4] > 0, (pname, oname, got[1])


# ------------------------------------------------------------------ one textured plane: what the feature is for
PLANE_CAM = dict(height=48, width=64, fx=56.0, fy=56.0, cx=31.5, cy=23.5)
# (voxels in the plane along (0.8, -0.6), degrees about the normal); every start also half a voxel along the normal
PLANE_STARTS = [(2.0, 2.0), (5.0, 4.0), (8.0, 4.0), (12.0, 6.0)]
PLANE_OPTS = dict(centre_depth=1.5, **TRACK_EPS)
# measured on the restatement (see test_one_textured_plane): the rung used and its (degrees, voxels in the plane, voxels along the normal)
PLANE_USED = 3
PLANE_ERROR = (0.0000, 0.0014, 0.0001)


def plane_intensity(X, Y):
    return np.floor(3.0 * (127.5 + 110.0 * (np.sin(9.0 * X + 1.0) + np.sin(7.0 * Y + 2.0) + np.sin(5.0 * X - 6.0 * Y)) / 3.0) + 0.5)


def textured_plane_renderer(cam, depth_of_plane=1.5):
    """render(pose) -> (bgr, depth): the analytic ray-cast of the world plane z = depth_of_plane, coloured by plane_intensity of the
    hit's world (X, Y) split over the three channels so that b + g + r is that intensity."""
    v, u = np.meshgrid(np.arange(cam["height"], dtype=f64), np.arange(cam["width"], dtype=f64), indexing="ij")
    ray = np.stack([(u - f64(f32(cam["cx"]))) / f64(f32(cam["fx"])), (v - f64(f32(cam["cy"]))) / f64(f32(cam["fy"])), np.ones_like(u)], axis=-1)

    def render(pose):
        T = np.asarray(pose, f64).reshape(4, 4)
        dirs = ray @ T[:3, :3].T
        z = (depth_of_plane - T[2, 3]) / dirs[..., 2]
        hit = z > 0
        P = T[:3, 3] + dirs * np.where(hit, z, 0.0)[..., None]
        y = plane_intensity(P[..., 0], P[..., 1]).astype(np.int64)
        bgr = np.stack([y // 3, (y + 1) // 3, (y + 2) // 3], axis=-1)
        return np.where(hit[..., None], bgr, 0).astype(np.uint8), np.where(hit, z, 0.0).astype(f32)
    return render


def plane_start(k):
    vox, deg = PLANE_STARTS[k]
    return start_near(np.eye(4), (0, 0, 1), deg, (0.8 * vox, -0.6 * vox, 0.5), VS)


def plane_errors(T):
    """(degrees, voxels in the plane, voxels along the normal) of T against the identity."""
    a, _ = scene_errors(T, np.eye(4), VS)
    return a, float(np.hypot(T[0, 3], T[1, 3]) / VS), float(abs(T[2, 3]) / VS)


@pytest.fixture(scope="module")
def plane():
    cam = camera(VS, **PLANE_CAM)
    render = textured_plane_renderer(cam)
    bgr, depth = render(np.eye(4, dtype=f32))
    return dict(cam=cam, render=render, bgr=bgr, depth=depth)


def test_one_textured_plane(HC, plane):
    """The point of the call.  One textured plane at z = 1.5 m, a 48x64 camera, 2 cm voxels, the frame rendered at the identity.
    Geometry alone is DEGENERATE at the first evaluation, from every start.  With colour (default weight, TRACK_EPS, centre_depth
    1.5), from starts in the plane along (0.8, -0.6) plus half a voxel along the normal, turned about the normal -- MEASURED on the
    restatement, (voxels, degrees): status, renders, evaluations, then degrees / voxels in the plane / voxels along the normal:
      (2, 2):  CONVERGED, 2 renders, 4 evaluations, 0.00000 / 0.00436 / 0.00019
      (5, 4):  CONVERGED, 2 renders, 4 evaluations, 0.01978 / 0.00988 / 0.00090
      (8, 4):  CONVERGED, 2 renders, 5 evaluations, 0.00000 / 0.00170 / 0.00043
      (12, 6): CONVERGED, 3 renders, 7 evaluations, 0.00000 / 0.00140 / 0.00013
    (3 072 samples, 2 852 valid, 2 640 with a colour term at the last evaluation of each).
    The largest start that ends CONVERGED is used; its in-plane error is below one voxel -- inside the four-voxel band that
    drf_locate_frame needs, and where the geometric call leaves the start untouched."""
    p = plane
    cam, render = p["cam"], p["render"]
    runs = []
    for k in range(len(PLANE_STARTS)):
        start = plane_start(k)
        geo = np_track_colour_frame(render, cam, p["bgr"], p["depth"], start, colour=False, **PLANE_OPTS)
        assert geo["status"] == DEGENERATE and geo["iterations"] == 1
        r = np_track_colour_frame(render, cam, p["bgr"], p["depth"], start, **PLANE_OPTS)
        runs.append(r)
        print("start %s: status %d after %d renders and %d evaluations, counts %s, %.5f degrees %.5f voxels in the plane %.5f along the normal" %
              ((PLANE_STARTS[k], r["status"], r["renders"], r["iterations"], r["counts"]) + plane_errors(r["T"])))
        assert r["status"] != DEGENERATE
    converged = [k for k, r in enumerate(runs) if r["status"] == CONVERGED]
    assert converged, "no rung converges on the restatement: the rule is wrong"
    used = max(converged)
    a, t, nrm = plane_errors(runs[used]["T"])
    assert t < 1.0, "the in-plane error from the start used must end below one voxel"
    assert used == PLANE_USED
    assert abs(a - PLANE_ERROR[0]) < 1e-3 and abs(t - PLANE_ERROR[1]) < 1e-3 and abs(nrm - PLANE_ERROR[2]) < 1e-3, (a, t, nrm)
    start = plane_start(used)
    got = cpp_frame(HC, render, cam, p["bgr"], p["depth"], start, **PLANE_OPTS)
    assert_same_result(got, runs[used], "the textured plane on the host")
    assert got["counts"] == runs[used]["counts"] and got["renders"] == runs[used]["renders"]
    geo = cpp_frame(HC, render, cam, p["bgr"], p["depth"], start, colour=False, **PLANE_OPTS)
    assert geo["status"] == DEGENERATE and geo["iterations"] == 1 and np.array_equal(geo["T"], start.astype(f64))


# ------------------------------------------------------------------ the loop on a map: the oracle's ray-cast is the renderer
@pytest.fixture(scope="module")
def scene_map():
    s = track_scene()
    s["render_both"] = lambda pose: s["oracle"].render(pose)
    return s


def test_loop_on_the_map_against_the_restatement(HC, scene_map):
    """track_colour_frame_host over the oracle's renders of colour and depth from the first basin start: the sums of every
    evaluation, the five counters, the renders and the pose bit for bit, with and without colour.  MEASURED on the restatement:
    with colour MAX_ITERS after 10 renders and 40 evaluations, 2.6623 degrees and 9.6531 voxels off the scan's pose; without colour
    CONVERGED after 6 renders and 13 evaluations, 0.6672 degrees and 0.5076 voxels off.  Colour makes this scene WORSE at the
    default weight: a render that aliases the texture pulls the pose towards chance matches.
    No improvement is asserted on this scene: its texture reaches 110 rad/m, above what a 96x128 render resolves; bits and
    statuses only."""
    s = scene_map
    start = basin_start(s, 0)
    opt = track_opts(s)
    want = np_track_colour_frame(s["render_both"], s["cam"], s["bgr"], s["depth"], start, **opt)
    got = cpp_frame(HC, s["render_both"], s["cam"], s["bgr"], s["depth"], start, **opt)
    assert_same_result(got, want, "the scene with colour")
    assert got["counts"] == want["counts"] and got["renders"] == want["renders"] and len(got["trace"]) == want["iterations"]
    assert want["counts"][4] > 1000 and want["status"] in (CONVERGED, MAX_ITERS)
    geo = cpp_frame(HC, s["render_both"], s["cam"], s["bgr"], s["depth"], start, colour=False, **opt)
    ref = MT.np_track_frame(s["render"], s["cam"], s["depth"], start, **opt)
    assert_same_result(geo, ref, "the scene without colour")
    for name, r in (("with colour", want), ("without", ref)):
        a, t = scene_errors(r["T"], s["pose"])
        print("%s: status %d after %d renders and %d evaluations, %.4f degrees %.4f voxels off" % (name, r["status"], r["renders"], r["iterations"], a, t))


# ------------------------------------------------------------------ options, defaults, refusals
def test_options_and_their_defaults(HC):
    out, wbits, name = np.zeros(11, f64), C.c_uint32(0), C.create_string_buffer(32)
    vs = f32(0.02)
    assert HC.mtc_options(None, vs, out.ctypes.data_as(f64p), C.byref(wbits), name) == 0
    assert out[:10].tolist() == [10, 4, 1, float(f32(25.0) * vs), float(f32(5.0) * vs), 1.0, 0.0, 1e-7, 1e-5, 0.25]
    assert wbits.value == int(f32(1.0 / 27.0).view(np.uint32)) == 0x3D17B426
    assert HC.mtc_options(C.byref(colour_options(0.0, huber=0.25)), vs, out.ctypes.data_as(f64p), C.byref(wbits), name) == 0
    assert wbits.value == int((f32(1.0 / 27.0) * f32(0.25)).view(np.uint32)), "the default is 1/27 times huber, huber resolved first"
    assert HC.mtc_options(C.byref(colour_options(0.5, huber=0.25, step=2)), vs, out.ctypes.data_as(f64p), C.byref(wbits), name) == 0
    assert out[10] == 0.5 and out[2] == 2 and out[5] == 0.25
    for bad in (-1.0, float("nan"), float("inf")):
        assert HC.mtc_options(C.byref(colour_options(bad)), vs, out.ctypes.data_as(f64p), C.byref(wbits), name) == 1
        assert name.value.decode() == "photo_weight"
    assert HC.mtc_options(C.byref(colour_options(-1.0, step=-1)), vs, out.ctypes.data_as(f64p), C.byref(wbits), name) == 1
    assert name.value.decode() == "step", "the tracking's own options are judged first"
    assert C.sizeof(ColourOptions) == 64 and ColourOptions.photo_weight.offset == 56


def test_refusals_and_an_image_without_a_sample(HC):
    case = colour_pair(5, 24, 32)
    cam = case["cam"]
    scaled, nan = np.eye(4, dtype=f32), np.eye(4, dtype=f32)
    scaled[:3, :3] *= 1.01
    nan[2, 3] = np.nan
    cm, b, d, mb, md, pm = Camera(**cam), _u8(case["bgr"]), _f32(case["depth"]), _u8(case["model_bgr"]), _f32(case["model"]), _f32(PM).reshape(16)
    sums, counts = np.zeros(28, f64), np.zeros(5, np.uint64)
    args = (C.byref(cm), b.ctypes.data_as(u8p), d.ctypes.data_as(f32p), mb.ctypes.data_as(u8p), md.ctypes.data_as(f32p))
    for bad in (scaled, nan):
        bb = _f32(bad).reshape(16)
        for mp, p in ((pm, bb), (bb, pm)):
            assert HC.mtc_system(*args, mp.ctypes.data_as(f32p), p.ctypes.data_as(f32p), None, sums.ctypes.data_as(f64p), counts.ctypes.data_as(u64p)) == 2
    assert HC.mtc_system(*args, pm.ctypes.data_as(f32p), pm.ctypes.data_as(f32p), C.byref(colour_options(float("nan"))), sums.ctypes.data_as(f64p),
                         counts.ctypes.data_as(u64p)) == 1
    for name, depth, model in (("no samples", np.zeros((24, 32), f32), case["model"]), ("no hit", case["depth"], np.zeros((24, 32), f32))):
        want = np_track_colour_system(cam, case["bgr"], depth, case["model_bgr"], model, PM, MT.pose_near())
        got = cpp_system(HC, cam, case["bgr"], depth, case["model_bgr"], model, PM, MT.pose_near())
        assert_same_system(got, want, name)
        assert not got[0].any() and got[1][1] == 0 and got[1][3] == 0 and got[1][4] == 0
    assert got[1][0] > 300 and got[1][2] == got[1][0]


# ------------------------------------------------------------------ sanitizers, the C ABI and the shim
def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """track_model_colour_host, track_colour_system_host and track_colour_frame_host under AddressSanitizer and UBSan: a plain
    executable, nothing preloaded, nothing loaded into Python.  It reads one synthetic pair from a file and prints the sums, which
    are the restatement's bit for bit; then cases of its own."""
    exe, data = str(tmp_path / "map_track_colour_san"), str(tmp_path / "case.bin")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_track_colour_san.cpp"), "-o", exe])
    case = colour_pair(31, 24, 32)
    opt = dict(step=2, centre_depth=1.5, dist_max=0.04)
    pose = MT.pose_near()
    with open(data, "wb") as fh:
        fh.write(bytes(Camera(**case["cam"])) + bytes(colour_options(0.05, **opt)) + _u8(case["bgr"]).tobytes() + _f32(case["depth"]).tobytes() +
                 _u8(case["model_bgr"]).tobytes() + _f32(case["model"]).tobytes() + _f32(PM).tobytes() + _f32(pose).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_track_colour_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    line = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("system")][0]
    want = np_track_colour_system(case["cam"], case["bgr"], case["depth"], case["model_bgr"], case["model"], PM, pose, photo_weight=0.05, **opt)
    assert np.array_equal(np.array([int(x, 16) for x in line[:28]], np.uint64), bits(want[0])) and tuple(int(x) for x in line[28:]) == want[1]
    assert want[1][1] > 20 and want[1][4] > 10


def test_abi_declares_exports_and_types_the_five_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_track_colour_system", "drf_track_colour_frame", "drf_track_colour_system_device", "drf_track_colour_frame_device",
                            "drf_track_colour_stats"])
    assert "drf_track_colour_options_t" in src
    assert C.sizeof(L.TrackColourOptions) == C.sizeof(ColourOptions) == 64
    assert L.TrackColourOptions.photo_weight.offset == 56 and L.TrackColourOptions.track.offset == 0
    assert C.sizeof(L.TrackOptions) == 56
    lib = L.lib()
    T = (C.c_float * 16)(*np.eye(4, dtype=f32).reshape(16))
    depth, bgr = (C.c_float * 4)(), (C.c_uint8 * 12)()
    sums, counts, out = (C.c_double * 28)(), (C.c_uint64 * 5)(), (C.c_uint64 * 6)()
    assert lib.drf_track_colour_system(None, bgr, depth, bgr, depth, T, T, None, sums, counts) == 1
    assert lib.drf_track_colour_frame(None, bgr, depth, T, None, T, None) == 1
    assert lib.drf_track_colour_system_device(None, None, None, None, None, T, T, None, sums, counts) == 1
    assert lib.drf_track_colour_frame_device(None, None, None, T, None, T, None) == 1
    assert lib.drf_track_colour_stats(None, out) == 1
    import tandem_amd.dr_fusion as F
    for name in ("track_colour_system", "track_colour_frame", "track_colour_stats"):
        assert callable(getattr(F.DrFusion, name))
    hdr = open(os.path.join(ROOT, "include", "dr_mi355x.h")).read()
    assert "colour / photometric terms" not in hdr, "colour is no longer out of scope of drf_track_*"


def test_shim_compiles(tmp_path):
    """tandem_amd/libdr/dr_fusion.h TrackColourFrame as a TANDEM translation unit would call it
    (tests/cpp/map_track_colour_shim.cpp): it compiles and links against the library; tests/test_fusion_track_colour_gpu.py runs it."""
    abi_module()
    exe = str(tmp_path / "map_track_colour_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_track_colour_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert os.path.isfile(exe)
