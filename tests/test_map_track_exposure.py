"""CPU: the host half of drf_track_exposure_system / drf_track_exposure_frame (include/dr_mi355x.h "Tracks a frame whose exposure
differs from the map's", DESIGN.md §7c "Tracking under a change of exposure").  track_exposure_point, exposure_step and
track_exposure_frame_host of tandem_amd/csrc/pose_host.h compiled with plain g++ (tests/cpp/map_track_exposure_check.cpp) and
held, bit for bit, to np_exposure_eval / np_exposure_step / np_track_exposure_frame, numpy restatements written here from the
header's statement -- the reference of tests/test_fusion_track_exposure_gpu.py too; the invariant at gain 1, offset 0 against the
pyramid family; a map of one colour, where the exposure is held; what the call is for, measured on the restatement with the
textured plane re-exposed; the clamp of the gain; options and refusals; the same under AddressSanitizer and UBSan as a stand-alone
program (tests/cpp/map_track_exposure_san.cpp); the names of the C ABI.  The single-level and pyramid restatements, the synthetic
pairs, the plane and the scene come from tests/test_map_track*.py by import."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import test_map_track as MT
import test_map_track_colour as TC
import test_map_track_pyramid as TP
from fusion_helpers import abi_module, check_symbols
from test_map_align import CONVERGED, DEGENERATE, LOST, MAX_ITERS, Result, assert_same_result, bits, butterfly, np_step
from test_map_locate import Camera, camera
from test_map_track import PM, basin_start, np_centre, pair_poses, track_opts, track_scene
from test_map_transform import motion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p, u64p, f32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_double)
VS = MT.VS
f32, f64 = np.float32, np.float64
_f32, _u8 = TC._f32, TC._u8
EXPOSURE_FIELDS = ("gain_init", "offset_init", "gain_min", "gain_max", "eps_gain", "eps_offset")
OFFSET_MAX = 765.0


# ------------------------------------------------------------------ the rule, restated
def np_exposure_options(opt):
    """The exposure's own options taken out of opt (a dict, changed) with their defaults: float fields go through float32."""
    x = dict(gain_init=1.0, offset_init=0.0, gain_min=0.25, gain_max=4.0, eps_gain=1e-4, eps_offset=1e-2)
    for k in EXPOSURE_FIELDS:
        v = opt.pop(k, 0)
        if k.startswith("eps"):
            x[k] = float(v) if v else x[k]
        elif v or k == "offset_init":
            x[k] = float(f32(v))
    return x


def np_exposure_eval(cam, bgr, depth, model, Ym, model_pose, R, tv, o, lam, G, B):
    """One evaluation at the pose (R, tv) and the exposure (G, B) in float64: (sums (45,), (samples, valid, unassociated, rejected,
    photometric)).  np_colour_eval's walk; the photometric term reads I and gm and the exposure; 17 sums behind the 28."""
    Wd, Hd, step = int(cam["width"]), int(cam["height"]), int(o["step"])
    Wg, Hg = -(-Wd // step), -(-Hd // step)
    total = Wg * Hg
    groups = -(-total // 512)
    depth = np.ascontiguousarray(depth, f32).reshape(Hd, Wd)
    yimg = TC.np_intensity(np.asarray(bgr).reshape(Hd, Wd, 3))
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
    lam64, G, B = f64(f32(lam)), f64(G), f64(B)
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

        def jac(nv):
            return [x[1] * nv[2] - x[2] * nv[1], x[2] * nv[0] - x[0] * nv[2], x[0] * nv[1] - x[1] * nv[0], nv[0], nv[1], nv[2]]

        def weight(r):
            a = np.abs(r)
            return np.where(a <= hub, 1.0, hub / a)

        # the photometric term: track_photo_model's conditions, I and gm
        upc, vpc = np.where(inimg, up, 0.0), np.where(inimg, vp, 0.0)
        fu, fv = np.floor(upc), np.floor(vpc)
        inside2 = (fu >= 0.0) & (fu + 1.0 <= float(Wd - 1)) & (fv >= 0.0) & (fv + 1.0 <= float(Hd - 1))
        ju, jv = np.where(inside2, fu, 0.0).astype(np.int64), np.where(inside2, fv, 0.0).astype(np.int64)
        if Wd < 2 or Hd < 2:
            exists = np.zeros(n.shape, bool)
            I = np.zeros(n.shape, f64)
            gm = [I, I, I]
        else:
            Y = np.ascontiguousarray(Ym, f32).reshape(Hd, Wd)
            c00, c10, c01, c11 = Y[jv, ju], Y[jv, ju + 1], Y[jv + 1, ju], Y[jv + 1, ju + 1]
            corners = (c00 >= f32(0)) & (c10 >= f32(0)) & (c01 >= f32(0)) & (c11 >= f32(0))
            y00, y10, y01, y11 = c00.astype(f64), c10.astype(f64), c01.astype(f64), c11.astype(f64)
            a, b = upc - fu, vpc - fv
            oa, ob = 1.0 - a, 1.0 - b
            I = ob * (oa * y00 + a * y10) + b * (oa * y01 + a * y11)
            Iu = ob * (y10 - y00) + b * (y11 - y01)
            Iv = oa * (y01 - y00) + a * (y11 - y10)
            gm0, gm1 = (Iu * fx) / m[2], (Iv * fy) / m[2]
            gm = [gm0, gm1, -((gm0 * m[0] + gm1 * m[1]) / m[2])]
            exists = inside2 & corners
        rp = lam64 * ((G * I + B) - yf.astype(f64))
        npv = [(lam64 * ((Rm[k, 0] * gm[0] + Rm[k, 1] * gm[1]) + Rm[k, 2] * gm[2])) * G for k in range(3)]
        photo = valid & exists
        Jg, Jp = jac(nw), jac(npv)
        wg, wp = weight(rg), weight(rp)
        tg = np.where(valid[..., None], np.stack(TC._terms(wg, Jg, rg), axis=-1), 0.0).reshape(groups, 8, 64, 28)
        tp = np.where(photo[..., None], np.stack(TC._terms(wp, Jp, rp), axis=-1), 0.0).reshape(groups, 8, 64, 28)
        J6, J7 = lam64 * I, lam64 + 0.0 * I
        wj = [wp * Jp[k] for k in range(6)]
        w6, w7 = wp * J6, wp * J7
        ext = [wj[k] * J6 for k in range(6)] + [wj[k] * J7 for k in range(6)] + [w6 * J6, w6 * J7, w7 * J7, w6 * rp, w7 * rp]
        te = np.where(photo[..., None], np.stack(ext, axis=-1), 0.0).reshape(groups, 8, 64, 17)
    assert tg.dtype == f64 and tp.dtype == f64 and te.dtype == f64
    acc = np.zeros((groups, 64, 45), f64)
    for k in range(8):
        acc[..., :28] = acc[..., :28] + tg[:, k]
        acc[..., :28] = acc[..., :28] + tp[:, k]
        acc[..., 28:] = acc[..., 28:] + te[:, k]
    sums = np_fold45(butterfly(acc)[:, 0, :]) if groups else np.zeros(45)
    counts = (int(sample.sum()), int(valid.sum()), int((sample & ~assoc).sum()), int(rejected.sum()), int(photo.sum()))
    assert counts[0] == counts[1] + counts[2] + counts[3]
    return sums, counts, c


def np_fold45(partial):
    """k_exposure_fold: per component lane l adds partial[l], partial[l + 64], ... from +0.0, then the butterfly."""
    n = len(partial)
    pad = np.zeros((-n % 64, 45), f64)
    rows = np.concatenate([partial, pad]).reshape(-1, 64, 45)
    lane = np.zeros((64, 45), f64)
    for j in range(len(rows)):
        lane = lane + rows[j]
    return butterfly(lane)[0]


def np_exposure_system(cam, L, bgr, depth, model_bgr, model_depth, model_pose, pose, gain=1.0, offset=0.0, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
    """drf_track_exposure_system: both pairs reduced to level L, then np_exposure_eval on the level's camera: (sums (45,), counts)."""
    opt = dict(opt)
    np_exposure_options(opt)
    o, lam, levels, coarse = TP.np_pyramid_options(cam, levels, coarse_renders, photo_weight, **opt)
    oL, camL = TP.np_level_options(o, coarse, L), TP.np_level_cam(cam, L)
    Hd, Wd = int(cam["height"]), int(cam["width"])
    fc, fd = TP.np_reduce(np.asarray(bgr).reshape(Hd, Wd, 3), np.asarray(depth, f32).reshape(Hd, Wd), L, oL["max_jump"])
    mc, md = TP.np_reduce(np.asarray(model_bgr).reshape(Hd, Wd, 3), np.asarray(model_depth, f32).reshape(Hd, Wd), L, oL["max_jump"])
    R, tv = motion(pose, cam["voxel_size"])
    model, Ym = TC.np_colour_model(camL, mc, md, oL["max_jump"])
    return np_exposure_eval(camL, fc, fd, model, Ym, model_pose, R, tv, oL, lam, gain, offset)[:2]


def _solve(H, b, top, N):
    """align_solve in Python floats: (index of the failing pivot or -1, d)."""
    Lm = [[0.0] * N for _ in range(N)]
    for j in range(N):
        p = H[j][j]
        for k in range(j):
            p = p - Lm[j][k] * Lm[j][k]
        if not p > 1e-12 * top:
            return j, None
        Lm[j][j] = math.sqrt(p)
        for i in range(j + 1, N):
            t = H[i][j]
            for k in range(j):
                t = t - Lm[i][k] * Lm[j][k]
            Lm[i][j] = t / Lm[j][j]
    y, d = [0.0] * N, [0.0] * N
    for i in range(N):
        t = -b[i]
        for k in range(i):
            t = t - Lm[i][k] * y[k]
        y[i] = t / Lm[i][i]
    for i in range(N - 1, -1, -1):
        t = y[i]
        for k in range(i + 1, N):
            t = t - Lm[k][i] * d[k]
        d[i] = t / Lm[i][i]
    return -1, d


def _move(d, oo, c, R, tv):
    """align_move in Python floats"""
    a = 1.0 / math.sqrt(1.0 + oo / 4.0)
    qw, qx, qy, qz = a, (a * d[0]) / 2.0, (a * d[1]) / 2.0, (a * d[2]) / 2.0
    Rq = [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
          [2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)],
          [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]]
    Rl, tl, cl = [[float(v) for v in row] for row in R], [float(v) for v in tv], [float(v) for v in c]
    e = [tl[k] - cl[k] for k in range(3)]
    R2 = np.array([[(Rq[i][0] * Rl[0][j] + Rq[i][1] * Rl[1][j]) + Rq[i][2] * Rl[2][j] for j in range(3)] for i in range(3)], f64)
    t2 = np.array([(cl[i] + ((Rq[i][0] * e[0] + Rq[i][1] * e[1]) + Rq[i][2] * e[2])) + d[3 + i] for i in range(3)], f64)
    return R2, t2


def np_exposure_step(sums, c, R, tv, eps_rot, eps_trans, x):
    """exposure_step in Python floats: (status or -1, R, tv); x (gain, offset, the bounds, the thresholds, held) is updated."""
    S = [float(v) for v in sums]
    H = [[0.0] * 8 for _ in range(8)]
    idx = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = H[j][i] = S[idx]
            idx += 1
    for i in range(6):
        H[i][6] = H[6][i] = S[28 + i]
        H[i][7] = H[7][i] = S[34 + i]
    H[6][6], H[6][7], H[7][6], H[7][7] = S[40], S[41], S[41], S[42]
    b = S[21:27] + [S[43], S[44]]
    top = H[0][0]
    for j in range(1, 8):
        top = H[j][j] if H[j][j] > top else top
    if not top > 0.0:
        return DEGENERATE, R, tv
    failed, d = _solve(H, b, top, 8)
    if failed >= 6:
        x["held"] += 1
        return np_step(sums[:28], c, R, tv, eps_rot, eps_trans)
    if failed >= 0:
        return DEGENERATE, R, tv
    oo = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    vv = (d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]
    if oo != oo or vv != vv or d[6] != d[6] or d[7] != d[7]:
        return DEGENERATE, R, tv
    if math.sqrt(oo) < eps_rot and math.sqrt(vv) < eps_trans and abs(d[6]) < x["eps_gain"] and abs(d[7]) < x["eps_offset"]:
        return CONVERGED, R, tv
    R2, t2 = _move(d, oo, c, R, tv)
    x["gain"] = min(max(x["gain"] + d[6], x["gain_min"]), x["gain_max"])
    x["offset"] = min(max(x["offset"] + d[7], -OFFSET_MAX), OFFSET_MAX)
    return -1, R2, t2


def np_exposure_loop(system, cam, pose_init, o, x):
    """track_loop with the exposure in the state, over system(p16, R, tv, G, B) -> (sums45, counts, c): np_loop's dict."""
    p16 = np.ascontiguousarray(pose_init, f32).reshape(4, 4).copy()
    out = dict(status=MAX_ITERS, iterations=0, sums=np.zeros(28), samples=0, valid0=0, valid=0, cost0=0.0, cost=0.0, trace=[], counts=(), T=p16.astype(f64), renders=0)
    for rnd in range(o["max_renders"]):
        R, tv = motion(p16, cam["voxel_size"])
        good, status, its = (R, tv, x["gain"], x["offset"]), MAX_ITERS, 0
        for it in range(o["inner_iters"]):
            s45, cnt, c = system(p16, R, tv, x["gain"], x["offset"])
            sums, x["ext"] = s45[:28].copy(), s45[28:].copy()
            valid = cnt[1]
            cost = float(sums[27]) / float(valid) if valid else 0.0
            out["trace"].append(sums)
            out.update(sums=sums, samples=cnt[0], valid=valid, cost=cost, counts=cnt, iterations=out["iterations"] + 1)
            its = it + 1
            if rnd == 0 and it == 0:
                out.update(valid0=valid, cost0=cost)
            if float(valid) < o["min_valid"] * float(cnt[0]) or valid < 6:
                status = LOST
                R, tv, x["gain"], x["offset"] = good
                break
            good = (R, tv, x["gain"], x["offset"])
            s, R, tv = np_exposure_step(s45, c, R, tv, o["eps_rot"], o["eps_trans"], x)
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


def np_track_exposure_frame(render, cam, bgr, depth, pose_init, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
    """drf_track_exposure_frame over render(pose (4, 4) float32) -> (bgr, depth) at full resolution: level 0's dict (np_loop's) plus
    gain, offset, ext, held, photometric, levels, stats8."""
    opt = dict(opt)
    xo = np_exposure_options(opt)
    o, lam, levels, coarse = TP.np_pyramid_options(cam, levels, coarse_renders, photo_weight, **opt)
    x = dict(gain=xo["gain_init"], offset=xo["offset_init"], gain_min=xo["gain_min"], gain_max=xo["gain_max"], eps_gain=xo["eps_gain"], eps_offset=xo["eps_offset"],
             held=0, ext=np.zeros(17))
    Hd, Wd = int(cam["height"]), int(cam["width"])
    depth = np.asarray(depth, f32).reshape(Hd, Wd)
    bgr = np.asarray(bgr).reshape(Hd, Wd, 3)
    p16 = np.ascontiguousarray(pose_init, f32).reshape(4, 4).copy()
    stats, per_level, trace = [0] * 8, {}, []
    for L in range(levels - 1, -1, -1):
        camL, oL = TP.np_level_cam(cam, L), TP.np_level_options(o, coarse, L)
        fc, fd = (bgr, depth) if L == 0 else TP.np_reduce(bgr, depth, L, oL["max_jump"])
        state = {}

        def system(p, R, tv, G, B, L=L, oL=oL, camL=camL, fc=fc, fd=fd, state=state):
            if state.get("at") is None or not np.array_equal(state["at"], p):
                Cm, Dm = render(p)
                if L > 0:
                    Cm, Dm = TP.np_reduce(np.asarray(Cm).reshape(Hd, Wd, 3), np.asarray(Dm, f32).reshape(Hd, Wd), L, oL["max_jump"])
                state["model"], state["Ym"] = TC.np_colour_model(camL, Cm, Dm, oL["max_jump"])
                state["at"] = p.copy()
            return np_exposure_eval(camL, fc, fd, state["model"], state["Ym"], p, R, tv, oL, lam, G, B)
        began = (x["gain"], x["offset"])
        r = np_exposure_loop(system, camL, p16, oL, x)
        per_level[L] = (r["status"], r["renders"], r["iterations"], r["valid"])
        trace += r["trace"]
        Wg, Hg = -(-camL["width"] // oL["step"]), -(-camL["height"] // oL["step"])
        stats[0] += Wg * Hg; stats[1] += r["samples"]; stats[2] += r["valid"]; stats[3] += r["iterations"]; stats[4] += r["renders"]; stats[6] += 1
        if L == 0:
            return dict(r, trace=trace, levels=per_level, stats8=tuple(stats), gain=x["gain"], offset=x["offset"], ext=x["ext"], held=x["held"],
                        photometric=r["counts"][4] if r["counts"] else 0)
        if r["status"] in (LOST, DEGENERATE):
            stats[7] += 1
            x["gain"], x["offset"] = began
            continue
        p16 = r["T"].astype(f32)


# ------------------------------------------------------------------ the compiled host half
class ExposureOptions(C.Structure):
    """drf_track_exposure_options_t"""
    _fields_ = [("pyramid", TP.PyramidOptions), ("gain_init", C.c_float), ("offset_init", C.c_float), ("gain_min", C.c_float), ("gain_max", C.c_float),
                ("eps_gain", C.c_double), ("eps_offset", C.c_double)]


class ExposureResult(C.Structure):
    """drf_exposure_result_t"""
    _fields_ = [("pose", Result), ("gain", C.c_double), ("offset", C.c_double), ("ext", C.c_double * 17), ("photometric", C.c_uint64), ("held", C.c_uint64)]


def exposure_options(levels=0, coarse_renders=0, photo_weight=0.0, **opt):
    own = {k: opt.pop(k) for k in EXPOSURE_FIELDS if k in opt}
    return ExposureOptions(TP.pyramid_options(levels, coarse_renders, photo_weight, **opt), **own)


RENDER_FN = TC.RENDER_FN


def build_check(directory):
    so = os.path.join(str(directory), "libmap_track_exposure_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_track_exposure_check.cpp"), "-o", so])
    h = C.CDLL(so)
    cam, xo = C.POINTER(Camera), C.POINTER(ExposureOptions)
    h.mte_options.argtypes = [xo, C.c_float, C.c_int, C.c_int, f64p, C.c_char_p]
    h.mte_system.argtypes = [cam, C.c_int, u8p, f32p, u8p, f32p, f32p, f32p, C.c_double, C.c_double, xo, f64p, u64p]
    h.mte_step.argtypes = [f64p, f64p, C.c_double, C.c_double, f64p, f64p, u64p]
    h.mte_frame.argtypes = [cam, u8p, f32p, RENDER_FN, C.c_void_p, f32p, xo, C.POINTER(ExposureResult), f64p, C.c_size_t, u64p]
    return h


@pytest.fixture(scope="module")
def HX(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("map_track_exposure"))


@pytest.fixture(scope="module")
def HC(tmp_path_factory):
    return TC.build_check(tmp_path_factory.mktemp("map_track_exposure_colour"))


@pytest.fixture(scope="module")
def HP(tmp_path_factory):
    return TP.build_check(tmp_path_factory.mktemp("map_track_exposure_pyramid"))


def cpp_system(HX, cam, L, bgr, depth, model_bgr, model_depth, model_pose, pose, gain=1.0, offset=0.0, **opt):
    b, d, mb, md = _u8(bgr), _f32(depth), _u8(model_bgr), _f32(model_depth)
    model_pose, pose = _f32(model_pose).reshape(16), _f32(pose).reshape(16)
    sums, counts = np.zeros(45, f64), np.zeros(5, np.uint64)
    rc = HX.mte_system(C.byref(Camera(**cam)), L, b.ctypes.data_as(u8p), d.ctypes.data_as(f32p), mb.ctypes.data_as(u8p), md.ctypes.data_as(f32p),
                       model_pose.ctypes.data_as(f32p), pose.ctypes.data_as(f32p), gain, offset, C.byref(exposure_options(**opt)), sums.ctypes.data_as(f64p),
                       counts.ctypes.data_as(u64p))
    assert rc == 0, rc
    return sums, tuple(int(v) for v in counts)


def cpp_frame(HX, render, cam, bgr, depth, pose, **opt):
    """track_exposure_frame_host over the Python renderer as a dict shaped like np_track_exposure_frame's."""
    depth, pose, b = _f32(depth), _f32(pose).reshape(16), _u8(bgr)
    npix = cam["height"] * cam["width"]

    def call(p16, cout, dout, user):
        c, d = render(np.ctypeslib.as_array(p16, (16,)).reshape(4, 4).copy())
        c, d = _u8(c), _f32(d)
        C.memmove(cout, c.ctypes.data, npix * 3)
        C.memmove(dout, d.ctypes.data, npix * 4)

    res = ExposureResult()
    nl, nc = int(opt.get("levels", 0)) or 3, int(opt.get("coarse_renders", 0)) or 3
    cap = (int(opt.get("max_renders", 0) or 10) + (nl - 1) * nc) * int(opt.get("inner_iters", 0) or 4)
    trace, stats = np.zeros((cap, 28), f64), np.zeros(28, np.uint64)
    assert HX.mte_frame(C.byref(Camera(**cam)), b.ctypes.data_as(u8p), depth.ctypes.data_as(f32p), RENDER_FN(call), None, pose.ctypes.data_as(f32p),
                        C.byref(exposure_options(**opt)), C.byref(res), trace.ctypes.data_as(f64p), cap, stats.ctypes.data_as(u64p)) == 0
    st, r = [int(v) for v in stats], res.pose
    return dict(T=np.array(r.T, f64).reshape(4, 4), sums=np.array(r.sums, f64), samples=int(r.samples), valid0=int(r.valid0), valid=int(r.valid),
                cost0=float(r.cost0), cost=float(r.cost), iterations=int(r.iterations), status=int(r.status), trace=[trace[i] for i in range(st[3])],
                stats8=tuple(st[:8]), levels={L: tuple(st[8 + 4 * L:12 + 4 * L]) for L in range(5) if st[8 + 4 * L + 2]},
                gain=float(res.gain), offset=float(res.offset), ext=np.array(res.ext, f64), held=int(res.held), photometric=int(res.photometric))


def assert_same_exposure(got, want, what):
    """Two runs of the whole call, bit for bit: the pose's result, every evaluation, the levels, and the exposure's own fields"""
    assert_same_result(got, want, what)
    assert len(got["trace"]) == len(want["trace"]), what
    assert got["levels"] == want["levels"], "%s: levels %s against %s" % (what, got["levels"], want["levels"])
    assert got["stats8"][:5] == want["stats8"][:5] and got["stats8"][6:] == want["stats8"][6:], "%s: %s against %s" % (what, got["stats8"], want["stats8"])
    for k in ("gain", "offset", "ext"):
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s: %s differs: %s against %s" % (what, k, got[k], want[k])
    assert (got["held"], got["photometric"]) == (want["held"], want["photometric"]), what


def assert_same_sums(got, want, what):
    assert got[1] == want[1], "%s: counts %s against %s" % (what, got[1], want[1])
    bad = np.flatnonzero(bits(got[0]) != bits(want[0]))
    assert bad.size == 0, "%s: sums differ at %s: got %s want %s" % (what, bad.tolist(), got[0][bad[:3]], want[0][bad[:3]])


# ------------------------------------------------------------------ 1, 2: the system against the restatement; the invariant at (1, 0)
SHAPES = [(5, 7), (16, 32), (18, 32), (96, 128)]                      # 35, 512, 576 and 12 288 positions
EXPOSURES = [(1.0, 0.0), (0.7, 12.5), (1.6, -40.0)]


@pytest.mark.parametrize("height,width", SHAPES, ids=["%dx%d" % g for g in SHAPES])
def test_system_against_the_restatement(HX, HP, HC, height, width):
    """colour_pair under COLOUR_OPTS' option sets at three exposures, level 0 and level 1 where the camera has one: the 45 sums
    and the five counts bit for bit; and at (1, 0) sums[0..27] and the counts are drf_track_pyramid_system's host rule, bit for
    bit -- while the 17 others are not zero.  (5x7 is below the pyramid family's 8 pixels on a side: there the invariant is held
    against drf_track_colour_system's host rule, which the pyramid's level 0 is wherever it runs.)"""
    case = TC.colour_pair(7 + height, height, width)
    cam, d, bgr, mb, md = case["cam"], case["depth"], case["bgr"], case["model_bgr"], case["model"]
    ran = 0
    for L in (0, 1):
        if L > 0 and not TP.level_fits(cam, L):                         # level 0 is the camera itself: 5x7 has it, and no other
            continue
        for pname, pose in pair_poses(cam)[:3]:
            for oname, opt in TC.COLOUR_OPTS:
                opt = dict(opt, levels=L + 1)
                for G, B in EXPOSURES:
                    want = np_exposure_system(cam, L, bgr, d, mb, md, PM, pose, G, B, **opt)
                    got = cpp_system(HX, cam, L, bgr, d, mb, md, PM, pose, G, B, **opt)
                    assert_same_sums(got, want, "level %d, %s, %s at (%g, %g)" % (L, pname, oname, G, B))
                    ran += 1
                    if (G, B) == (1.0, 0.0):
                        if TP.level_fits(cam, L):
                            pyr = TP.cpp_system(HP, cam, L, bgr, d, mb, md, PM, pose, **opt)
                        else:
                            pyr = TC.cpp_system(HC, cam, bgr, d, mb, md, PM, pose, **{k: v for k, v in opt.items() if k != "levels"})
                        assert np.array_equal(bits(got[0][:28]), bits(pyr[0])) and got[1] == pyr[1], "the invariant: level %d, %s, %s" % (L, pname, oname)
                        if got[1][4] > 0:
                            assert got[0][28:].any() and got[0][40] > 0 and got[0][42] > 0
                        else:
                            assert not got[0][28:].any()
                print("%dx%d level %d %s, %s: counts %s" % (height, width, L, pname, oname, want[1]))
    assert ran == (36 if height == 5 else 72)


def test_step_against_the_restatement(HX):
    """exposure_step on systems of the 96x128 pair: a step that moves all eight unknowns, the clamp of the gain, a step that
    converges under loose thresholds, a held exposure (the two columns made dependent; no photometric sums at all) and a pose
    pivot that fails, each bit for bit with np_exposure_step."""
    case = TC.colour_pair(103, 96, 128)
    cam = case["cam"]
    pose = MT.pose_near()
    R, tv = motion(pose, cam["voxel_size"])
    o = MT.np_options(cam, centre_depth=1.5)
    c = np_centre(R, tv, cam, o)
    base, counts = np_exposure_system(cam, 0, case["bgr"], case["depth"], case["model_bgr"], case["model"], PM, pose, 0.8, 20.0, centre_depth=1.5)
    assert counts[4] > 1000
    dependent = base.copy()
    dependent[34:40], dependent[41], dependent[42], dependent[44] = 2.0 * base[28:34], 2.0 * base[40], 4.0 * base[40], 2.0 * base[43]
    none = base.copy()
    none[28:] = 0.0
    flat = base.copy()
    flat[0] = 0.0
    seen = set()
    for name, sums, x0, eps in (("moves", base, (0.8, 20.0, 0.25, 4.0), (1e-7, 1e-5, 1e-4, 1e-2)), ("clamped", base, (0.8, 20.0, 0.79, 0.81), (1e-7, 1e-5, 1e-4, 1e-2)),
                                ("converges", base, (0.8, 20.0, 0.25, 4.0), (10.0, 1e3, 10.0, 1e4)), ("the gain alone keeps it going", base, (0.8, 20.0, 0.25, 4.0), (10.0, 1e3, 1e-9, 1e4)),
                                ("dependent columns", dependent, (1.0, 0.0, 0.25, 4.0), (1e-7, 1e-5, 1e-4, 1e-2)), ("no photometric sums", none, (1.3, -5.0, 0.25, 4.0), (1e-7, 1e-5, 1e-4, 1e-2)),
                                ("a pose pivot fails", flat, (1.0, 0.0, 0.25, 4.0), (1e-7, 1e-5, 1e-4, 1e-2))):
        x = dict(gain=x0[0], offset=x0[1], gain_min=x0[2], gain_max=x0[3], eps_gain=eps[2], eps_offset=eps[3], held=0)
        ws, wR, wt = np_exposure_step(sums, c, R, tv, eps[0], eps[1], x)
        x6 = np.array([x0[0], x0[1], x0[2], x0[3], eps[2], eps[3]], f64)
        Rt, held = np.concatenate([R.reshape(9), tv]).astype(f64), C.c_uint64(0)
        gs = HX.mte_step(np.ascontiguousarray(sums).ctypes.data_as(f64p), np.ascontiguousarray(c).ctypes.data_as(f64p), eps[0], eps[1], x6.ctypes.data_as(f64p),
                         Rt.ctypes.data_as(f64p), C.byref(held))
        assert gs == ws and held.value == x["held"], name
        assert np.array_equal(bits(Rt[:9]), bits(wR.reshape(9))) and np.array_equal(bits(Rt[9:]), bits(wt)), name
        assert np.array_equal(bits(x6[:2]), bits(np.array([x["gain"], x["offset"]]))), name
        seen.add((name, ws, x["held"], x["gain"] != x0[0]))
        print("%s: status %d, held %d, exposure (%.6f, %.4f)" % (name, ws, x["held"], x["gain"], x["offset"]))
    assert ("moves", -1, 0, True) in seen and ("converges", CONVERGED, 0, False) in seen and ("the gain alone keeps it going", -1, 0, True) in seen
    assert ("dependent columns", -1, 1, False) in seen and ("no photometric sums", -1, 1, False) in seen and ("a pose pivot fails", DEGENERATE, 0, False) in seen
    assert [s for s in seen if s[0] == "clamped"][0][1] == -1


# ------------------------------------------------------------------ 3: a map of one colour holds the exposure
@pytest.fixture(scope="module")
def scene_map():
    s = track_scene()
    cache = {}

    def render_both(pose):
        key = np.ascontiguousarray(pose, f32).tobytes()
        if key not in cache:
            cache[key] = s["oracle"].render(pose)
        return cache[key]
    s["render_both"] = render_both
    return s


def test_one_colour_holds_the_exposure(HX, HP, scene_map):
    """The scene's geometry under one grey (93, 93, 93) in frame and model: the gain and offset columns are dependent, every
    evaluation holds, and the whole call from (1, 0) is track_pyramid_frame_host's -- pose, sums, every evaluation, the levels --
    bit for bit; held equals the evaluations; gain and offset stay (1, 0).  Both against the restatement."""
    s = scene_map
    grey = np.full((MT.H, MT.W, 3), 93, np.uint8)
    render = lambda pose: (grey, s["render_both"](pose)[1])  # noqa: E731
    start, opt = basin_start(s, 0), track_opts(s, max_renders=2, coarse_renders=2)
    pyr = TP.cpp_frame(HP, render, s["cam"], grey, s["depth"], start, levels=3, **opt)
    got = cpp_frame(HX, render, s["cam"], grey, s["depth"], start, levels=3, **opt)
    want = np_track_exposure_frame(render, s["cam"], grey, s["depth"], start, levels=3, **opt)
    assert_same_exposure(got, want, "one colour against the restatement")
    assert_same_result(got, pyr, "one colour against the pyramid call")
    assert got["levels"] == pyr["levels"] and got["stats8"][:5] == pyr["stats8"][:5] and got["stats8"][6:] == pyr["stats8"][6:]
    assert got["held"] == got["stats8"][3] > 3 and (got["gain"], got["offset"]) == (1.0, 0.0)
    assert got["photometric"] == pyr["counts"][4] > 1000, "the terms were there"
    print("one colour: status %d, levels %s, held %d of %d evaluations" % (got["status"], got["levels"], got["held"], got["stats8"][3]))


# ------------------------------------------------------------------ 4: what the call is for
def re_expose(bgr, g, o):
    """The frame as a camera with another exposure writes it: per channel clip(floor(g c + o / 3 + 0.5), 0, 255)."""
    return np.clip(np.floor(g * np.asarray(bgr, np.uint8).astype(f64) + o / 3.0 + 0.5), 0.0, 255.0).astype(np.uint8)


PLANE_EXPOSURES = [(0.7, 0.0), (0.6, 60.0), (0.5, 90.0), (1.3, -45.0)]     # the last saturates 2.3 % of the channel values
# The plane's thresholds for the exposure, what TRACK_EPS is for the pose: the default 1e-4 / 1e-2 stand to these as the default
# eps_rot / eps_trans stand to TRACK_EPS.  A channel is a whole number, so the frame's intensity carries up to 0.75 of rounding:
# eps_offset is a third of that, and eps_gain what that offset is at mid-grey (0.25 / 255).
EXPOSURE_EPS = dict(eps_gain=1e-3, eps_offset=0.25)
PLANE_OPTS = dict(TC.PLANE_OPTS, **EXPOSURE_EPS)
# measured on the restatement (test_the_plane_under_a_change_of_exposure): the bounds on |gain - g| and |offset - o|
GAIN_TOL, OFFSET_TOL = 1.5e-3, 2.5


@pytest.fixture(scope="module")
def plane():
    cam = camera(VS, **TC.PLANE_CAM)
    render = TC.textured_plane_renderer(cam)
    bgr, depth = render(np.eye(4, dtype=f32))
    return dict(cam=cam, render=render, bgr=bgr, depth=depth)


def test_the_plane_under_a_change_of_exposure(HX, plane):
    """The textured plane of tests/test_map_track_colour.py (48x64, PLANE_OPTS, PLANE_STARTS), the frame re-exposed per channel as
    c' = clip(floor(g c + o / 3 + 0.5), 0, 255).  MEASURED on the restatements, every start of PLANE_STARTS, in-plane error in
    voxels:
      (g, o)        drf_track_colour_frame's rule (today)          drf_track_exposure_frame's (3 levels, PLANE_OPTS with EXPOSURE_EPS)
      (1.0, 0)      0.001 to 0.010, CONVERGED                      0.0007 to 0.0065, CONVERGED, gain 0.99995 to 1.00055, offset -0.22 to 0.03
      (0.7, 0)      4.27 to 4.74, one CONVERGED 4.7 off            0.002 to 0.012, CONVERGED, gain 0.7004 to 0.7009, offset -0.13 to 0.09
      (0.6, +60)    2.54 to 3.03, all MAX_ITERS                    0.0007 to 0.0013, CONVERGED, gain 0.59996 to 0.60000, offset 60.01 to 60.03
      (0.5, +90)    3.23 to 3.61, all MAX_ITERS                    0.0009 to 0.0014, CONVERGED, gain 0.50001, offset 90.73 to 90.74
      (1.3, -45)    1.29 to 1.42, all MAX_ITERS                    0.005 to 0.015, CONVERGED, gain 1.2882 to 1.2891, offset -41.3 to -41.4
    The first column documents the defect: today's call ends outside the one-voxel criterion of test_one_textured_plane under
    every change of exposure.  For the three exposures that do not saturate, and at (1, 0), the recovered gain and offset are held
    to the truth within GAIN_TOL = 1.5e-3 and OFFSET_TOL = 2.5.  MEASURED: the largest errors are 8.6e-4 and 0.738.  The bounds
    are reasoned, not fitted: the call stops when a step is below eps_gain = 1e-3 / eps_offset = 0.25, so that much may remain, and
    the rounding of three channels to whole numbers moves the offset by up to 0.75 (which the 0.738 is) and the gain by that over
    the intensity's range of about 500, 1.5e-3: 1e-3 + a third of 1.5e-3 and 0.25 + 3 x 0.75.  With the default thresholds (1e-4,
    1e-2) the errors are 3e-5 and 0.743, and the saturating frame ends MAX_ITERS 0.003 voxels off: DESIGN.md has what was tried.
    The host run from the largest start is the restatement's bit for bit at every exposure."""
    p = plane
    cam, render = p["cam"], p["render"]
    worst_gain, worst_offset = 0.0, 0.0
    for g, o in [(1.0, 0.0)] + PLANE_EXPOSURES:
        frame = re_expose(p["bgr"], g, o)
        sat = float(((frame == 0) | (frame == 255)).mean())
        for k in range(len(TC.PLANE_STARTS)):
            start = TC.plane_start(k)
            old = TC.np_track_colour_frame(render, cam, frame, p["depth"], start, **TC.PLANE_OPTS)
            new = np_track_exposure_frame(render, cam, frame, p["depth"], start, **PLANE_OPTS)
            eo, en = TC.plane_errors(old["T"])[1], TC.plane_errors(new["T"])[1]
            print("(%g, %g) start %s: today status %d %.3f voxels; exposure status %d %.4f voxels, %d renders at level 0, gain %.5f offset %.3f, held %d (saturated %.3f)" %
                  (g, o, TC.PLANE_STARTS[k], old["status"], eo, new["status"], en, new["renders"], new["gain"], new["offset"], new["held"], sat))
            if (g, o) != (1.0, 0.0):
                assert eo > 1.0, "today's rule ends more than one voxel off under a change of exposure"
            assert new["status"] == CONVERGED and en < 1.0, "the call ends CONVERGED below one voxel in the plane"
            if (g, o) != (1.3, -45.0):
                worst_gain, worst_offset = max(worst_gain, abs(new["gain"] - g)), max(worst_offset, abs(new["offset"] - o))
                assert abs(new["gain"] - g) < GAIN_TOL and abs(new["offset"] - o) < OFFSET_TOL, (g, o, new["gain"], new["offset"])
        got = cpp_frame(HX, render, cam, frame, p["depth"], start, **PLANE_OPTS)
        assert_same_exposure(got, new, "the plane at (%g, %g) on the host" % (g, o))
    print("largest errors over the exposures that do not saturate: gain %.2e, offset %.3f" % (worst_gain, worst_offset))


# ------------------------------------------------------------------ 5: the clamp
def test_the_clamp_of_the_gain(HX, plane):
    """The (12 voxel, 6 degree) start under (0.7, 0), once with gain_min = 1e-3 -- next to no lower bound -- and once with the
    default 0.25.  What each ends on is printed and the default must end CONVERGED below one voxel; whether the loose bound fails
    on the restatement as it did in the issue's prototype is measured here and recorded in DESIGN.md.  Both runs are the host's
    bit for bit."""
    p = plane
    frame, start = re_expose(p["bgr"], 0.7, 0.0), TC.plane_start(3)
    runs = {}
    for name, extra in (("gain_min 1e-3", dict(gain_min=1e-3)), ("default", {})):
        opt = dict(PLANE_OPTS, **extra)
        r = np_track_exposure_frame(p["render"], p["cam"], frame, p["depth"], start, **opt)
        runs[name] = r
        print("%s: status %d, %.4f voxels in the plane, gain %.5f offset %.3f, levels %s" % (name, r["status"], TC.plane_errors(r["T"])[1], r["gain"], r["offset"], r["levels"]))
        assert_same_exposure(cpp_frame(HX, p["render"], p["cam"], frame, p["depth"], start, **opt), r, name)
    d = runs["default"]
    assert d["status"] == CONVERGED and TC.plane_errors(d["T"])[1] < 1.0 and 0.25 <= d["gain"] <= 4.0


# ------------------------------------------------------------------ 6: options, defaults, refusals
def test_options_and_their_defaults(HX):
    out, name = np.zeros(6, f64), C.create_string_buffer(32)
    vs = f32(0.02)
    assert HX.mte_options(None, vs, 128, 96, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [1.0, 0.0, 0.25, 4.0, 1e-4, 1e-2]
    assert HX.mte_options(C.byref(exposure_options(gain_init=0.5, offset_init=-30.0, gain_min=0.5, gain_max=2.0, eps_gain=1e-3, eps_offset=0.5)), vs, 128, 96,
                          out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [0.5, -30.0, 0.5, 2.0, 1e-3, 0.5]
    nan, inf = float("nan"), float("inf")
    for bad, which in ((dict(levels=-1, gain_init=-1.0), "levels"), (dict(step=-1, gain_min=5.0), "step"), (dict(coarse_renders=-1, eps_gain=-1.0), "coarse_renders"),
                       (dict(gain_init=-1.0, offset_init=nan), "gain_init"), (dict(gain_init=nan), "gain_init"), (dict(offset_init=inf, gain_min=-1.0), "offset_init"),
                       (dict(gain_min=-0.5, gain_max=-1.0), "gain_min"), (dict(gain_max=inf, eps_gain=-1.0), "gain_max"), (dict(eps_gain=-1e-3, eps_offset=-1.0), "eps_gain"),
                       (dict(eps_offset=nan, gain_min=5.0), "eps_offset"), (dict(gain_min=5.0, gain_init=9.0), "gain_min"), (dict(gain_min=2.0, gain_max=1.0, gain_init=1.5), "gain_min"),
                       (dict(gain_init=0.2, offset_init=900.0), "gain_init"), (dict(gain_init=4.5), "gain_init"), (dict(offset_init=766.0), "offset_init"),
                       (dict(offset_init=-765.5), "offset_init")):
        assert HX.mte_options(C.byref(exposure_options(**bad)), vs, 128, 96, out.ctypes.data_as(f64p), name) == 1, bad
        assert name.value.decode() == which, (bad, name.value)
    assert HX.mte_options(C.byref(exposure_options(offset_init=-765.0, gain_init=0.25)), vs, 128, 96, out.ctypes.data_as(f64p), name) == 0
    assert HX.mte_options(C.byref(exposure_options(levels=4)), vs, 63, 96, out.ctypes.data_as(f64p), name) == 1 and name.value.decode() == "levels"
    assert C.sizeof(ExposureOptions) == 104 and ExposureOptions.gain_init.offset == 72 and ExposureOptions.eps_gain.offset == 88
    assert C.sizeof(ExposureResult) == C.sizeof(Result) + 8 * 21


def test_refusals_and_an_image_without_a_sample(HX, plane):
    case = TC.colour_pair(5, 24, 32)
    cam = case["cam"]
    nan = np.eye(4, dtype=f32)
    nan[2, 3] = np.nan
    cm, b, d, mb, md, pm = Camera(**cam), _u8(case["bgr"]), _f32(case["depth"]), _u8(case["model_bgr"]), _f32(case["model"]), _f32(PM).reshape(16)
    sums, counts = np.zeros(45, f64), np.zeros(5, np.uint64)
    args = (b.ctypes.data_as(u8p), d.ctypes.data_as(f32p), mb.ctypes.data_as(u8p), md.ctypes.data_as(f32p))
    tail = (sums.ctypes.data_as(f64p), counts.ctypes.data_as(u64p))
    bb = _f32(nan).reshape(16)
    two = exposure_options(levels=2)
    for mp, p in ((pm, bb), (bb, pm)):
        assert HX.mte_system(C.byref(cm), 1, *args, mp.ctypes.data_as(f32p), p.ctypes.data_as(f32p), 1.0, 0.0, C.byref(two), *tail) == 2
    for L in (-1, 2, 5):                                                # 24 >> 2 = 6 pixels
        assert HX.mte_system(C.byref(cm), L, *args, pm.ctypes.data_as(f32p), pm.ctypes.data_as(f32p), 1.0, 0.0, C.byref(exposure_options(levels=1)), *tail) == 1
    # the colour image stands behind the options and before the pose
    assert HX.mte_system(C.byref(cm), 1, None, args[1], args[2], args[3], pm.ctypes.data_as(f32p), bb.ctypes.data_as(f32p), 1.0, 0.0, C.byref(two), *tail) == 3
    assert HX.mte_system(C.byref(cm), 1, None, args[1], args[2], args[3], pm.ctypes.data_as(f32p), pm.ctypes.data_as(f32p), 1.0, 0.0,
                         C.byref(exposure_options(levels=2, gain_init=9.0)), *tail) == 1
    zero = np.zeros((24, 32), f32)
    for name, depth, model in (("no samples", zero, case["model"]), ("no hit", case["depth"], zero)):
        want = np_exposure_system(cam, 1, case["bgr"], depth, case["model_bgr"], model, PM, MT.pose_near(), 0.7, 12.5, levels=2)
        got = cpp_system(HX, cam, 1, case["bgr"], depth, case["model_bgr"], model, PM, MT.pose_near(), 0.7, 12.5, levels=2)
        assert_same_sums(got, want, name)
        assert not got[0].any() and got[1][1] == 0 and got[1][4] == 0
    assert got[1][0] > 50 and got[1][2] == got[1][0]
    # a frame without a sample is LOST at the first evaluation of every level, as for the colour call, and keeps pose and exposure
    p = plane
    empty = np.zeros_like(p["depth"])
    start = TC.plane_start(0)
    want = np_track_exposure_frame(p["render"], p["cam"], p["bgr"], empty, start, gain_init=0.8, offset_init=10.0, **PLANE_OPTS)
    got = cpp_frame(HX, p["render"], p["cam"], p["bgr"], empty, start, gain_init=0.8, offset_init=10.0, **PLANE_OPTS)
    assert_same_exposure(got, want, "a frame without a sample")
    assert got["status"] == LOST and got["stats8"][6:] == (3, 2) and got["iterations"] == 1 and got["held"] == 0
    assert np.array_equal(got["T"].astype(f32), start) and got["gain"] == float(f32(0.8)) and got["offset"] == 10.0


# ------------------------------------------------------------------ 7, 8: sanitizers, the C ABI and the shim
def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """track_exposure_system_at_host, exposure_step and track_exposure_frame_host under AddressSanitizer and UBSan: a plain
    executable, nothing preloaded, nothing loaded into Python.  It reads one synthetic pair from a file and prints the level-1
    sums at (0.7, 12.5), which are the restatement's bit for bit; then the plane case under a change of exposure and refusals."""
    exe, data = str(tmp_path / "map_track_exposure_san"), str(tmp_path / "case.bin")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_track_exposure_san.cpp"), "-o", exe])
    case = TC.colour_pair(31, 48, 70)
    opt = dict(step=2, centre_depth=1.5)
    pose = MT.pose_near()
    with open(data, "wb") as fh:
        fh.write(bytes(Camera(**case["cam"])) + bytes(exposure_options(2, 0, 0.05, **opt)) + _u8(case["bgr"]).tobytes() + _f32(case["depth"]).tobytes() +
                 _u8(case["model_bgr"]).tobytes() + _f32(case["model"]).tobytes() + _f32(PM).tobytes() + _f32(pose).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_track_exposure_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    line = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("system")][0]
    want = np_exposure_system(case["cam"], 1, case["bgr"], case["depth"], case["model_bgr"], case["model"], PM, pose, 0.7, 12.5, levels=2, photo_weight=0.05, **opt)
    assert np.array_equal(np.array([int(x, 16) for x in line[:45]], np.uint64), bits(want[0])) and tuple(int(x) for x in line[45:]) == want[1]
    assert want[1][1] > 10 and want[1][4] > 5


def test_abi_declares_exports_and_types_the_six_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_track_exposure_system", "drf_track_exposure_system_device", "drf_track_exposure_frame", "drf_track_exposure_frame_device",
                            "drf_track_exposure_stats", "drf_track_exposure_level_stats"])
    assert "drf_track_exposure_options_t" in src and "drf_exposure_result_t" in src
    assert C.sizeof(L.TrackExposureOptions) == C.sizeof(ExposureOptions) == 104
    assert L.TrackExposureOptions.gain_init.offset == 72 and L.TrackExposureOptions.eps_offset.offset == 96 and L.TrackExposureOptions.pyramid.offset == 0
    assert C.sizeof(L.ExposureResultStruct) == C.sizeof(ExposureResult) and L.ExposureResultStruct.gain.offset == C.sizeof(Result)
    lib = L.lib()
    T = (C.c_float * 16)(*np.eye(4, dtype=f32).reshape(16))
    depth, bgr = (C.c_float * 4)(), (C.c_uint8 * 12)()
    sums, counts, out = (C.c_double * 45)(), (C.c_uint64 * 5)(), (C.c_uint64 * 8)()
    assert lib.drf_track_exposure_system(None, 1, bgr, depth, bgr, depth, T, T, 1.0, 0.0, None, sums, counts) == 1
    assert lib.drf_track_exposure_system_device(None, 1, None, None, None, None, T, T, 1.0, 0.0, None, sums, counts) == 1
    assert lib.drf_track_exposure_frame(None, bgr, depth, T, None, T, None) == 1
    assert lib.drf_track_exposure_frame_device(None, None, None, T, None, T, None) == 1
    assert lib.drf_track_exposure_stats(None, out) == 1
    assert lib.drf_track_exposure_level_stats(None, 0, out) == 1
    import tandem_amd.dr_fusion as F
    for name in ("track_exposure_system", "track_exposure_frame", "track_exposure_stats", "track_exposure_level_stats"):
        assert callable(getattr(F.DrFusion, name))
    hdr = open(os.path.join(ROOT, "include", "dr_mi355x.h")).read()
    assert "DESIGN.md §7c \"Tracking under a change of exposure\"" in hdr
    for out_of_scope in ("exposure in drf_score_colour_poses and in drf_locate_*", "the tracking stage of drf_search_colour_frame", "per-channel gains, response curves and vignetting",
                         "compensation on the device"):
        assert out_of_scope in " ".join(hdr.replace(" * ", " ").split()), out_of_scope


def test_compensate_exposure_inverts_the_model():
    """compensate_exposure is numpy alone: it brings a re-exposed frame back to within one level per channel where nothing
    saturated, and the rounding rule is the stated one."""
    from tandem_amd.dr_fusion import compensate_exposure
    rng = np.random.default_rng(4)
    bgr = rng.integers(0, 256, (12, 16, 3)).astype(np.uint8)
    for g, o in ((0.7, 0.0), (0.6, 60.0), (0.5, 90.0)):
        back = compensate_exposure(re_expose(bgr, g, o), g, o)
        assert back.dtype == np.uint8 and back.shape == bgr.shape
        assert np.abs(back.astype(int) - bgr.astype(int)).max() <= math.ceil(0.5 / g)
    assert compensate_exposure(np.array([[[10, 100, 250]]], np.uint8), 0.5, 30.0).tolist() == [[[0, 180, 255]]]
    assert np.array_equal(compensate_exposure(bgr, 1.0, 0.0), bgr)


def test_shim_compiles(tmp_path):
    """tandem_amd/libdr/dr_fusion.h TrackExposureFrame and TrackExposureSystem as a TANDEM translation unit would call them
    (tests/cpp/map_track_exposure_shim.cpp): it compiles and links against the library; tests/test_fusion_track_exposure_gpu.py
    runs it."""
    abi_module()
    exe = str(tmp_path / "map_track_exposure_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_track_exposure_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert os.path.isfile(exe)
