"""CPU: the host half of drf_track_reduce / drf_track_pyramid_system / drf_track_pyramid_frame (include/dr_mi355x.h "Tracks a frame
coarse to fine", DESIGN.md §7c "Tracking coarse to fine").  track_level_grid, track_reduce_host, track_pyramid_system_host and
track_pyramid_frame_host of tandem_amd/csrc/pose_host.h compiled with plain g++ (tests/cpp/map_track_pyramid_check.cpp) and held,
bit for bit, to np_level_cam / np_reduce / np_pyramid_system / np_track_pyramid_frame, numpy restatements written here from the
header's statement -- the reference of tests/test_fusion_track_pyramid_gpu.py too; what the pyramid is for, measured on the
restatement; options and refusals; the same under AddressSanitizer and UBSan as a stand-alone program
(tests/cpp/map_track_pyramid_san.cpp); the names of the C ABI.  The single-level restatements, the synthetic pairs, the textured
plane and the scene come from tests/test_map_track.py and tests/test_map_track_colour.py by import."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_map_track as MT
import test_map_track_colour as TC
from fusion_helpers import abi_module, check_symbols
from test_map_align import CONVERGED, DEGENERATE, LOST, MAX_ITERS, Result, assert_same_result, assert_same_system, bits
from test_map_locate import Camera, camera, np_locate_frame, scene_errors
from test_map_track import PM, TRACK_EPS, basin_start, pair_poses, track_opts, track_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p, u64p, f32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_double)
VS = MT.VS
f32, f64 = np.float32, np.float64
_f32, _u8 = TC._f32, TC._u8


# ------------------------------------------------------------------ the rule, restated
def np_level_cam(cam, L):
    """Level L's camera as a dict like cam: W / s, H / s by integer division; fx / s, (cx + 0.5f) / s - 0.5f in float32; level 0 is
    the camera itself."""
    if L == 0:
        return dict(cam)
    s, sf = 1 << L, f32(1 << L)
    c = dict(cam)
    c["width"], c["height"] = int(cam["width"]) // s, int(cam["height"]) // s
    c["fx"], c["fy"] = float(f32(cam["fx"]) / sf), float(f32(cam["fy"]) / sf)
    c["cx"] = float((f32(cam["cx"]) + f32(0.5)) / sf - f32(0.5))
    c["cy"] = float((f32(cam["cy"]) + f32(0.5)) / sf - f32(0.5))
    return c


def level_fits(cam, L):
    return 0 <= L < 5 and (int(cam["width"]) >> L) >= 8 and (int(cam["height"]) >> L) >= 8


def np_reduce(bgr, depth, L, max_jump):
    """The reduction of a full-resolution pair to level L: (bgr (H_L, W_L, 3) uint8 or None, depth (H_L, W_L) float32).  Every
    floating operation is a float32 array operation, one per operation of the rule; the row sums are the butterfly's."""
    depth = np.ascontiguousarray(depth, f32)
    Hd, Wd = depth.shape
    s = 1 << L
    HL, WL = Hd // s, Wd // s
    d = depth[:HL * s, :WL * s].reshape(HL, s, WL, s).transpose(0, 2, 1, 3)          # (v, u, row, column)
    with np.errstate(all="ignore"):
        valid = d > f32(0)
        some = valid.any(axis=(2, 3))
        z0 = np.where(valid, d, f32(np.inf)).min(axis=(2, 3)).astype(f32)
        accepted = valid & ((d - z0[..., None, None]) <= f32(max_jump))
        n = accepted.sum(axis=(2, 3)).astype(np.int64)
        t = np.where(accepted, d, f32(0)).astype(f32)
        off = s >> 1
        while off:
            t = t + t[..., np.arange(s) ^ off]
            off >>= 1
        rows = t[..., 0]
        S = rows[..., 0]
        for r in range(1, s):
            S = S + rows[..., r]
        assert S.dtype == f32 and (d - z0[..., None, None]).dtype == f32
        keep = some & (2 * n >= s * s)
        dout = np.where(keep, S / np.where(n > 0, n, 1).astype(f32), f32(0)).astype(f32)
    if bgr is None:
        return None, dout
    c = np.ascontiguousarray(bgr, np.uint8).reshape(Hd, Wd, 3)[:HL * s, :WL * s].reshape(HL, s, WL, s, 3).transpose(0, 2, 1, 3, 4).astype(np.int64)
    csum = np.where(accepted[..., None], c, 0).sum(axis=(2, 3))
    nn = np.where(n > 0, n, 1)[..., None]
    cout = np.where(keep[..., None], (2 * csum + nn) // (2 * nn), 0).astype(np.uint8)
    return cout, dout


def np_pyramid_options(cam, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
    """(drf_track_options_t's dict, photo_weight float32, levels, coarse_renders) with the defaults resolved"""
    o, lam = TC.np_colour_options(cam, photo_weight, **opt)
    return o, lam, int(levels) or 3, int(coarse_renders) or 3


def np_level_options(o, coarse, L):
    oL = dict(o, max_jump=f32(1 << L) * f32(o["max_jump"]))
    if L > 0:
        oL["max_renders"] = coarse
    assert oL["max_jump"].dtype == f32
    return oL


def np_pyramid_system(cam, L, bgr, depth, model_bgr, model_depth, model_pose, pose, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
    """drf_track_pyramid_system: both pairs reduced to level L, then the single-level restatement on the level's camera.  bgr
    None: the geometric system, counts[4] = 0."""
    o, lam, levels, coarse = np_pyramid_options(cam, levels, coarse_renders, photo_weight, **opt)
    oL, camL = np_level_options(o, coarse, L), np_level_cam(cam, L)
    Hd, Wd = int(cam["height"]), int(cam["width"])
    colour = bgr is not None
    fc, fd = np_reduce(np.asarray(bgr).reshape(Hd, Wd, 3) if colour else None, np.asarray(depth, f32).reshape(Hd, Wd), L, oL["max_jump"])
    mc, md = np_reduce(np.asarray(model_bgr).reshape(Hd, Wd, 3) if colour else None, np.asarray(model_depth, f32).reshape(Hd, Wd), L, oL["max_jump"])
    R, tv = TC.motion(pose, cam["voxel_size"])
    if colour:
        model, Ym = TC.np_colour_model(camL, mc, md, oL["max_jump"])
        return TC.np_colour_eval(camL, fc, fd, model, Ym, model_pose, R, tv, oL, lam)
    sums, c4 = MT.np_system(camL, fd, MT.np_track_model(camL, md, oL["max_jump"]), model_pose, R, tv, oL)[:2]
    return sums, tuple(c4) + (0,)


def np_track_pyramid_frame(render, cam, bgr, depth, pose_init, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
    """drf_track_pyramid_frame over render(pose (4, 4) float32) -> (bgr (H, W, 3) uint8, depth (H, W) float32) at full resolution.
    bgr None: geometry only.  Level 0's dict (np_loop's), plus levels = {L: (status, renders, evaluations, valid)}, stats8 and
    the trace of every evaluation in the order they ran."""
    o, lam, levels, coarse = np_pyramid_options(cam, levels, coarse_renders, photo_weight, **opt)
    Hd, Wd = int(cam["height"]), int(cam["width"])
    colour = bgr is not None
    depth = np.asarray(depth, f32).reshape(Hd, Wd)
    bgr = np.asarray(bgr).reshape(Hd, Wd, 3) if colour else None
    p16 = np.ascontiguousarray(pose_init, f32).reshape(4, 4).copy()
    stats, per_level, trace = [0] * 8, {}, []
    for L in range(levels - 1, -1, -1):
        camL, oL = np_level_cam(cam, L), np_level_options(o, coarse, L)
        fc, fd = (bgr, depth) if L == 0 else np_reduce(bgr, depth, L, oL["max_jump"])

        def render_level(p, L=L, oL=oL, camL=camL):
            Cm, Dm = render(p)
            if L > 0:
                Cm, Dm = np_reduce(np.asarray(Cm).reshape(Hd, Wd, 3) if colour else None, np.asarray(Dm, f32).reshape(Hd, Wd), L, oL["max_jump"])
            return (Cm if colour else np.zeros((camL["height"], camL["width"], 3), np.uint8)), Dm
        r = TC.np_track_colour_frame(render_level, camL, fc if colour else np.zeros((camL["height"], camL["width"], 3), np.uint8), fd, p16,
                                     photo_weight=float(lam), colour=colour, **oL)
        per_level[L] = (r["status"], r["renders"], r["iterations"], r["valid"])
        trace += r["trace"]
        Wg, Hg = -(-camL["width"] // oL["step"]), -(-camL["height"] // oL["step"])
        stats[0] += Wg * Hg; stats[1] += r["samples"]; stats[2] += r["valid"]; stats[3] += r["iterations"]; stats[4] += r["renders"]; stats[6] += 1
        if L == 0:
            out = dict(r, trace=trace, levels=per_level, stats8=tuple(stats))
            return out
        if r["status"] in (LOST, DEGENERATE):
            stats[7] += 1
            continue
        p16 = r["T"].astype(f32)


# ------------------------------------------------------------------ the compiled host half
class PyramidOptions(C.Structure):
    """drf_track_pyramid_options_t"""
    _fields_ = [("colour", TC.ColourOptions), ("levels", C.c_int), ("coarse_renders", C.c_int)]


def pyramid_options(levels=0, coarse_renders=0, photo_weight=0.0, **opt):
    return PyramidOptions(TC.colour_options(photo_weight, **opt), levels, coarse_renders)


RENDER_FN = TC.RENDER_FN


def build_check(directory):
    so = os.path.join(str(directory), "libmap_track_pyramid_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_track_pyramid_check.cpp"), "-o", so])
    h = C.CDLL(so)
    cam, po = C.POINTER(Camera), C.POINTER(PyramidOptions)
    h.mtp_options.argtypes = [po, C.c_float, C.c_int, C.c_int, f64p, C.c_char_p]
    h.mtp_level.argtypes = [cam, po, C.c_int, C.POINTER(C.c_int), f32p, f32p, C.POINTER(C.c_int)]
    h.mtp_reduce.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, u8p, f32p, u8p, f32p]
    h.mtp_system.argtypes = [cam, C.c_int, u8p, f32p, u8p, f32p, f32p, f32p, po, f64p, u64p]
    h.mtp_frame.argtypes = [cam, u8p, f32p, RENDER_FN, C.c_void_p, f32p, po, C.POINTER(Result), f64p, C.c_size_t, u64p]
    return h


@pytest.fixture(scope="module")
def HP(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("map_track_pyramid"))


def cpp_reduce(HP, bgr, depth, L, max_jump):
    depth = _f32(depth)
    Hd, Wd = depth.shape
    HL, WL = Hd >> L, Wd >> L
    dout = np.full((HL, WL), -7.0, f32)
    cout = np.full((HL, WL, 3), 77, np.uint8) if bgr is not None else None
    b = _u8(bgr) if bgr is not None else None
    assert HP.mtp_reduce(Wd, Hd, L, f32(max_jump), b.ctypes.data_as(u8p) if b is not None else None, depth.ctypes.data_as(f32p),
                         cout.ctypes.data_as(u8p) if cout is not None else None, dout.ctypes.data_as(f32p)) == 0
    return cout, dout


def cpp_system(HP, cam, L, bgr, depth, model_bgr, model_depth, model_pose, pose, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
    depth, model_depth = _f32(depth), _f32(model_depth)
    b, mb = (_u8(bgr), _u8(model_bgr)) if bgr is not None else (None, None)
    model_pose, pose = _f32(model_pose).reshape(16), _f32(pose).reshape(16)
    sums, counts = np.zeros(28, f64), np.zeros(5, np.uint64)
    rc = HP.mtp_system(C.byref(Camera(**cam)), L, b.ctypes.data_as(u8p) if b is not None else None, depth.ctypes.data_as(f32p),
                       mb.ctypes.data_as(u8p) if mb is not None else None, model_depth.ctypes.data_as(f32p), model_pose.ctypes.data_as(f32p), pose.ctypes.data_as(f32p),
                       C.byref(pyramid_options(levels, coarse_renders, photo_weight, **opt)), sums.ctypes.data_as(f64p), counts.ctypes.data_as(u64p))
    assert rc == 0, rc
    return sums, tuple(int(v) for v in counts)


def cpp_frame(HP, render, cam, bgr, depth, pose, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
    """track_pyramid_frame_host over the Python renderer as a dict shaped like np_track_pyramid_frame's."""
    depth, pose = _f32(depth), _f32(pose).reshape(16)
    b = _u8(bgr) if bgr is not None else None
    npix = cam["height"] * cam["width"]

    def call(p16, cout, dout, user):
        c, d = render(np.ctypeslib.as_array(p16, (16,)).reshape(4, 4).copy())
        c, d = _u8(c), _f32(d)
        C.memmove(cout, c.ctypes.data, npix * 3)
        C.memmove(dout, d.ctypes.data, npix * 4)

    r = Result()
    nl, nc = int(levels) or 3, int(coarse_renders) or 3
    cap = (int(opt.get("max_renders", 0) or 10) + (nl - 1) * nc) * int(opt.get("inner_iters", 0) or 4)
    trace, stats = np.zeros((cap, 28), f64), np.zeros(33, np.uint64)
    assert HP.mtp_frame(C.byref(Camera(**cam)), b.ctypes.data_as(u8p) if b is not None else None, depth.ctypes.data_as(f32p), RENDER_FN(call), None,
                        pose.ctypes.data_as(f32p), C.byref(pyramid_options(levels, coarse_renders, photo_weight, **opt)), C.byref(r), trace.ctypes.data_as(f64p), cap,
                        stats.ctypes.data_as(u64p)) == 0
    st = [int(v) for v in stats]
    return dict(T=np.array(r.T, f64).reshape(4, 4), sums=np.array(r.sums, f64), samples=int(r.samples), valid0=int(r.valid0), valid=int(r.valid),
                cost0=float(r.cost0), cost=float(r.cost), iterations=int(r.iterations), status=int(r.status), trace=[trace[i] for i in range(st[3])],
                counts=tuple(st[28:33 if bgr is not None else 32]), renders=st[8 + 1], stats8=tuple(st[:8]),
                levels={L: tuple(st[8 + 4 * L:12 + 4 * L]) for L in range(5) if st[8 + 4 * L + 2]})


def assert_same_pyramid(got, want, what):
    assert_same_result(got, want, what)
    assert len(got["trace"]) == len(want["trace"]), what
    assert got["levels"] == want["levels"], "%s: levels %s against %s" % (what, got["levels"], want["levels"])
    assert got["stats8"][:5] == want["stats8"][:5] and got["stats8"][6:] == want["stats8"][6:], "%s: %s against %s" % (what, got["stats8"], want["stats8"])
    assert got["counts"] == tuple(want["counts"])[:len(got["counts"])], what


# ------------------------------------------------------------------ the reduction
REDUCE_SHAPES = [(16, 32), (18, 35), (96, 128)]                      # 18x35: remainders on both axes at every level


def reduce_pair(seed, height, width):
    """A depth image with a slope, steps and every kind of invalid pixel, and a random colour image."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(height, dtype=f64), np.arange(width, dtype=f64), indexing="ij")
    depth = (1.2 + 0.004 * u + 0.003 * v + 0.4 * (u > 0.6 * width) + rng.uniform(0, 0.002, (height, width))).astype(f32)
    pick = rng.integers(0, 12, (height, width))
    depth[pick == 0] = 0.0
    depth[pick == 1] = np.nan
    depth[pick == 2] = -1.0
    depth[pick == 3] = np.inf
    depth[: height // 4, : width // 4] = 0.0                          # whole blocks without a valid pixel
    return rng.integers(0, 256, (height, width, 3)).astype(np.uint8), depth


@pytest.mark.parametrize("height,width", REDUCE_SHAPES, ids=["%dx%d" % g for g in REDUCE_SHAPES])
def test_reduction_against_the_restatement(HP, height, width):
    bgr, depth = reduce_pair(height, height, width)
    for L in (1, 2, 3):
        for mj in (0.1 * (1 << L), 0.003):
            wc, wd = np_reduce(bgr, depth, L, mj)
            gc, gd = cpp_reduce(HP, bgr, depth, L, mj)
            assert gd.shape == (height >> L, width >> L)
            assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (L, mj)
            assert np.array_equal(gc, wc), (L, mj)
            _, alone = cpp_reduce(HP, None, depth, L, mj)
            assert np.array_equal(alone.view(np.uint32), wd.view(np.uint32)), "the depth alone"
            assert (wd[: height // 4 >> L, : width // 4 >> L] == 0).all() and (wc[wd == 0] == 0).all()
            assert np.isfinite(wd).all() and ((wd > 0).any() or mj < 0.01)   # (the image's slope leaves a 3 mm jump no block beyond level 1)
    print("%dx%d: kept %s of the level-1 pixels at max_jump 0.003" % (height, width, float((np_reduce(bgr, depth, 1, 0.003)[1] > 0).mean())))


def test_reduction_at_level_0(HP):
    """s = 1: a valid finite pixel is itself, every other one (0, negative, NaN, +inf) is 0 with colour 0."""
    bgr, depth = reduce_pair(3, 8, 8)
    wc, wd = np_reduce(bgr, depth, 0, 0.1)
    gc, gd = cpp_reduce(HP, bgr, depth, 0, 0.1)
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)) and np.array_equal(gc, wc)
    ok = np.isfinite(depth) & (depth > 0)
    assert np.array_equal(wd[ok], depth[ok]) and (wd[~ok] == 0).all() and np.array_equal(wc[ok], bgr[ok]) and (wc[~ok] == 0).all()
    assert (~ok).sum() > 8 and ok.sum() > 8


def _block(L, values, colours=None):
    """One level pixel's block, row-major values (s * s), inside an 8 x 8 image of far-away valid depth elsewhere."""
    s = 1 << L
    depth = np.full((8, 8), 9.0, f32)
    depth[:s, :s] = np.asarray(values, f32).reshape(s, s)
    bgr = np.full((8, 8, 3), 10, np.uint8)
    if colours is not None:
        bgr[:s, :s] = np.asarray(colours, np.uint8).reshape(s, s, 3)
    return bgr, depth


REDUCE_CASES = {
    # name: (L, max_jump, depths, colours or None, expected depth or None (only the restatement), expected colour or None)
    "all invalid": (1, 0.1, [0, np.nan, -1, 0], None, 0.0, (0, 0, 0)),
    "only +inf": (1, 0.1, [np.inf, np.inf, 0, 0], None, 0.0, (0, 0, 0)),
    "exactly half accepted is kept": (1, 0.1, [1.0, 0, 1.05, np.nan], [(10, 20, 30), (200, 200, 200), (20, 30, 40), (200, 200, 200)], 1.025, (15, 25, 35)),
    "one fewer than half is dropped": (2, 0.1, [1.0] * 7 + [0] * 9, None, 0.0, (0, 0, 0)),
    "half of sixteen is kept": (2, 0.1, [1.0] * 8 + [0] * 8, None, 1.0, (10, 10, 10)),
    "a depth step: the far pixels are excluded": (1, 0.1, [1.0, 1.5, 1.0, 1.5], [(10, 10, 10), (250, 250, 250), (30, 30, 30), (250, 250, 250)], 1.0, (20, 20, 20)),
    "inf next to valid": (1, 0.1, [1.0, np.inf, 1.0, 1.0], None, 1.0, (10, 10, 10)),
    "n = 3 is no power of two": (1, 0.1, [1.0, 1.01, 1.02, 0], [(1, 2, 3), (2, 3, 5), (3, 4, 5), (99, 99, 99)], None, (2, 3, 4)),
    "n = 11 of 16": (2, 0.5, [1.0 + 0.01 * k for k in range(11)] + [0, np.nan, -2, 3.0, np.inf], None, None, (10, 10, 10)),
    "a colour sum exactly on a half rounds up": (1, 0.1, [1.0, 1.0, 0, 0], [(10, 0, 254), (11, 1, 255), (0, 0, 0), (0, 0, 0)], 1.0, (11, 1, 255)),
    "three quarters: 2 c + n over 2 n": (1, 0.1, [1.0, 1.0, 1.0, 1.0], [(1, 0, 0), (1, 0, 0), (1, 0, 0), (0, 3, 0)], 1.0, (1, 1, 0)),
}


@pytest.mark.parametrize("name", list(REDUCE_CASES))
def test_reduction_named_cases(HP, name):
    L, mj, values, colours, want_depth, want_colour = REDUCE_CASES[name]
    bgr, depth = _block(L, values, colours)
    wc, wd = np_reduce(bgr, depth, L, mj)
    gc, gd = cpp_reduce(HP, bgr, depth, L, mj)
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)) and np.array_equal(gc, wc), name
    if want_depth is not None:
        assert wd[0, 0] == f32(want_depth), (name, wd[0, 0])
    if want_colour is not None:
        assert tuple(int(x) for x in wc[0, 0]) == want_colour, (name, wc[0, 0])
    assert wd[0, 1] == f32(9.0) and tuple(wc[0, 1]) == (10, 10, 10), "the neighbour block is untouched by this one"


def test_row_sums_are_the_butterfly(HP):
    """Sixteen depths whose sum depends on the order: the rule's order -- (t0 + t2) + (t1 + t3) per row, the rows ascending -- against
    a plain left-to-right sum, which differs in the last place for this block."""
    rng = np.random.default_rng(5)
    for trial in range(200):
        vals = (1.0 + rng.uniform(0, 0.09, 16)).astype(f32)
        bgr, depth = _block(2, vals)
        _, wd = np_reduce(bgr, depth, 2, 0.1)
        plain = f32(0)
        for x in vals:
            plain = f32(plain + x)
        if f32(plain / f32(16)) != wd[0, 0]:
            _, gd = cpp_reduce(HP, bgr, depth, 2, 0.1)
            assert gd[0, 0].view(np.uint32) == wd[0, 0].view(np.uint32)
            return
    raise AssertionError("no block told the two orders apart")


# ------------------------------------------------------------------ the level's camera
def test_level_intrinsics_as_bit_patterns(HP):
    for cam in (camera(VS, 96, 128), camera(VS, 18, 35, fx=31.7, fy=29.3, cx=17.1, cy=8.3), camera(VS, 480, 640, fx=525.0, fy=525.0, cx=319.5, cy=239.5)):
        levels = max(L for L in range(5) if level_fits(cam, L)) + 1
        for step in (1, 3):
            for L in range(5):
                ints, floats, mj, mr = (C.c_int * 5)(), np.zeros(6, f32), C.c_float(0), C.c_int(0)
                rc = HP.mtp_level(C.byref(Camera(**cam)), C.byref(pyramid_options(levels, 2, step=step, max_jump=0.07)), L, ints, floats.ctypes.data_as(f32p),
                                  C.byref(mj), C.byref(mr))
                assert rc == (0 if level_fits(cam, L) else 1), (cam["width"], cam["height"], L)
                if rc:
                    continue
                c = np_level_cam(cam, L)
                assert list(ints) == [c["width"], c["height"], step, -(-c["width"] // step), -(-c["height"] // step)]
                want = np.array([c["fx"], c["fy"], c["cx"], c["cy"], cam["min_sensor_depth"], cam["max_sensor_depth"]], f32)
                assert np.array_equal(floats.view(np.uint32), want.view(np.uint32)), (L, floats, want)
                assert f32(mj.value).view(np.uint32) == (f32(1 << L) * f32(0.07)).view(np.uint32)
                assert mr.value == (10 if L == 0 else 2)
    c = np_level_cam(camera(VS, 96, 128), 2)
    assert (c["width"], c["height"], c["fx"], c["cx"], c["cy"]) == (32, 24, 27.5, 15.5, 11.5)


# ------------------------------------------------------------------ one evaluation at a level
SYSTEM_SHAPES = [(16, 32), (18, 35), (96, 128)]


@pytest.mark.parametrize("height,width", SYSTEM_SHAPES, ids=["%dx%d" % g for g in SYSTEM_SHAPES])
def test_level_system_against_the_restatement(HP, height, width):
    """Levels 1 to 3 (those that keep 8 pixels on a side; the others are refused), strides 1 to 3, with and without colour: the
    sums and every count class bit for bit."""
    case = TC.colour_pair(7 + height, height, width)
    cam, d, bgr, mb, md = case["cam"], case["depth"], case["bgr"], case["model_bgr"], case["model"]
    ran = 0
    for L in (1, 2, 3):
        if not level_fits(cam, L):
            sums, counts = np.zeros(28, f64), np.zeros(5, np.uint64)
            assert HP.mtp_system(C.byref(Camera(**cam)), L, None, _f32(d).ctypes.data_as(f32p), None, _f32(md).ctypes.data_as(f32p), _f32(PM).reshape(16).ctypes.data_as(f32p),
                                 _f32(PM).reshape(16).ctypes.data_as(f32p), C.byref(pyramid_options(1)), sums.ctypes.data_as(f64p), counts.ctypes.data_as(u64p)) == 1
            continue
        for pname, pose in pair_poses(cam)[:3]:
            for step in (1, 2, 3):
                opt = dict(levels=L + 1, step=step, centre_depth=1.5)
                for colour in (True, False):
                    b, m = (bgr, mb) if colour else (None, None)
                    want = np_pyramid_system(cam, L, b, d, m, md, PM, pose, **opt)
                    assert_same_system(cpp_system(HP, cam, L, b, d, m, md, PM, pose, **opt), want, "level %d, %s, step %d, colour %s" % (L, pname, step, colour))
                    assert want[1][4] == 0 or colour
                    ran += 1
                print("%dx%d level %d %s step %d: counts %s" % (height, width, L, pname, step, want[1]))
    assert ran >= (18 if height < 96 else 54)
    if height == 96:
        big = np_pyramid_system(cam, 1, bgr, d, mb, md, PM, MT.pose_near(), levels=2)
        assert big[1][1] > 500 and big[1][4] > 300 and big[1][2] > 0, big[1]


# ------------------------------------------------------------------ the schedule on a map: the oracle's ray-cast is the renderer
@pytest.fixture(scope="module")
def scene_map():
    s = track_scene()
    s["render_both"] = lambda pose: s["oracle"].render(pose)
    return s


def test_one_level_is_the_single_level_call(HP, scene_map):
    """levels = 1 against np_track_colour_frame and, with bgr null, np_track_frame: every field and every evaluation bit for bit."""
    s = scene_map
    start, opt = basin_start(s, 0), track_opts(s, max_renders=3)
    for colour in (True, False):
        b = s["bgr"] if colour else None
        got = cpp_frame(HP, s["render_both"], s["cam"], b, s["depth"], start, levels=1, **opt)
        want = TC.np_track_colour_frame(s["render_both"], s["cam"], s["bgr"], s["depth"], start, colour=colour, **opt)
        assert_same_result(got, want, "levels = 1, colour %s" % colour)
        assert got["counts"] == tuple(want["counts"]) and got["renders"] == want["renders"] and got["stats8"][6:] == (1, 0)
        assert got["levels"] == {0: (want["status"], want["renders"], want["iterations"], want["valid"])}
    geo = MT.np_track_frame(s["render"], s["cam"], s["depth"], start, **opt)
    assert_same_result(got, geo, "levels = 1 without colour against np_track_frame")


def test_schedule_against_the_restatement_on_every_evaluation(HP, scene_map):
    """Three levels over the oracle's renders from the first basin start, with and without colour: the sums of every evaluation of
    every level, the per-level outcomes, the totals and level 0's result, bit for bit."""
    s = scene_map
    start = basin_start(s, 0)
    for colour, opt in ((True, track_opts(s, max_renders=3, coarse_renders=2)), (False, track_opts(s, max_renders=2, step=2))):
        b = s["bgr"] if colour else None
        want = np_track_pyramid_frame(s["render_both"], s["cam"], b, s["depth"], start, levels=3, **opt)
        got = cpp_frame(HP, s["render_both"], s["cam"], b, s["depth"], start, levels=3, **opt)
        assert_same_pyramid(got, want, "three levels, colour %s" % colour)
        assert sorted(want["levels"]) == [0, 1, 2] and want["stats8"][6] == 3
        print("colour %s: levels %s stats %s" % (colour, want["levels"], want["stats8"]))


def test_every_level_abandoned_ends_lost_at_the_start(HP, scene_map):
    """The 20-voxel, 10-degree start: its samples fall outside the model at every resolution.  Levels 2 and 1 are abandoned, level 0
    starts from the start pose and the call ends LOST with it."""
    s = scene_map
    start = basin_start(s, 2)
    for colour in (True, False):
        b = s["bgr"] if colour else None
        want = np_track_pyramid_frame(s["render_both"], s["cam"], b, s["depth"], start, levels=3, **track_opts(s))
        got = cpp_frame(HP, s["render_both"], s["cam"], b, s["depth"], start, levels=3, **track_opts(s))
        assert_same_pyramid(got, want, "the far start, colour %s" % colour)
        assert got["status"] == LOST and got["stats8"][6:] == (3, 2) and got["stats8"][4] == 3 and got["stats8"][3] == 3
        assert all(got["levels"][L][0] == LOST for L in (0, 1, 2))
        assert np.array_equal(got["T"].astype(f32), start)


# ------------------------------------------------------------------ what the pyramid is for
# measured on the restatement (test_the_scene_with_colour): (degrees, voxels) off the scan's pose after one level and after three
SCENE_ONE_LEVEL = (2.6623, 9.6531)
SCENE_THREE_LEVELS = (0.1451, 0.0959)


def test_the_scene_with_colour(HP, scene_map):
    """The one-scan scene, whose texture (110 rad/m) a 96x128 render aliases, with colour from basin_start(s, 0) (8 voxels, 4
    degrees; TRACK_EPS, every other option its default).  MEASURED on the restatement, exact summation order:
      one level (drf_track_colour_frame): MAX_ITERS after 10 renders, 2.6623 degrees and 9.6531 voxels off the scan's pose;
      three levels, three coarse renders:  level 2 MAX_ITERS (3 renders, 12 evaluations, 479 valid), level 1 MAX_ITERS (3, 12,
        2 496), level 0 MAX_ITERS (10, 40, 9 921): 0.1451 degrees and 0.0959 voxels off -- below one voxel, the bound
        test_one_textured_plane asserts, and inside the four-voxel band of drf_locate_frame, whose restatement from that pose ends
        CONVERGED at 0.0593 degrees and 0.1986 voxels, the minimum of this map.
    The throw-away prototype of the issue (numpy's summation order) gave 0.17 degrees and 0.10 voxels: the exact-order restatement
    confirms it.  Geometry only is MIXED on this scene, printed as information and not asserted: start 0 ends MAX_ITERS 0.1787
    degrees and 3.1769 voxels off where one level gives CONVERGED 0.6672 / 0.5076 (worse); start 1 ends CONVERGED 0.0592 / 0.5818
    where one level gives MAX_ITERS 1.2170 / 0.5975 (better in rotation and status, the same in translation)."""
    s = scene_map
    start, opt = basin_start(s, 0), track_opts(s)
    one = TC.np_track_colour_frame(s["render_both"], s["cam"], s["bgr"], s["depth"], start, **opt)
    pyr = np_track_pyramid_frame(s["render_both"], s["cam"], s["bgr"], s["depth"], start, levels=3, **opt)
    a1, t1 = scene_errors(one["T"], s["pose"])
    a3, t3 = scene_errors(pyr["T"], s["pose"])
    print("one level: status %d, %d renders, %.4f degrees %.4f voxels off" % (one["status"], one["renders"], a1, t1))
    print("three levels: status %d, levels %s, stats %s, %.4f degrees %.4f voxels off" % (pyr["status"], pyr["levels"], pyr["stats8"], a3, t3))
    for colour_name, b in (("geometry only", None),):
        for k in (0, 1):
            g1 = MT.np_track_frame(s["render"], s["cam"], s["depth"], basin_start(s, k), **opt)
            g3 = np_track_pyramid_frame(s["render_both"], s["cam"], b, s["depth"], basin_start(s, k), levels=3, **opt)
            print("%s, start %d: one level status %d %.4f degrees %.4f voxels; three levels status %d %.4f degrees %.4f voxels" %
                  ((colour_name, k, g1["status"]) + scene_errors(g1["T"], s["pose"]) + (g3["status"],) + scene_errors(g3["T"], s["pose"])))
    located = np_locate_frame(s["blocks"], s["cam"], s["depth"], pyr["T"].astype(f32), centre_depth=s["centre_depth"])
    print("pyramid, then locate: status %d, %.4f degrees %.4f voxels off" % ((located["status"],) + scene_errors(located["T"], s["pose"])))
    assert abs(a1 - SCENE_ONE_LEVEL[0]) < 1e-3 and abs(t1 - SCENE_ONE_LEVEL[1]) < 1e-3
    assert t3 < t1, "the pyramid must end nearer the scan's pose in translation than the single-level call"
    assert t3 < 1.0, "and below one voxel"
    assert located["status"] == CONVERGED
    if SCENE_THREE_LEVELS is not None:
        assert abs(a3 - SCENE_THREE_LEVELS[0]) < 1e-3 and abs(t3 - SCENE_THREE_LEVELS[1]) < 1e-3
    got = cpp_frame(HP, s["render_both"], s["cam"], s["bgr"], s["depth"], start, levels=3, **opt)
    assert_same_pyramid(got, pyr, "the scene with colour on the host")


HF_CAM = dict(height=96, width=128, fx=112.0, fy=112.0, cx=63.5, cy=47.5)
HF_STARTS = [(5.0, 4.0), (8.0, 4.0), (12.0, 6.0)]
HF_LEVELS = (1, 3, 4)
# measured on the restatement (test_the_high_frequency_plane): the largest start that ends CONVERGED below one voxel with some levels <= 4
HF_LARGEST = 2


def hf_intensity(X, Y):
    """plane_intensity with its three sines scaled by 0.4, plus 0.9 sin(85 X + 0.3) + 0.9 sin(75 Y + 1.1): texture near and above
    what a 96x128 render of the plane at 1.5 m resolves (one pixel is 13 mm: 85 rad/m is 0.9 pixels per radian)."""
    low = 0.4 * (np.sin(9.0 * X + 1.0) + np.sin(7.0 * Y + 2.0) + np.sin(5.0 * X - 6.0 * Y))
    return np.floor(3.0 * (127.5 + 110.0 * (low + 0.9 * np.sin(85.0 * X + 0.3) + 0.9 * np.sin(75.0 * Y + 1.1)) / 3.0) + 0.5)


def test_the_high_frequency_plane(HP, monkeypatch):
    """The textured plane of tests/test_map_track_colour.py at 96x128 with texture at and above what a render resolves
    (hf_intensity), PLANE_OPTS.  MEASURED on the restatement -- status, then degrees / voxels in the plane:
      start (voxels, degrees)   1 level                   3 levels                    4 levels
      (5, 4)                    MAX_ITERS 2.9034 / 3.9695  CONVERGED 0.0000 / 0.0028   CONVERGED 4.3435 / 2.8140 (a wrong minimum)
      (8, 4)                    MAX_ITERS 4.4556 / 8.2589  MAX_ITERS 4.3638 / 2.7344   CONVERGED 0.0610 / 0.0185
      (12, 6)                   MAX_ITERS 4.3471 / 11.0912 CONVERGED 0.0671 / 5.5417 (a wrong minimum)  CONVERGED 0.0000 / 0.0083
    One level converges from none of them; every start ends CONVERGED below one voxel with SOME levels <= 4, the largest being
    (12, 6) with four -- but no single depth serves every start: CONVERGED is no proof of the right minimum, and the pyramid is no
    global search.  The prototype of the issue agrees in every cell."""
    monkeypatch.setattr(TC, "plane_intensity", hf_intensity)
    monkeypatch.setattr(TC, "PLANE_STARTS", [(2.0, 2.0)] + HF_STARTS)          # plane_start(k + 1) is HF_STARTS[k]
    cam = camera(VS, **HF_CAM)
    render = TC.textured_plane_renderer(cam)
    bgr, depth = render(np.eye(4, dtype=f32))
    table = {}
    for k, st in enumerate(HF_STARTS):
        start = TC.plane_start(k + 1)
        for levels in HF_LEVELS:
            r = np_track_pyramid_frame(render, cam, bgr, depth, start, levels=levels, **TC.PLANE_OPTS)
            a, t, nrm = TC.plane_errors(r["T"])
            table[(k, levels)] = (r["status"], a, t)
            print("start %s, %d levels: status %d, levels %s, %.4f degrees %.4f voxels in the plane %.4f along the normal" % (st, levels, r["status"], r["levels"], a, t, nrm))
    for k in range(len(HF_STARTS)):
        assert not (table[(k, 1)][0] == CONVERGED and table[(k, 1)][2] < 1.0), "one level converges from none of the starts"
    good = [k for k in range(len(HF_STARTS)) if any(table[(k, n)][0] == CONVERGED and table[(k, n)][2] < 1.0 for n in HF_LEVELS)]
    print("starts that end CONVERGED below one voxel with some levels <= 4:", [HF_STARTS[k] for k in good])
    assert good, "no start converges with a pyramid: the rule is wrong"
    if HF_LARGEST is not None:
        assert max(good) == HF_LARGEST
    k = max(good)
    n = [n for n in HF_LEVELS if table[(k, n)][0] == CONVERGED and table[(k, n)][2] < 1.0][0]
    got = cpp_frame(HP, render, cam, bgr, depth, TC.plane_start(k + 1), levels=n, **TC.PLANE_OPTS)
    want = np_track_pyramid_frame(render, cam, bgr, depth, TC.plane_start(k + 1), levels=n, **TC.PLANE_OPTS)
    assert_same_pyramid(got, want, "the high-frequency plane on the host")


# ------------------------------------------------------------------ options, defaults, refusals
def test_options_and_their_defaults(HP):
    out, name = np.zeros(4, f64), C.create_string_buffer(32)
    vs = f32(0.02)
    assert HP.mtp_options(None, vs, 128, 96, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [3, 3, 10, float(f32(5.0) * vs)]
    assert HP.mtp_options(C.byref(pyramid_options(5, 1, max_renders=2)), vs, 128, 128, out.ctypes.data_as(f64p), name) == 0
    assert out[:3].tolist() == [5, 1, 2]
    for bad, which, (w, h) in ((pyramid_options(-1), "levels", (128, 96)), (pyramid_options(6), "levels", (640, 480)), (pyramid_options(5), "levels", (128, 96)),
                               (pyramid_options(4), "levels", (63, 96)), (pyramid_options(0), "levels", (31, 96)), (pyramid_options(2, -1), "coarse_renders", (128, 96)),
                               (pyramid_options(-1, -1, step=-1), "step", (128, 96)), (pyramid_options(-1, -1, photo_weight=-1.0), "photo_weight", (128, 96)),
                               (pyramid_options(9, -1), "levels", (128, 96))):
        assert HP.mtp_options(C.byref(bad), vs, w, h, out.ctypes.data_as(f64p), name) == 1
        assert name.value.decode() == which
    assert HP.mtp_options(C.byref(pyramid_options(4)), vs, 64, 96, out.ctypes.data_as(f64p), name) == 0, "64 >> 3 = 8 is the smallest side"
    assert HP.mtp_options(C.byref(pyramid_options(1)), vs, 8, 8, out.ctypes.data_as(f64p), name) == 0
    assert HP.mtp_options(C.byref(pyramid_options(1)), vs, 7, 8, out.ctypes.data_as(f64p), name) == 1
    assert C.sizeof(PyramidOptions) == 72 and PyramidOptions.levels.offset == 64 and PyramidOptions.coarse_renders.offset == 68


def test_refusals_and_an_image_without_a_sample(HP):
    case = TC.colour_pair(5, 24, 32)
    cam = case["cam"]
    nan = np.eye(4, dtype=f32)
    nan[2, 3] = np.nan
    cm, b, d, mb, md, pm = Camera(**cam), _u8(case["bgr"]), _f32(case["depth"]), _u8(case["model_bgr"]), _f32(case["model"]), _f32(PM).reshape(16)
    sums, counts = np.zeros(28, f64), np.zeros(5, np.uint64)
    args = (b.ctypes.data_as(u8p), d.ctypes.data_as(f32p), mb.ctypes.data_as(u8p), md.ctypes.data_as(f32p))
    bb = _f32(nan).reshape(16)
    for mp, p in ((pm, bb), (bb, pm)):
        assert HP.mtp_system(C.byref(cm), 1, *args, mp.ctypes.data_as(f32p), p.ctypes.data_as(f32p), C.byref(pyramid_options(2)), sums.ctypes.data_as(f64p),
                             counts.ctypes.data_as(u64p)) == 2
    for L in (-1, 2, 5):                                                # 24 >> 2 = 6 pixels
        assert HP.mtp_system(C.byref(cm), L, *args, pm.ctypes.data_as(f32p), pm.ctypes.data_as(f32p), C.byref(pyramid_options(1)), sums.ctypes.data_as(f64p),
                             counts.ctypes.data_as(u64p)) == 1
    zero = np.zeros((24, 32), f32)
    for name, depth, model in (("no samples", zero, case["model"]), ("no hit", case["depth"], zero)):
        want = np_pyramid_system(cam, 1, case["bgr"], depth, case["model_bgr"], model, PM, MT.pose_near(), levels=2)
        got = cpp_system(HP, cam, 1, case["bgr"], depth, case["model_bgr"], model, PM, MT.pose_near(), levels=2)
        assert_same_system(got, want, name)
        assert not got[0].any() and got[1][1] == 0 and got[1][4] == 0
    assert got[1][0] > 50 and got[1][2] == got[1][0]


# ------------------------------------------------------------------ sanitizers, the C ABI and the shim
def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """track_reduce_host, track_pyramid_system_host and track_pyramid_frame_host under AddressSanitizer and UBSan: a plain
    executable, nothing preloaded, nothing loaded into Python.  It reads one synthetic pair from a file and prints the level-1
    sums, which are the restatement's bit for bit; then cases of its own, a level one pixel too small among them."""
    exe, data = str(tmp_path / "map_track_pyramid_san"), str(tmp_path / "case.bin")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_track_pyramid_san.cpp"), "-o", exe])
    case = TC.colour_pair(31, 48, 70)
    opt = dict(step=2, centre_depth=1.5)
    pose = MT.pose_near()
    with open(data, "wb") as fh:
        fh.write(bytes(Camera(**case["cam"])) + bytes(pyramid_options(2, 0, 0.05, **opt)) + _u8(case["bgr"]).tobytes() + _f32(case["depth"]).tobytes() +
                 _u8(case["model_bgr"]).tobytes() + _f32(case["model"]).tobytes() + _f32(PM).tobytes() + _f32(pose).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_track_pyramid_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    line = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("system")][0]
    want = np_pyramid_system(case["cam"], 1, case["bgr"], case["depth"], case["model_bgr"], case["model"], PM, pose, levels=2, photo_weight=0.05, **opt)
    assert np.array_equal(np.array([int(x, 16) for x in line[:28]], np.uint64), bits(want[0])) and tuple(int(x) for x in line[28:]) == want[1]
    assert want[1][1] > 10 and want[1][4] > 5


def test_abi_declares_exports_and_types_the_eight_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_track_reduce", "drf_track_reduce_device", "drf_track_pyramid_system", "drf_track_pyramid_system_device", "drf_track_pyramid_frame",
                            "drf_track_pyramid_frame_device", "drf_track_pyramid_stats", "drf_track_pyramid_level_stats"])
    assert "drf_track_pyramid_options_t" in src
    assert C.sizeof(L.TrackPyramidOptions) == C.sizeof(PyramidOptions) == 72
    assert L.TrackPyramidOptions.levels.offset == 64 and L.TrackPyramidOptions.coarse_renders.offset == 68 and L.TrackPyramidOptions.colour.offset == 0
    lib = L.lib()
    T = (C.c_float * 16)(*np.eye(4, dtype=f32).reshape(16))
    depth, bgr = (C.c_float * 4)(), (C.c_uint8 * 12)()
    sums, counts, out = (C.c_double * 28)(), (C.c_uint64 * 5)(), (C.c_uint64 * 8)()
    assert lib.drf_track_reduce(None, 1, 0.1, bgr, depth, bgr, depth) == 1
    assert lib.drf_track_reduce_device(None, 1, 0.1, None, None, None, None) == 1
    assert lib.drf_track_pyramid_system(None, 1, bgr, depth, bgr, depth, T, T, None, sums, counts) == 1
    assert lib.drf_track_pyramid_system_device(None, 1, None, None, None, None, T, T, None, sums, counts) == 1
    assert lib.drf_track_pyramid_frame(None, bgr, depth, T, None, T, None) == 1
    assert lib.drf_track_pyramid_frame_device(None, None, None, T, None, T, None) == 1
    assert lib.drf_track_pyramid_stats(None, out) == 1
    assert lib.drf_track_pyramid_level_stats(None, 0, out) == 1
    import tandem_amd.dr_fusion as F
    for name in ("track_reduce", "track_pyramid_system", "track_pyramid_frame", "track_pyramid_stats", "track_pyramid_level_stats"):
        assert callable(getattr(F.DrFusion, name))
    hdr = open(os.path.join(ROOT, "include", "dr_mi355x.h")).read()
    assert "and an image pyramid" not in hdr and "an image\n * pyramid, a global search" not in hdr, "the pyramid is no longer out of scope of the tracking calls"
    assert "no reference counterpart; DESIGN.md §7c \"Tracking coarse to fine\"" in hdr


def test_shim_compiles(tmp_path):
    """tandem_amd/libdr/dr_fusion.h TrackPyramidFrame as a TANDEM translation unit would call it
    (tests/cpp/map_track_pyramid_shim.cpp): it compiles and links against the library; tests/test_fusion_track_pyramid_gpu.py runs it."""
    abi_module()
    exe = str(tmp_path / "map_track_pyramid_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_track_pyramid_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert os.path.isfile(exe)
