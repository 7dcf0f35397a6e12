"""CPU: the host half of drf_score_colour_poses / drf_search_colour_frame (include/dr_mi355x.h "The search with an appearance term
from the voxel colours", DESIGN.md §7c "Searching with colour").  score_sample with colour, score_colour_candidates_host and
search_colour_refine of tandem_amd/csrc/pose_host.h compiled with plain g++ (tests/cpp/map_search_colour_check.cpp) and held, bit
for bit, to np_score_colour_candidates / np_search_colour_frame -- the reference of tests/test_fusion_search_colour_gpu.py too.  The
restatement is np_score_candidates of tests/test_map_search.py plus the lines of the colour rule, and its cost and counts are held
to that function's; the refinement is np_track_pyramid_frame and np_locate_frame of the existing modules, by import.  Then what the
feature is for: on one wall the geometric score is the same at every in-plane offset and the colour score finds the nearest lattice
point, on an analytic map and end to end on a map the CPU oracle integrated; the options, status and refusal paths; the same under
AddressSanitizer and UBSan as a stand-alone program (tests/cpp/map_search_colour_san.cpp); the four new names of the C ABI and the
shim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_map_search as MS
import test_map_track_colour as TC
import test_map_track_pyramid as TP
from fusion_helpers import abi_module, check_symbols
from test_map_align import CONVERGED, DEGENERATE, LOST, MAX_ITERS, bits
from test_map_locate import NONE, Camera, camera, np_locate_frame, random_case
from test_map_locate import Options as LocateOptions
from test_map_search import MapIndex, _butterfly, candidate_pose16, np_candidates, np_points, np_score_candidates, np_score_options, np_select, random_poses, small_lattice
from test_map_transform import motion, sorted_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p, u32p, u64p, f32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_double)
f32, f64 = np.float32, np.float64
VS, H, W = MS.VS, MS.H, MS.W
MAX_TOP = 32


# ------------------------------------------------------------------ the rule, restated
def np_score_colour_options(cam, photo_weight=0.0, photo_cap=0.0, **opt):
    """drf_score_colour_options_t with its defaults: np_score_options' dict plus lam = (double)photo_weight (0: (float)(1.0 / 27.0) *
    huber in fp32) and pc (0: oc)."""
    o = np_score_options(cam, **opt)
    w = f32(photo_weight) if photo_weight else TC.DEFAULT_WEIGHT * f32(o["huber"])
    assert w.dtype == f32
    o["photo_weight"], o["lam"] = w, f64(w)
    o["pc"] = f64(f32(photo_cap)) if photo_cap else o["oc"]
    return o


class ColourIndex(MapIndex):
    """MapIndex with the voxels' intensity: y = ((float)c0 + (float)c1) + (float)c2 of bytes 4, 5, 6 (bits 0-7, 8-15, 16-23 of the
    second word)."""

    def __init__(self, blocks):
        super().__init__(blocks)
        if self.n:
            c = np.asarray(blocks[1], np.uint8).reshape(self.n, 512, 8)[:, :, 4:7].astype(f32)
            self.y = (c[:, :, 0] + c[:, :, 1]) + c[:, :, 2]

    def fetch_y(self, p):
        if self.n == 0:
            return np.zeros(p.shape[:-1], f32)
        rel = (p >> 3) - self.lo
        ok = ((rel >= 0) & (rel < self.shape)).all(-1)
        rel = np.where(ok[..., None], rel, 0)
        idx = self.grid[rel[..., 0], rel[..., 1], rel[..., 2]]
        found = ok & (idx >= 0)
        idx = np.where(found, idx, 0)
        vi = ((p[..., 0] & 7) << 6) | ((p[..., 1] & 7) << 3) | (p[..., 2] & 7)
        return np.where(found, self.y[idx, vi], f32(0))


def np_frame_intensity(cam, bgr, step, sample):
    """yf per padded grid position: the intensity of the sample's own pixel, 0 where the position is no sample"""
    Wd, Hd = int(cam["width"]), int(cam["height"])
    Wg = -(-Wd // step)
    total = Wg * -(-Hd // step)
    n = np.arange(len(sample))
    inside = n < total
    j, i = np.where(inside, n // Wg, 0), np.where(inside, n % Wg, 0)
    y = TC.np_intensity(np.asarray(bgr, np.uint8).reshape(Hd, Wd, 3))[step * j, step * i]
    return np.where(sample, y, f32(0))


def _fold(t, c, groups):
    """the one sum of the rule over t (c, positions): per lane, the group butterfly, lane i % 64 adds partial i, the last butterfly"""
    t = t.reshape(c, groups, 8, 64)                                   # position 512 i + l + 64 k -> [i][k][l]
    acc = np.zeros((c, groups, 64), f64)
    for k in range(8):
        acc = acc + t[:, :, k]
    partial = _butterfly(acc)[..., 0]                                 # (c, groups)
    rows = np.concatenate([partial, np.zeros((c, -groups % 64), f64)], axis=1).reshape(c, -1, 64)   # rows[j][l] = partial[l + 64 j]
    lane = np.zeros((c, 64), f64)
    for j in range(rows.shape[1]):
        lane = lane + rows[:, j]
    return _butterfly(lane)[:, 0]


def np_score_colour_candidates(blocks, cam, bgr, depth, R, tv, o, batch=64, detail=None):
    """cost (C,), photo (C,) float64, counts (C, 4), score (C,) float64 of the poses (R (C, 3, 3), tv (C, 3) in lattice units).
    np_score_candidates line for line, then the colour rule's lines, both sums in the fixed order.  detail, a dict if given,
    receives how many valid samples had Huber's weight below 1 and how many were capped."""
    index = blocks if isinstance(blocks, ColourIndex) else ColourIndex(blocks)
    sample, g, groups = np_points(cam, depth, o["step"])
    yf = np_frame_intensity(cam, bgr, o["step"], sample)
    vs64, hub = f64(f32(cam["voxel_size"])), f64(o["huber"])
    R, tv = np.asarray(R, f64).reshape(-1, 3, 3), np.asarray(tv, f64).reshape(-1, 3)
    n = len(R)
    cost, photo, counts = np.zeros(n, f64), np.zeros(n, f64), np.zeros((n, 4), np.int64)
    corners = [(cx, cy, cz) for cx in range(2) for cy in range(2) for cz in range(2)]
    if detail is not None:
        detail.update(huber=0, capped=0)
    for at in range(0, n, batch):
        Rb, tb = R[at:at + batch], tv[at:at + batch]
        c = len(Rb)
        q = np.stack([((Rb[:, k, 0, None] * g[0] + Rb[:, k, 1, None] * g[1]) + Rb[:, k, 2, None] * g[2]) + tb[:, k, None] for k in range(3)], axis=-1)
        inr = ((q > -2.0 ** 30) & (q < 2.0 ** 30)).all(-1)
        q = np.where(inr[..., None], q, 0.0)
        b = np.floor(q)
        f = (q - b).astype(f32)
        bi = b.astype(np.int64)
        observed = sample[None] & inr
        s = np.zeros((2, 2, 2, c, len(sample)), f32)
        y = np.zeros((2, 2, 2, c, len(sample)), f32)
        for cx, cy, cz in corners:
            sd, wt = index.fetch(bi + np.array([cx, cy, cz]))
            observed &= wt >= o["min_weight"]
            s[cx, cy, cz] = sd
            y[cx, cy, cz] = index.fetch_y(bi + np.array([cx, cy, cz]))
        fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
        with np.errstate(all="ignore"):
            e = s[:, :, 0] + fz * (s[:, :, 1] - s[:, :, 0])
            d = e[:, 0] + fy * (e[:, 1] - e[:, 0])
            phi = d[0] + fx * (d[1] - d[0])
            assert phi.dtype == f32
            near = np.abs(phi) < o["band"]
            valid, outside = observed & near, observed & ~near
            r = phi.astype(f64) / vs64
            a = np.abs(r)
            w = np.where(a <= hub, 1.0, hub / a)
            t = np.where(valid, (w * r) * r, 0.0)
            # the colour term
            yz = y[:, :, 0] + fz * (y[:, :, 1] - y[:, :, 0])
            yd = yz[:, 0] + fy * (yz[:, 1] - yz[:, 0])
            Ym = yd[0] + fx * (yd[1] - yd[0])
            assert Ym.dtype == f32
            rp = o["lam"] * (Ym.astype(f64) - yf[None].astype(f64))
            ap = np.abs(rp)
            wp = np.where(ap <= hub, 1.0, hub / ap)
            tp = (wp * rp) * rp
            capped = tp > o["pc"]
            tp = np.where(capped, o["pc"], tp)
            tp = np.where(valid, tp, 0.0)
        if detail is not None:
            detail["huber"] += int((valid & (ap > hub)).sum())
            detail["capped"] += int((valid & capped).sum())
        cost[at:at + c] = _fold(t, c, groups)
        photo[at:at + c] = _fold(tp, c, groups)
        counts[at:at + c] = np.stack([np.full(c, sample.sum()), valid.sum(1), (sample[None] & ~observed).sum(1), outside.sum(1)], axis=1)
    assert (counts[:, 0] == counts[:, 1:].sum(1)).all()
    with np.errstate(all="ignore"):
        score = np.where(counts[:, 0] == 0, o["uc"],
                         (((cost + photo) + o["oc"] * counts[:, 3].astype(f64)) + o["uc"] * counts[:, 2].astype(f64)) / counts[:, 0].astype(f64))
    return cost, photo, counts, score


def np_score_colour_poses(blocks, cam, bgr, depth, poses, detail=None, **opt):
    poses = np.ascontiguousarray(poses, f32).reshape(-1, 4, 4)
    mv = [motion(p, cam["voxel_size"]) for p in poses]
    return np_score_colour_candidates(blocks, cam, bgr, depth, np.stack([m[0] for m in mv]), np.stack([m[1] for m in mv]), np_score_colour_options(cam, **opt),
                                      detail=detail)


def np_search_colour_frame(blocks, render, cam, bgr, depth, anchors, rotations, half=(0, 0, 0), trans_step=0.0, top_k=0, score_only=False, accept_valid=0.0,
                           photo_weight=0.0, photo_cap=0.0, score=None, track=None, locate=None, index=None):
    """drf_search_colour_frame over render(pose) -> (bgr, depth): np_search_frame's dict, the entries with photo, final_score and
    final_photo; plus photos, every candidate's photo.  track: np_track_pyramid_frame's keywords."""
    o = np_score_colour_options(cam, photo_weight, photo_cap, **(score or {}))
    index = index or ColourIndex(blocks)
    R, tv = np_candidates(cam, anchors, rotations, half, trans_step)
    cost, photo, counts, sc = np_score_colour_candidates(index, cam, bgr, depth, R, tv, o)
    sel = np_select(sc, top_k or 8)
    p16 = [candidate_pose16(cam, R[c], tv[c]) for c in sel]
    entries = [dict(index=int(c), score=float(sc[c]), cost=float(cost[c]), photo=float(photo[c]), counts=tuple(int(v) for v in counts[c]), track_status=-1,
                    locate_status=-1, samples=0, valid=0, located_cost=0.0, final_score=0.0, final_photo=0.0, T=p16[k].astype(f64)) for k, c in enumerate(sel)]
    out = dict(status=LOST, winner=-1, refined=0, n_candidates=len(sc), T32=p16[0], scores=sc, photos=photo, entries=entries)
    if score_only:
        out.update(status=MAX_ITERS, winner=0)
        return out
    qual, accepted = [], -1
    for k, en in enumerate(entries):
        tr = TP.np_track_pyramid_frame(render, cam, bgr, depth, p16[k], **(track or {}))
        out["refined"] += 1
        en.update(track_status=tr["status"], T=tr["T"])
        if tr["status"] > MAX_ITERS:
            continue
        lr = np_locate_frame(blocks, cam, depth, tr["T"].astype(f32), **(locate or {}))
        en.update(locate_status=lr["status"], samples=lr["samples"], valid=lr["valid"], located_cost=lr["cost"], T=lr["T"])
        if lr["status"] > MAX_ITERS:
            continue
        qual.append(k)
        if accept_valid > 0.0 and float(en["valid"]) >= accept_valid * float(en["samples"]):
            accepted = k
            break
    if not qual:
        return out
    mv = [motion(entries[k]["T"].astype(f32), cam["voxel_size"]) for k in qual]
    _, fp, _, fs = np_score_colour_candidates(index, cam, bgr, depth, np.stack([m[0] for m in mv]), np.stack([m[1] for m in mv]), o)
    for j, k in enumerate(qual):
        entries[k].update(final_score=float(fs[j]), final_photo=float(fp[j]))
        if out["winner"] < 0 or entries[k]["final_score"] < entries[out["winner"]]["final_score"]:
            out["winner"] = k
    if accepted >= 0:
        out["winner"] = accepted
    out.update(status=entries[out["winner"]]["locate_status"], T32=entries[out["winner"]]["T"].astype(f32))
    return out


# ------------------------------------------------------------------ the compiled host half
class ScoreColourOptions(C.Structure):
    """drf_score_colour_options_t"""
    _fields_ = [("score", MS.ScoreOptions), ("photo_weight", C.c_float), ("photo_cap", C.c_float)]


class SearchColourOptions(C.Structure):
    """drf_search_colour_options_t"""
    _fields_ = [("search", MS.SearchOptions), ("photo_weight", C.c_float), ("photo_cap", C.c_float)]


class SearchColourEntry(C.Structure):
    """drf_search_colour_entry_t"""
    _fields_ = MS.SearchEntry._fields_ + [("photo", C.c_double), ("final_score", C.c_double), ("final_photo", C.c_double)]


class SearchColourResult(C.Structure):
    """drf_search_colour_result_t"""
    _fields_ = [("status", C.c_int), ("n_entries", C.c_int), ("winner", C.c_int), ("refined", C.c_int), ("n_candidates", C.c_uint64),
                ("entries", SearchColourEntry * MAX_TOP)]


def score_colour_options(photo_weight=0.0, photo_cap=0.0, **opt):
    return ScoreColourOptions(MS.ScoreOptions(**opt), photo_weight, photo_cap)


def search_colour_options(photo_weight=0.0, photo_cap=0.0, **search):
    return SearchColourOptions(MS.search_options(**search), photo_weight, photo_cap)


def build_check(directory):
    so = os.path.join(str(directory), "libmap_search_colour_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_search_colour_check.cpp"), "-o", so])
    h = C.CDLL(so)
    head = [u64p, u8p, C.c_size_t, C.POINTER(Camera), u8p, f32p]
    h.msc_options.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, f64p, C.c_char_p]
    h.msc_score.argtypes = head + [f32p, C.c_size_t, C.POINTER(ScoreColourOptions), f64p, f64p, u32p, f64p, f64p]
    h.msc_search.argtypes = head + [TC.RENDER_FN, C.c_void_p, f32p, C.c_size_t, f64p, C.c_size_t, C.POINTER(SearchColourOptions), C.POINTER(TP.PyramidOptions),
                                    C.POINTER(LocateOptions), f32p, C.POINTER(SearchColourResult), f64p, f64p, C.c_char_p]
    return h


@pytest.fixture(scope="module")
def HS(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("map_search_colour"))


def _head(blocks, cam, bgr, depth):
    rk, rv = sorted_source(*blocks)
    depth = np.ascontiguousarray(depth, f32)
    bgr = np.ascontiguousarray(bgr, np.uint8)
    assert depth.size == cam["height"] * cam["width"] and bgr.size == 3 * depth.size
    cm = Camera(**cam)
    return (rk, rv, bgr, depth, cm), [rk.ctypes.data_as(u64p), rv.ctypes.data_as(u8p), len(rk), C.byref(cm), bgr.ctypes.data_as(u8p), depth.ctypes.data_as(f32p)]


def cpp_score(HS, blocks, cam, bgr, depth, poses, expect=0, geometric=False, **opt):
    """(cost, photo, counts, score) of the host half; geometric: and score_candidates_host's score behind them (the host itself
    then holds cost and counts to that function's)"""
    keep, head = _head(blocks, cam, bgr, depth)
    poses = np.ascontiguousarray(poses, f32).reshape(-1, 16)
    n = len(poses)
    cost, photo, counts, score, geo = np.zeros(n, f64), np.zeros(n, f64), np.zeros((n, 4), np.uint32), np.zeros(n, f64), np.zeros(n, f64)
    rc = HS.msc_score(*head, poses.ctypes.data_as(f32p), n, C.byref(score_colour_options(**opt)), cost.ctypes.data_as(f64p), photo.ctypes.data_as(f64p),
                      counts.ctypes.data_as(u32p), score.ctypes.data_as(f64p), geo.ctypes.data_as(f64p) if geometric else None)
    assert rc == expect, rc
    return (cost, photo, counts.astype(np.int64), score) + ((geo,) if geometric else ())


def entry_dict(e):
    return dict(MS.entry_dict(e), photo=float(e.photo), final_score=float(e.final_score), final_photo=float(e.final_photo))


def cpp_search(HS, blocks, render, cam, bgr, depth, anchors, rotations, track=None, locate=None, expect=0, **search):
    """search_colour_refine over the host's pyramid tracking, localisation and colour score and the Python renderer, as a dict
    shaped like np_search_colour_frame's; a refused call returns (code, name)."""
    keep, head = _head(blocks, cam, bgr, depth)
    anchors = np.ascontiguousarray(anchors, f32).reshape(-1, 16)
    rot = np.ascontiguousarray(rotations, f64).reshape(-1, 9)
    npix = cam["height"] * cam["width"]

    def call(p16, cout, dout, user):
        c, d = render(np.ctypeslib.as_array(p16, (16,)).reshape(4, 4).copy())
        c, d = np.ascontiguousarray(c, np.uint8), np.ascontiguousarray(d, f32)
        C.memmove(cout, c.ctypes.data, npix * 3)
        C.memmove(dout, d.ctypes.data, npix * 4)

    so = search_colour_options(**search)
    n = len(anchors) * len(rot) * int(np.prod([2 * h + 1 for h in so.search.half]))
    size = max(n, 1) if 0 < n <= 1 << 24 else 1
    scores, photos = np.zeros(size, f64), np.zeros(size, f64)
    T32, r, name = np.zeros(16, f32), SearchColourResult(), C.create_string_buffer(32)
    rc = HS.msc_search(*head, TC.RENDER_FN(call), None, anchors.ctypes.data_as(f32p), len(anchors), rot.ctypes.data_as(f64p), len(rot), C.byref(so),
                       C.byref(TP.pyramid_options(**(track or {}))), C.byref(LocateOptions(**(locate or {}))), T32.ctypes.data_as(f32p), C.byref(r),
                       scores.ctypes.data_as(f64p), photos.ctypes.data_as(f64p), name)
    assert rc == expect, (rc, name.value)
    if rc != 0:
        return rc, name.value.decode()
    return dict(status=int(r.status), winner=int(r.winner), refined=int(r.refined), n_candidates=int(r.n_candidates), T32=np.array(T32, f32).reshape(4, 4), scores=scores,
                photos=photos, entries=[entry_dict(e) for e in r.entries[:r.n_entries]])


def assert_same_colour_scores(got, want, what):
    assert np.array_equal(np.asarray(got[2], np.int64), np.asarray(want[2], np.int64)), f"{what}: counts differ"
    for k, name in ((0, "cost"), (1, "photo"), (3, "score")):
        bad = np.flatnonzero(bits(got[k]) != bits(want[k]))
        assert bad.size == 0, f"{what}: {name} differs at {bad[:5].tolist()}: got {got[k][bad[:3]]} want {want[k][bad[:3]]}"


def assert_same_colour_search(got, want, what):
    """two results of the colour search, bit for bit"""
    MS.assert_same_search(got, want, what)
    if got.get("photos") is not None and want.get("photos") is not None:
        assert np.array_equal(bits(got["photos"]), bits(want["photos"])), f"{what}: the photo sums differ"
    for i, (a, b) in enumerate(zip(got["entries"], want["entries"])):
        for k in ("photo", "final_score", "final_photo"):
            assert bits(a[k]) == bits(b[k]), f"{what}: entry {i} {k} differs: {a[k]} against {b[k]}"


# ------------------------------------------------------------------ random maps with random colours
def random_colour_case(seed, height=H, width=W, shift=(0, 0, 0)):
    """random_case with its colour bytes overwritten by seeded random bytes per voxel, and a seeded random bgr image"""
    case = random_case(seed, height, width, shift)
    rng = np.random.default_rng(1000 + seed)
    vox = np.array(case["blocks"][1], np.uint8).reshape(-1, 512, 8)
    vox[:, :, 4:7] = rng.integers(0, 256, (len(vox), 512, 3), dtype=np.uint8)
    case["blocks"] = (case["blocks"][0], vox.reshape(len(vox), 4096))
    case["bgr"] = rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    return case


# 1 grey level of the three-channel sum at weight 1/27 is 1/27 voxel: random colours differ by some 250 units, far above Huber's
# threshold at every weight here but the last, and a term is huber * |rp|: some 9 voxels^2 at the default weight, above the default
# cap of 4 (oc).  So: the defaults cap nearly every sample; a large cap leaves Huber's branch alone; a tiny weight the quadratic one.
COLOUR_SETS = [("defaults", {}, dict(capped=True, huber=True)),
               ("own weight and cap", dict(photo_weight=0.01, photo_cap=3.0), dict(capped=True, huber=True)),
               ("a cap small enough to bind always", dict(photo_cap=0.125, huber=0.5), dict(capped=True, huber=True)),
               ("a weight large enough that Huber binds, no cap in reach", dict(photo_weight=0.5, photo_cap=1e6), dict(capped=False, huber=True)),
               ("a weight small enough that neither binds", dict(photo_weight=0.0005, photo_cap=1e6), dict(capped=False, huber=False))]
COLOUR_SHAPES = [(96, 128, 1), (96, 128, 3), (96, 128, 4), (168, 200, 1)]


@pytest.mark.parametrize("height,width,step", COLOUR_SHAPES, ids=["96x128 step 1", "96x128 step 3", "96x128 step 4", "168x200 step 1 (66 groups)"])
def test_score_against_the_restatement_on_random_maps(HS, height, width, step):
    """The four output arrays of the host half against the restatement, bit for bit, under every option set; the restatement's cost
    and counts are np_score_candidates'; every branch of the colour term is taken where the set says so."""
    case = random_colour_case(3, height, width)
    poses = random_poses(case, 24 if height > H else 40)
    if height > H:
        sample, _, groups = np_points(case["cam"], case["depth"], step)
        assert groups == 66
    geo = MS.np_score_poses(case["blocks"], case["cam"], case["depth"], poses, step=step)
    for name, opt, branch in COLOUR_SETS:
        detail = {}
        sopt = {k: v for k, v in opt.items() if k not in ("photo_weight", "photo_cap")}
        want = np_score_colour_poses(case["blocks"], case["cam"], case["bgr"], case["depth"], poses, detail=detail, step=step, **opt)
        if not sopt:
            assert np.array_equal(bits(want[0]), bits(geo[0])) and np.array_equal(want[2], geo[1]), name
        got = cpp_score(HS, case["blocks"], case["cam"], case["bgr"], case["depth"], poses, geometric=True, step=step, **opt)
        assert_same_colour_scores(got, want, "%s, %s" % (name, (height, width, step)))
        valid = int(want[2][:, 1].sum())
        assert valid > 500 and (want[2][:, 1] == 0).any()
        if not name.startswith("a cap small"):                               # (there photo is a count times the cap)
            assert len(np.unique(bits(want[1]))) >= int((want[2][:, 1] > 0).sum()) // 2 >= 5, name
        assert (detail["capped"] > 0) == branch["capped"] and (detail["huber"] > 0) == branch["huber"], (name, detail)
        if name == "own weight and cap":
            assert 0 < detail["capped"] < valid and 0 < detail["huber"] < valid, (name, detail, valid)   # both sides of both branches
        assert ((want[1] > 0) == (want[2][:, 1] > 0)).all()


def test_at_least_a_hundred_photo_bit_patterns_and_some_capped_samples():
    """the issue's count on the full grid: 259 poses at step 1, own weight and cap"""
    case = random_colour_case(3)
    detail = {}
    want = np_score_colour_poses(case["blocks"], case["cam"], case["bgr"], case["depth"], random_poses(case, 259), detail=detail, photo_weight=0.01, photo_cap=3.0)
    assert len(np.unique(bits(want[1]))) >= 100 and detail["capped"] > 0 and detail["huber"] > 0


def test_far_blocks(HS):
    case = random_colour_case(3, shift=(300, -270, 5))
    poses = random_poses(case, 12)
    want = np_score_colour_poses(case["blocks"], case["cam"], case["bgr"], case["depth"], poses)
    assert_same_colour_scores(cpp_score(HS, case["blocks"], case["cam"], case["bgr"], case["depth"], poses), want, "far")
    assert want[2][:, 1].max() > 10 and want[1].max() > 0


def test_the_two_invariants(HS):
    """A map of one colour -- random_case with every voxel's colour bytes set to (40, 130, 220), the colour planes_case gives its
    voxels (random_case's own colour bytes are random) -- and an image of that colour: photo is +0.0 at every pose and the score
    has the geometric score's bits; cost and counts are the geometric call's (the host checks them itself)."""
    case = random_case(3)
    vox = np.array(case["blocks"][1], np.uint8).reshape(-1, 512, 8)
    vox[:, :, 4:7] = (40, 130, 220)
    case["blocks"] = (case["blocks"][0], vox.reshape(len(vox), 4096))
    bgr = np.broadcast_to(np.array((40, 130, 220), np.uint8), (H, W, 3))
    poses = random_poses(case, 40)
    for opt in ({}, dict(step=1), dict(step=3, huber=0.25, band=0.03, min_weight=3), dict(photo_weight=0.7, photo_cap=0.01)):
        got = cpp_score(HS, case["blocks"], case["cam"], bgr, case["depth"], poses, geometric=True, **opt)
        assert (bits(got[1]) == 0).all(), opt
        assert np.array_equal(bits(got[3]), bits(got[4])), opt
        sopt = {k: v for k, v in opt.items() if k not in ("photo_weight", "photo_cap")}
        geo = MS.np_score_poses(case["blocks"], case["cam"], case["depth"], poses, **sopt)
        assert np.array_equal(bits(got[0]), bits(geo[0])) and np.array_equal(got[2], geo[1]) and np.array_equal(bits(got[3]), bits(geo[2]))
        want = np_score_colour_poses(case["blocks"], case["cam"], bgr, case["depth"], poses, **opt)
        assert_same_colour_scores(got[:4], want, "uniform")
    assert got[2][:, 1].max() > 30


# ------------------------------------------------------------------ the wall: what the feature is for
WALL_Z = 75                                  # voxels: the plane z = 1.5 m
WALL_ANCHOR = (-13.0, 10.0, 2.0)             # voxels off the truth (the identity)
WALL_HALF = (3, 3, 1)
WALL_NEAREST = 112                           # offsets (5, 2, 1) of 7 x 7 x 3: (3, 2, 2) voxels off
# measured on the restatement (test_the_wall prints it): the colour score of the nearest lattice point, of the best other
# candidate of its z layer, and the margin between them, voxels^2 per sample
WALL_MEASURED = (3.4272, 4.3327, 0.9056)


def wall_camera():
    return camera(VS, **TC.PLANE_CAM)


def wall_map():
    """The analytic wall: the plane z = 75 voxels at 2 cm voxels; blocks x -11..10, y -9..8, z 8..10, every voxel weight 5, sdf the
    signed distance 1.5 m - z (not truncated: beyond the band a sample is OUTSIDE), coloured by plane_intensity at its world
    (X, Y), split over the channels as textured_plane_renderer splits it."""
    vs64 = f64(f32(VS))
    coords = np.array([(x, y, z) for x in range(-11, 11) for y in range(-9, 9) for z in range(8, 11)], np.int64)
    off = np.array([(x, y, z) for x in range(8) for y in range(8) for z in range(8)], np.int64)
    pts = (coords[:, None, :] * 8 + off[None]).astype(f64) * vs64
    vox = np.zeros((len(coords), 512, 8), np.uint8)
    sdf = (WALL_Z * vs64 - pts[..., 2]).astype(f32)
    vox[:, :, :4] = np.ascontiguousarray(sdf).view(np.uint8).reshape(len(coords), 512, 4)
    y = TC.plane_intensity(pts[..., 0], pts[..., 1]).astype(np.int64)
    vox[:, :, 4], vox[:, :, 5], vox[:, :, 6] = y // 3, (y + 1) // 3, (y + 2) // 3
    vox[:, :, 7] = 5
    return coords, vox.reshape(len(coords), 4096)


def wall_anchor():
    a = np.eye(4, dtype=f32)
    a[:3, 3] = (np.array(WALL_ANCHOR) * f64(f32(VS))).astype(f32)
    return a


WALL_SEARCH = dict(half=WALL_HALF, score=dict(step=2))


@pytest.fixture(scope="module")
def wall():
    cam = wall_camera()
    render = TC.textured_plane_renderer(cam, WALL_Z * float(f64(f32(VS))))
    bgr, depth = render(np.eye(4, dtype=f32))
    blocks = wall_map()
    return dict(cam=cam, render=render, bgr=bgr, depth=depth, blocks=blocks, index=ColourIndex(blocks))


def test_the_wall(HS, wall):
    """One wall, the frame rendered at the identity (48x64, step 2: 768 samples), the lattice 7 x 7 x 3 about an anchor (-13, 10, 2)
    voxels off, 8-voxel steps: 147 candidates, the nearest (candidate 112) (3, 2, 2) voxels off.  MEASURED on the restatement:
    the geometric score is 2.000002 at all 49 in-plane offsets of that z layer, 768 of 768 samples valid at each; the geometric best
    is candidate 1, 39.6 voxels off; the nearest point ranks 38th.  The colour score of the nearest point is 3.4272, rank 0; the
    best other candidate of its layer scores 4.3327 (margin 0.9056); a candidate whose samples are all OUTSIDE scores 4.0.  At
    the truth itself: geometric 0, colour 0.0003."""
    w = wall
    cam, eye = w["cam"], np.eye(3).reshape(1, 9)
    R, tv = np_candidates(cam, wall_anchor()[None], eye, WALL_HALF)
    assert len(R) == 147
    dist = np.linalg.norm(tv, axis=1)
    assert int(np.argmin(dist)) == WALL_NEAREST and np.allclose(tv[WALL_NEAREST], (3, 2, 2), atol=1e-5)
    gcost, gcounts, gscore = np_score_candidates(w["index"], cam, w["depth"], R, tv, np_score_options(cam, step=2))
    cost, photo, counts, score = np_score_colour_candidates(w["index"], cam, w["bgr"], w["depth"], R, tv, np_score_colour_options(cam, step=2))
    assert np.array_equal(bits(cost), bits(gcost)) and np.array_equal(counts, gcounts)
    layer = np.flatnonzero(np.arange(147) % 3 == WALL_NEAREST % 3)
    assert len(layer) == 49 and WALL_NEAREST in layer
    truth = np_score_colour_poses(w["index"], cam, w["bgr"], w["depth"], np.eye(4, dtype=f32)[None], step=2)
    gbest, cbest = int(np_select(gscore, 1)[0]), int(np_select(score, 1)[0])
    others = layer[layer != WALL_NEAREST]
    margin = float(score[others].min() - score[WALL_NEAREST])
    print("geometric: layer scores %.6f .. %.6f, valid %d .. %d of %d; best candidate %d, %.1f voxels off; the nearest ranks %d" %
          (gscore[layer].min(), gscore[layer].max(), gcounts[layer, 1].min(), gcounts[layer, 1].max(), gcounts[0, 0], gbest, dist[gbest],
           int(np.flatnonzero(np_select(gscore, 147) == WALL_NEAREST)[0])))
    print("colour: nearest %.4f (rank %d), best other of its layer %.4f, margin %.4f, all-OUTSIDE %.4f; at the truth geometric %.6f colour %.6f" %
          (score[WALL_NEAREST], int(np.flatnonzero(np_select(score, 147) == WALL_NEAREST)[0]), score[others].min(), margin, score[counts[:, 3] == counts[:, 0]].min(),
           truth[0][0] / truth[2][0, 0], truth[3][0]))
    assert (gcounts[layer, 1] == gcounts[layer[0], 1]).all() and gcounts[layer[0], 1] == 768      # every sample valid at every in-plane offset
    assert np.abs(gscore[layer] / gscore[layer[0]] - 1.0).max() <= 1e-5
    assert gbest != WALL_NEAREST
    assert cbest == WALL_NEAREST
    assert abs(margin - WALL_MEASURED[2]) < 1e-3 and abs(score[WALL_NEAREST] - WALL_MEASURED[0]) < 1e-3, (score[WALL_NEAREST], score[others].min(), margin)
    assert margin >= 0.5 * WALL_MEASURED[2]
    want = np_search_colour_frame(w["blocks"], None, cam, w["bgr"], w["depth"], wall_anchor()[None], eye, score_only=True, index=w["index"], **WALL_SEARCH)
    got = cpp_search(HS, w["blocks"], None, cam, w["bgr"], w["depth"], wall_anchor()[None], eye, score_only=True, **WALL_SEARCH)
    assert_same_colour_search(got, want, "the wall")
    assert got["entries"][0]["index"] == WALL_NEAREST and np.array_equal(bits(got["scores"]), bits(score))


# ------------------------------------------------------------------ end to end on a wall the CPU oracle integrated
def wall_scans(cam):
    """The textured wall seen from a 5 x 5 grid of camera positions, sideways and up, as plane_scans of
    tests/test_fusion_track_colour_gpu.py does: 0.5 m and 0.4 m apart, which with the 1.7 m x 1.3 m the camera sees at 1.5 m covers
    +-1.85 m x +-1.44 m -- the 43 x 32 voxels of the frame's half extent plus the lattice's 37 x 34 is 1.6 m x 1.32 m."""
    render = TC.textured_plane_renderer(cam, WALL_Z * float(f64(f32(VS))))
    out = []
    for dy in (0.0, 0.4, -0.4, 0.8, -0.8):
        for dx in (0.0, 0.5, -0.5, 1.0, -1.0):
            p = np.eye(4, dtype=f32)
            p[0, 3], p[1, 3] = dx, dy
            out.append(render(p) + (p,))
    return out


def integrated_wall():
    """dict(cam, oracle, blocks, render, bgr, depth): the scans of wall_scans in the CPU oracle, whose render is the engine's"""
    from oracle.tsdf_oracle import TsdfOracle
    cam = camera(VS, num_blocks=8000, num_buckets=8000, **TC.PLANE_CAM)
    orc = TsdfOracle(**cam)
    scans = wall_scans(cam)
    for scan in scans:
        orc.integrate(*scan)
    blk = orc.export_blocks()
    coords = np.array(sorted(blk), np.int64).reshape(-1, 3)
    vox = np.stack([blk[tuple(c)] for c in coords.tolist()])
    return dict(cam=cam, oracle=orc, scans=scans, blocks=(coords, vox), render=lambda p: orc.render(p), bgr=scans[0][0], depth=scans[0][1])


WALL_TRACK = dict(levels=1, centre_depth=1.5, **TC.TRACK_EPS)
WALL_LOCATE = dict(centre_depth=1.5)
WALL_END_TO_END = dict(half=WALL_HALF, top_k=3, score=dict(step=2), track=WALL_TRACK, locate=WALL_LOCATE)


def wall_errors(T):
    """(voxels in the plane, voxels along the normal) of a pose against the truth, the identity"""
    T = np.asarray(T, f64)
    return float(np.hypot(T[0, 3], T[1, 3]) / f64(f32(VS))), float(abs(T[2, 3]) / f64(f32(VS)))


@pytest.fixture(scope="module")
def owall():
    w = integrated_wall()
    w["index"] = ColourIndex(w["blocks"])
    return w


def test_the_search_with_colour_ends_on_the_truth_where_geometry_cannot(HS, owall):
    """End to end on the CPU, the oracle's ray-cast the renderer: the 147-candidate wall lattice on the map of 25 integrated scans,
    the 3 best colour scores tracked with colour (one level: drf_track_colour_frame's rule) and located, the winner by final_score.
    The host equals the restatement bit for bit and the winner is within one voxel in the plane and 0.25 voxels along the normal.
    MEASURED on the restatement: the entries are candidates 112 (the nearest lattice point, score 3.5717), 91 (4.4554) and 88
    (4.4599); each is tracked (MAX_ITERS) and located (CONVERGED, 3 072 of 3 072 valid) onto the same pose, 0.1331 voxels off in
    the plane and 0.0227 along the normal, final_score 0.0571 -- the colour tracking reaches the truth from all three, and entry 1
    wins by the last bits of its final_score.  The geometric np_search_frame on the same inputs selects candidates 145, 103 and
    124, every one CONVERGED, and ends 33.8062 voxels off in the plane (0.0257 along the normal): a pose that explains the depth
    image and is in the wrong place."""
    w = owall
    cam, eye, anchor = w["cam"], np.eye(3).reshape(1, 9), wall_anchor()[None]
    want = np_search_colour_frame(w["blocks"], w["render"], cam, w["bgr"], w["depth"], anchor, eye, index=w["index"], **WALL_END_TO_END)
    for k, e in enumerate(want["entries"]):
        print("entry %d: candidate %d score %.4f photo %.2f track %d locate %d, %d of %d valid, final %.4f, %.4f voxels in the plane %.4f along the normal" %
              ((k, e["index"], e["score"], e["photo"], e["track_status"], e["locate_status"], e["valid"], e["samples"], e["final_score"]) + wall_errors(e["T"])))
    assert want["n_candidates"] == 147 and want["refined"] == 3 and want["entries"][0]["index"] == WALL_NEAREST
    assert want["status"] in (CONVERGED, MAX_ITERS) and want["winner"] >= 0
    t, nrm = wall_errors(want["T32"])
    print("colour winner: entry %d, %.4f voxels in the plane, %.4f along the normal" % (want["winner"], t, nrm))
    assert t <= 1.0 and nrm <= 0.25, (t, nrm)
    ok = [k for k, e in enumerate(want["entries"]) if 0 <= e["locate_status"] <= MAX_ITERS]
    assert want["winner"] == min(ok, key=lambda k: (want["entries"][k]["final_score"], k))
    got = cpp_search(HS, w["blocks"], w["render"], cam, w["bgr"], w["depth"], anchor, eye, **WALL_END_TO_END)
    assert_same_colour_search(got, want, "end to end")
    geo = MS.np_search_frame(w["blocks"], lambda p: w["render"](p)[1], cam, w["depth"], anchor, eye, half=WALL_HALF, top_k=3, score=dict(step=2),
                             track=dict(centre_depth=1.5, **TC.TRACK_EPS), locate=WALL_LOCATE, index=w["index"])
    gt, gn = wall_errors(geo["T32"])
    print("geometric: status %d winner %d, %.4f voxels in the plane, %.4f along the normal; entries %s" %
          (geo["status"], geo["winner"], gt, gn, [(e["index"], e["track_status"], e["locate_status"]) for e in geo["entries"]]))
    assert geo["status"] in (LOST, DEGENERATE) or gt > 8.0, (geo["status"], gt)


# ------------------------------------------------------------------ options, defaults, refusals and status paths
def test_options_and_their_defaults(HS):
    out, name = np.zeros(16, f64), C.create_string_buffer(32)
    tr, vs = f32(0.08), f32(0.02)
    oc = float(f64(tr) / f64(vs))
    w = TC.DEFAULT_WEIGHT * f32(1.0)
    assert HS.msc_options(None, 0, tr, vs, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [4, 1, float(tr), 1.0, oc, 2.0 * oc, float(f64(f32(2.0) * tr) / f64(vs)), 1, 1, 1, 8, 0, 0.0, float(w), float(f64(w)), oc]
    assert HS.msc_options(None, 1, tr, vs, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist()[:6] == [4, 1, float(tr), 1.0, oc, 2.0 * oc] and out.tolist()[13:] == [float(w), float(f64(w)), oc]
    full = search_colour_options(photo_weight=0.3, photo_cap=2.5, half=(1, 2, 3), trans_step=0.1, top_k=32, score_only=True, accept_valid=0.5,
                                 score=dict(step=2, min_weight=3, band=0.05, huber=2.0, outside_cost=1.5, unobserved_cost=2.5))
    assert HS.msc_options(C.byref(full), 0, tr, vs, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [2, 3, float(f32(0.05)), 2.0, 1.5, 2.5, float(f64(f32(0.1)) / f64(vs)), 3, 5, 7, 32, 1, 0.5, float(f32(0.3)), float(f64(f32(0.3))), 2.5]
    huber2 = score_colour_options(huber=2.0)                                # the weight follows the resolved huber, the cap the resolved oc
    assert HS.msc_options(C.byref(huber2), 1, tr, vs, out.ctypes.data_as(f64p), name) == 0
    assert out[13] == float(TC.DEFAULT_WEIGHT * f32(2.0)) and out[15] == 2.0 * oc
    for bad, which in ((dict(photo_weight=-1.0), "photo_weight"), (dict(photo_weight=float("nan")), "photo_weight"), (dict(photo_cap=-0.5), "photo_cap"),
                       (dict(photo_cap=float("inf")), "photo_cap"), (dict(photo_weight=-1.0, photo_cap=-1.0), "photo_weight"),
                       (dict(photo_weight=-1.0, score=dict(huber=-1.0)), "huber"), (dict(photo_cap=-1.0, top_k=33), "top_k")):
        assert HS.msc_options(C.byref(search_colour_options(**bad)), 0, tr, vs, out.ctypes.data_as(f64p), name) == 1, bad
        assert name.value.decode() == which
    assert HS.msc_options(C.byref(score_colour_options(photo_cap=-1.0, band=-1.0)), 1, tr, vs, out.ctypes.data_as(f64p), name) == 1 and name.value == b"band"
    assert C.sizeof(ScoreColourOptions) == 32 and C.sizeof(SearchColourOptions) == 64 and C.sizeof(SearchColourEntry) == 224


def test_score_only_accept_valid_and_no_qualifying_entry(HS, owall):
    w = owall
    cam, eye, anchor = w["cam"], np.eye(3).reshape(1, 9), wall_anchor()[None]
    kw = dict(WALL_END_TO_END, score_only=True)
    want = np_search_colour_frame(w["blocks"], w["render"], cam, w["bgr"], w["depth"], anchor, eye, index=w["index"], **kw)
    got = cpp_search(HS, w["blocks"], w["render"], cam, w["bgr"], w["depth"], anchor, eye, **kw)
    assert_same_colour_search(got, want, "score_only")
    assert got["status"] == MAX_ITERS and got["winner"] == 0 and got["refined"] == 0
    assert all(e["track_status"] == -1 and e["final_score"] == 0.0 and e["photo"] > 0 for e in got["entries"])
    kw = dict(WALL_END_TO_END, accept_valid=0.5)
    want = np_search_colour_frame(w["blocks"], w["render"], cam, w["bgr"], w["depth"], anchor, eye, index=w["index"], **kw)
    got = cpp_search(HS, w["blocks"], w["render"], cam, w["bgr"], w["depth"], anchor, eye, **kw)
    assert_same_colour_search(got, want, "accept_valid")
    assert got["refined"] == 1 and got["winner"] == 0 and got["entries"][1]["track_status"] == -1
    assert got["entries"][0]["final_score"] > 0 and got["entries"][1]["final_score"] == 0.0
    miss = lambda p: (np.zeros((cam["height"], cam["width"], 3), np.uint8), np.zeros((cam["height"], cam["width"]), f32))   # noqa: E731
    kw = dict(WALL_END_TO_END, top_k=2)
    want = np_search_colour_frame(w["blocks"], miss, cam, w["bgr"], w["depth"], anchor, eye, index=w["index"], **kw)
    got = cpp_search(HS, w["blocks"], miss, cam, w["bgr"], w["depth"], anchor, eye, **kw)
    assert_same_colour_search(got, want, "no qualifying entry")
    assert got["status"] == LOST and got["winner"] == -1 and got["refined"] == 2
    assert np.array_equal(got["T32"], got["entries"][0]["T"].astype(f32)) and got["entries"][0]["index"] == WALL_NEAREST


def test_an_image_without_a_sample_and_an_empty_map(HS):
    case = random_colour_case(4)
    poses = random_poses(case, 8)
    o = np_score_colour_options(case["cam"])
    for name, blocks, depth in (("no samples", case["blocks"], np.zeros((H, W), f32)), ("NaN only", case["blocks"], np.full((H, W), np.nan, f32)),
                                ("empty map", NONE, case["depth"])):
        want = np_score_colour_poses(blocks, case["cam"], case["bgr"], depth, poses)
        got = cpp_score(HS, blocks, case["cam"], case["bgr"], depth, poses, geometric=True)
        assert_same_colour_scores(got, want, name)
        assert not got[0].any() and not got[1].any() and (got[3] == o["uc"]).all() and np.array_equal(bits(got[3]), bits(got[4]))
    anchors, rot = small_lattice(case)
    none = lambda p: (np.zeros((H, W, 3), np.uint8), np.zeros((H, W), f32))   # noqa: E731
    got = cpp_search(HS, NONE, none, case["cam"], case["bgr"], case["depth"], anchors, rot, top_k=2)
    assert got["status"] == LOST and got["entries"][0]["index"] == 0 and got["refined"] == 2


def test_refusals(HS):
    case = random_colour_case(3)
    anchors, rot = small_lattice(case)
    args = (HS, case["blocks"], None, case["cam"], case["bgr"], case["depth"])
    assert cpp_search(*args, anchors, rot, expect=1, photo_weight=-1.0) == (1, "photo_weight")
    assert cpp_search(*args, anchors, rot, expect=1, photo_cap=float("nan")) == (1, "photo_cap")
    assert cpp_search(*args, anchors, rot, expect=1, photo_cap=-1.0, top_k=33) == (1, "top_k")
    assert cpp_search(*args, anchors, rot, expect=1, photo_cap=-1.0, track=dict(levels=9)) == (1, "photo_cap")
    assert cpp_search(*args, anchors, rot, expect=1, track=dict(levels=9), locate=dict(eps_rot=-1.0)) == (1, "levels")
    assert cpp_search(*args, anchors, rot, expect=1, track=dict(photo_weight=-1.0)) == (1, "photo_weight")
    assert cpp_search(*args, anchors, rot, expect=1, locate=dict(eps_rot=-1.0)) == (1, "eps_rot")
    assert cpp_search(*args, anchors[:0], rot, expect=3)[0] == 3
    assert cpp_search(*args, anchors, rot, expect=3, half=(200, 200, 200))[0] == 3
    scaled = anchors.copy()
    scaled[1, :3, :3] *= 1.01
    assert cpp_search(*args, scaled, rot, expect=2)[1].startswith("anchor 1 is not a rigid motion")
    poses = random_poses(case, 3)
    poses[1, :3, :3] *= 1.01
    cpp_score(HS, case["blocks"], case["cam"], case["bgr"], case["depth"], poses, expect=2)
    cpp_score(HS, case["blocks"], case["cam"], case["bgr"], case["depth"], poses[:1], expect=1, photo_cap=-1.0)


def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """score_colour_candidates_host and search_colour_refine under AddressSanitizer and UBSan: a plain executable with its own main,
    nothing preloaded, nothing loaded into Python.  It reads a case from a file -- the random map with random colours, an image, 21
    poses, a lattice -- and prints cost and photo, which are the restatement's bit for bit."""
    exe, data = str(tmp_path / "map_search_colour_san"), str(tmp_path / "case.bin")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_search_colour_san.cpp"), "-o", exe])
    case = random_colour_case(3)
    poses = random_poses(case, 21).reshape(-1, 16)
    anchors, rot = small_lattice(case)
    rk, rv = sorted_source(*case["blocks"])
    with open(data, "wb") as fh:
        fh.write(np.uint64(len(rk)).tobytes() + rk.tobytes() + rv.tobytes() + bytes(Camera(**case["cam"])))
        fh.write(np.ascontiguousarray(case["bgr"], np.uint8).tobytes() + np.ascontiguousarray(case["depth"], f32).tobytes() + np.uint64(len(poses)).tobytes() + poses.tobytes())
        fh.write(np.uint64(len(anchors)).tobytes() + anchors.tobytes() + np.uint64(len(rot)).tobytes() + rot.tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_search_colour_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith(("cost", "photo", "lattice"))}
    want = np_score_colour_poses(case["blocks"], case["cam"], case["bgr"], case["depth"], poses, step=3, photo_weight=0.01, photo_cap=3.0)
    assert np.array_equal(np.array([int(x, 16) for x in lines["cost"]], np.uint64), bits(want[0]))
    assert np.array_equal(np.array([int(x, 16) for x in lines["photo"]], np.uint64), bits(want[1]))
    full = np_search_colour_frame(case["blocks"], None, case["cam"], case["bgr"], case["depth"], anchors, rot, half=(1, 2, 0), trans_step=0.08, top_k=5, score_only=True,
                                  photo_weight=0.01, photo_cap=3.0, score=dict(step=3))
    assert np.array_equal(np.array([int(x, 16) for x in lines["lattice"]], np.uint64), bits(full["scores"]))


# ------------------------------------------------------------------ the C ABI, the mirror and the shim
def test_abi_declares_exports_and_types_the_four_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_score_colour_poses", "drf_score_colour_poses_device", "drf_search_colour_frame", "drf_search_colour_frame_device"])
    for t in ("drf_score_colour_options_t", "drf_search_colour_options_t", "drf_search_colour_entry_t", "drf_search_colour_result_t"):
        assert t in src
    for mine, theirs, size in ((ScoreColourOptions, L.ScoreColourOptions, 32), (SearchColourOptions, L.SearchColourOptions, 64),
                               (SearchColourEntry, L.SearchColourEntryStruct, 224), (SearchColourResult, L.SearchColourResultStruct, 24 + 32 * 224)):
        assert C.sizeof(mine) == C.sizeof(theirs) == size
        assert [n for n, _ in mine._fields_] == [n for n, _ in theirs._fields_]
        assert [getattr(mine, n).offset for n, _ in mine._fields_] == [getattr(theirs, n).offset for n, _ in theirs._fields_]
    lib = L.lib()
    T = (C.c_float * 16)(*np.eye(4, dtype=f32).reshape(16))
    Rr = (C.c_double * 9)(*np.eye(3).reshape(9))
    bgr, depth, cost = (C.c_uint8 * 12)(), (C.c_float * 4)(), (C.c_double * 1)()
    assert lib.drf_score_colour_poses(None, bgr, depth, T, 1, None, cost, None, None, None) == 1
    assert lib.drf_score_colour_poses_device(None, None, None, T, 1, None, cost, None, None, None) == 1
    assert lib.drf_search_colour_frame(None, bgr, depth, T, 1, Rr, 1, None, None, None, T, None, None) == 1
    assert lib.drf_search_colour_frame_device(None, None, None, T, 1, Rr, 1, None, None, None, T, None, None) == 1


def test_shim_compiles(tmp_path):
    """tandem_amd/libdr/dr_fusion.h ScoreColourPoses / SearchColourFrame as a TANDEM translation unit would call them
    (tests/cpp/map_search_colour_shim.cpp): it compiles and links against the library; tests/test_fusion_search_colour_gpu.py runs it."""
    abi_module()
    exe = str(tmp_path / "map_search_colour_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_search_colour_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert os.path.isfile(exe)
