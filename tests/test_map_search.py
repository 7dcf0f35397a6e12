"""CPU: the host half of drf_score_poses / drf_search_frame (include/dr_mi355x.h "Finds a depth frame in the map from a lattice of
poses", DESIGN.md §7c "Searching a pose lattice").  score_point, search_candidate, score_candidates_host, search_select and
search_refine of tandem_amd/csrc/pose_host.h compiled with plain g++ (tests/cpp/map_search_check.cpp) and held, bit for bit, to
np_score_poses / np_search_frame -- the reference of tests/test_fusion_map_search_gpu.py too.  The restatement is vectorised over
candidates (a lattice has 10^4 of them) and is itself held to np_system of tests/test_map_locate.py pose by pose; the refinement is
np_track_frame and np_locate_frame of the existing modules, by import.  Then: the score stage finds the scan's pose on the scene
from 52 voxels and 14 degrees off; the whole search ends on it; the status and refusal paths; the same under AddressSanitizer and
UBSan as a stand-alone program (tests/cpp/map_search_san.cpp); the five new names of the C ABI and the shim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import abi_module, check_symbols
from test_map_align import CONVERGED, LOST, MAX_ITERS, bits
from test_map_locate import NONE, SCENE_MEASURED, Camera, np_locate_frame, np_options as np_locate_options, np_system, random_case, scene_errors
from test_map_locate import Options as LocateOptions
from test_map_track import Options as TrackOptions
from test_map_track import RENDER_FN, np_track_frame, track_opts, track_scene
from test_map_transform import motion, rotation, sorted_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p, u32p, u64p, f32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_double)
f32, f64 = np.float32, np.float64
VS, H, W = 0.02, 96, 128
MAX_TOP = 32
_LANES = np.arange(64)


# ------------------------------------------------------------------ the rule, restated
def np_score_options(cam, **opt):
    """drf_score_options_t with its defaults: a zero (or missing) field is its default."""
    o = dict(step=4, min_weight=1, band=f32(cam["truncation_distance"]), huber=f32(1.0), outside_cost=f32(0.0), unobserved_cost=f32(0.0))
    for k, v in opt.items():
        assert k in o, k
        if v:
            o[k] = int(v) if k in ("step", "min_weight") else f32(v)
    o["oc"] = f64(o["outside_cost"]) if o["outside_cost"] else f64(o["huber"]) * (f64(o["band"]) / f64(f32(cam["voxel_size"])))
    o["uc"] = f64(o["unobserved_cost"]) if o["unobserved_cost"] else 2.0 * o["oc"]
    return o


def np_points(cam, depth, step):
    """The grid positions of all groups (512 each, the last padded): which are samples, and their points g (three float64 arrays),
    as np_system's first lines state them."""
    Wd, Hd = int(cam["width"]), int(cam["height"])
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
    g = [(((u.astype(f64) - f64(f32(cam["cx"]))) / f64(f32(cam["fx"]))) * z) / vs64, (((v.astype(f64) - f64(f32(cam["cy"]))) / f64(f32(cam["fy"]))) * z) / vs64, z / vs64]
    return sample, g, groups


class MapIndex:
    """The map as a dense array of block indices over the blocks' bounding box: the voxel at a lattice point in one gather, for
    millions of points at once.  A block outside the box is absent, as one outside the key range is."""

    def __init__(self, blocks):
        coords, vox = np.asarray(blocks[0], np.int64).reshape(-1, 3), np.asarray(blocks[1], np.uint8)
        self.n = len(coords)
        if self.n == 0:
            return
        self.lo = coords.min(0)
        self.shape = coords.max(0) - self.lo + 1
        self.grid = np.full(self.shape, -1, np.int64)
        self.grid[tuple((coords - self.lo).T)] = np.arange(self.n)
        v = vox.reshape(self.n, 512, 8)
        self.sdf = np.ascontiguousarray(v[:, :, :4]).view(f32)[:, :, 0]
        self.weight = v[:, :, 7].astype(np.int64)

    def fetch(self, p):
        """(sdf float32, weight) of the voxels at the lattice points p (..., 3) int64; an absent block: weight 0"""
        if self.n == 0:
            return np.zeros(p.shape[:-1], f32), np.zeros(p.shape[:-1], np.int64)
        rel = (p >> 3) - self.lo
        ok = ((rel >= 0) & (rel < self.shape)).all(-1)
        rel = np.where(ok[..., None], rel, 0)
        idx = self.grid[rel[..., 0], rel[..., 1], rel[..., 2]]
        found = ok & (idx >= 0)
        idx = np.where(found, idx, 0)
        vi = ((p[..., 0] & 7) << 6) | ((p[..., 1] & 7) << 3) | (p[..., 2] & 7)
        return np.where(found, self.sdf[idx, vi], f32(0)), np.where(found, self.weight[idx, vi], 0)


def _butterfly(x):
    """x = x + x[lane ^ off] for off = 32 .. 1 along the last axis (64 lanes)"""
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[..., _LANES ^ off]
    return x


def np_score_candidates(blocks, cam, depth, R, tv, o, batch=256):
    """cost (C,) float64, counts (C, 4) = samples, valid, unobserved, outside, score (C,) float64 of the poses (R (C, 3, 3), tv (C, 3)
    in lattice units, float64).  One float64 / float32 array operation per operation of the rule, over a batch of candidates and all
    grid positions at once: np_system's lines up to phi, then the one sum in its order."""
    index = blocks if isinstance(blocks, MapIndex) else MapIndex(blocks)
    sample, g, groups = np_points(cam, depth, o["step"])
    vs64, hub = f64(f32(cam["voxel_size"])), f64(o["huber"])
    R, tv = np.asarray(R, f64).reshape(-1, 3, 3), np.asarray(tv, f64).reshape(-1, 3)
    n = len(R)
    cost, counts = np.zeros(n, f64), np.zeros((n, 4), np.int64)
    corners = [(cx, cy, cz) for cx in range(2) for cy in range(2) for cz in range(2)]
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
        for cx, cy, cz in corners:
            sd, wt = index.fetch(bi + np.array([cx, cy, cz]))
            observed &= wt >= o["min_weight"]
            s[cx, cy, cz] = sd
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
        t = t.reshape(c, groups, 8, 64)                                   # position 512 i + l + 64 k -> [i][k][l]
        acc = np.zeros((c, groups, 64), f64)
        for k in range(8):
            acc = acc + t[:, :, k]
        partial = _butterfly(acc)[..., 0]                                 # (c, groups)
        rows = np.concatenate([partial, np.zeros((c, -groups % 64), f64)], axis=1).reshape(c, -1, 64)   # rows[j][l] = partial[l + 64 j]
        lane = np.zeros((c, 64), f64)
        for j in range(rows.shape[1]):
            lane = lane + rows[:, j]
        cost[at:at + c] = _butterfly(lane)[:, 0]
        counts[at:at + c] = np.stack([np.full(c, sample.sum()), valid.sum(1), (sample[None] & ~observed).sum(1), outside.sum(1)], axis=1)
    assert (counts[:, 0] == counts[:, 1:].sum(1)).all()
    with np.errstate(all="ignore"):
        score = np.where(counts[:, 0] == 0, o["uc"], ((cost + o["oc"] * counts[:, 3].astype(f64)) + o["uc"] * counts[:, 2].astype(f64)) / counts[:, 0].astype(f64))
    return cost, counts, score


def np_score_poses(blocks, cam, depth, poses, **opt):
    poses = np.ascontiguousarray(poses, f32).reshape(-1, 4, 4)
    mv = [motion(p, cam["voxel_size"]) for p in poses]
    return np_score_candidates(blocks, cam, depth, np.stack([m[0] for m in mv]), np.stack([m[1] for m in mv]), np_score_options(cam, **opt))


def np_candidates(cam, anchors, rotations, half, trans_step=0.0):
    """(R (C, 3, 3), tv (C, 3)) of the lattice in index order c = (((a n_rot + r) Nx + ix) Ny + iy) Nz + iz: Rd = Rr Ra entry by entry
    in the rule's order, tv_k = ta_k + (double)(i_k - half_k) * ((double)trans_step / vs)."""
    anchors = np.ascontiguousarray(anchors, f32).reshape(-1, 4, 4)
    rot = np.ascontiguousarray(rotations, f64).reshape(-1, 3, 3)
    ts = f32(trans_step) if trans_step else f32(2.0) * f32(cam["truncation_distance"])
    dstep = f64(ts) / f64(f32(cam["voxel_size"]))
    offs = np.stack(np.meshgrid(*[np.arange(-h, h + 1) for h in half], indexing="ij"), axis=-1).reshape(-1, 3).astype(f64)
    Rs, ts_ = [], []
    for A in anchors:
        Ra, ta = motion(A, cam["voxel_size"])
        for Rr in rot:
            Rd = np.array([[(Rr[i, 0] * Ra[0, j] + Rr[i, 1] * Ra[1, j]) + Rr[i, 2] * Ra[2, j] for j in range(3)] for i in range(3)], f64)
            Rs.append(np.broadcast_to(Rd, (len(offs), 3, 3)))
            ts_.append(ta[None] + offs * dstep)
    return np.concatenate(Rs), np.concatenate(ts_)


def candidate_pose16(cam, R, tv):
    """locate_pose16: the float pose of (R, tv)"""
    T = np.eye(4, dtype=f32)
    T[:3, :3] = R.astype(f32)
    T[:3, 3] = (tv * f64(f32(cam["voxel_size"]))).astype(f32)
    return T


def np_select(score, top_k):
    """the top_k smallest scores, ties to the lower index, a NaN behind every number"""
    key = np.where(np.isnan(score), np.inf, score)
    return np.lexsort((np.arange(len(score)), key))[:top_k]


def np_search_frame(blocks, render, cam, depth, anchors, rotations, half=(0, 0, 0), trans_step=0.0, top_k=0, score_only=False, accept_valid=0.0, score=None,
                    track=None, locate=None, index=None):
    """drf_search_frame: dict(status, winner, refined, n_candidates, T32 the pose handed out, scores, entries), an entry a dict
    shaped like drf_search_entry_t.  index: the MapIndex of blocks, if the caller has one."""
    o = np_score_options(cam, **(score or {}))
    R, tv = np_candidates(cam, anchors, rotations, half, trans_step)
    cost, counts, sc = np_score_candidates(index or blocks, cam, depth, R, tv, o)
    sel = np_select(sc, top_k or 8)
    p16 = [candidate_pose16(cam, R[c], tv[c]) for c in sel]
    entries = [dict(index=int(c), score=float(sc[c]), cost=float(cost[c]), counts=tuple(int(v) for v in counts[c]), track_status=-1, locate_status=-1, samples=0,
                    valid=0, located_cost=0.0, T=p16[k].astype(f64)) for k, c in enumerate(sel)]
    out = dict(status=LOST, winner=-1, refined=0, n_candidates=len(sc), T32=p16[0], scores=sc, entries=entries)
    if score_only:
        out.update(status=MAX_ITERS, winner=0)
        return out
    for k, en in enumerate(entries):
        tr = np_track_frame(render, cam, depth, p16[k], **(track or {}))
        out["refined"] += 1
        en.update(track_status=tr["status"], T=tr["T"])
        if tr["status"] > MAX_ITERS:
            continue
        lr = np_locate_frame(blocks, cam, depth, tr["T"].astype(f32), **(locate or {}))
        en.update(locate_status=lr["status"], samples=lr["samples"], valid=lr["valid"], located_cost=lr["cost"], T=lr["T"])
        if lr["status"] > MAX_ITERS:
            continue
        w = entries[out["winner"]] if out["winner"] >= 0 else None
        if w is None or en["valid"] > w["valid"] or (en["valid"] == w["valid"] and en["located_cost"] < w["located_cost"]):
            out["winner"] = k
        if accept_valid > 0.0 and float(en["valid"]) >= accept_valid * float(en["samples"]):
            out["winner"] = k
            break
    if out["winner"] >= 0:
        out.update(status=entries[out["winner"]]["locate_status"], T32=entries[out["winner"]]["T"].astype(f32))
    return out


# ------------------------------------------------------------------ the compiled host half
class ScoreOptions(C.Structure):
    """drf_score_options_t"""
    _fields_ = [("step", C.c_int), ("min_weight", C.c_int), ("band", C.c_float), ("huber", C.c_float), ("outside_cost", C.c_float), ("unobserved_cost", C.c_float)]


class SearchOptions(C.Structure):
    """drf_search_options_t"""
    _fields_ = [("score", ScoreOptions), ("trans_step", C.c_float), ("half", C.c_int * 3), ("top_k", C.c_int), ("score_only", C.c_int), ("accept_valid", C.c_double)]


class SearchEntry(C.Structure):
    """drf_search_entry_t"""
    _fields_ = [("index", C.c_uint64), ("score", C.c_double), ("cost", C.c_double), ("counts", C.c_uint32 * 4), ("track_status", C.c_int), ("locate_status", C.c_int),
                ("samples", C.c_uint64), ("valid", C.c_uint64), ("located_cost", C.c_double), ("T", C.c_double * 16)]


class SearchResult(C.Structure):
    """drf_search_result_t"""
    _fields_ = [("status", C.c_int), ("n_entries", C.c_int), ("winner", C.c_int), ("refined", C.c_int), ("n_candidates", C.c_uint64), ("entries", SearchEntry * MAX_TOP)]


def search_options(half=(0, 0, 0), trans_step=0.0, top_k=0, score_only=False, accept_valid=0.0, score=None):
    return SearchOptions(score=ScoreOptions(**(score or {})), trans_step=trans_step, half=(C.c_int * 3)(*half), top_k=top_k, score_only=int(score_only),
                         accept_valid=accept_valid)


def build_check(directory):
    so = os.path.join(str(directory), "libmap_search_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_search_check.cpp"), "-o", so])
    h = C.CDLL(so)
    head = [u64p, u8p, C.c_size_t, C.POINTER(Camera), f32p]
    h.ms_options.argtypes = [C.POINTER(SearchOptions), C.c_float, C.c_float, f64p, C.c_char_p]
    h.ms_point.argtypes = head + [f32p, C.POINTER(ScoreOptions), u64p]
    h.ms_score.argtypes = head + [f32p, C.c_size_t, C.POINTER(ScoreOptions), f64p, u32p, f64p]
    h.ms_search.argtypes = head + [RENDER_FN, C.c_void_p, f32p, C.c_size_t, f64p, C.c_size_t, C.POINTER(SearchOptions), C.POINTER(TrackOptions),
                                   C.POINTER(LocateOptions), f32p, C.POINTER(SearchResult), f64p, C.c_char_p]
    return h


@pytest.fixture(scope="module")
def HS(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("map_search"))


def _head(blocks, cam, depth):
    rk, rv = sorted_source(*blocks)
    depth = np.ascontiguousarray(depth, f32)
    assert depth.size == cam["height"] * cam["width"]
    cm = Camera(**cam)
    return (rk, rv, depth, cm), [rk.ctypes.data_as(u64p), rv.ctypes.data_as(u8p), len(rk), C.byref(cm), depth.ctypes.data_as(f32p)]


def cpp_score(HS, blocks, cam, depth, poses, expect=0, **opt):
    keep, head = _head(blocks, cam, depth)
    poses = np.ascontiguousarray(poses, f32).reshape(-1, 16)
    n = len(poses)
    cost, counts, score = np.zeros(n, f64), np.zeros((n, 4), np.uint32), np.zeros(n, f64)
    rc = HS.ms_score(*head, poses.ctypes.data_as(f32p), n, C.byref(ScoreOptions(**opt)), cost.ctypes.data_as(f64p), counts.ctypes.data_as(u32p), score.ctypes.data_as(f64p))
    assert rc == expect, rc
    return cost, counts.astype(np.int64), score


def entry_dict(e):
    return dict(index=int(e.index), score=float(e.score), cost=float(e.cost), counts=tuple(int(v) for v in e.counts), track_status=int(e.track_status),
                locate_status=int(e.locate_status), samples=int(e.samples), valid=int(e.valid), located_cost=float(e.located_cost), T=np.array(e.T, f64).reshape(4, 4))


def result_dict(r, T32, scores):
    return dict(status=int(r.status), winner=int(r.winner), refined=int(r.refined), n_candidates=int(r.n_candidates), T32=np.array(T32, f32).reshape(4, 4), scores=scores,
                entries=[entry_dict(e) for e in r.entries[:r.n_entries]])


def cpp_search(HS, blocks, render, cam, depth, anchors, rotations, track=None, locate=None, expect=0, **search):
    """search_refine over the host's track and locate and the Python renderer, as a dict shaped like np_search_frame's; a refused
    call returns (code, name)."""
    keep, head = _head(blocks, cam, depth)
    anchors = np.ascontiguousarray(anchors, f32).reshape(-1, 16)
    rot = np.ascontiguousarray(rotations, f64).reshape(-1, 9)
    npix = cam["height"] * cam["width"]

    def call(p16, out, user):
        d = np.ascontiguousarray(render(np.ctypeslib.as_array(p16, (16,)).reshape(4, 4).copy()), f32)
        C.memmove(out, d.ctypes.data, npix * 4)

    so = search_options(**search)
    n = len(anchors) * len(rot) * int(np.prod([2 * h + 1 for h in so.half]))
    scores = np.zeros(max(n, 1) if 0 < n <= 1 << 24 else 1, f64)
    T32, r, name = np.zeros(16, f32), SearchResult(), C.create_string_buffer(32)
    rc = HS.ms_search(*head, RENDER_FN(call), None, anchors.ctypes.data_as(f32p), len(anchors), rot.ctypes.data_as(f64p), len(rot), C.byref(so),
                      C.byref(TrackOptions(**(track or {}))), C.byref(LocateOptions(**(locate or {}))), T32.ctypes.data_as(f32p), C.byref(r), scores.ctypes.data_as(f64p), name)
    assert rc == expect, (rc, name.value)
    return result_dict(r, T32, scores) if rc == 0 else (rc, name.value.decode())


def assert_same_scores(got, want, what):
    assert np.array_equal(np.asarray(got[1], np.int64), np.asarray(want[1], np.int64)), f"{what}: counts differ"
    for k, name in ((0, "cost"), (2, "score")):
        bad = np.flatnonzero(bits(got[k]) != bits(want[k]))
        assert bad.size == 0, f"{what}: {name} differs at {bad[:5].tolist()}: got {got[k][bad[:3]]} want {want[k][bad[:3]]}"


def assert_same_search(got, want, what):
    """two results of the search (dicts shaped like np_search_frame's), bit for bit"""
    for k in ("status", "winner", "refined", "n_candidates"):
        assert got[k] == want[k], f"{what}: {k} {got[k]} against {want[k]}"
    assert np.array_equal(got["T32"].view(np.uint32), want["T32"].view(np.uint32)), f"{what}: the pose differs"
    if got["scores"] is not None and want["scores"] is not None:
        assert np.array_equal(bits(got["scores"]), bits(want["scores"])), f"{what}: all_scores differ"
    assert len(got["entries"]) == len(want["entries"]), what
    for i, (a, b) in enumerate(zip(got["entries"], want["entries"])):
        for k in ("index", "counts", "track_status", "locate_status", "samples", "valid"):
            assert a[k] == b[k], f"{what}: entry {i} {k} {a[k]} against {b[k]}"
        for k in ("score", "cost", "located_cost", "T"):
            assert np.array_equal(bits(a[k]), bits(b[k])), f"{what}: entry {i} {k} differs: {a[k]} against {b[k]}"


# ------------------------------------------------------------------ poses and lattices
def random_poses(case, n, seed=5):
    """n poses around the random map's: turned by up to 12 degrees and moved by up to 20 voxels; every seventh looks away (turned by
    180 degrees about y: it sees nothing), every eleventh sits 300 blocks off."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        T = np.array(case["pose"], f64)
        T[:3, :3] = rotation(rng.normal(size=3), rng.uniform(0, 12)) @ T[:3, :3]
        T[:3, 3] += rng.uniform(-20, 20, 3) * VS
        if i % 7 == 3:
            T[:3, :3] = rotation((0, 1, 0), 180.0) @ T[:3, :3]
        if i % 11 == 5:
            T[:3, 3] += 300 * 8 * VS
        out.append(T.astype(f32))
    return np.stack(out)


def small_lattice(case):
    """2 anchors x 3 rotations x (3 x 5 x 2... half (1, 2, 0) gives 3 x 5 x 1) around the random map's pose, 4-voxel steps"""
    a0 = np.array(case["pose"], f32)
    a1 = a0.copy()
    a1[:3, 3] += f32(0.11)
    from tandem_amd.dr_fusion import pose_rotations
    return np.stack([a0, a1]), pose_rotations([-5.0, 0.0, 5.0])


# ------------------------------------------------------------------ the score against the restatement
def test_the_vectorised_restatement_is_np_system(HS):
    """np_score_candidates against np_system of tests/test_map_locate.py, pose by pose: cost = sums[27] and the four counts, bit for
    bit, at steps 1, 3 and 4 -- what makes the fast restatement the existing one."""
    case = random_case(3)
    poses = random_poses(case, 9)
    for step in (1, 3, 4):
        got = np_score_poses(case["blocks"], case["cam"], case["depth"], poses, step=step)
        for i, p in enumerate(poses):
            R, tv = motion(p, VS)
            sums, c4 = np_system(case["blocks"], case["cam"], case["depth"], R, tv, np_locate_options(case["cam"], step=step))
            assert tuple(got[1][i]) == c4, (step, i)
            assert bits(got[0][i]) == bits(sums[27]), (step, i)
        assert got[1][:, 1].max() > 30 and (got[1][:, 1] == 0).any()


SCORE_CASES = [("step 1", dict(step=1)), ("step 3", dict(step=3)), ("defaults (step 4)", {}), ("step 1, min_weight 3, tight huber, narrow band", dict(step=1, min_weight=3, huber=0.25, band=0.03)),
               ("costs given", dict(outside_cost=0.5, unobserved_cost=7.0))]


@pytest.mark.parametrize("name,opt", SCORE_CASES, ids=[c[0] for c in SCORE_CASES])
def test_score_against_the_restatement_on_random_maps(HS, name, opt):
    case = random_case(3)
    poses = random_poses(case, 40)
    want = np_score_poses(case["blocks"], case["cam"], case["depth"], poses, **opt)
    assert_same_scores(cpp_score(HS, case["blocks"], case["cam"], case["depth"], poses, **opt), want, name)
    assert want[1][:, 1].max() > (10 if "band" in opt else 30) and (want[1][:, 1] == 0).any() and (want[1][:, 2] > 0).all()
    if "band" in opt:
        assert want[1][:, 3].max() > 20


def test_poses_that_see_nothing_an_image_without_a_sample_and_an_empty_map(HS):
    case = random_case(4)
    poses = random_poses(case, 8)
    o = np_score_options(case["cam"])
    for name, blocks, depth in (("no samples", case["blocks"], np.zeros((H, W), f32)), ("NaN only", case["blocks"], np.full((H, W), np.nan, f32)),
                                ("empty map", NONE, case["depth"])):
        want = np_score_poses(blocks, case["cam"], depth, poses)
        got = cpp_score(HS, blocks, case["cam"], depth, poses)
        assert_same_scores(got, want, name)
        assert not got[0].any() and not got[1][:, 1].any()
        if name == "empty map":
            assert (got[1][:, 0] > 100).all() and (got[1][:, 2] == got[1][:, 0]).all() and (got[2] == o["uc"]).all()
        else:
            assert not got[1].any() and (got[2] == o["uc"]).all()
    away = np_score_poses(case["blocks"], case["cam"], case["depth"], poses[3:4])
    assert away[1][0, 1] == 0 and away[2][0] == o["uc"]
    assert o["oc"] == 4.0 and o["uc"] == 8.0


def test_far_blocks(HS):
    case = random_case(3, shift=(300, -270, 5))
    poses = random_poses(case, 12)
    want = np_score_poses(case["blocks"], case["cam"], case["depth"], poses)
    assert_same_scores(cpp_score(HS, case["blocks"], case["cam"], case["depth"], poses), want, "far")
    assert want[1][:, 1].max() > 10


def test_score_point_is_align_point(HS):
    """score_point against align_point<true> sample by sample on the host: the same code and the same bits in the one sum it keeps."""
    case = random_case(3)
    keep, head = _head(case["blocks"], case["cam"], case["depth"])
    for k, p in enumerate(random_poses(case, 12)):
        for opt in (dict(step=1), dict(step=1, min_weight=3, huber=0.25, band=0.03)):
            seen = np.zeros(4, np.uint64)
            bad = HS.ms_point(*head, np.ascontiguousarray(p, f32).ctypes.data_as(f32p), C.byref(ScoreOptions(**opt)), seen.ctypes.data_as(u64p))
            assert bad == 0, (k, opt, bad)
            assert seen[3] > 5000 and seen[3] == seen[:3].sum()
            if k == 0:
                assert seen[1] > 100 and seen[0] > 0


def test_lattice_against_the_restatement(HS):
    """The candidates' poses and their order: all_scores of a 2 x 3 x (3 x 5 x 1) lattice, and its entries, score stage alone."""
    case = random_case(3)
    anchors, rot = small_lattice(case)
    kw = dict(half=(1, 2, 0), trans_step=0.08, top_k=5, score_only=True, score=dict(step=3))
    want = np_search_frame(case["blocks"], None, case["cam"], case["depth"], anchors, rot, **kw)
    got = cpp_search(HS, case["blocks"], None, case["cam"], case["depth"], anchors, rot, **kw)
    assert_same_search(got, want, "lattice")
    assert got["n_candidates"] == 90 and len(got["entries"]) == 5 and got["status"] == MAX_ITERS and got["winner"] == 0
    assert [e["score"] for e in got["entries"]] == sorted(got["scores"])[:5]
    assert len(np.unique(bits(got["scores"]))) > 60


def test_options_and_their_defaults(HS):
    out, name = np.zeros(13, f64), C.create_string_buffer(32)
    tr, vs = f32(0.08), f32(0.02)
    assert HS.ms_options(None, tr, vs, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [4, 1, float(tr), 1.0, float(f64(tr) / f64(vs)), 2.0 * float(f64(tr) / f64(vs)), float(f64(f32(2.0) * tr) / f64(vs)), 1, 1, 1, 8, 0, 0.0]
    full = search_options(half=(1, 2, 3), trans_step=0.1, top_k=32, score_only=True, accept_valid=0.5,
                          score=dict(step=2, min_weight=3, band=0.05, huber=2.0, outside_cost=1.5, unobserved_cost=2.5))
    assert HS.ms_options(C.byref(full), tr, vs, out.ctypes.data_as(f64p), name) == 0
    assert out.tolist() == [2, 3, float(f32(0.05)), 2.0, 1.5, 2.5, float(f64(f32(0.1)) / f64(vs)), 3, 5, 7, 32, 1, 0.5]
    for bad, which in ((dict(score=dict(step=-1)), "step"), (dict(score=dict(min_weight=-1)), "min_weight"), (dict(score=dict(band=-1.0)), "band"),
                       (dict(score=dict(huber=float("nan"))), "huber"), (dict(score=dict(outside_cost=-1.0)), "outside_cost"),
                       (dict(score=dict(unobserved_cost=float("inf"))), "unobserved_cost"), (dict(trans_step=-0.1), "trans_step"), (dict(half=(0, -1, 0)), "half"),
                       (dict(top_k=33), "top_k"), (dict(top_k=-1), "top_k"), (dict(accept_valid=-0.5), "accept_valid"), (dict(accept_valid=float("nan")), "accept_valid")):
        assert HS.ms_options(C.byref(search_options(**bad)), tr, vs, out.ctypes.data_as(f64p), name) == 1, bad
        assert name.value.decode() == which


# ------------------------------------------------------------------ meaning: the scene
# The anchor of the scene tests: the scan's pose turned 14 degrees about world y, then -3 degrees about world x, and moved
# (37, -22, 29) voxels: 51.9 voxels and 14.3 degrees off.  Rounded to float.
ANCHOR_OFF = (37.0, -22.0, 29.0)
SCENE_STEP = 4
# measured on the restatement with the double candidate poses (degrees, voxels): the best candidate, the worst of the 8 best
SCORE_BEST = (2.2360, 4.6904)
SCORE_TOP8 = (3.6054, 13.4907)


def scene_anchor(s):
    T = np.array(s["pose"], f64)
    T[:3, :3] = rotation((1, 0, 0), -3.0) @ rotation((0, 1, 0), 14.0) @ T[:3, :3]
    T[:3, 3] += np.array(ANCHOR_OFF) * f64(f32(VS))
    return T.astype(f32)


def candidate_errors(cam, R, tv, pose):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = tv * f64(f32(cam["voxel_size"]))
    return scene_errors(T, pose)


@pytest.fixture(scope="module")
def scene_map():
    s = track_scene()
    s["index"] = MapIndex(s["blocks"])
    return s


def scene_lattice():
    from tandem_amd.dr_fusion import pose_rotations
    return pose_rotations([-20.0, -16.0, -12.0, -8.0], [0.0, 4.0]), (5, 5, 5)


def test_the_score_finds_the_scan_pose_on_the_scene(scene_map):
    """The point of the score.  synth.scene seed 11 at 96x128, one scan, 1968 blocks; the anchor 52 voxels and 14.3 degrees off the
    scan's pose; rotations yaw {-20, -16, -12, -8} x pitch {0, 4} about the world axes, half (5, 5, 5), 8-voxel steps (2 x the
    truncation), pixel step 4 (752 samples): 10 648 candidates.  The lattice does not contain the scan's pose: its nearest point is
    (-3, 2, -3) voxels = 4.69 voxels and 2.24 degrees off (the anchor's 14 and -3 degrees against -16 / -12 and 4 / 0).
    MEASURED on the restatement with the double candidate poses (SCORE_BEST, SCORE_TOP8): the best-scoring candidate is that
    nearest point, 4.6904 voxels and 2.2360 degrees off (score 3.7374 voxels per sample, 503 of 752 valid); the 8 best are all within
    13.4907 voxels and 3.6054 degrees.  Asserted
    with the bounds the design set before measuring: the best within 10 voxels and 5 degrees -- inside what drf_track_frame
    converges from (tests/test_map_track.py: 8 voxels / 4 degrees converges, 12 / 6 still creeps in) -- the 8 best within 20 voxels
    and 8 degrees."""
    s = scene_map
    anchor = scene_anchor(s)
    a0, t0 = scene_errors(anchor.astype(f64), s["pose"])
    assert abs(t0 - 51.9) < 0.1 and abs(a0 - 14.3) < 0.1, (a0, t0)
    rot, half = scene_lattice()
    R, tv = np_candidates(s["cam"], anchor[None], rot, half)
    assert len(R) == 10648
    cost, counts, score = np_score_candidates(s["index"], s["cam"], s["depth"], R, tv, np_score_options(s["cam"], step=SCENE_STEP))
    assert counts[0, 0] == 752
    top = np_select(score, 8)
    errs = [candidate_errors(s["cam"], R[c], tv[c], s["pose"]) for c in top]
    for c, (a, t) in zip(top, errs):
        print("candidate %5d: score %.4f, %d of %d valid, %.4f degrees %.4f voxels off" % (c, score[c], counts[c, 1], counts[c, 0], a, t))
    dist = np.linalg.norm(tv - np.asarray(s["pose"], f64)[:3, 3] / f64(f32(VS)), axis=1)
    print("nearest lattice points: %.4f voxels, candidates %s" % (dist.min(), np.flatnonzero(dist == dist.min()).tolist()))
    assert errs[0][1] <= 10.0 and errs[0][0] <= 5.0, errs[0]
    assert max(e[1] for e in errs) <= 20.0 and max(e[0] for e in errs) <= 8.0, errs
    assert abs(errs[0][0] - SCORE_BEST[0]) < 1e-3 and abs(errs[0][1] - SCORE_BEST[1]) < 1e-3, errs[0]
    assert abs(max(e[0] for e in errs) - SCORE_TOP8[0]) < 1e-3 and abs(max(e[1] for e in errs) - SCORE_TOP8[1]) < 1e-3, errs


# the end-to-end lattice: 2 x 2 rotations x 3 x 3 x 3 offsets about the offset (-40, 24, -32) voxels from the anchor
def end_to_end_case(s):
    from tandem_amd.dr_fusion import pose_rotations
    anchor = scene_anchor(s)
    anchor[:3, 3] = (anchor[:3, 3].astype(f64) + np.array([-40.0, 24.0, -32.0]) * f64(f32(VS))).astype(f32)
    return anchor[None], pose_rotations([-16.0, -12.0], [0.0, 4.0]), dict(half=(1, 1, 1), top_k=3, score=dict(step=SCENE_STEP), track=track_opts(s),
                                                                          locate=dict(centre_depth=s["centre_depth"]))


def test_the_search_ends_on_the_scan_pose(HS, scene_map):
    """End to end on the CPU, the oracle's ray-cast the renderer: 108 candidates around the winner of the score stage, the 3 best
    tracked and located.  The winner ends CONVERGED within 2 x SCENE_MEASURED of the scan's pose -- the bound of
    test_integrated_scene_recovers_the_scan_pose, the last stage being that very minimisation -- the host equals the restatement
    bit for bit, and the entry table is in ascending score with the winner the rule names."""
    s = scene_map
    anchors, rot, kw = end_to_end_case(s)
    want = np_search_frame(s["blocks"], s["render"], s["cam"], s["depth"], anchors, rot, index=s["index"], **kw)
    for k, e in enumerate(want["entries"]):
        a, t = scene_errors(e["T"], s["pose"])
        print("entry %d: candidate %d score %.4f track %d locate %d, %d of %d valid, cost %.4g, %.4f degrees %.4f voxels off" %
              (k, e["index"], e["score"], e["track_status"], e["locate_status"], e["valid"], e["samples"], e["located_cost"], a, t))
    assert want["n_candidates"] == 108 and want["refined"] == 3 and want["status"] == CONVERGED
    a, t = scene_errors(want["T32"].astype(f64), s["pose"])
    assert a <= 2 * SCENE_MEASURED[0] and t <= 2 * SCENE_MEASURED[1], (a, t)
    scores = [e["score"] for e in want["entries"]]
    assert scores == sorted(scores) and scores == sorted(want["scores"])[:3]
    ok = [k for k, e in enumerate(want["entries"]) if 0 <= e["locate_status"] <= MAX_ITERS]
    assert want["winner"] == min(ok, key=lambda k: (-want["entries"][k]["valid"], want["entries"][k]["located_cost"], k))
    sblocks = s["blocks"]
    got = cpp_search(HS, sblocks, s["render"], s["cam"], s["depth"], anchors, rot, **kw)
    assert_same_search(got, want, "end to end")


def test_accept_valid_stops_early(HS, scene_map):
    s = scene_map
    anchors, rot, kw = end_to_end_case(s)
    kw["accept_valid"] = 0.5
    want = np_search_frame(s["blocks"], s["render"], s["cam"], s["depth"], anchors, rot, index=s["index"], **kw)
    got = cpp_search(HS, s["blocks"], s["render"], s["cam"], s["depth"], anchors, rot, **kw)
    assert_same_search(got, want, "accept_valid")
    assert got["refined"] == 1 and got["winner"] == 0 and got["status"] == CONVERGED
    assert got["entries"][1]["track_status"] == -1 and got["entries"][2]["locate_status"] == -1
    assert got["entries"][0]["valid"] >= 0.5 * got["entries"][0]["samples"]


# ------------------------------------------------------------------ status and refusal paths
def test_a_map_far_away_is_lost(HS, scene_map):
    s = scene_map
    far = (s["blocks"][0] + np.array([50, 0, 0], np.int64), s["blocks"][1])
    anchors, rot, kw = end_to_end_case(s)
    kw.update(top_k=2)
    miss = lambda p: np.zeros((H, W), f32)   # a ray-cast of a map 50 blocks away finds nothing
    want = np_search_frame(far, miss, s["cam"], s["depth"], anchors, rot, **kw)
    got = cpp_search(HS, far, miss, s["cam"], s["depth"], anchors, rot, **kw)
    assert_same_search(got, want, "far")
    assert got["status"] == LOST and got["winner"] == -1 and got["refined"] == 2
    assert all(e["track_status"] == LOST and e["locate_status"] == -1 for e in got["entries"])
    R, tv = np_candidates(s["cam"], anchors, rot, kw["half"])
    assert got["entries"][0]["index"] == 0 and np.array_equal(got["T32"], candidate_pose16(s["cam"], R[0], tv[0]))   # all scores tie: the lowest index


def test_refusals(HS):
    case = random_case(3)
    anchors, rot = small_lattice(case)
    args = (HS, case["blocks"], None, case["cam"], case["depth"])
    assert cpp_search(*args, anchors, rot, expect=1, top_k=33) == (1, "top_k")
    assert cpp_search(*args, anchors, rot, expect=1, half=(0, 0, -2)) == (1, "half")
    assert cpp_search(*args, anchors, rot, expect=1, score=dict(huber=-1.0)) == (1, "huber")
    assert cpp_search(*args, anchors, rot, expect=1, track=dict(max_renders=-1)) == (1, "max_renders")
    assert cpp_search(*args, anchors, rot, expect=1, locate=dict(eps_rot=-1.0)) == (1, "eps_rot")
    assert cpp_search(*args, anchors[:0], rot, expect=3)[0] == 3
    assert cpp_search(*args, anchors, rot[:0], expect=3)[0] == 3
    assert cpp_search(*args, anchors, rot, expect=3, half=(200, 200, 200))[0] == 3          # 401^3 x 6 > 2^24
    scaled, nan = anchors.copy(), anchors.copy()
    scaled[1, :3, :3] *= 1.01
    nan[0, 2, 3] = np.nan
    assert cpp_search(*args, scaled, rot, expect=2) [1].startswith("anchor 1 is not a rigid motion")
    assert cpp_search(*args, nan, rot, expect=2)[1].startswith("anchor 0 has a non-finite")
    mirror, skew = rot.copy(), rot.copy()
    mirror[2] = np.diag([1.0, -1.0, 1.0]).reshape(9)
    skew[1, 0] = 1.1
    assert cpp_search(*args, anchors, mirror, expect=2)[1].startswith("rotation 2 is a reflection")
    assert cpp_search(*args, anchors, skew, expect=2)[1].startswith("rotation 1 is not a rigid")
    poses = random_poses(case, 3)
    poses[1, :3, :3] *= 1.01
    cpp_score(HS, case["blocks"], case["cam"], case["depth"], poses, expect=2)
    cpp_score(HS, case["blocks"], case["cam"], case["depth"], poses[:1], expect=1, band=-1.0)


def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """score_candidates_host and search_refine under AddressSanitizer and UBSan: a plain executable with its own main, nothing
    preloaded, nothing loaded into Python.  It reads a case from a file -- the random map, 21 poses, a lattice -- and prints the
    costs, which are the restatement's bit for bit."""
    exe, data = str(tmp_path / "map_search_san"), str(tmp_path / "case.bin")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_search_san.cpp"), "-o", exe])
    case = random_case(3)
    poses = random_poses(case, 21).reshape(-1, 16)
    anchors, rot = small_lattice(case)
    rk, rv = sorted_source(*case["blocks"])
    with open(data, "wb") as fh:
        fh.write(np.uint64(len(rk)).tobytes() + rk.tobytes() + rv.tobytes() + bytes(Camera(**case["cam"])))
        fh.write(np.ascontiguousarray(case["depth"], f32).tobytes() + np.uint64(len(poses)).tobytes() + poses.tobytes())
        fh.write(np.uint64(len(anchors)).tobytes() + anchors.tobytes() + np.uint64(len(rot)).tobytes() + rot.tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_search_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith(("score", "lattice"))}
    want = np_score_poses(case["blocks"], case["cam"], case["depth"], poses, step=3)
    assert np.array_equal(np.array([int(x, 16) for x in lines["score"]], np.uint64), bits(want[0]))
    full = np_search_frame(case["blocks"], None, case["cam"], case["depth"], anchors, rot, half=(1, 2, 0), trans_step=0.08, top_k=5, score_only=True, score=dict(step=3))
    assert np.array_equal(np.array([int(x, 16) for x in lines["lattice"]], np.uint64), bits(full["scores"]))


# ------------------------------------------------------------------ the C ABI, the mirror and the shim
def test_abi_declares_exports_and_types_the_five_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_score_poses", "drf_score_poses_device", "drf_search_frame", "drf_search_frame_device", "drf_search_stats"])
    assert "drf_score_options_t" in src and "drf_search_options_t" in src and "drf_search_result_t" in src and "#define DRF_SEARCH_MAX_TOP 32" in src
    for mine, theirs, size in ((ScoreOptions, L.ScoreOptions, 24), (SearchOptions, L.SearchOptions, 56), (SearchEntry, L.SearchEntryStruct, 200),
                               (SearchResult, L.SearchResultStruct, 24 + 32 * 200)):
        assert C.sizeof(mine) == C.sizeof(theirs) == size
        assert [n for n, _ in mine._fields_] == [n for n, _ in theirs._fields_]
        assert [getattr(mine, n).offset for n, _ in mine._fields_] == [getattr(theirs, n).offset for n, _ in theirs._fields_]
    assert L.SEARCH_MAX_TOP == MAX_TOP
    lib = L.lib()
    T = (C.c_float * 16)(*np.eye(4, dtype=f32).reshape(16))
    Rr = (C.c_double * 9)(*np.eye(3).reshape(9))
    depth, cost, out = (C.c_float * 4)(), (C.c_double * 1)(), (C.c_uint64 * 8)()
    assert lib.drf_score_poses(None, depth, T, 1, None, cost, None, None) == 1
    assert lib.drf_score_poses_device(None, None, T, 1, None, cost, None, None) == 1
    assert lib.drf_search_frame(None, depth, T, 1, Rr, 1, None, None, None, T, None, None) == 1
    assert lib.drf_search_frame_device(None, None, T, 1, Rr, 1, None, None, None, T, None, None) == 1
    assert lib.drf_search_stats(None, out) == 1


def test_pose_rotations():
    from tandem_amd.dr_fusion import pose_rotations
    r = pose_rotations([-20.0, 10.0], [0.0, 4.0], [0.0])
    assert r.shape == (4, 9) and r.dtype == np.float64
    assert np.array_equal(pose_rotations(), np.eye(3).reshape(1, 9))
    for k, (y, p) in enumerate([(-20.0, 0.0), (-20.0, 4.0), (10.0, 0.0), (10.0, 4.0)]):
        want = rotation((0, 1, 0), y) @ rotation((1, 0, 0), p)
        assert np.abs(r[k].reshape(3, 3) - want).max() < 1e-15
    z = pose_rotations(roll_deg=[90.0])[0].reshape(3, 3)
    assert np.abs(z @ np.array([1.0, 0.0, 0.0]) - np.array([0.0, 1.0, 0.0])).max() < 1e-15


def test_shim_compiles(tmp_path):
    """tandem_amd/libdr/dr_fusion.h ScorePoses / SearchDepthFrame as a TANDEM translation unit would call them
    (tests/cpp/map_search_shim.cpp): it compiles and links against the library; tests/test_fusion_map_search_gpu.py runs it."""
    abi_module()
    exe = str(tmp_path / "map_search_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/map_search_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert os.path.isfile(exe)
