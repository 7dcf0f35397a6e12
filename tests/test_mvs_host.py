"""CPU: the host half of DrMvsnet (tandem_amd/csrc/mvs_host.h -- the weight blob and its folds, the per-call camera geometry, the
feature cache's index, the kernel choice functions) compiled with plain g++ (tests/cpp/mvs_host_check.cpp) and held to restatements
written here, on seeded inputs.  tests/cpp/mvs_host_san.cpp runs the same header as a stand-alone program under ASan + UBSan."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import mvs_stage_ref as R
from tandem_amd import weights as Wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
u64p, i32p, f32p = (C.POINTER(t) for t in (C.c_uint64, C.c_int, C.c_float))
f32 = np.float32


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mvs_host") / "libmvs_host_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                           os.path.join(ROOT, "tests/cpp/mvs_host_check.cpp"), "-o", so])
    h = C.CDLL(so)
    h.mh_last_error.restype = C.c_char_p
    h.mh_image_key.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, u64p]
    h.mh_index_new.restype = C.c_void_p
    h.mh_index_new.argtypes = [C.c_int]
    h.mh_index_free.argtypes = [C.c_void_p]
    h.mh_index_plan.argtypes = [C.c_void_p, C.c_int, u64p, i32p, i32p, u64p]
    h.mh_index_commit.argtypes = [C.c_void_p, C.c_int]
    h.mh_index_collision.argtypes = [C.c_void_p]
    h.mh_index_holds.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    h.mh_geometry.argtypes = [C.c_int] * 4 + [f32p, f32p, C.c_float, C.c_float, C.c_float, i32p, f32p, C.c_int, C.c_int, f32p, f32p, i32p, i32p,
                              C.POINTER(C.c_uint)]
    h.mh_blob_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    h.mh_blob_free.argtypes = [C.c_void_p]
    h.mh_blob_meta.argtypes = [C.c_void_p, i32p, f32p, i32p]
    h.mh_blob_count.argtypes = [C.c_void_p]
    h.mh_blob_tensor.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, i32p, C.POINTER(C.c_size_t)]
    h.mh_blob_data.argtypes = [C.c_void_p, C.c_char_p, f32p]
    h.mh_fold_bn.argtypes = [C.c_void_p, C.c_char_p, C.c_int, f32p, f32p]
    h.mh_fold_gate.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p]
    h.mh_compose_out3.argtypes = [C.c_void_p, f32p, f32p, f32p]
    h.mh_prob_taps.argtypes = [C.c_void_p, C.c_int, f32p]
    h.mh_pad_cin.argtypes = [f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p]
    h.mh_choice_names.argtypes = [C.c_int, C.c_int, C.c_int, i32p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_size_t, i32p, i32p]
    return h


def fp(a):
    return a.ctypes.data_as(f32p)


# ------------------------------------------------------------------ image key
def restated_key(buf, height, width):
    """first / last 64 bytes and, where the image has 4 KiB or more, 511 words at multiples of (n / 512) & ~7: two 64-bit mixes with wrap-around"""
    n = len(buf)
    a, b = 0xcbf29ce484222325 ^ height, 0x9e3779b97f4a7c15 ^ width

    def mix(w):
        nonlocal a, b
        a = ((a ^ w) * 0x100000001b3) & M64
        b = ((b + w) * 0xff51afd7ed558ccd) & M64
        b ^= b >> 29

    def word(off):
        return int.from_bytes(buf[off:off + 8], "little")
    for o in range(0, 64, 8):
        mix(word(o))
        mix(word(n - 64 + o))
    step = (n // 512) & ~7
    for k in range(1, 512 if step else 0):
        mix(word(k * step))
    return a, b


def engine_key(H, buf, height, width):
    k = (C.c_uint64 * 2)()
    raw = (C.c_ubyte * len(buf)).from_buffer_copy(buf)
    H.mh_image_key(raw, len(buf), height, width, k)
    return k[0], k[1]


@pytest.mark.parametrize("height,width,step", [(32, 32, 0), (64, 96, 32), (480, 640, 1800)])
def test_image_key_equals_its_restatement(H, height, width, step):
    img = np.random.default_rng(height).integers(0, 256, height * width * 3, dtype=np.uint8).tobytes()
    assert (len(img) // 512) & ~7 == step
    key = engine_key(H, img, height, width)
    assert key == restated_key(img, height, width)
    # the shape alone changes the key (same bytes)
    assert engine_key(H, img, height * 2, width // 2) != key and engine_key(H, img, height, width + 1) != key and engine_key(H, img, height + 1, width) != key

    def flipped(off):
        b = bytearray(img)
        b[off] ^= 0x40
        return engine_key(H, bytes(b), height, width)
    n = len(img)
    for off in (0, 5, 63, n - 64, n - 3, n - 1):  # the two 64-byte ends
        assert flipped(off) != key, off
    if step:
        for off in (step, step + 7, 100 * step + 3, 511 * step + 7):  # inside a sampled word
            assert flipped(off) != key, off
        for off in (3 * step + 8, 100 * step + 8, 100 * step + step - 1, 511 * step + 8):  # between two samples
            assert 64 <= off < n - 64 and flipped(off) == key, off
    else:
        for off in (64, 1000, n - 65):  # a short image: nothing between the ends is read
            assert flipped(off) == key, off


# ------------------------------------------------------------------ cache index
class LruModel:
    """Entry index -> [image id, last-used clock, valid].  A view hits the first valid entry that holds its image and that no earlier view of the
    window took; a view without a hit takes the first invalid entry outside the window, else the least recently used one outside it (first on
    ties).  One miss at most: the window is fast; more: every view is computed and files its features (fill).  An entry taken for a miss is invalid
    until the forward behind the window has run (commit)."""

    def __init__(self, capacity):
        self.e = {i: [None, 0, False] for i in range(capacity)}
        self.clock = 0
        self.hits = self.misses = self.batch = self.collisions = 0
        self.fast = self.fill = False
        self.miss = -1
        self.slot = []

    def plan(self, ids):
        V = len(ids)
        self.fast = self.fill = False
        self.miss, self.slot, self.evicted = -1, [-1] * V, []
        if len(self.e) < V + 1:
            return
        self.clock += 1
        for v, i in enumerate(ids):
            for k in sorted(self.e):
                if self.e[k][2] and self.e[k][0] == i and k not in self.slot[:v]:
                    self.slot[v] = k
                    self.e[k][1] = self.clock
                    break
                if self.e[k][2] and self.e[k][0] == i:
                    break  # the first entry with this image is another view's: no second look
        missing = [v for v in range(V) if self.slot[v] < 0]

        def take(v):
            free = [k for k in sorted(self.e) if k not in self.slot]
            invalid = [k for k in free if not self.e[k][2]]
            k = invalid[0] if invalid else min(free, key=lambda k: (self.e[k][1], k))
            self.evicted.append(k)
            self.e[k] = [ids[v], self.clock, False]
            self.slot[v] = k
        if len(missing) <= 1:
            self.fast = True
            if missing:
                self.miss = missing[0]
                take(self.miss)
            self.hits += V - len(missing)
            self.misses += len(missing)
        else:
            self.fill = True
            for v in missing:
                take(v)
            self.misses += V
            self.batch += 1

    def commit(self):
        if self.fast and self.miss >= 0:
            self.e[self.slot[self.miss]][2] = True
        if self.fill:
            for k in self.slot:
                self.e[k][2] = True

    def collision(self):
        self.collisions += 1
        for k in self.e:
            self.e[k][2] = False
        self.fast = self.fill = False


def run_windows(H, capacity, windows):
    """windows: lists of image ids, or "collision".  After every window: slots, miss, fast / fill and the four counters against the model; the window's
    hits still hold their images (nothing the window uses was evicted); distinct views own distinct entries."""
    idx, model = H.mh_index_new(capacity), LruModel(capacity)
    log = []
    try:
        for w in windows:
            if w == "collision":
                H.mh_index_collision(idx)
                model.collision()
                continue
            V = len(w)
            ids = (C.c_uint64 * V)(*w)
            slot, state, cnt = (C.c_int * 8)(), (C.c_int * 3)(), (C.c_uint64 * 4)()
            H.mh_index_plan(idx, V, ids, slot, state, cnt)
            model.plan(list(w))
            assert (bool(state[0]), bool(state[1]), state[2]) == (model.fast, model.fill, model.miss), (w, list(state))
            assert list(cnt) == [model.hits, model.misses, model.batch, model.collisions], (w, list(cnt))
            if model.fast or model.fill:
                got = list(slot[:V])
                assert got == model.slot, (w, got, model.slot)
                assert len(set(got)) == V and all(0 <= s < capacity for s in got)
                for v in range(V):  # a hit's entry still holds the view's image, valid: no eviction took an entry the window uses
                    assert bool(H.mh_index_holds(idx, got[v], w[v])) == (got[v] not in model.evicted), (w, v)
            H.mh_index_commit(idx, V)
            model.commit()
            log.append((model.fast, model.fill, model.miss))
    finally:
        H.mh_index_free(idx)
    return log, model


@pytest.mark.parametrize("V", [2, 7, 8])
def test_cache_index_on_a_window_sliding_by_one(H, V):
    log, m = run_windows(H, V + 1, [list(range(t, t + V)) for t in range(12)])
    assert log[0] == (False, True, -1) or V == 1
    assert all(fast and not fill for fast, fill, _ in log[1:])  # V - 1 hits and one miss per window
    assert (m.hits, m.misses, m.batch) == (11 * (V - 1), V + 11, 1)


@pytest.mark.parametrize("V,stride", [(7, 2), (7, 3), (2, 2), (8, 5)])
def test_cache_index_on_windows_sliding_by_two_or_more_are_batch_windows(H, V, stride):
    log, m = run_windows(H, V + 3, [list(range(t * stride, t * stride + V)) for t in range(8)])
    assert all(fill and not fast for fast, fill, _ in log)
    assert m.batch == 8 and m.hits == 0 and m.misses == 8 * V


def test_cache_index_through_a_reset_a_collision_and_a_repeated_window(H):
    V = 7
    slide = [list(range(t, t + V)) for t in range(5)]
    fresh = [list(range(100 + t, 100 + t + V)) for t in range(4)]  # a reset: every image new, then sliding again
    log, m = run_windows(H, V + 1, slide + fresh + ["collision"] + [fresh[-1], fresh[-1]] + slide)
    kinds = ["fill" if fill else ("fast" if fast else "off") for fast, fill, _ in log]
    assert kinds == ["fill"] + ["fast"] * 4 + ["fill"] + ["fast"] * 3 + ["fill", "fast"] + ["fill"] + ["fast"] * 4
    assert log[10] == (True, False, -1)  # the repeated window: every view hits, nothing is computed
    assert m.collisions == 1 and m.batch == 4


@pytest.mark.parametrize("V", [2, 8])
def test_cache_index_two_views_with_one_image_share_no_entry(H, V):
    base = list(range(V))
    twice = base[:-1] + [base[0]]  # the last view shows the first view's image
    log, m = run_windows(H, V + 1, [base, twice, twice, base])
    # the second view of the image finds the entry its first view owns, so it misses (one miss: fast) and files an entry of its own -- in every such window:
    # the look-up stops at the first entry that holds the image
    assert log[1] == (True, False, V - 1) and log[2] == (True, False, V - 1)
    assert log[3][0] and log[3][2] in (-1, V - 1)
    assert m.batch == 1


@pytest.mark.parametrize("V", [2, 8])
def test_cache_index_of_capacity_v_never_answers(H, V):
    log, m = run_windows(H, V, [list(range(t, t + V)) for t in range(4)] + [list(range(3, 3 + V))])
    assert all(k == (False, False, -1) for k in log)
    assert (m.hits, m.misses, m.batch) == (0, 0, 0)
    log, m = run_windows(H, V + 1, [list(range(t, t + V)) for t in range(4)])  # capacity V + 1: the smallest that does
    assert [fast for fast, _, _ in log] == [False, True, True, True]


def test_cache_index_random_windows(H):
    rng = np.random.default_rng(11)
    for V, cap in ((2, 3), (3, 5), (7, 8), (8, 12)):
        windows = []
        for _ in range(60):
            w = [int(x) for x in rng.integers(0, cap + 3, V)]  # repeats inside a window included
            windows.append(w if rng.random() > 0.05 else "collision")
        run_windows(H, cap, windows)


# ------------------------------------------------------------------ geometry
MODELS = {"48/32/8": ((48, 32, 8), (1.0, 0.5, 0.25)), "48/4/4": ((48, 4, 4), (1.0, 0.5, 0.25)), "16/8/8": ((16, 8, 8), (1.0, 0.7, 0.3))}


def engine_geometry(H, height, width, V, ref, K, c2ws, dmin, dmax, disc, depth_num, ratio, va=1, shard=0):
    Mo, pl = np.zeros((3, 7, 12), f32), np.zeros((3, 5), f32)
    D, order, rank = (C.c_int * 3)(), (C.c_int * 8)(), C.c_uint()
    K9, cw = np.ascontiguousarray(K, f32).reshape(9), np.ascontiguousarray(c2ws, f32).reshape(V, 16)
    rc = H.mh_geometry(height, width, V, ref, fp(K9), fp(cw), dmin, dmax, disc, (C.c_int * 3)(*depth_num), (C.c_float * 3)(*ratio), va, shard, fp(Mo), fp(pl), D,
                       order, C.byref(rank))
    return rc, Mo, pl, list(D), list(order[:V]), rank.value


def restated_planes(dmin, dmax, depth_num, ratio, stage):
    """the engine's expressions, operation by operation in float32"""
    base = (f32(dmax) - f32(dmin)) / f32(depth_num[0] - 1)
    if stage == 1:
        return f32(dmin), base, f32(0), f32(0)
    D = depth_num[stage - 1]
    delta = f32(ratio[stage - 1]) * base
    return f32(dmin), base, (f32(D) / f32(2)) * delta, f32(D) * delta


def restated_rank(height, width, disc):
    cut = f32(height * width) * (f32(100) - f32(disc))
    cut = cut / f32(100)
    return min(max(int(cut), 0), height * width - 1)


@pytest.mark.parametrize("V", [2, 3, 8])
@pytest.mark.parametrize("pose", R.POSES)
def test_geometry_against_the_float64_homography(H, V, pose):
    height, width = 64, 96
    win = R.make_case(height, width, V, pose)
    depth_num, ratio = MODELS["48/32/8"]
    for ref in range(V):
        rc, Mo, pl, D, order, rank = engine_geometry(H, height, width, V, ref, win["K"], win["c2ws"], win["depth_min"], win["depth_max"], 2.5, depth_num, ratio)
        assert rc == 0, H.mh_last_error()
        assert order == R.model_order(V, ref) and D == list(depth_num)
        c2w = np.asarray(win["c2ws"], f32)
        for s in (1, 2, 3):
            for v in range(1, V):
                want = R.homography(R.stage_K(win["K"], s), c2w[order[0]], c2w[order[v]])[:3, :4].reshape(12).astype(f32)
                bound = 2.0 ** -22 * np.abs(want).max()  # one float32 rounding of the largest entry: both sides round a float64 result of another elimination order
                err = np.abs(Mo[s - 1, v - 1].astype(np.float64) - want.astype(np.float64)).max()
                assert err <= bound, (pose, ref, s, v, err, bound)
            assert not Mo[s - 1, V - 1:].any()
            assert np.array_equal(pl[s - 1, 4:].view(np.uint32), np.array([f32(V - 1)]).view(np.uint32))


@pytest.mark.parametrize("model", list(MODELS))
def test_plane_ranges_and_filter_rank_equal_their_float32_restatements(H, model):
    height, width, V = 64, 96, 3
    depth_num, ratio = MODELS[model]
    win = R.make_case(height, width, V, "scene")
    for dmin, dmax in ((0.5, 5.0), (0.3, 1.2), (0.01, 10.0), (0.1, 7.3)):
        for disc in (2.5, 0.0, 100.0, -5.0, 250.0, 33.3, 99.99):
            rc, _, pl, _, _, rank = engine_geometry(H, height, width, V, 1, win["K"], win["c2ws"], dmin, dmax, disc, depth_num, ratio)
            assert rc == 0
            for s in (1, 2, 3):
                want = np.array(restated_planes(dmin, dmax, depth_num, ratio, s), f32)
                assert np.array_equal(pl[s - 1, :4].view(np.uint32), want.view(np.uint32)), (model, dmin, dmax, s, pl[s - 1], want)
            assert rank == restated_rank(height, width, disc), (disc, rank)
    assert restated_rank(height, width, 100.0) == 0 and restated_rank(height, width, 0.0) == height * width - 1  # both ends of the clamp are among the cases
    assert restated_rank(height, width, 250.0) == 0 and 0 < restated_rank(height, width, 33.3) < height * width - 1


def test_view_shard_divisor_and_its_refusal(H):
    win = R.make_case(64, 96, 2, "scene")
    depth_num, ratio = MODELS["48/32/8"]
    rc, _, pl, _, _, _ = engine_geometry(H, 64, 96, 2, 0, win["K"], win["c2ws"], 0.5, 5.0, 2.5, depth_num, ratio, va=1, shard=6)
    assert rc == 0 and list(pl[:, 4]) == [6.0, 6.0, 6.0]  # the divisor is the whole window's source count
    rc = engine_geometry(H, 64, 96, 2, 0, win["K"], win["c2ws"], 0.5, 5.0, 2.5, depth_num, ratio, va=0, shard=6)[0]
    assert rc == 6 and b"view sharding" in H.mh_last_error()


# ------------------------------------------------------------------ blob and folds
@pytest.fixture(scope="module")
def blob(H, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("blob") / "m.tdmw")
    sd = Wt.random_state((48, 4, 4), seed=3)
    Wt.write_blob(path, sd, depth_num=(48, 4, 4), interval_ratio=(1.0, 0.5, 0.25), view_aggregation=True)
    b = C.c_void_p()
    assert H.mh_blob_load(path.encode(), C.byref(b)) == 0, H.mh_last_error()
    yield b, sd, path
    H.mh_blob_free(b)


def test_blob_comes_back_exact(H, blob):
    b, sd, _ = blob
    dn, ratio, vb = (C.c_int * 3)(), (C.c_float * 3)(), (C.c_int * 2)()
    H.mh_blob_meta(b, dn, ratio, vb)
    assert (list(dn), list(ratio), list(vb)) == ([48, 4, 4], [1.0, 0.5, 0.25], [1, 8])
    assert H.mh_blob_count(b) == len(sd)
    names = []
    for i in range(len(sd)):
        name, dims, cnt = C.create_string_buffer(256), (C.c_int * 8)(), C.c_size_t()
        nd = H.mh_blob_tensor(b, i, name, 256, dims, C.byref(cnt))
        names.append(name.value.decode())
        want = np.asarray(sd[names[-1]], f32)
        assert tuple(dims[:nd]) == want.shape and cnt.value == want.size
        got = np.zeros(want.size, f32)
        assert H.mh_blob_data(b, name.value, fp(got)) == 0
        assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32)), names[-1]
    assert names == sorted(sd)


def test_blob_error_paths_and_their_codes(H, blob, tmp_path):
    b, _, path = blob
    raw = open(path, "rb").read()
    out = C.c_void_p()

    def load(data, name="bad.tdmw"):
        q = tmp_path / name
        q.write_bytes(data)
        return H.mh_blob_load(str(q).encode(), C.byref(out))
    for cut in (len(raw) - 1, len(raw) // 2, 41, 36, 7, 0):  # inside the last tensor, the middle, the tensor count, the header, the magic
        assert load(raw[:cut]) == 4 and b"truncated" in H.mh_last_error(), cut
    assert load(b"TDMW0002" + raw[8:]) == 4 and b"not a TDMW blob" in H.mh_last_error()
    assert load(raw[:36] + struct.pack("<i", 16) + raw[40:]) == 6 and b"base_channels=8" in H.mh_last_error()
    assert H.mh_blob_load(str(tmp_path / "missing.tdmw").encode(), C.byref(out)) == 4 and b"cannot open" in H.mh_last_error()
    assert load(raw) == 0
    H.mh_blob_free(out)
    got = np.zeros(8, f32)
    assert H.mh_blob_data(b, b"feature_net.no.such.weight", fp(got)) == 4 and b"missing tensor feature_net.no.such.weight" in H.mh_last_error()
    assert H.mh_fold_bn(b, b"feature_net.conv0.0.nobn", 8, fp(got), fp(got)) == 4


def bits(a):
    return np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32)


def test_folds_equal_their_float64_restatements(H, blob):
    b, sd, _ = blob
    t = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    # BatchNorm: scale = g / sqrt(var + eps), bias = b - mean * scale
    for p, Cn in (("feature_net.conv0.0.bn", 8), ("feature_net.conv2.2.bn", 32), ("cost_regularization_net.stage2.conv6.bn", 64)):
        sc, bi = np.zeros(Cn, f32), np.zeros(Cn, f32)
        assert H.mh_fold_bn(b, p.encode(), Cn, fp(sc), fp(bi)) == 0
        s64 = t[p + ".weight"] / np.sqrt(t[p + ".running_var"] + 1e-5)
        assert np.array_equal(bits(sc), bits(s64)) and np.array_equal(bits(bi), bits(t[p + ".bias"] - t[p + ".running_mean"] * s64)), p
    # the gate: conv (C -> 1, bias b0), BN 1, ReLU, conv (1 -> 1: w3, b3), BN 4, ReLU as two affine maps
    for s in (1, 2, 3):
        Cn, g = 32 >> (s - 1), "volume_gates.stage%d." % s
        out = np.zeros(36, f32)
        assert H.mh_fold_gate(b, s, Cn, fp(out)) == 0

        def bn(p):
            A = t[g + p + ".weight"][0] / np.sqrt(t[g + p + ".running_var"][0] + 1e-5)
            return A, t[g + p + ".bias"][0] - t[g + p + ".running_mean"][0] * A
        (A1, B1), (A2, B2) = bn("1"), bn("4")
        b0, w3, b3 = t[g + "0.bias"].reshape(-1)[0], t[g + "3.weight"].reshape(-1)[0], t[g + "3.bias"].reshape(-1)[0]
        assert np.array_equal(bits(out[:Cn]), bits(t[g + "0.weight"])) and not out[Cn:32].any()
        assert np.array_equal(bits(out[32:]), bits([A1, b0 * A1 + B1, w3 * A2, b3 * A2 + B2])), s
    # out.stage3 (8, 32, 3, 3) o skip.stage3 (32, 8, 1, 1) + bias (32)
    wo, w3, b3 = t["feature_net.out.stage3.weight"].reshape(8, 32, 9), t["feature_net.skip.stage3.weight"].reshape(32, 8), t["feature_net.skip.stage3.bias"]
    wa, T, bint = np.zeros(8 * 8 * 9, f32), np.zeros(72, f32), np.zeros(8, f32)
    assert H.mh_compose_out3(b, fp(wa), fp(T), fp(bint)) == 0
    T64 = np.einsum("oct,c->to", wo, b3)
    # (a 32-term float64 dot product in another order moves the 17th digit: equal after the rounding to float32 unless it sits on a tie, which these seeded weights do not)
    assert np.array_equal(bits(wa), bits(np.einsum("oct,ck->okt", wo, w3)))
    assert np.array_equal(bits(T), bits(T64))
    assert np.array_equal(bits(bint), bits(T64.astype(f32).astype(np.float64).sum(0)))  # the interior bias sums the ROUNDED table: what the border kernel subtracts
    for s in (1, 2, 3):
        wt = np.zeros(27 * 8, f32)
        assert H.mh_prob_taps(b, s, fp(wt)) == 0
        assert np.array_equal(bits(wt), bits(np.asarray(sd["cost_regularization_net.stage%d.prob.weight" % s], f32).reshape(8, 27).T))
    w = np.asarray(sd["feature_net.conv0.0.conv.weight"], f32)  # (8, 3, 3, 3): RGB -> RGB0
    padded = np.full(8 * 4 * 9, 7, f32)
    H.mh_pad_cin(fp(np.ascontiguousarray(w)), 8, 3, 4, 9, fp(padded))
    want = np.zeros((8, 4, 9), f32)
    want[:, :3] = w.reshape(8, 3, 9)
    assert np.array_equal(bits(padded), bits(want))


# ------------------------------------------------------------------ kernel choice
def expected_kernels(depth_num, view_aggregation, zchunk):
    """tests/test_mvs_stages_gpu.py::_expected_kernels, for its 64 x 96-class frames"""
    want = {}
    for s in (1, 2, 3):
        D, Cn = depth_num[s - 1], 32 >> (s - 1)
        want["costvol%d" % s] = "k_costvol5<%d,4>" % Cn if view_aggregation else "k_costvol3<%d>" % Cn
        want["prob%d" % s] = "k_prob2_regress<8>" if D == 8 and zchunk is not None and zchunk >= 8 else "k_prob2<1>"
    return want


def chosen(H, height, width, V, depth_num, va, zchunk, dchunk=0):
    cv, pr = C.create_string_buffer(3 * 64), C.create_string_buffer(3 * 64)
    rg, fused = (C.c_int * 3)(), (C.c_int * 3)()
    H.mh_choice_names(height, width, V, (C.c_int * 3)(*depth_num), va, zchunk or 0, dchunk, cv, pr, 64, rg, fused)
    got = {}
    for s in (1, 2, 3):
        got["costvol%d" % s] = cv.raw[64 * (s - 1):64 * s].split(b"\0")[0].decode()
        got["prob%d" % s] = pr.raw[64 * (s - 1):64 * s].split(b"\0")[0].decode()
    return got, list(rg), list(fused)


@pytest.mark.parametrize("depth_num", [(48, 32, 8), (48, 4, 4), (16, 8, 8)])
@pytest.mark.parametrize("va", [1, 0])
@pytest.mark.parametrize("zchunk", [None, 3, 5, 8])
def test_choice_functions_name_the_kernels_the_stage_tests_expect(H, depth_num, va, zchunk, monkeypatch):
    for name in [k for k in os.environ if k.startswith("DR_")]:
        monkeypatch.delenv(name)
    got, regress, fused = chosen(H, 64, 96, 3, depth_num, va, zchunk)
    assert got == expected_kernels(depth_num, va, zchunk)
    # the regression kernel follows from the plane count alone; PROB answers for it exactly where it is k_prob2_regress
    assert regress == [D if D in (48, 32, 8, 4) else 0 for D in depth_num]
    assert fused == [int(got["prob%d" % s] == "k_prob2_regress<8>") for s in (1, 2, 3)]


def test_choice_at_the_headline_shape_and_with_depth_chunks_of_eight(H, monkeypatch):
    for name in [k for k in os.environ if k.startswith("DR_")]:
        monkeypatch.delenv(name)
    # 480 x 640, planes 48/32/8: stage 3's 8 planes in one z chunk still make 120 x 10 = 1200 >= 1024 workgroups, so the default chunk is 8 and the regression rides along
    got, _, fused = chosen(H, 480, 640, 7, (48, 32, 8), 1, None)
    assert got == {"costvol1": "k_costvol5<32,4>", "costvol2": "k_costvol5<16,4>", "costvol3": "k_costvol5<8,4>", "prob1": "k_prob2<1>", "prob2": "k_prob2<1>",
                   "prob3": "k_prob2_regress<8>"} and fused == [0, 0, 1]
    # DR_CV_DCHUNK{1,2,3}=8 (tests/test_mvs_stages_gpu.py::test_stage_tensors_with_depth_chunks_of_eight)
    got, _, _ = chosen(H, 64, 96, 4, (48, 32, 8), 1, None, dchunk=8)
    assert [got["costvol%d" % s] for s in (1, 2, 3)] == ["k_costvol5<32,8>", "k_costvol5<16,8>", "k_costvol5<8,8>"]


# ------------------------------------------------------------------ sanitizers
def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """mvs_host.h under AddressSanitizer and UBSan: a plain executable, nothing preloaded, nothing loaded into Python."""
    exe = str(tmp_path / "mvs_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/mvs_host_san.cpp"), "-o", exe])
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mvs_host_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
