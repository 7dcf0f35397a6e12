"""CPU: the host half of drf_merge_map (include/dr_mi355x.h "map files", DESIGN.md §7c "Merging a map file").  merge_voxel,
merge_block and plan_merge of tandem_amd/csrc/fusion_host.h compiled with plain g++ (tests/cpp/map_merge_check.cpp) and held to
a numpy restatement of the rule written here -- the reference of tests/test_fusion_map_merge_gpu.py too; the same under
AddressSanitizer and UBSan as a stand-alone program (tests/cpp/map_merge_san.cpp); the two new names of the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import abi_module, check_symbols
from test_map_file import pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 1 << 20
u8p, u64p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int)


# ------------------------------------------------------------------ the rule, restated
def np_merge_voxels(a, b, W):
    """a = the map's voxels, b = the file's, (n, 8) uint8 each ({f32 sdf, u8 b, g, r, u8 weight}) -> (merged (n, 8) uint8,
    case (n,) in {1, 2, 3}).  float32 arithmetic operation by operation, astype(uint8) for the colour truncation, the weight
    sum in Python-sized integers."""
    a, b = np.ascontiguousarray(a, np.uint8).reshape(-1, 8), np.ascontiguousarray(b, np.uint8).reshape(-1, 8)
    out = a.copy()
    wa, wb = a[:, 7].astype(np.int64), b[:, 7].astype(np.int64)
    case = np.where(wb == 0, 1, np.where(wa == 0, 2, 3))
    two, three = case == 2, case == 3
    out[two] = b[two]
    out[two, 7] = np.minimum(wb[two], W).astype(np.uint8)
    x, y = a[three], b[three]
    fa, fb = wa[three].astype(np.float32), wb[three].astype(np.float32)
    den = fa + fb
    m = np.empty((len(x), 8), np.uint8)
    sa, sb = x[:, :4].copy().view(np.float32)[:, 0], y[:, :4].copy().view(np.float32)[:, 0]
    m[:, :4] = np.ascontiguousarray(((sa * fa + sb * fb) / den).astype(np.float32)).view(np.uint8).reshape(-1, 4)
    for k in (4, 5, 6):
        m[:, k] = ((x[:, k].astype(np.float32) * fa + y[:, k].astype(np.float32) * fb) / den).astype(np.uint8)
    m[:, 7] = np.minimum(wa[three] + wb[three], W).astype(np.uint8)
    out[three] = m
    return out, case


def np_merge_maps(A, F, W):
    """{coord: 4096 bytes} of the map, the same of the file -> (the merged map, stats): the union of the blocks, shared blocks
    merged voxel by voxel.  stats = dict(file, added, combined, verbatim, averaged, unchanged): blocks, blocks, blocks, voxels of
    case 2, of case 3, of case 1 within the combined blocks."""
    out = {c: np.array(v, np.uint8) for c, v in A.items()}
    st = dict(file=len(F), added=0, combined=0, verbatim=0, averaged=0, unchanged=0)
    shared = [c for c in F if c in A]
    for c in F:
        if c not in A:
            out[c] = np.array(F[c], np.uint8)
            st["added"] += 1
    if shared:
        a = np.stack([A[c] for c in shared]).reshape(-1, 8)
        b = np.stack([F[c] for c in shared]).reshape(-1, 8)
        m, case = np_merge_voxels(a, b, W)
        m = m.reshape(len(shared), 4096)
        for i, c in enumerate(shared):
            out[c] = m[i]
        st.update(combined=len(shared), verbatim=int((case == 2).sum()), averaged=int((case == 3).sum()), unchanged=int((case == 1).sum()))
    return out, st


# ------------------------------------------------------------------ the compiled host half
@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("map_merge") / "libmap_merge_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_merge_check.cpp"), "-o", so])
    h = C.CDLL(so)
    h.mm_merge_voxels.argtypes = [u8p, u8p, C.c_size_t, C.c_int, u8p]
    h.mm_merge_voxels.restype = None
    h.mm_merge_blocks.argtypes = [u8p, u8p, C.c_size_t, C.c_int, u64p]
    h.mm_merge_blocks.restype = None
    h.mm_plan.argtypes = [u64p, i32p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, i32p, i32p, i32p, u64p, i32p, u64p, u64p, u64p, u64p, u64p]
    h.mm_plan.restype = C.c_size_t
    return h


def cpp_merge_voxels(H, a, b, W):
    out, case = np.ascontiguousarray(a, np.uint8).copy(), np.zeros(len(a), np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    H.mm_merge_voxels(out.ctypes.data_as(u8p), b.ctypes.data_as(u8p), len(out), W, case.ctypes.data_as(u8p))
    return out, case


def random_voxels(rng, weights):
    """(n, 8) voxels with the given weights: sdf of both signs, a few metres down to fractions of a voxel; random colours."""
    n = len(weights)
    v = np.empty((n, 8), np.uint8)
    scale = rng.choice(np.array([0.08, 1.0, 1000.0, 1e-3], np.float32), n)
    v[:, :4] = (rng.uniform(-1.0, 1.0, n).astype(np.float32) * scale).view(np.uint8).reshape(n, 4)
    v[:, 4:7] = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    v[:, 7] = weights
    return v


DRAWS = 200


@pytest.mark.parametrize("W", [1, 64, 255])
def test_merge_voxel_over_all_weight_pairs(H, W):
    rng = np.random.default_rng(40 + W)
    wa, wb = (g.reshape(-1).astype(np.uint8) for g in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    seen = np.zeros(4, np.int64)
    for lo in range(0, DRAWS, 50):
        reps = min(50, DRAWS - lo)
        a, b = random_voxels(rng, np.tile(wa, reps)), random_voxels(rng, np.tile(wb, reps))
        want, wcase = np_merge_voxels(a, b, W)
        got, gcase = cpp_merge_voxels(H, a, b, W)
        assert np.array_equal(gcase, wcase)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"{bad.size} voxels differ, first a={a[bad[0]]} b={b[bad[0]]} got={got[bad[0]]} want={want[bad[0]]}"
        assert np.array_equal(got[wcase == 1], a[wcase == 1]), "a voxel of case 1 changed"
        seen += np.bincount(wcase, minlength=4)
        sa, sb = a[:, :4].copy().view(np.float32)[:, 0], b[:, :4].copy().view(np.float32)[:, 0]
        three = wcase == 3
        assert ((sa < 0) & (sb > 0) & three).any() and ((sa > 0) & (sb < 0) & three).any() and ((sa < 0) & (sb < 0) & three).any()
        over = three & (a[:, 7].astype(int) + b[:, 7] > 255)
        assert over.any() and (got[over, 7] == W).all(), "a weight sum above 255 wrapped"
        assert (got[wcase != 1, 7] <= W).all()
    assert seen[1] == 256 * DRAWS and seen[2] == 255 * DRAWS and seen[3] == 255 * 255 * DRAWS


def test_blocks_of_case_one_leave_the_target_unchanged(H):
    rng = np.random.default_rng(3)
    dst = rng.integers(0, 256, (3, 4096), dtype=np.uint8)
    src = rng.integers(0, 256, (3, 4096), dtype=np.uint8)
    src.reshape(-1, 8)[:, 7] = 0
    got, counts = dst.copy(), (C.c_uint64 * 2)(0, 0)
    H.mm_merge_blocks(got.ctypes.data_as(u8p), src.ctypes.data_as(u8p), 3, 64, counts)
    assert np.array_equal(got, dst) and tuple(counts) == (0, 0)
    merged, st = np_merge_maps({(i, 0, 0): dst[i] for i in range(3)}, {(i, 0, 0): src[i] for i in range(3)}, 64)
    assert all(np.array_equal(merged[(i, 0, 0)], dst[i]) for i in range(3)) and st["unchanged"] == 3 * 512
    # and a block with all three cases counts them as the restatement does
    src2 = rng.integers(0, 256, (3, 4096), dtype=np.uint8)
    src2.reshape(-1, 8)[::3, 7] = 0
    dst2 = dst.copy()
    dst2.reshape(-1, 8)[::5, 7] = 0
    for d in (dst2, src2):  # finite sdf
        d.reshape(-1, 8)[:, :4] = rng.uniform(-0.1, 0.1, 3 * 512).astype(np.float32).view(np.uint8).reshape(-1, 4)
    want, case = np_merge_voxels(dst2.reshape(-1, 8), src2.reshape(-1, 8), 64)
    got, counts = dst2.copy(), (C.c_uint64 * 2)(0, 0)
    H.mm_merge_blocks(got.ctypes.data_as(u8p), src2.ctypes.data_as(u8p), 3, 64, counts)
    assert np.array_equal(got.reshape(-1, 8), want)
    assert tuple(counts) == (int((case == 2).sum()), int((case == 3).sum())) and min(counts) > 0


# ------------------------------------------------------------------ the classification
def cpp_plan(H, res, slots, sto, file, chunk):
    """Per chunk: (resident [(position, slot)], added [(position, key)], stored [(position, key)])."""
    n = len(file)
    arr64 = lambda v: np.ascontiguousarray(v, np.uint64)  # noqa: E731
    res, sto, fil, slots = arr64(res), arr64(sto), arr64(file), np.ascontiguousarray(slots, np.int32)
    r_src, r_slot, a_src, s_src = (np.zeros(n + 2, np.int32) for _ in range(4))
    a_key, s_key, rb, ab, sb = (np.zeros(n + 2, np.uint64) for _ in range(5))
    counts = (C.c_uint64 * 3)()
    p64, p32 = (lambda v: v.ctypes.data_as(u64p)), (lambda v: v.ctypes.data_as(i32p))
    nc = H.mm_plan(p64(res), p32(slots), len(res), p64(sto), len(sto), p64(fil), n, chunk, p32(r_src), p32(r_slot), p32(a_src), p64(a_key), p32(s_src),
                   p64(s_key), p64(rb), p64(ab), p64(sb), counts)
    assert (int(rb[nc]), int(ab[nc]), int(sb[nc])) == tuple(counts) and sum(counts) == n
    out = []
    for c in range(nc):
        r, a, s = (slice(int(x[c]), int(x[c + 1])) for x in (rb, ab, sb))
        out.append((list(zip(r_src[r].tolist(), r_slot[r].tolist())), list(zip(a_src[a].tolist(), a_key[a].tolist())), list(zip(s_src[s].tolist(), s_key[s].tolist()))))
    return out


def py_plan(res, slots, sto, file, chunk):
    slot_of, stored = dict(zip(res, slots)), set(sto)
    out = []
    for lo in range(0, len(file), chunk):
        part = list(enumerate(file[lo:lo + chunk]))
        out.append(([(i, slot_of[k]) for i, k in part if k in slot_of], [(i, k) for i, k in part if k not in slot_of and k not in stored],
                    [(i, k) for i, k in part if k in stored]))
    return out


def key_lists():
    rng = np.random.default_rng(8)
    ends = [pack((-(B - 1),) * 3), pack((B - 1,) * 3)]
    pool = sorted({pack(tuple(int(v) for v in rng.integers(-300, 300, 3))) for _ in range(90)})
    a, b, c = pool[0::3], pool[1::3], pool[2::3]
    return {
        "empty file": (a, b, []),
        "empty map": ([], [], c),
        "disjoint": (a, b, c),
        "identical to the pool": (a, [], a),
        "identical to the store": ([], b, b),
        "interleaved": (a, b, sorted(a[::2] + b[1::2] + c[::3])),
        "both ends in the file only": (a, b, sorted(c + ends)),
        "both ends resident": (sorted(a + ends), b, sorted(c[:5] + ends)),
        "both ends stored": (a, sorted(b + ends), sorted(a[:4] + ends)),
        "one end each": (sorted(a + ends[:1]), sorted(b + ends[1:]), sorted(ends + c[:3])),
    }


@pytest.mark.parametrize("chunk", [1, 5, 1000])
def test_plan_against_a_set_computation(H, chunk):
    rng = np.random.default_rng(chunk)
    for what, (res, sto, file) in key_lists().items():
        slots = rng.permutation(len(res)).tolist()  # the pool order has nothing to do with the key order
        got, want = cpp_plan(H, res, slots, sto, file, chunk), py_plan(res, slots, sto, file, chunk)
        assert got == want, what
        assert len(got) == (len(file) + chunk - 1) // chunk, what


def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """The same entry points under AddressSanitizer and UBSan: a plain executable, nothing preloaded, nothing loaded into Python."""
    exe = str(tmp_path / "map_merge_san")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_merge_san.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_merge_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


# ------------------------------------------------------------------ the C ABI
def test_abi_declares_exports_and_types_the_two_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_merge_map", "drf_merge_stats"])
    assert "uint64_t out[6]" in src
    lib = L.lib()
    out = (C.c_uint64 * 6)()
    assert lib.drf_merge_map(None, b"x.drfmap", 0) == 1 and lib.drf_merge_stats(None, out) == 1
