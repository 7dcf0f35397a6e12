"""The host rule of the search scope (drf_set_search_scope(DRF_SEARCH_MAP); tandem_amd/csrc/fusion_host.h select_render_blocks'
widening and "the search scope", engine_host.h select_search_unit / plan_search_stage), compiled by g++ from
tests/cpp/search_scope_check.cpp -- no GPU:
  * select_render_blocks with extra = 0 is select_render_blocks without the argument;
  * the widened selection at a unit's centre pose holds the plain selection at every candidate of the unit, for lattices with
    turned entries, a non-cubic half and a sub-range of ix;
  * the plan is sufficient end to end: the restatement of tests/test_map_search.py over only a pass's keys scores the pass's
    candidates as it does over all blocks, bit for bit, for a lattice and for a plain table of 259 poses;
  * the plan's shape; the same plans under AddressSanitizer and UBSan in a stand-alone program; the C ABI, its mirror and the shim.
The random map of tests/test_map_locate.py is 7 blocks across, and render_margin alone is almost 3: at the case's sensor range of
10 m every unit that faces the map selects all of it, and no capacity above one unit's selection makes a second pass.  The plans
here (and their runs in tests/test_fusion_search_scope_gpu.py) therefore take the case with max_sensor_depth = 0.6 m (SCOPE_DEPTH),
where the far end of the map falls outside the selection and the units differ; the depth image then has about 1 300 samples at
pixel step 1.  DESIGN.md §7c "Searching the whole map"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import ROOT, abi_module, check_symbols
from test_locate_scope import BOX, CAMS, pack, random_pose
from test_map_align import bits
from test_map_locate import Camera, f32p, f64p, random_case, u64p
from test_map_search import VS, assert_same_scores, np_candidates, np_score_candidates, np_score_options, random_poses, small_lattice
from test_map_transform import motion

f32, f64 = np.float32, np.float64
SCOPE_DEPTH = 0.6
LATTICE = dict(half=(1, 2, 0), trans_step=0.08)     # 2 anchors x 3 rotations x (3 x 5 x 1): 90 candidates, 4-voxel steps
N_POSES = 259
SCOPE_STEP = 1                                      # the pixel step of the scores over the plans
MARGIN = 3                                          # blocks of capacity above the largest single-slab selection


# ------------------------------------------------------------------ the compiled rule
def build_check(directory):
    so = os.path.join(str(directory), "libsearch_scope_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/search_scope_check.cpp"), "-o", so])
    h = C.CDLL(so)
    cam, i3 = C.POINTER(Camera), C.POINTER(C.c_int)
    h.ss_select.argtypes = [u64p, C.c_int, cam, f32p, C.c_int, C.c_double, u64p, C.c_int]
    h.ss_table.argtypes = [f32p, C.c_size_t, f64p, C.c_size_t, C.c_float, f64p]
    h.ss_plain_table.argtypes = [f32p, C.c_size_t, C.c_float, f64p]
    h.ss_candidate.argtypes = [f64p, i3, C.c_double, C.c_int, C.c_size_t, C.c_float, f32p, f64p]
    h.ss_unit.argtypes = [u64p, C.c_int, cam, f64p, i3, C.c_double, C.c_int, C.c_size_t, C.c_int, C.c_int, u64p, C.c_int]
    h.ss_plan.argtypes = [u64p, C.c_int, cam, f64p, i3, C.c_double, C.c_int, C.c_size_t, C.c_size_t, u64p, u64p, u64p, C.c_int, u64p, C.c_size_t, u64p]
    return h


@pytest.fixture(scope="module")
def SS(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("search_scope"))


def _i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


def dstep_of(cam, trans_step):
    """(double)trans_step / vs, as search_options makes it"""
    ts = f32(trans_step) if trans_step else f32(2.0) * f32(cam["truncation_distance"])
    return float(f64(ts) / f64(f32(cam["voxel_size"])))


def lattice_table(SS, cam, anchors, rot):
    a = np.ascontiguousarray(anchors, f32).reshape(-1, 16)
    r = np.ascontiguousarray(rot, f64).reshape(-1, 9)
    table = np.zeros(len(a) * len(r) * 12, f64)
    assert SS.ss_table(a.ctypes.data_as(f32p), len(a), r.ctypes.data_as(f64p), len(r), f32(cam["voxel_size"]), table.ctypes.data_as(f64p)) == 0
    return table


def plain_table(SS, cam, poses):
    p = np.ascontiguousarray(poses, f32).reshape(-1, 16)
    table = np.zeros(len(p) * 12, f64)
    SS.ss_plain_table(p.ctypes.data_as(f32p), len(p), f32(cam["voxel_size"]), table.ctypes.data_as(f64p))
    return table


def select(SS, keys, cam, pose, extra=None):
    """select_render_blocks at the pose (extra None: called without the argument): (did it cut, the ascending keys)"""
    out = np.zeros(len(keys), np.uint64)
    p = np.ascontiguousarray(pose, f32).reshape(16)
    n = SS.ss_select(keys.ctypes.data_as(u64p), len(keys), C.byref(Camera(**cam)), p.ctypes.data_as(f32p), int(extra is not None), float(extra or 0.0),
                     out.ctypes.data_as(u64p), len(out))
    cut = n >= 0
    return cut, out[:n if cut else -n - 1].copy()


def unit(SS, keys, cam, table, half, dstep, plain, e, x0=0, x1=1):
    out = np.zeros(len(keys), np.uint64)
    n = SS.ss_unit(keys.ctypes.data_as(u64p), len(keys), C.byref(Camera(**cam)), table.ctypes.data_as(f64p), _i3(half), dstep, int(plain), e, x0, x1,
                   out.ctypes.data_as(u64p), len(out))
    assert n >= 0, "the unit's keys are not ascending"
    return out[:n].copy()


def candidate(SS, cam, table, half, dstep, plain, c):
    """(the float pose16, R, tv) of candidate c"""
    p16, rtv = np.zeros(16, f32), np.zeros(12, f64)
    SS.ss_candidate(table.ctypes.data_as(f64p), _i3(half), dstep, int(plain), c, f32(cam["voxel_size"]), p16.ctypes.data_as(f32p), rtv.ctypes.data_as(f64p))
    return p16.reshape(4, 4), rtv[:9].reshape(3, 3), rtv[9:]


def plan(SS, keys, cam, table, half, dstep, plain, n, capacity):
    """plan_search_stage: a list of (first, count, keys), or ("failed", count)"""
    room = 4096
    first, count, nk = (np.zeros(room, np.uint64) for _ in range(3))
    allk, too = np.zeros(room * max(len(keys), 1), np.uint64), C.c_uint64(0)
    r = SS.ss_plan(keys.ctypes.data_as(u64p), len(keys), C.byref(Camera(**cam)), table.ctypes.data_as(f64p), _i3(half), dstep, int(plain), n, capacity,
                   first.ctypes.data_as(u64p), count.ctypes.data_as(u64p), nk.ctypes.data_as(u64p), room, allk.ctypes.data_as(u64p), len(allk), C.byref(too))
    if r == -1:
        return ("failed", int(too.value))
    assert r > 0, r
    at = np.concatenate([[0], np.cumsum(nk[:r])]).astype(np.int64)
    return [(int(first[i]), int(count[i]), allk[at[i]:at[i + 1]].copy()) for i in range(r)]


def check_shape(passes, n, capacity):
    at = 0
    for first, count, keys in passes:
        assert first == at and count > 0, "the passes tile [0, n) in order"
        assert (np.diff(keys.astype(np.int64)) > 0).all() and len(keys) <= capacity
        at += count
    assert at == n


def scope_case():
    """random_case(3) with the sensor range at which the units of its lattices differ, the keys of its blocks, its map as a MapIndex"""
    case = random_case(3)
    case["cam"] = dict(case["cam"], max_sensor_depth=SCOPE_DEPTH)
    case["keys"] = np.sort(pack(case["blocks"][0]))
    return case


def lattice_plan(SS, case, margin=MARGIN):
    """The lattice of LATTICE around small_lattice(case): (anchors, rot, table, dstep, n, capacity, the largest single-slab selection,
    the per-entry selections, the plan at capacity = largest slab + margin)"""
    anchors, rot = small_lattice(case)
    cam, half = case["cam"], LATTICE["half"]
    table, dstep = lattice_table(SS, cam, anchors, rot), dstep_of(cam, LATTICE["trans_step"])
    entries = len(anchors) * len(rot)
    slabs = [len(unit(SS, case["keys"], cam, table, half, dstep, 0, e, x, x + 1)) for e in range(entries) for x in range(2 * half[0] + 1)]
    whole = [len(unit(SS, case["keys"], cam, table, half, dstep, 0, e, 0, 2 * half[0] + 1)) for e in range(entries)]
    n = entries * int(np.prod([2 * h + 1 for h in half]))
    cap = max(slabs) + margin
    return dict(anchors=anchors, rot=rot, table=table, dstep=dstep, n=n, capacity=cap, largest=max(slabs), whole=whole,
                passes=plan(SS, case["keys"], cam, table, half, dstep, 0, n, cap))


def plain_plan(SS, case, margin=MARGIN):
    poses = random_poses(case, N_POSES)
    table = plain_table(SS, case["cam"], poses)
    sizes = [len(unit(SS, case["keys"], case["cam"], table, (0, 0, 0), 0.0, 1, e)) for e in range(N_POSES)]
    cap = max(sizes) + margin
    return dict(poses=poses, table=table, n=N_POSES, capacity=cap, largest=max(sizes), sizes=sizes,
                passes=plan(SS, case["keys"], case["cam"], table, (0, 0, 0), 0.0, 1, N_POSES, cap))


# ------------------------------------------------------------------ the widening
def random_store(rng, share=0.5):
    return BOX[rng.random(len(BOX)) < share].copy()


def test_extra_zero_changes_nothing(SS):
    """300 random poses over a random store, two sets of intrinsics, and the poses the function answers with the whole store: with
    extra = 0 the selection is the one without the argument, key for key."""
    rng = np.random.default_rng(3)
    keys = random_store(rng)
    sizes = set()
    for k in range(300):
        cam = CAMS[k % 2]
        pose = np.array(random_pose(rng), f32)
        if k % 50 == 7:
            pose[:3, :3] *= f32(1.01)                                   # not rigid: the whole store, with the argument too
        a, b = select(SS, keys, cam, pose), select(SS, keys, cam, pose, 0.0)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), k
        assert a[0] == (k % 50 != 7) and (a[0] or len(a[1]) == len(keys))
        sizes.add(len(a[1]))
    assert len(sizes) > 100 and min(sizes) < len(keys) // 4
    wide = select(SS, keys, CAMS[0], np.array(random_pose(rng), f32), 0.2)
    assert wide[0] and len(wide[1]) > 0
    for bad in (-0.1, float("nan"), float("inf")):                      # no widening the bound is defined for: the whole store
        got = select(SS, keys, CAMS[0], np.array(random_pose(rng), f32), bad)
        assert not got[0] and len(got[1]) == len(keys)


def test_the_widened_selection_is_a_superset(SS):
    """Random lattices over the dense box of tests/test_locate_scope.py (max_sensor_depth 1 m): a random anchor, rotations that
    turn it by up to 40 degrees about two axes, a non-cubic half, a sub-range of ix.  The unit's selection holds the plain
    selection at the float pose of every candidate of the unit, and the rule is not vacuous: the unit selects less than the store,
    and a unit is more than any one of its candidates."""
    from tandem_amd.dr_fusion import pose_rotations
    rng = np.random.default_rng(5)
    grew = 0
    for it in range(6):
        cam = CAMS[it % 2]
        anchor = np.array(random_pose(rng), f32)
        rot = pose_rotations([0.0, float(rng.uniform(-40, 40))], [float(rng.uniform(-25, 25))])
        half = [(2, 1, 0), (3, 0, 2), (1, 2, 1)][it % 3]
        ts = float(rng.uniform(0.04, 0.12))
        table, dstep = lattice_table(SS, cam, anchor[None], rot), dstep_of(cam, ts)
        N = [2 * h + 1 for h in half]
        for e in range(len(rot)):
            x0 = int(rng.integers(0, N[0]))
            x1 = int(rng.integers(x0 + 1, N[0] + 1))
            if it == 0 and e == 0:
                x0, x1 = 0, N[0]                                        # a whole entry
            sel = unit(SS, BOX, cam, table, half, dstep, 0, e, x0, x1)
            assert 0 < len(sel) < len(BOX)
            have = set(sel.tolist())
            first, count = (e * N[0] + x0) * N[1] * N[2], (x1 - x0) * N[1] * N[2]
            largest = 0
            for c in range(first, first + count):
                p16, R, tv = candidate(SS, cam, table, half, dstep, 0, c)
                cut, mine = select(SS, BOX, cam, p16)
                assert cut and len(mine) > 0
                assert set(mine.tolist()) <= have, (it, e, x0, x1, c)
                largest = max(largest, len(mine))
            grew += len(sel) > largest
    assert grew >= 6


# ------------------------------------------------------------------ the plan
@pytest.fixture(scope="module")
def P(SS):
    case = scope_case()
    return dict(case=case, lattice=lattice_plan(SS, case), plain=plain_plan(SS, case))


def sub_blocks(case, keys):
    """the blocks of the case whose keys are among `keys`"""
    mine = np.isin(pack(case["blocks"][0]), keys)
    return case["blocks"][0][mine], case["blocks"][1][mine]


def test_plan_shape(SS, P):
    """Passes tile [0, n) in order without gaps, keys ascend without repeats, every pass is within the capacity; the capacities
    force at least 3 passes and, for the lattice, an ix split; an empty store gives one pass without keys; a capacity one below the
    largest single-slab selection fails with that count."""
    case = P["case"]
    lat, pl = P["lattice"], P["plain"]
    for name, p in (("lattice", lat), ("plain", pl)):
        print("%s: largest single selection %d of %d blocks, capacity %d, passes %s" %
              (name, p["largest"], len(case["keys"]), p["capacity"], [(f, c, len(k)) for f, c, k in p["passes"]]))
        assert p["largest"] + MARGIN < len(case["keys"])
        check_shape(p["passes"], p["n"], p["capacity"])
        assert len(p["passes"]) >= 3
    cells = 15
    assert max(lat["whole"]) > lat["capacity"]                         # a whole entry does not fit: it is halved along ix
    assert any(f % cells or c % cells for f, c, _ in lat["passes"])      # ... and a pass ends inside an entry
    assert any(len(k) == 0 for _, _, k in pl["passes"]) or min(pl["sizes"]) == 0   # poses that look away or sit 300 blocks off select nothing
    none = np.zeros(0, np.uint64)
    for table, half, ds, plain, n in ((lat["table"], LATTICE["half"], lat["dstep"], 0, lat["n"]), (pl["table"], (0, 0, 0), 0.0, 1, pl["n"])):
        got = plan(SS, none, case["cam"], table, half, ds, plain, n, 4)
        assert len(got) == 1 and got[0][0] == 0 and got[0][1] == n and len(got[0][2]) == 0
    assert plan(SS, case["keys"], case["cam"], lat["table"], LATTICE["half"], lat["dstep"], 0, lat["n"], lat["largest"] - 1) == ("failed", lat["largest"])
    assert plan(SS, case["keys"], case["cam"], pl["table"], (0, 0, 0), 0.0, 1, pl["n"], pl["largest"] - 1) == ("failed", pl["largest"])
    # a capacity that holds the store: one pass, the union of everything
    got = plan(SS, case["keys"], case["cam"], lat["table"], LATTICE["half"], lat["dstep"], 0, lat["n"], len(case["keys"]))
    assert len(got) == 1 and got[0][1] == lat["n"] and len(got[0][2]) >= lat["largest"]


def test_the_plan_is_sufficient_for_the_lattice(SS, P):
    """Every pass of the lattice's plan: the restatement over only the pass's keys scores the pass's candidates as the restatement
    over all blocks does, bit for bit -- and a pass is no formality: over no block at all the same candidates score otherwise."""
    case, lat = P["case"], P["lattice"]
    cam = case["cam"]
    o = np_score_options(cam, step=SCOPE_STEP)
    R, tv = np_candidates(cam, lat["anchors"], lat["rot"], LATTICE["half"], LATTICE["trans_step"])
    assert len(R) == lat["n"]
    want = np_score_candidates(case["blocks"], cam, case["depth"], R, tv, o)
    assert want[1][:, 1].max() > 300 and want[1][0, 0] > 1000
    for first, count, keys in lat["passes"]:
        s = slice(first, first + count)
        got = np_score_candidates(sub_blocks(case, keys), cam, case["depth"], R[s], tv[s], o)
        assert_same_scores(got, tuple(w[s] for w in want), "pass at %d" % first)
        assert len(keys) < len(case["keys"])
    none = np_score_candidates(sub_blocks(case, np.zeros(0, np.uint64)), cam, case["depth"], R, tv, o)
    assert (bits(none[2]) != bits(want[2])).any()
    # the candidates the plan was made for are the restatement's
    for c in (0, 17, lat["n"] - 1):
        _, Rc, tc = candidate(SS, cam, lat["table"], LATTICE["half"], lat["dstep"], 0, c)
        assert np.array_equal(bits(Rc), bits(R[c])) and np.array_equal(bits(tc), bits(tv[c]))


def test_the_plan_is_sufficient_for_a_plain_table(SS, P):
    """The same for the plain table of 259 poses (no multiple of 4 or 64; every seventh looks away, every eleventh sits 300 blocks off)."""
    case, pl = P["case"], P["plain"]
    cam = case["cam"]
    o = np_score_options(cam, step=SCOPE_STEP)
    mv = [motion(p, cam["voxel_size"]) for p in pl["poses"]]
    R, tv = np.stack([m[0] for m in mv]), np.stack([m[1] for m in mv])
    want = np_score_candidates(case["blocks"], cam, case["depth"], R, tv, o)
    assert want[1][:, 1].max() > 300 and (want[1][:, 1] == 0).any()
    for first, count, keys in pl["passes"]:
        s = slice(first, first + count)
        got = np_score_candidates(sub_blocks(case, keys), cam, case["depth"], R[s], tv[s], o)
        assert_same_scores(got, tuple(w[s] for w in want), "pass at %d" % first)


def test_sanitizer_run_of_the_stand_alone_program(SS, P, tmp_path):
    """plan_search_stage under AddressSanitizer and UBSan: a plain executable with its own main, nothing preloaded, nothing loaded
    into Python.  It reads the inputs of the two plans above from a file, checks each plan's shape and that every pass holds the
    plain selection of each of its candidates, and prints the passes, which are the ones made here."""
    exe, data = str(tmp_path / "search_scope_san"), str(tmp_path / "case.bin")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/search_scope_san.cpp"), "-o", exe])
    case, lat, pl = P["case"], P["lattice"], P["plain"]
    anchors, rot = np.ascontiguousarray(lat["anchors"], f32).reshape(-1, 16), np.ascontiguousarray(lat["rot"], f64).reshape(-1, 9)
    poses = np.ascontiguousarray(pl["poses"], f32).reshape(-1, 16)
    with open(data, "wb") as fh:
        fh.write(np.uint64(len(case["keys"])).tobytes() + case["keys"].tobytes() + bytes(Camera(**case["cam"])))
        fh.write(np.uint64(len(anchors)).tobytes() + anchors.tobytes() + np.uint64(len(rot)).tobytes() + rot.tobytes())
        fh.write(np.int32(LATTICE["half"]).tobytes() + f32(LATTICE["trans_step"]).tobytes() + np.uint64(lat["capacity"]).tobytes())
        fh.write(np.uint64(len(poses)).tobytes() + poses.tobytes() + np.uint64(pl["capacity"]).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "search_scope_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith(("lattice", "plain"))}
    for name, p in (("lattice", lat), ("plain", pl)):
        assert lines[name] == ["%d:%d:%d" % (f, c, len(k)) for f, c, k in p["passes"]], name


# ------------------------------------------------------------------ the C ABI, the mirror and the shim
def test_abi_declares_exports_and_types_the_two_functions():
    L = abi_module()
    src = check_symbols(L, ["drf_set_search_scope", "drf_search_stage_stats"])
    assert "#define DRF_SEARCH_RESIDENT 0" in src and "#define DRF_SEARCH_MAP      1" in src
    assert "int drf_set_search_scope(drf_t *h, int scope, size_t stage_capacity_blocks);" in src
    assert "int drf_search_stage_stats(drf_t *h, uint64_t out[4]);" in src
    with open(os.path.join(ROOT, "include", "dr_mi355x.h")) as fh:
        assert "DRF_LOCATE_MAP does not apply to the score" in fh.read()
    lib = L.lib()
    assert lib.drf_set_search_scope(None, 1, 0) == 1 and lib.drf_search_stage_stats(None, (C.c_uint64 * 4)()) == 1
    from tandem_amd import dr_fusion
    assert (dr_fusion.SEARCH_RESIDENT, dr_fusion.SEARCH_MAP) == (0, 1)
    assert callable(dr_fusion.DrFusion.set_search_scope) and callable(dr_fusion.DrFusion.search_stage_stats)


def test_shim_compiles(tmp_path):
    """tandem_amd/libdr/dr_fusion.h SetSearchScope / SearchStageStats as a TANDEM translation unit would call them
    (tests/cpp/search_scope_shim.cpp): it compiles and links against the library; tests/test_fusion_search_scope_gpu.py runs it."""
    abi_module()
    exe = str(tmp_path / "search_scope_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tandem_amd", "libdr"),
                           os.path.join(ROOT, "tests/cpp/search_scope_shim.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert os.path.isfile(exe)
