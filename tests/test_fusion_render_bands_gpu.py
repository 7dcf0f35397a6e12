"""-m gpu: depth-banded map-scope renders (drf_set_render_bands): a RenderAsync whose stored blocks exceed the render staging is
staged and ray-cast one depth band after the other, and equals the CPU oracle, whose pool never runs out -- depth (as uint32) and
colour bit for bit -- while no block moves.  DESIGN.md §7c "Rendering beyond the staging".

The scene: three depth layers.  A 96x128 camera (1 cm voxels, 4 cm truncation, 3 m depth range) sees vertical stripes of constant
depth 0.8, 1.6 and 2.4 m from one place; the map goes through a map file into the HOST STORE of a streaming engine, so every
block a render reads is staged.  The staging capacity C of each test is chosen here, on the CPU, with the planner itself
(tests/cpp/render_bands_check.cpp) on the blocks the engine stores: the smallest of a few fractions of the union at which the
plan has at least the wanted number of passes -- and the tests assert union > C, the number of passes and largest pass <= C
from the engine's own statistics, so that none can pass by fitting in one pass."""
import math
import os
import subprocess

import numpy as np
import pytest

from fusion_helpers import options, shifted
from test_fusion_render_bands import build_check_library, pack, plan, union
from test_fusion_render_scope_gpu import hit_blocks, same_render, step
from test_fusion_streaming_gpu import assert_same_blocks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_PASSES = 8


def rot(axis, deg):
    a, (i, j) = math.radians(deg), {"x": (1, 2), "y": (2, 0)}[axis]
    R = np.eye(4, dtype=np.float64)
    R[i, i], R[i, j], R[j, i], R[j, j] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    return R


def at(R, centre):
    T = np.array(R, np.float64)
    T[:3, 3] = centre
    return T.astype(np.float32)


def layer_scans(H, W, seed):
    """Two scans from one place (the second turned by 1 degree): vertical stripes at 0.8, 1.6 and 2.4 m, seeded colour."""
    rng = np.random.default_rng(seed)
    stripe = (np.arange(W) * 6 // W) % 3
    depth = np.tile(np.array([0.8, 1.6, 2.4], np.float32)[stripe], (H, 1))
    depth[:2, :] = 0.0  # a border of invalid pixels
    scans = []
    for k in range(2):
        bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        scans.append((bgr, depth.copy(), at(rot("y", float(k)), (0.05, -0.03, 0.1))))
    return scans


def build_world(tmp, H, W, f, seed):
    """The scans in the oracle and in an engine whose pool holds them all (checked against each other scan by scan); the
    engine's map file; the planner library."""
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions
    sc = dict(fx=f, fy=f, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0)
    opt = options(sc, H, W, 0.01, max_sensor_depth=3.0, num_blocks=20000, num_buckets=20000)
    assert opt["truncation_distance"] == 0.04
    scans = layer_scans(H, W, seed)
    u, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**opt)
    for k, (bgr, depth, pose) in enumerate(scans):
        step(u, o, bgr, depth, pose, [pose], f"scan {k}")
    path = str(tmp / f"layers_{H}x{W}.drfmap")
    u.save_map(path)
    u.close()
    blocks = o.export_blocks()
    assert 1000 < len(blocks) < opt["num_blocks"]
    return dict(o=o, opt=opt, path=path, scans=scans, blocks=blocks, lib=build_check_library(str(tmp / f"librb_{H}x{W}.so")))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return build_world(tmp_path_factory.mktemp("render_bands"), 96, 128, 200.0, seed=5)


def streaming_engine(w, streams=1):
    """A streaming engine with the whole map in its host store, in map scope."""
    from tandem_amd.dr_fusion import RENDER_MAP, DrFusion, DrFusionOptions, streaming_min_radius
    f = DrFusion(DrFusionOptions(**dict(w["opt"], num_render_streams=streams)))
    f.set_streaming(streaming_min_radius(f.options))
    f.load_map(w["path"])
    st = f.streaming_stats()
    assert st["resident"] == 0 and st["host"] == len(w["blocks"])
    f.set_render_scope(RENDER_MAP)
    return f


def stored_keys(f):
    return np.sort(pack(np.array(sorted(f.export_host_blocks()), np.int64)))


def choose_capacity(w, f, poses, min_passes=3):
    """(C, passes, union): the smallest of a few fractions of the union at which the planner -- run here on the engine's stored
    blocks -- finds at least min_passes passes within MAX_PASSES."""
    keys = stored_keys(f)
    n = len(union(w["lib"], keys, f.options, poses))
    for frac in (0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9):
        cap = int(math.ceil(frac * n))
        got = plan(w["lib"], keys, f.options, poses, cap, MAX_PASSES)
        if got is not None and len(got[1]) >= min_passes:
            assert all(len(p) <= cap for p in got[1]) and cap < n
            return cap, len(got[1]), n
    raise AssertionError(f"no capacity bands the {n} blocks of these poses in {min_passes}..{MAX_PASSES} passes")


def render(f, poses):
    f.RenderAsync(poses)
    return f.GetRenderResult()


def refused(f, poses):
    from tandem_amd import _lib
    with pytest.raises(_lib.DrError) as e:
        f.RenderAsync(poses)
    return e.value.code


def assert_banded(f, cap, n_union, min_passes=3):
    bs, rs = f.render_band_stats(), f.render_stats()
    assert n_union > cap and rs[0] == n_union, (rs, cap, n_union)
    assert bs[0] >= min_passes and bs[1] <= cap and bs[3] == 1, (bs, cap)
    assert bs[2] >= n_union and rs[1] == bs[2] * (8 + 4096), (bs, rs)


SCAN = at(rot("y", 0.0), (0.05, -0.03, 0.1))
TURNED = at(rot("y", 30.0) @ rot("x", 10.0), (-0.75, 0.12, 0.35))   # camera z is not world z
BACK = at(rot("y", 180.0) @ rot("x", -4.0), (0.1, 0.05, 2.95))      # from behind the far layer, looking back
POSES = {"scan pose": SCAN, "turned 30 degrees": TURNED, "looking back": BACK}


def test_banded_render_equals_the_oracle_where_one_pass_is_refused(world):
    """Cannot pass without the feature: at capacity C one pass is DR_ERR_CAPACITY (code 5), and only depth bands get through."""
    from tandem_amd.dr_fusion import RENDER_MAP
    f, o = streaming_engine(world), world["o"]
    before = (f.streaming_stats(), f.export_host_blocks())
    for what, pose in POSES.items():
        want = o.render(pose)
        assert (want[1] > 0).mean() > 0.3, f"{what}: the pose must see the layers"
        f.set_render_scope(RENDER_MAP, 0)
        f.set_render_bands(0)
        rb, rd = render(f, [pose])
        same_render(rb[0], rd[0], want, f"{what}, one pass")
        n = f.render_stats()[0]
        assert f.render_band_stats() == (1, n, n, 0)
        cap, passes, n_plan = choose_capacity(world, f, [pose])
        assert n_plan == n
        f.set_render_scope(RENDER_MAP, cap)
        assert refused(f, [pose]) == 5, f"{what}: {n} blocks must not fit {cap}"
        f.set_render_bands(MAX_PASSES)
        rb, rd = render(f, [pose])
        assert_banded(f, cap, n)
        assert f.render_band_stats()[0] == passes
        same_render(rb[0], rd[0], want, f"{what}, {passes} bands of at most {cap} of {n} blocks")
    assert f.streaming_stats() == before[0]
    assert_same_blocks(f.export_host_blocks(), before[1], "host store after the banded renders")
    assert f.export_blocks() == {}
    f.close()


def test_two_render_streams_share_the_bands(world):
    from tandem_amd.dr_fusion import RENDER_MAP
    f, o = streaming_engine(world, streams=2), world["o"]
    poses = [TURNED, SCAN]
    cap, passes, n = choose_capacity(world, f, poses)
    f.set_render_scope(RENDER_MAP, cap)
    f.set_render_bands(MAX_PASSES)
    rb, rd = render(f, poses)
    assert_banded(f, cap, n)
    for i, p in enumerate(poses):
        same_render(rb[i], rd[i], o.render(p), f"stream {i} of a render in {passes} bands")
    rb, rd = render(f, poses[::-1])                                     # the per-stream state is reused: the first band starts it afresh
    for i, p in enumerate(poses[::-1]):
        same_render(rb[i], rd[i], o.render(p), f"stream {i} of the second banded render")
    f.close()


def test_rays_cross_resident_blocks_then_staged_blocks_of_several_bands(world):
    from tandem_amd.dr_fusion import RENDER_MAP
    f, o, opt = streaming_engine(world), world["o"], world["opt"]
    f.stream_in_region((-10.0, -10.0, -10.0), (10.0, 10.0, 1.0))       # the near layer and the space before it
    resident, host = f.export_blocks(), f.export_host_blocks()
    assert len(resident) > 200 and len(host) > 200 and len(resident) + len(host) == len(world["blocks"])
    st = f.streaming_stats()
    cap, passes, n = choose_capacity(world, f, [SCAN], min_passes=2)
    f.set_render_scope(RENDER_MAP, cap)
    f.set_render_bands(MAX_PASSES)
    rb, rd = render(f, [SCAN])
    assert_banded(f, cap, n, min_passes=2)
    want = o.render(SCAN)
    same_render(rb[0], rd[0], want, f"pool and {passes} bands")
    hits = hit_blocks(opt, SCAN, want[1])
    assert sum(b in resident for b in hits) > 500 and sum(b in host for b in hits) > 500
    assert f.streaming_stats() == st
    assert_same_blocks(f.export_blocks(), resident, "pool after the banded render")
    assert_same_blocks(f.export_host_blocks(), host, "host store after the banded render")
    f.close()


def test_refusals_leave_everything_as_it_was(world):
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import RENDER_MAP
    f, o = streaming_engine(world), world["o"]
    cap, passes, n = choose_capacity(world, f, [SCAN])
    rb, rd = render(f, [SCAN])                                          # a first render, so that there are statistics to keep
    kept = (f.streaming_stats(), f.export_host_blocks(), f.render_stats(), f.render_band_stats())
    assert kept[3] == (1, n, n, 0)

    def unchanged(what):
        assert f.streaming_stats() == kept[0], what
        assert_same_blocks(f.export_host_blocks(), kept[1], what)
        assert f.render_stats() == kept[2] and f.render_band_stats() == kept[3], what
        with pytest.raises(_lib.DrError) as e:                          # the protocol still expects RenderAsync
            f.GetRenderResult()
        assert e.value.code == 2, what
    f.set_render_scope(RENDER_MAP, cap)
    f.set_render_bands(2)                                               # the plan needs at least three passes
    assert passes >= 3 and refused(f, [SCAN]) == 5
    unchanged("two passes allowed")
    f.set_render_bands(MAX_PASSES)
    f.set_render_scope(RENDER_MAP, 20)                                  # below the thinnest band
    assert refused(f, [SCAN]) == 5
    unchanged("capacity below the thinnest band")
    bad = SCAN.copy()
    bad[0, 1] += 0.01                                                   # not rigid: the whole store in every pass
    f.set_render_scope(RENDER_MAP, len(world["blocks"]) - 1)
    assert refused(f, [bad]) == 5
    unchanged("a pose that is not rigid")
    f.set_render_scope(RENDER_MAP, cap)
    for bad_passes in (-1, 65):
        with pytest.raises(_lib.DrError) as e:
            f.set_render_bands(bad_passes)
        assert e.value.code == 1
    assert f._L.drf_render_band_stats(f._h, None) == 1
    f.RenderAsync([SCAN])                                               # the retry with 8 goes through
    with pytest.raises(_lib.DrError) as e:                              # between RenderAsync and GetRenderResult
        f.set_render_bands(4)
    assert e.value.code == 2
    rb, rd = f.GetRenderResult()
    assert_banded(f, cap, n)
    same_render(rb[0], rd[0], o.render(SCAN), "the retry with eight passes allowed")
    f.set_render_bands(1)                                               # off again: the same call is refused as before
    assert refused(f, [SCAN]) == 5
    f.close()


def test_a_union_that_fits_runs_in_one_pass_whatever_max_passes_is(world):
    f, o = streaming_engine(world), world["o"]
    rb, rd = render(f, [TURNED])
    off = (f.render_stats(), f.render_band_stats())
    n = off[0][0]
    assert n > 0 and off[1] == (1, n, n, 0)
    f.set_render_bands(64)
    rb, rd = render(f, [TURNED])
    assert (f.render_stats(), f.render_band_stats()) == off
    same_render(rb[0], rd[0], o.render(TURNED), "bands allowed, one pass")
    away = at(rot("y", 0.0), (50.0, 0.0, 0.0))                          # nothing in reach: nothing staged
    rb, rd = render(f, [away])
    assert f.render_stats() == (0, 0, 0, 0) and f.render_band_stats() == (0, 0, 0, 0)
    assert not rd[0].any()
    f.close()


def test_untiled_image_size(tmp_path):
    """50x70: neither a multiple of 8, so the kernels index pixels row-wise and the last wave is partly idle."""
    from tandem_amd.dr_fusion import RENDER_MAP
    w = build_world(tmp_path, 50, 70, 110.0, seed=8)
    f, o = streaming_engine(w), w["o"]
    for what, pose in POSES.items():
        cap, passes, n = choose_capacity(w, f, [pose])
        f.set_render_scope(RENDER_MAP, cap)
        f.set_render_bands(0)
        assert refused(f, [pose]) == 5
        f.set_render_bands(MAX_PASSES)
        rb, rd = render(f, [pose])
        assert_banded(f, cap, n)
        want = o.render(pose)
        assert (want[1] > 0).mean() > 0.3
        same_render(rb[0], rd[0], want, f"50x70, {what}, {passes} bands")
    f.close()


def test_literal_pass_across_bands(tmp_path):
    """The scene of tests/test_fusion_render_scope_gpu.py::test_stored_blocks_beyond_the_dense_grid: stored blocks on both sides
    of block coordinate 256, so pixels bail out of the fast ray-caster into k_raycast_fix -- here in a banded render.
    How the test knows that pixels were flagged: the product exposes no counter, but the fast ray-caster cannot read a block
    outside the dense grid at all (it bails instead), so every pixel whose final sample lies in a STORED block with x >= 256
    and that still equals the oracle went through the literal pass; the test asserts more than 100 such pixels."""
    from synth import scene
    from oracle.tsdf_oracle import TsdfOracle
    from tandem_amd.dr_fusion import RENDER_MAP, DrFusion, DrFusionOptions, streaming_min_radius
    H, W, vs = 96, 128, 0.02
    sc = scene.make_scans(4, H, W, seed=6)
    opt = options(sc, H, W, vs)
    S = np.eye(4, dtype=np.float32)
    c, s = np.cos(1.45), np.sin(1.45)
    S[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    S[:3, 3] = (40.2, 0.3, -0.2)
    far_scans = shifted(sc["scans"], S)
    f, o = DrFusion(DrFusionOptions(**opt)), TsdfOracle(**opt)
    f.set_streaming(streaming_min_radius(f.options))
    f.set_render_scope(RENDER_MAP)
    for i in range(2):
        step(f, o, *far_scans[i], [far_scans[i][2]], f"shifted scan {i}")
    back = far_scans[1][2]
    step(f, o, *sc["scans"][0], [back], "scan 0 at the origin, looking back")   # 40 m away: everything above is evicted
    bgr, depth, pose = sc["scans"][1]
    f.IntegrateScanAsync(bgr, depth, pose)
    assert o.integrate(bgr, depth, pose) == 0
    stored = set(f.export_host_blocks())
    assert max(k[0] for k in stored) >= 256 > min(k[0] for k in stored)
    cap, passes, n = choose_capacity(dict(lib=build_check_library(str(tmp_path / "librb.so"))), f, [back], min_passes=2)
    f.set_render_scope(RENDER_MAP, cap)
    assert refused(f, [back]) == 5
    f.set_render_bands(MAX_PASSES)
    rb, rd = render(f, [back])
    assert_banded(f, cap, n, min_passes=2)
    want = o.render(back)
    same_render(rb[0], rd[0], want, f"look back in {passes} bands")
    hits = hit_blocks(opt, back, want[1])
    assert sum(b[0] >= 256 and b in stored for b in hits) > 100, "the render back must hit stored blocks beyond the border"
    assert_same_blocks(f.export_all_blocks(), o.export_blocks(), "whole map")
    f.close()


def test_shim_renders_in_bands(world, tmp_path):
    """tandem_amd/libdr/dr_fusion.h: SetRenderBands.  tests/cpp/render_bands_shim.cpp renders its own scene from the pool and,
    banded, from the host store of a second DrFusion.  Its capacity comes from here: the program's map, loaded into an engine
    with the program's options, is refused at that capacity with bands off -- the shim exits on a refusal, so its success is
    a banded render."""
    from tandem_amd.dr_fusion import RENDER_MAP, DrFusion, DrFusionOptions, streaming_min_radius
    exe, path = str(tmp_path / "render_bands_shim"), str(tmp_path / "shim.drfmap")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tandem_amd", "libdr"), os.path.join(ROOT, "tests/cpp/render_bands_shim.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x", "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    r = subprocess.run([exe, path, "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "render_bands_shim ok" in r.stdout, r.stdout + r.stderr
    opt = dict(world["opt"], fx=200.0, fy=200.0, cx=63.5, cy=47.5, height=96, width=128)   # the program's options
    pose = np.array([1, 0, 0, 0.1, 0, 1, 0, -0.05, 0, 0, 1, 0.2, 0, 0, 0, 1], np.float32).reshape(4, 4)
    f = DrFusion(DrFusionOptions(**opt))
    f.set_streaming(streaming_min_radius(f.options))
    f.load_map(path)
    cap, passes, n = choose_capacity(world, f, [pose], min_passes=2)
    f.set_render_scope(RENDER_MAP, cap)
    assert refused(f, [pose]) == 5
    f.close()
    r = subprocess.run([exe, path, str(cap)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "render_bands_shim ok" in r.stdout, r.stdout + r.stderr
