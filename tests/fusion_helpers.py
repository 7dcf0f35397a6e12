"""Scaffolding shared by tests/test_fusion_*.py (a plain module, imported by them): engine options, the operator round against the
oracle, mesh comparison, the synthetic scenes, and the check of the C ABI surface."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 100000  # blocks of the reference engines and of the oracle: their pools never run out


def options(sc, H, W, vs, **kw):
    d = dict(voxel_size=vs, num_buckets=40000, bucket_size=10, num_blocks=40000, block_size=8, max_sdf_weight=64,
             truncation_distance=4 * vs, max_sensor_depth=10.0, min_sensor_depth=0.1, num_render_streams=1,
             fx=sc["fx"], fy=sc["fy"], cx=sc["cx"], cy=sc["cy"], height=H, width=W)
    d.update(kw)
    return d


def unbounded(opt):
    return dict(opt, num_blocks=BIG, num_buckets=BIG)


def feed(f, bgr, depth, pose):
    f.IntegrateScanAsync(bgr, depth, pose)
    f.RenderAsync([pose])
    f.GetRenderResult()


def step(f, o, bgr, depth, pose, what):
    """One operator round on the engine and the oracle: the ray-cast at the scan pose and the update count must agree.
    Returns the oracle's depth image."""
    f.IntegrateScanAsync(bgr, depth, pose)
    f.RenderAsync([pose])
    rb, rd = f.GetRenderResult()
    assert o.integrate(bgr, depth, pose) == 0
    ob, od = o.render(pose)
    assert np.array_equal(rd[0].view(np.uint32), od.view(np.uint32)), f"{what}: ray-cast depth differs at {(rd[0] != od).sum()} px"
    assert np.array_equal(rb[0], ob), f"{what}: ray-cast colour differs"
    assert f.stats()["updated_last"] == o.stats()["updated_last"], what
    return od


def rows(vert, cols):
    """(ntri, 18) uint32: the triangle's 9 coordinates and 9 colour values, bit patterns, in the order returned."""
    return np.concatenate([vert.reshape(-1, 9), cols.reshape(-1, 9)], axis=1).view(np.uint32)


def canon(vert, cols):
    """rows(), sorted (as tests/test_mesh_gpu.py compares meshes)."""
    t = rows(vert, cols)
    return t[np.lexsort(t.T[::-1])]


def assert_same_mesh(a, b, what):
    """Byte for byte, triangle order included."""
    ra, rb = rows(*a), rows(*b)
    assert ra.shape == rb.shape, f"{what}: {len(ra)} vs {len(rb)} triangles"
    bad = np.flatnonzero((ra != rb).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(ra)} triangles differ, first at {bad[0]}"


def box_of(blocks, vs):
    c = np.array(list(blocks), np.int64)
    return tuple(float(v) for v in (c.min(0) * 8 - 2) * vs), tuple(float(v) for v in ((c.max(0) + 1) * 8 + 2) * vs)


def shifted(scans, S):
    return [(b, d, (S @ p).astype(np.float32)) for b, d, p in scans]


def places(n_places, scans_per_place=2, seed=3, spacing=20.0, **kw):
    """The scans of synth.scene at n_places places `spacing` metres apart along x, and the engine options (kw overrides them)."""
    from synth import scene
    H, W = 96, 128
    sc = scene.make_scans(scans_per_place, H, W, seed=seed)
    out = []
    for p in range(n_places):
        S = np.eye(4, dtype=np.float32)
        S[:3, 3] = (spacing * p, 0.0, 0.0)
        out.append(shifted(sc["scans"], S))
    return out, options(sc, H, W, 0.02, **dict(dict(max_sensor_depth=6.0), **kw))


def room_frames():
    """The 60-frame loop through synth.room at 96x128 (body of the per-file room fixtures): the rendered frames, them as
    (bgr, depth, pose) scans, H, W."""
    import torch  # noqa: F401  (synth.room renders with torch)
    from synth import room
    H, W, N = 96, 128, 60
    poses = room.loop_poses(N, seed=0)
    fr = room.render_frames(poses, H, W)
    frames = [(fr["bgr"][k].numpy(), fr["depth"][k].numpy(), np.asarray(poses[k], np.float32)) for k in range(N)]
    return fr, frames, H, W


# ---- the C ABI surface (CPU tests) ----
def abi_module():
    """tandem_amd._lib, the library built first if it is not there (body of the per-file L fixtures)."""
    import __graft_entry__ as g
    if not os.path.isfile(os.path.join(ROOT, "tandem_amd", "libdr_mi355x.so")):
        g.build()
    from tandem_amd import _lib
    return _lib


def header():
    """include/dr_mi355x.h without its block comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dr_mi355x.h")).read(), flags=re.S)


def check_symbols(L, names):
    """Every name is declared in the header, exported by the library and typed in tandem_amd/_lib.py; returns the header."""
    src = header()
    lib = C.CDLL(L.LIB_PATH)
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    return src
