"""CPU: marching cubes.  (1) The packed triangle table (tandem_amd/csrc/mc_tables.h, Paul Bourke's public-domain
polygonise table) is checked structurally: every configuration's triangles use only cut edges, use every cut edge,
and form a closed, consistently cut surface inside the cube.  When the reference checkout is present its copy of the
published table (marching_cubes/lookup_tables.h) must pack to the same words.  (2) The oracle's ExtractMesh
restatement (mesh_extractor.cu:24-265) is pinned by a hand-derived known answer and by domain properties."""
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_CORNER = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
# Bourke corner positions: v0..v3 bottom ring, v4..v7 top ring
CORNER_XYZ = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]


def packed_table():
    src = open(os.path.join(ROOT, "tandem_amd", "csrc", "mc_tables.h")).read()
    body = re.search(r"kMcTri\[256\] = \{(.*?)\};", src, re.S).group(1)
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull", body)]
    assert len(words) == 256
    return words


def rows():
    out = []
    for w in packed_table():
        r = []
        for i in range(16):
            e = (w >> (4 * i)) & 15
            if e == 15:
                break
            r.append(e)
        out.append(r)
    return out


def faces_of_edge(e):
    a, b = (CORNER_XYZ[c] for c in EDGE_CORNER[e])
    return {(ax, a[ax]) for ax in range(3) if a[ax] == b[ax]}  # the two cube faces the edge lies in


def test_table_structure():
    T = rows()
    assert T[0] == [] and T[255] == []
    for c in range(256):
        r = T[c]
        assert len(r) % 3 == 0 and len(r) <= 15
        cut = {e for e, (a, b) in enumerate(EDGE_CORNER) if ((c >> a) & 1) != ((c >> b) & 1)}
        assert set(r) == cut, (c, r, cut)  # only cut edges, and every cut edge is used
        # undirected triangle sides: interior sides are shared by exactly 2 triangles; sides on a cube face appear
        # once and are the iso-contour segments of that face
        sides = Counter()
        for i in range(0, len(r), 3):
            t = r[i:i + 3]
            assert len(set(t)) == 3
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                sides[frozenset((a, b))] += 1
        boundary_per_edge = Counter()
        for s, n in sides.items():
            a, b = tuple(s)
            on_face = bool(faces_of_edge(a) & faces_of_edge(b))
            assert n == (1 if on_face else 2) or (on_face and n == 2), (c, s, n)
            if n == 1:
                assert on_face, (c, s)
                boundary_per_edge[a] += 1
                boundary_per_edge[b] += 1
        # closed contour on the cube surface: every cut edge is met by exactly two boundary segments
        assert all(boundary_per_edge[e] == 2 for e in cut), (c, boundary_per_edge)


def test_table_complement_symmetry():
    """Inside/outside swap cuts the same edges; the published table uses the same number of triangles or differs
    only in the ambiguous cases -- the cut-edge sets must be identical."""
    T = rows()
    for c in range(256):
        assert set(T[c]) == set(T[255 - c])


def test_table_equals_published_copy_in_reference():
    """tests/golden/mc_tri_table_reference.npz: the reference's triTable[256][16] (ref:tandem/libdr/dr_fusion/src/marching_cubes/
    lookup_tables.h, read by tools/pack_mc_tables.py::parse) as int8 rows."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pack_mc_tables
    ref = np.load(os.path.join(ROOT, "tests", "golden", "mc_tri_table_reference.npz"))["tri_table"].astype(int).tolist()
    assert len(ref) == 256 and all(len(r) == 16 and r[-1] == -1 for r in ref)
    assert [pack_mc_tables.pack(r) for r in ref] == packed_table()


# ------------------------------------------------------------------------------------------------ oracle mesh
def plane_oracle(vs=0.02, d0=1.0, H=48, W=64, n=1):
    from oracle.tsdf_oracle import TsdfOracle
    f = 0.78125 * W
    o = TsdfOracle(voxel_size=vs, num_buckets=20000, bucket_size=10, num_blocks=20000, block_size=8, max_sdf_weight=64,
                   truncation_distance=4 * vs, max_sensor_depth=10.0, min_sensor_depth=0.1, num_render_streams=1,
                   fx=f, fy=f, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0, height=H, width=W)
    bgr = np.zeros((H, W, 3), np.uint8)
    bgr[..., 0], bgr[..., 1], bgr[..., 2] = 10, 120, 250  # B, G, R
    for _ in range(n):
        assert o.integrate(bgr, np.full((H, W), d0, np.float32), np.eye(4, dtype=np.float32)) == 0
    return o


def test_oracle_mesh_of_a_plane():
    """Fronto-parallel plane at z = d0 seen from the origin: the zero crossing of the ray-length SDF is the plane
    itself, so every vertex lies within a fraction of a voxel of z = d0, inside the frustum, with the voxel colour
    (B,G,R) = (10,120,250) reported as RGB / 255."""
    vs, d0 = 0.02, 1.0
    o = plane_oracle(vs, d0)
    vert, cols = o.extract_mesh([-1.0, -1.0, 0.5], [1.0, 1.0, 1.5])
    assert len(vert) % 3 == 0 and len(vert) > 3000
    assert np.abs(vert[:, 2] - d0).max() < 0.5 * vs
    assert np.abs(vert[:, 0]).max() < 0.7 and np.abs(vert[:, 1]).max() < 0.55
    assert np.array_equal(cols, np.broadcast_to(np.array([250, 120, 10], np.float32) / np.float32(255), cols.shape))
    # no degenerate triangles, and the surface is oriented consistently (all normals on one side)
    t = vert.reshape(-1, 3, 3).astype(np.float64)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    area = np.linalg.norm(nrm, axis=1)
    assert (area > 0).mean() > 0.99
    assert (np.sign(nrm[area > 0][:, 2]) == np.sign(nrm[area > 0][0, 2])).all()
    # total area ~ area of the meshed part of the plane (bounded by the frustum footprint at d0)
    assert 0.5 < area.sum() / 2 < (2 * 0.7) * (2 * 0.55)


def test_oracle_mesh_empty_and_box_clipping():
    o = plane_oracle()
    v, c = o.extract_mesh([2.0, 2.0, 2.0], [3.0, 3.0, 3.0])  # observed nowhere
    assert len(v) == 0 and len(c) == 0
    v, _ = o.extract_mesh([0.0, 0.0, 0.5], [0.0, 1.0, 1.5])  # degenerate box: zero cells along x
    assert len(v) == 0
    full, _ = o.extract_mesh([-1.0, -1.0, 0.5], [1.0, 1.0, 1.5])
    half, _ = o.extract_mesh([0.0, -1.0, 0.5], [1.0, 1.0, 1.5])  # lattice starts at x = 0: only cells with x >= 0
    assert 0 < len(half) < len(full)
    assert half[:, 0].min() >= -0.02
    # swapping the corners changes nothing but the lattice origin (size = |lower - upper|, mesh_extractor.cu:241-242)
    swapped, _ = o.extract_mesh([1.0, 1.0, 1.5], [-1.0, -1.0, 0.5])
    assert len(swapped) == 0 or swapped[:, 0].min() >= 0.9  # lattice now starts at the upper corner


def test_oracle_mesh_known_answer_single_cell():
    """One lattice cell, by hand: with lower = voxel-aligned and box of one voxel, the cell position P sits on a
    voxel centre, each cube corner value is the mean of the 8 surrounding voxels' sdf (weights exactly 0.5), and a
    cut edge between corner values (a, b) puts the vertex at p1 + (-a / (b - a)) * (p2 - p1)."""
    vs, d0 = 0.02, 1.0
    o = plane_oracle(vs, d0)
    blocks = o.export_blocks()
    lo = np.array([0.1, 0.1, 1.0], np.float32)
    v, _ = o.extract_mesh(lo, lo + np.float32(vs) * np.float32(1.5))
    assert len(v) in (6, 3, 9, 12)  # one cell, a plane cuts it in 1-4 triangles

    def voxel(ix, iy, iz):
        b = (ix // 8, iy // 8, iz // 8)
        raw = blocks[b].reshape(512, 8)[(ix % 8) * 64 + (iy % 8) * 8 + (iz % 8)]
        return raw[:4].copy().view(np.float32)[0], raw[7]

    F = np.float32
    P = lo  # g = 0
    ctr = [int(F(P[a]) / F(vs) + F(0.5)) for a in range(3)]
    corner = {}
    for sx in (0, 1):
        for sy in (0, 1):
            for sz in (0, 1):
                acc = F(0)
                for kx, ky, kz in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)):
                    sdf, w = voxel(ctr[0] + sx - 1 + kx, ctr[1] + sy - 1 + ky, ctr[2] + sz - 1 + kz)
                    assert w != 0
                    acc = F(acc + F(F(F(0.5) * F(0.5)) * F(0.5)) * sdf)
                corner[(sx, sy, sz)] = acc
    # the surface crosses along z: vertices on the 4 z-edges, at the linear zero crossing of the corner values
    zs = sorted(set(np.round(v[:, 2], 6)))
    expect = []
    for sx in (0, 1):
        for sy in (0, 1):
            a, b = corner[(sx, sy, 0)], corner[(sx, sy, 1)]
            assert (a < 0) != (b < 0)
            z0, z1 = F(P[2] - F(vs) / F(2)), F(P[2] + F(vs) / F(2))
            expect.append(float(z0 + F(-a / F(b - a)) * F(z1 - z0)))
    assert np.allclose(sorted(set(np.round(expect, 6))), zs, atol=2e-6)
