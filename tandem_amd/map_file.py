"""The DrFusion map file (include/dr_mi355x.h "map files") in numpy: a reader, a writer, and two commands.

    python -m tandem_amd.map_file info PATH                  header fields and the blocks' bounding box (needs no device)
    python -m tandem_amd.map_file mesh PATH OUT.obj [--lower x y z --upper x y z]
                                                             loads the map into an engine sized for it and meshes it
    python -m tandem_amd.map_file merge OUT IN1 IN2 [IN3 ...] [--max-weight 64]
                                                             IN1 loaded, the others merged into it in order (drf_merge_map), saved
    python -m tandem_amd.map_file align SRC REF [--init <16 floats>] [--max-iters N]
                                                             SRC registered to REF (drf_align_map): one JSON line with the pose
                                                             SRC-world -> REF-world, status, iterations, samples, valid, costs;
                                                             the exit status is non-zero unless it converged
    python -m tandem_amd.map_file transform IN OUT --pose <16 floats>
                                                             IN resampled in the frame p_out = R p_in + t (drf_transform_map)

Layout, little-endian, 72 + 4104 n bytes: magic "DRFMAP01", u32 header size 64, u32 block edge 8, u32 bytes per voxel 8,
f32 voxel_size, u64 n, 32 zero bytes; n ascending u64 packed keys; n x 4096 voxel bytes; u64 checksum."""
import struct
import sys

import numpy as np

MAGIC = b"DRFMAP01"
HEADER = struct.Struct("<8sIIIfQ32s")  # 64 bytes
BLOCK_BYTES = 4096
_BIAS = 1 << 20
_MASK = (1 << 64) - 1


def pack_keys(coords):
    """(n, 3) block coordinates -> uint64 keys: 21 bits per axis, biased by 2^20, x in the high bits."""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    assert ((c >= -_BIAS) & (c < _BIAS)).all(), "block coordinate outside [-2^20, 2^20)"
    c = (c + _BIAS).astype(np.uint64)
    return (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]


def unpack_keys(keys):
    k = np.asarray(keys, np.uint64)
    m = np.uint64(0x1fffff)
    return np.stack([(k >> np.uint64(42)) & m, (k >> np.uint64(21)) & m, k & m], axis=-1).astype(np.int64).reshape(-1, 3) - _BIAS


def checksum(*parts):
    """h = 0xcbf29ce484222325; for every little-endian u64 word w of the parts in order: h = (h ^ w) * 0x100000001b3 mod 2^64.
    A Python loop (the recurrence does not vectorise): meant for the maps of tools and tests; read() verifies through the library."""
    h = 0xcbf29ce484222325
    for p in parts:
        for w in np.frombuffer(np.ascontiguousarray(p).tobytes(), "<u8").tolist():
            h = ((h ^ w) * 0x100000001b3) & _MASK
    return h


def write(path, voxel_size, coords, voxels):
    """coords (n, 3) ints and voxels (n, 4096) uint8 in any order -> the file (blocks sorted by key)."""
    keys = pack_keys(coords)
    vox = np.ascontiguousarray(voxels, np.uint8).reshape(len(keys), BLOCK_BYTES)
    order = np.argsort(keys, kind="stable")
    keys, vox = np.ascontiguousarray(keys[order]).astype("<u8"), np.ascontiguousarray(vox[order])
    assert (keys[1:] > keys[:-1]).all(), "a block is listed twice"
    with open(path, "wb") as f:
        f.write(HEADER.pack(MAGIC, 64, 8, 8, np.float32(voxel_size), len(keys), bytes(32)))
        f.write(keys.tobytes())
        f.write(vox.tobytes())
        f.write(struct.pack("<Q", checksum(keys, vox)))


def read_header(path):
    """(voxel_size, n, keys) after the structural checks; the checksum is not looked at."""
    with open(path, "rb") as f:
        head = f.read(64)
        if len(head) != 64:
            raise ValueError("%s is shorter than a map file header" % path)
        magic, hb, edge, vb, vs, n, reserved = HEADER.unpack(head)
        if magic != MAGIC or hb != 64 or edge != 8 or vb != 8 or any(reserved):
            raise ValueError("%s is not a DrFusion map file" % path)
        f.seek(0, 2)
        if f.tell() != 72 + 4104 * n:
            raise ValueError("%s: size does not match its %d blocks" % (path, n))
        f.seek(64)
        keys = np.frombuffer(f.read(8 * n), "<u8")
    if n and (not (keys[1:] > keys[:-1]).all() or int(keys[-1]) >> 63):
        raise ValueError("%s: block keys are not strictly ascending" % path)
    return float(np.float32(vs)), int(n), keys


def read(path, verify=True):
    """(voxel_size, coords (n, 3) int64, voxels (n, 4096) uint8), blocks in the file's (ascending key) order.
    verify: the whole file validated by the library first (drf_map_info, host-only)."""
    if verify:
        from .dr_fusion import map_info
        map_info(path)
    vs, n, keys = read_header(path)
    vox = np.fromfile(path, np.uint8, count=n * BLOCK_BYTES, offset=64 + 8 * n).reshape(n, BLOCK_BYTES)
    return vs, unpack_keys(keys), vox


def info(path):
    """dict of the header fields and the blocks' bounding box (block coordinates and metres), the file validated as a whole."""
    from .dr_fusion import map_info
    vs, n = map_info(path)
    _, _, keys = read_header(path)
    d = dict(path=str(path), magic=MAGIC.decode(), header_bytes=64, block_edge=8, voxel_bytes=8, voxel_size=vs, blocks=n, bytes=72 + 4104 * n)
    if n:
        c = unpack_keys(keys)
        lo, hi = c.min(0), c.max(0)
        d.update(block_min=[int(v) for v in lo], block_max=[int(v) for v in hi],
                 lower=[float(v) * 8 * vs for v in lo], upper=[float(v + 1) * 8 * vs for v in hi])
    return d


def mesh(path, out, lower=None, upper=None):
    """Loads the map into an engine sized for it and writes the mesh of [lower, upper] (default: the blocks' bounding box)."""
    from .dr_fusion import DrFusion, DrFusionOptions
    d = info(path)
    if lower is None or upper is None:
        lower, upper = d.get("lower", [0.0] * 3), d.get("upper", [0.0] * 3)
    n = max(d["blocks"], 1)
    f = DrFusion(DrFusionOptions(voxel_size=d["voxel_size"], num_blocks=n, num_buckets=n, num_render_streams=0, height=8, width=8,
                                 truncation_distance=4 * d["voxel_size"]))
    try:
        f.load_map(path)
        f.SaveMeshToFile(out, lower, upper)
    finally:
        f.close()


def merge(out, inputs, max_weight=64):
    """load_map(inputs[0]), merge_map of the rest in order, save_map(out), in an engine sized for the sum of the inputs' block
    counts.  Returns the merge_stats() of every merge."""
    from .dr_fusion import DrFusion, DrFusionOptions
    infos = [info(p) for p in inputs]
    vs = infos[0]["voxel_size"]
    n = max(sum(d["blocks"] for d in infos), 1)
    f = DrFusion(DrFusionOptions(voxel_size=vs, num_blocks=n, num_buckets=n, num_render_streams=0, height=8, width=8,
                                 truncation_distance=4 * vs, max_sdf_weight=int(max_weight)))
    try:
        f.load_map(inputs[0])
        stats = []
        for p in inputs[1:]:
            f.merge_map(p)
            stats.append(f.merge_stats())
        f.save_map(out)
    finally:
        f.close()
    return stats


def transform(src, out, pose, chunk_blocks=0):
    """transform_map(src, pose, out) in a small engine with src's voxel_size; pose: 16 floats, row-major, rigid.  Returns the
    transform_stats()."""
    from .dr_fusion import DrFusion, DrFusionOptions
    vs = info(src)["voxel_size"]
    f = DrFusion(DrFusionOptions(voxel_size=vs, num_blocks=8192, num_buckets=8192, num_render_streams=0, height=8, width=8,
                                 truncation_distance=4 * vs))
    try:
        f.transform_map(src, np.asarray(pose, np.float32).reshape(4, 4), out, chunk_blocks)
        return f.transform_stats()
    finally:
        f.close()


def align(src, ref, init=None, **opt):
    """align_map(src, ref, init) in a small engine with src's voxel_size; init: 16 floats, row-major, rigid (default: the
    identity).  Returns the AlignResult whatever its status."""
    from .dr_fusion import DrFusion, DrFusionOptions
    vs = info(src)["voxel_size"]
    f = DrFusion(DrFusionOptions(voxel_size=vs, num_blocks=8192, num_buckets=8192, num_render_streams=0, height=8, width=8,
                                 truncation_distance=4 * vs))
    try:
        return f.align_map(src, ref, None if init is None else np.asarray(init, np.float32).reshape(4, 4), raise_on_failure=False, **opt)
    finally:
        f.close()


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m tandem_amd.map_file")
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("info").add_argument("path")
    m = sub.add_parser("mesh")
    m.add_argument("path")
    m.add_argument("out")
    m.add_argument("--lower", type=float, nargs=3)
    m.add_argument("--upper", type=float, nargs=3)
    g = sub.add_parser("merge")
    g.add_argument("out")
    g.add_argument("inputs", nargs="+")
    g.add_argument("--max-weight", type=int, default=64)
    t = sub.add_parser("transform")
    t.add_argument("src")
    t.add_argument("out")
    t.add_argument("--pose", type=float, nargs=16, required=True)
    al = sub.add_parser("align")
    al.add_argument("src")
    al.add_argument("ref")
    al.add_argument("--init", type=float, nargs=16)
    al.add_argument("--max-iters", type=int, default=0)
    a = ap.parse_args(argv)
    if a.cmd == "info":
        for k, v in info(a.path).items():
            print("%-12s %s" % (k, v))
    elif a.cmd == "merge":
        if len(a.inputs) < 2:
            ap.error("merge needs at least two input maps")
        for p, st in zip(a.inputs[1:], merge(a.out, a.inputs, a.max_weight)):
            print("%s: blocks %d added %d combined %d voxels_verbatim %d voxels_averaged %d" % (p, st[0], st[1], st[2] + st[3], st[4], st[5]))
    elif a.cmd == "transform":
        st = transform(a.src, a.out, a.pose)
        print("%s: blocks %d candidates %d written %d voxels %d refused %d" % (a.src, st[0], st[1], st[2], st[3], st[4]))
    elif a.cmd == "align":
        import json
        from .dr_fusion import ALIGN_CONVERGED, ALIGN_STATUS
        r = align(a.src, a.ref, a.init, max_iters=a.max_iters)
        print(json.dumps(dict(pose=[float(v) for v in r.T32.reshape(16)], status=ALIGN_STATUS[r.status], iterations=r.iterations, samples=r.samples,
                              valid=r.valid, cost0=r.cost0, cost=r.cost)))
        return 0 if r.status == ALIGN_CONVERGED else 1
    else:
        mesh(a.path, a.out, a.lower, a.upper)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
