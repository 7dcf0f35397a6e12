"""Times drf_merge_map on the map tools/time_map_io.py builds: the synth.room loop at TANDEM's shape (640x480, 1 cm voxels),
--frames frames (default 60), split into the first half in the engine and the second half in a file.

Legs (--legs, comma separated):
  off     streaming off: the engine's half is resident
  stored  the same with the engine's blocks whose origin has x <= --split metres moved to the host store (drf_stream_out_region)

Per leg, host wall clock (every call returns with the device idle), same box and same session:
  merge_s, merge_blocks_s, merge_gbs   DrFusion.merge_map of the file (median over --reps engines, each rebuilt by load_map
                                       (+ stream_out_region) of the first half's file); validate_s = drf_map_info of the file, the
                                       validation pass a merge starts with; blocks/s and GB/s count the file's blocks
  before_*                             what a user had to do before: export_s (drf_export_blocks + drf_export_host_blocks into
                                       arrays), read_s (tandem_amd.map_file.read of the file), numpy_s (the rule in numpy over the
                                       shared blocks), compose_s (tandem_amd.map_file.write of the merged map), load_s (load_map
                                       into a fresh engine); before_s is their sum
The merged map of the two ways is compared byte for byte (save_map of the merged engine against the composed file).
Files are written through the page cache and read back from it.  One JSON line per leg on stdout; --out writes all legs."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from _timing import fusion_options, room_loop  # noqa: E402


def numpy_merge(a, b, W):
    """(m, 4096) uint8 blocks of the map and of the file with the same keys -> merged (drf_merge_map's rule, float32)."""
    a, b = a.reshape(-1, 8), b.reshape(-1, 8)
    out = a.copy()
    wa, wb = a[:, 7].astype(np.int32), b[:, 7].astype(np.int32)
    two, three = (wb > 0) & (wa == 0), (wb > 0) & (wa > 0)
    out[two] = b[two]
    out[two, 7] = np.minimum(wb[two], W)
    x, y, fa, fb = a[three], b[three], wa[three].astype(np.float32), wb[three].astype(np.float32)
    den = fa + fb
    m = np.empty_like(x)
    sa, sb = x[:, :4].copy().view(np.float32)[:, 0], y[:, :4].copy().view(np.float32)[:, 0]
    m[:, :4] = np.ascontiguousarray((sa * fa + sb * fb) / den).view(np.uint8).reshape(-1, 4)
    for k in (4, 5, 6):
        m[:, k] = ((x[:, k].astype(np.float32) * fa + y[:, k].astype(np.float32) * fb) / den).astype(np.uint8)
    m[:, 7] = np.minimum(wa[three] + wb[three], W)
    out[three] = m
    return out.reshape(-1, 4096)


def export_arrays(f):
    i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    st = f.streaming_stats()
    parts = []
    for fn, m in ((f._L.drf_export_blocks, st["resident"]), (f._L.drf_export_host_blocks, st["host"])):
        coords, vox, got = np.empty((max(m, 1), 3), np.int32), np.empty((max(m, 1), 4096), np.uint8), C.c_int()
        assert fn(f._h, m, coords.ctypes.data_as(i32p), vox.ctypes.data_as(u8p), C.byref(got)) == 0 and got.value == m
        parts.append((coords[:m], vox[:m]))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def run_leg(leg, first, second, opt, args, work):
    from tandem_amd import map_file
    from tandem_amd.dr_fusion import DrFusion, map_info

    def target():
        f = DrFusion(opt)
        f.load_map(first)
        if leg == "stored":
            f.stream_out_region((-1e4, -1e4, -1e4), (args.split, 1e4, 1e4))
        return f

    size = os.path.getsize(second)
    n_file = (size - 72) // 4104
    t0 = time.perf_counter()
    map_info(second)
    validate_s = time.perf_counter() - t0
    times, stats, st = [], None, None
    for rep in range(args.reps + 1):  # the first one is the warm-up
        f = target()
        st = f.streaming_stats()
        t0 = time.perf_counter()
        f.merge_map(second)
        times.append(time.perf_counter() - t0)
        stats = f.merge_stats()
        if rep < args.reps:
            f.close()
    merged_path = os.path.join(work, leg + "_merged.drfmap")
    f.save_map(merged_path)
    f.close()
    merge_s = float(np.median(times[1:]))

    f = target()
    t = {}
    t0 = time.perf_counter()
    coords, vox = export_arrays(f)
    t["export_s"] = time.perf_counter() - t0
    f.close()
    t0 = time.perf_counter()
    _, fcoords, fvox = map_file.read(second)
    t["read_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ka, kb = map_file.pack_keys(coords), map_file.pack_keys(fcoords)
    order = np.argsort(ka)
    pos = np.searchsorted(ka[order], kb)
    hit = (pos < len(ka)) & (ka[order][np.minimum(pos, len(ka) - 1)] == kb)
    rows = order[pos[hit]]
    vox[rows] = numpy_merge(vox[rows], fvox[hit], opt.max_sdf_weight)
    all_coords, all_vox = np.concatenate([coords, fcoords[~hit]]), np.concatenate([vox, fvox[~hit]])
    t["numpy_s"] = time.perf_counter() - t0
    composed = os.path.join(work, leg + "_composed.drfmap")
    t0 = time.perf_counter()
    map_file.write(composed, opt.voxel_size, all_coords, all_vox)
    t["compose_s"] = time.perf_counter() - t0
    g = DrFusion(opt)
    t0 = time.perf_counter()
    g.load_map(composed)
    t["load_s"] = time.perf_counter() - t0
    g.close()
    same = open(composed, "rb").read() == open(merged_path, "rb").read()
    assert same, "merge_map and the numpy merge disagree"
    gb = size / 1e9
    return dict(leg=leg, file_blocks=int(n_file), file_bytes=size, resident=st["resident"], host=st["host"], reps=args.reps,
                merge_stats=list(stats), validate_s=validate_s, merge_s=merge_s, merge_blocks_s=n_file / merge_s, merge_gbs=gb / merge_s,
                merge_all=[round(x, 5) for x in times], before_s=sum(t.values()), identical_bytes=bool(same), **{"before_" + k: v for k, v in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,stored")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num-blocks", type=int, default=400000)
    ap.add_argument("--split", type=float, default=0.0, help="`stored` leg: the engine's blocks whose origin has x <= this go to the host store")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_map_merge.py needs a GPU: a timing taken without one says nothing"
    from tandem_amd.dr_fusion import DrFusion
    poses, frames = room_loop(args.frames, args.height, args.width, device="cuda")
    opt = fusion_options(frames, args.num_blocks, 10.0, args.height, args.width)
    results = []
    with tempfile.TemporaryDirectory(dir=args.dir) as work:
        half = args.frames // 2
        paths = []
        for name, ks in (("first", range(half)), ("second", range(half, args.frames))):
            f = DrFusion(opt)
            for k in ks:
                f.IntegrateScanAsync(frames["bgr"][k], frames["depth"][k], poses[k])
                f.RenderAsync([poses[k]])
                f.GetRenderResult(copy=False)
            paths.append(os.path.join(work, name + ".drfmap"))
            f.save_map(paths[-1])
            f.close()
        for leg in args.legs.split(","):
            out = run_leg(leg, paths[0], paths[1], opt, args, work)
            print(json.dumps(out), flush=True)
            results.append(out)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
