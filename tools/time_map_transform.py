"""Times drf_transform_map on the map tools/time_map_merge.py works on: the synth.room loop at TANDEM's shape (640x480, 1 cm
voxels), --frames frames (default 60) integrated into one engine and saved.  The motion is 37 degrees about (1, 2, 3) with
t = (0.313, -1.07, 2.5) metres.

Host wall clock (every call returns with the device idle), same box and same session:
  transform_s, blocks_in_s, blocks_out_s   DrFusion.transform_map of the file, median over --reps calls after one warm-up call;
                                           blocks/s count the file's blocks and the blocks written
  validate_s, validate_share               drf_map_info of the file, the validation pass a transform starts with, and its share
                                           of transform_s
  before_*                                 what a user had to do before: read_s (tandem_amd.map_file.read), numpy_s (the rule in
                                           numpy over the candidate region, in batches of --batch destination blocks), compose_s
                                           (tandem_amd.map_file.write); before_s is their sum, measured once
The two outputs are compared byte for byte.
As information: the moved map loaded into a second engine and ray-cast at T * P for --views of the loop's poses P, against the
source engine's ray-cast at P: render_median_abs_depth_diff_voxels (over the pixels valid in both) and render_valid_in_both (their
share of all pixels), with the share valid in the source render beside it.
Files are written through the page cache and read back from it.  One JSON line on stdout; --out writes it."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from _timing import fusion_options, room_loop  # noqa: E402

B = 1 << 20
_V = np.arange(512)
_OFF = np.stack([_V >> 6, (_V >> 3) & 7, _V & 7], axis=1).astype(np.int64)


def motion_matrix():
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(37.0)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = (0.313, -1.07, 2.5)
    return T


def region(coords, Rd, tv):
    """Destination blocks around the image of every source block (its lattice box [8b - 1, 8b + 8]^3 under g = R u + tv, one block
    added all round), ascending by key."""
    from tandem_amd import map_file
    ends = np.array([[x, y, z] for x in (-1.0, 8.0) for y in (-1.0, 8.0) for z in (-1.0, 8.0)])
    g = (coords[:, None, :] * 8 + ends[None]) @ Rd.T + tv
    lo, hi = np.floor(g.min(1) / 8).astype(np.int64) - 1, np.floor(g.max(1) / 8).astype(np.int64) + 1
    e = (hi - lo + 1).max(0)
    grid = np.stack(np.meshgrid(*[np.arange(k) for k in e], indexing="ij"), axis=-1).reshape(-1, 3)
    blocks = (lo[:, None, :] + grid[None]).reshape(-1, 3)
    blocks = blocks[(blocks <= np.repeat(hi, len(grid), axis=0)).all(1)]
    return map_file.unpack_keys(np.unique(map_file.pack_keys(blocks)))


def numpy_transform(coords, vox, T, vs, batch):
    """drf_transform_map's rule in numpy (float64 position, float32 weights and sums) -> (coords, voxels) of the blocks written."""
    from tandem_amd import map_file
    Rd, tv = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64) / np.float64(np.float32(vs))
    keys = map_file.pack_keys(coords)
    order = np.argsort(keys)
    keys, src, n = keys[order], vox[order].reshape(-1, 512, 8), len(keys)
    D = region(coords, Rd, tv)
    out_c, out_v = [], []
    for at in range(0, len(D), batch):
        d_blocks = D[at:at + batch]
        g = (d_blocks[:, None, :] * 8 + _OFF[None]).reshape(-1, 3)
        d = g.astype(np.float64) - tv
        u = np.stack([(Rd[0, k] * d[:, 0] + Rd[1, k] * d[:, 1]) + Rd[2, k] * d[:, 2] for k in range(3)], axis=1)
        b = np.floor(u)
        f = (u - b).astype(np.float32)
        b = b.astype(np.int64)
        a = (np.float32(1.0) - f, f)
        N = len(g)
        started, alls = np.zeros(N, bool), np.ones(N, bool)
        acc, wmin = np.zeros((N, 4), np.float32), np.full(N, 255, np.int64)
        for c in range(8):
            cx, cy, cz = c >> 2, (c >> 1) & 1, c & 1
            w = (a[cx][:, 0] * a[cy][:, 1]) * a[cz][:, 2]
            used = w != 0
            p = b + np.array([cx, cy, cz])
            blk = p >> 3
            ok = ((blk >= -B) & (blk < B)).all(1)
            k = map_file.pack_keys(np.where(ok[:, None], blk, 0))
            pos = np.minimum(np.searchsorted(keys, k), n - 1)
            v8 = src[pos, ((p[:, 0] & 7) << 6) | ((p[:, 1] & 7) << 3) | (p[:, 2] & 7)]
            wt = np.where(ok & (keys[pos] == k), v8[:, 7], 0).astype(np.int64)
            weighted = used & (wt > 0)
            alls &= ~used | (wt > 0)
            val = np.concatenate([np.ascontiguousarray(v8[:, :4]).view(np.float32), v8[:, 4:7].astype(np.float32)], axis=1)
            with np.errstate(all="ignore"):
                term = w[:, None] * val
                acc = np.where((weighted & ~started)[:, None], term, np.where((weighted & started)[:, None], acc + term, acc))
            started |= weighted
            wmin = np.where(weighted, np.minimum(wmin, wt), wmin)
        o = np.zeros((N, 8), np.uint8)
        o[alls, :4] = np.ascontiguousarray(acc[alls, :1]).view(np.uint8)
        o[alls, 4:7] = np.minimum(acc[alls, 1:] + np.float32(0.5), np.float32(255.0)).astype(np.uint8)
        o[alls, 7] = wmin[alls].astype(np.uint8)
        keep = alls.reshape(-1, 512).any(1)
        if (at // batch) % 10 == 9:
            print("numpy route: %d of %d destination blocks" % (at + len(d_blocks), len(D)), file=sys.stderr, flush=True)
        out_c.append(d_blocks[keep])
        out_v.append(o.reshape(-1, 4096)[keep])
    return np.concatenate(out_c), np.concatenate(out_v)


def render(f, pose):
    f.RenderAsync([pose])
    _, rd = f.GetRenderResult()
    return rd[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num-blocks", type=int, default=400000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--no-before", action="store_true", help="skip the numpy route (and the byte comparison with it)")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_map_transform.py needs a GPU: a timing taken without one says nothing"
    from tandem_amd import map_file
    from tandem_amd.dr_fusion import DrFusion, map_info
    poses, frames = room_loop(args.frames, args.height, args.width, device="cuda")
    opt = fusion_options(frames, args.num_blocks, 10.0, args.height, args.width)
    T = motion_matrix()
    with tempfile.TemporaryDirectory(dir=args.dir) as work:
        src, dst, composed = (os.path.join(work, n) for n in ("room.drfmap", "moved.drfmap", "numpy.drfmap"))
        f = DrFusion(opt)
        for k in range(args.frames):
            f.IntegrateScanAsync(frames["bgr"][k], frames["depth"][k], poses[k])
            f.RenderAsync([poses[k]])
            f.GetRenderResult(copy=False)
        f.save_map(src)
        size = os.path.getsize(src)
        n_in = (size - 72) // 4104
        t0 = time.perf_counter()
        map_info(src)
        validate_s = time.perf_counter() - t0
        times = []
        for _ in range(args.reps + 1):  # the first one is the warm-up
            t0 = time.perf_counter()
            f.transform_map(src, T, dst)
            times.append(time.perf_counter() - t0)
        stats = f.transform_stats()
        f.close()
        transform_s = float(np.median(times[1:]))
        n_out = (os.path.getsize(dst) - 72) // 4104
        out = dict(frames=args.frames, file_blocks_in=int(n_in), file_bytes_in=size, file_blocks_out=int(n_out), file_bytes_out=os.path.getsize(dst),
                   reps=args.reps, transform_stats=list(stats), validate_s=validate_s, transform_s=transform_s, validate_share=validate_s / transform_s,
                   blocks_in_s=n_in / transform_s, blocks_out_s=n_out / transform_s, transform_all=[round(x, 5) for x in times],
                   motion=[float(v) for v in T.reshape(16)])
        if not args.no_before:
            t = {}
            t0 = time.perf_counter()
            vs, coords, vox = map_file.read(src)
            t["read_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            oc, ov = numpy_transform(coords, vox, T, vs, args.batch)
            t["numpy_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            map_file.write(composed, vs, oc, ov)
            t["compose_s"] = time.perf_counter() - t0
            same = open(composed, "rb").read() == open(dst, "rb").read()
            assert same, "transform_map and the numpy route disagree"
            out.update(before_s=sum(t.values()), identical_bytes=bool(same), **{"before_" + k: v for k, v in t.items()})
        # information: the moved map seen from the moved poses (a loaded map may be ray-cast before its first scan)
        picks = [int(v) for v in np.linspace(0, args.frames - 1, args.views)]
        g = DrFusion(opt)
        g.load_map(src)
        views = [render(g, np.asarray(poses[k], np.float32)).copy() for k in picks]
        g.close()
        g = DrFusion(opt)
        g.load_map(dst)
        diffs, both, valid_src = [], 0, 0
        for k, a in zip(picks, views):
            b = render(g, (T.astype(np.float64) @ np.asarray(poses[k], np.float64)).astype(np.float32))
            m = (a > 0) & (b > 0)
            diffs.append(np.abs(a[m].astype(np.float64) - b[m]) / opt.voxel_size)
            both += int(m.sum())
            valid_src += int((a > 0).sum())
        g.close()
        npix = len(picks) * args.height * args.width
        d = np.concatenate(diffs)
        out.update(render_views=picks, render_median_abs_depth_diff_voxels=float(np.median(d)) if len(d) else None,
                   render_p90_abs_depth_diff_voxels=float(np.percentile(d, 90)) if len(d) else None,
                   render_valid_in_both=both / npix, render_valid_in_source=valid_src / npix)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
