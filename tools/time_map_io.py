"""Times drf_save_map / drf_load_map on the map tools/time_fusion_streaming.py builds: the synth.room loop at TANDEM's shape
(640x480, 1 cm voxels), --frames frames (default 60).

Legs (--legs, comma separated):
  off     streaming off: the whole map is resident
  stored  the same map with the blocks whose origin has x <= --split metres moved to the host store (drf_stream_out_region)

Per leg, medians over --reps repetitions, host wall clock (every call returns with the device idle and the file closed):
  save_s / save_gbs      DrFusion.save_map to --dir
  export_s / export_gbs  what a user had to do before map files: drf_export_blocks + drf_export_host_blocks into numpy arrays
                         (the C ABI directly, without the per-block dict of the Python wrappers), then numpy.save of the
                         coordinate and voxel arrays to --dir (split into its export and its write part)
  validate_s             drf_map_info: the validation pass of a load (the whole file read once, checksum included)
  load_s / load_gbs      DrFusion.load_map into a fresh engine (streaming off: into the pool; `stored`: a second load into an
                         engine with streaming on, i.e. into the host store); place_s = load_s - validate_s
Files are written through the page cache and read back from it: the figures are those of the transport, not of a disk.
One JSON line per leg on stdout; --out writes all legs to a file."""
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


def median_time(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), [round(x, 5) for x in t]


def run_leg(leg, frames, poses, args, work):
    from tandem_amd.dr_fusion import DrFusion, map_info, streaming_min_radius
    opt = fusion_options(frames, args.num_blocks, 10.0, args.height, args.width)
    f = DrFusion(opt)
    for k in range(len(poses)):
        f.IntegrateScanAsync(frames["bgr"][k], frames["depth"][k], poses[k])
        f.RenderAsync([poses[k]])
        f.GetRenderResult(copy=False)
    if leg == "stored":
        f.stream_out_region((-1e4, -1e4, -1e4), (args.split, 1e4, 1e4))
    st = f.streaming_stats()
    n = st["resident"] + st["host"]
    path = os.path.join(work, leg + ".drfmap")
    f.save_map(path)  # warm-up: staging allocated, code objects loaded
    size = os.path.getsize(path)
    assert size == 72 + 4104 * n, (size, n)
    save_s, save_all = median_time(lambda: f.save_map(path), args.reps)

    import ctypes as C
    i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)

    def export_only():  # the C ABI straight into numpy arrays (no per-block Python work)
        out = []
        for fn, m in ((f._L.drf_export_blocks, st["resident"]), (f._L.drf_export_host_blocks, st["host"])):
            coords, vox, got = np.empty((max(m, 1), 3), np.int32), np.empty((max(m, 1), 4096), np.uint8), C.c_int()
            assert fn(f._h, m, coords.ctypes.data_as(i32p), vox.ctypes.data_as(u8p), C.byref(got)) == 0 and got.value == m
            out.append((coords[:m], vox[:m]))
        return out

    def export_and_write():
        for name, (coords, vox) in zip(("res", "host"), export_only()):
            np.save(os.path.join(work, leg + "_" + name + "_coords.npy"), coords)
            np.save(os.path.join(work, leg + "_" + name + "_vox.npy"), vox)
    export_s, export_all = median_time(export_and_write, args.reps)
    export_only_s, _ = median_time(export_only, args.reps)
    f.close()

    validate_s, _ = median_time(lambda: map_info(path), args.reps)
    load_t = []
    for _ in range(args.reps + 1):  # the first one is the warm-up
        g = DrFusion(opt)
        if leg == "stored":
            g.set_streaming(streaming_min_radius(opt), 0)
        t0 = time.perf_counter()
        g.load_map(path)
        load_t.append(time.perf_counter() - t0)
        s2 = g.streaming_stats()
        assert s2["resident"] + s2["host"] == n
        g.close()
    load_s = float(np.median(load_t[1:]))
    gb = size / 1e9
    return dict(leg=leg, frames=len(poses), blocks=n, resident=st["resident"], host=st["host"], file_bytes=size, reps=args.reps,
                save_s=save_s, save_gbs=gb / save_s, save_all=save_all,
                export_s=export_s, export_gbs=gb / export_s, export_only_s=export_only_s, export_write_s=export_s - export_only_s, export_all=export_all,
                validate_s=validate_s, validate_gbs=gb / validate_s, load_s=load_s, load_gbs=gb / load_s, place_s=load_s - validate_s,
                load_into="host store" if leg == "stored" else "pool", load_all=[round(x, 5) for x in load_t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,stored")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num-blocks", type=int, default=400000)
    ap.add_argument("--split", type=float, default=0.0, help="`stored` leg: blocks whose origin has x <= this go to the host store")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_map_io.py needs a GPU: a timing taken without one says nothing"
    poses, frames = room_loop(args.frames, args.height, args.width, device="cuda")
    results = []
    with tempfile.TemporaryDirectory(dir=args.dir) as work:
        for leg in args.legs.split(","):
            out = run_leg(leg, frames, poses, args, work)
            print(json.dumps(out), flush=True)
            results.append(out)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
