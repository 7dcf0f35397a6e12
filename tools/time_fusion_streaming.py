"""Times DrFusion with and without voxel-block streaming on the synth.room loop at TANDEM's shape (640x480, 1 cm voxels, 4 cm
truncation) through the operator path: IntegrateScanAsync -> RenderAsync(scan pose) -> GetRenderResult per frame.

Legs (--legs, comma separated):
  off        streaming off, TANDEM's 10 m depth range
  idle       streaming on at drf_streaming_min_radius, 10 m (about 13 m: the whole room stays resident, nothing moves)
  move       streaming on at min radius + --margin, --short-depth range (blocks move every few frames)
  off_short  streaming off at --short-depth (what `move` would cost without streaming, and its k_cull growth)

Per leg: ms per frame (host wall clock around the three calls, which return after the ray-cast result is on the host, so it
spans integrate + render on the device), the device time of the streaming launches (drf_streaming_stats [5]), blocks moved per
frame and the resident block count.  One JSON line per leg on stdout; --out writes all legs (with the per-frame series) to a file.
For a kernel profile run one leg under `rocprofv3 --kernel-trace --stats -- python tools/time_fusion_streaming.py --legs X`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from _timing import fusion_options, room_loop  # noqa: E402


def run_leg(leg, frames, poses, args):
    from tandem_amd.dr_fusion import DrFusion, streaming_min_radius
    depth_max = args.short_depth if leg in ("move", "off_short") else 10.0
    opt = fusion_options(frames, args.num_blocks, depth_max, args.height, args.width)
    f = DrFusion(opt)
    rmin = streaming_min_radius(opt)
    radius = 0.0
    if leg == "idle":
        radius = rmin
    elif leg == "move":
        radius = rmin + args.margin
    if radius:
        f.set_streaming(radius, 0)
    if args.render_scope == "map":  # renders at the scan pose: nothing may be staged and no render may wait for its scan
        from tandem_amd.dr_fusion import RENDER_MAP
        f.set_render_scope(RENDER_MAP)
    staged_frames = 0
    ms, st_us, resident, moved = [], [], [], []
    last = dict(streamed_out=0, streamed_in=0)
    n = len(poses)
    for k in range(n):
        bgr, depth = frames["bgr"][k], frames["depth"][k]
        t0 = time.perf_counter()
        f.IntegrateScanAsync(bgr, depth, poses[k])
        f.RenderAsync([poses[k]])
        f.GetRenderResult(copy=False)
        ms.append(1e3 * (time.perf_counter() - t0))
        if args.render_scope == "map":
            staged_frames += f.render_stats() != (0, 0, 0, 0)
        if radius or k % 50 == 0 or k == n - 1:
            s = f.streaming_stats()
            resident.append((k, s["resident"]))
            st_us.append(s["last_scan_us"])
            moved.append(s["streamed_out"] - last["streamed_out"] + s["streamed_in"] - last["streamed_in"])
            last = s
    s = f.streaming_stats()
    f.close()
    w = args.warmup
    t = np.array(ms[w:])
    out = dict(leg=leg, render_scope=args.render_scope, frames_with_render_stats_nonzero=staged_frames, frames=n, max_sensor_depth=depth_max, radius=radius, min_radius=rmin, ms_per_frame_median=float(np.median(t)),
               ms_per_frame_mean=float(t.mean()), ms_per_frame_p90=float(np.percentile(t, 90)),
               ms_first_100=float(np.median(ms[w:100])), ms_last_100=float(np.median(ms[-100:])),
               streaming_us_per_frame_mean=float(np.mean(st_us)) if radius else 0.0,
               streaming_us_max=float(np.max(st_us)) if radius else 0.0,
               blocks_moved_per_frame_mean=float(np.mean(moved)) if radius else 0.0, blocks_moved_max=int(np.max(moved)) if radius else 0,
               resident_final=s["resident"], resident_max=int(max(r for _, r in resident)), host_final=s["host"],
               streamed_out=s["streamed_out"], streamed_in=s["streamed_in"], bytes_moved=s["bytes_moved"])
    series = dict(ms=[round(x, 4) for x in ms], resident=resident[::10] if radius else resident, moved=moved if radius else [])
    return out, series


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,idle,move,off_short")
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--short-depth", type=float, default=2.5)
    ap.add_argument("--margin", type=float, default=0.1, help="metres above drf_streaming_min_radius for the `move` leg")
    ap.add_argument("--num-blocks", type=int, default=400000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--render-scope", default="resident", choices=("resident", "map"), help="drf_set_render_scope of every leg's engine")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    poses, frames = room_loop(args.frames, args.height, args.width, device="cuda" if torch.cuda.is_available() else "cpu")
    results = []
    for leg in args.legs.split(","):
        out, series = run_leg(leg, frames, poses, args)
        print(json.dumps(out), flush=True)
        results.append(dict(out, series=series))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh)


if __name__ == "__main__":
    main()
