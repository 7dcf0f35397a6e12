"""Times map-scope renders (drf_set_render_scope(DRF_RENDER_MAP)) on the map of tools/time_map_mesh.py: synth.room loop,
640x480, 1 cm voxels, 2.5 m depth, streaming radius = drf_streaming_min_radius + 0.1 m, 1000 frames.  An unbounded engine
(streaming off) is fed the same frames.  After the loop several poses from the evicted half of the loop are rendered on both,
alternating in one process.  GPU required.

Reported (profiles/render_scope_time.json), per pose and as medians over the poses:
  map_ms           RenderAsync -> GetRenderResult on the streaming engine in map scope (median of --reps after a warm-up)
  map_call_ms      the part inside RenderAsync: selection of the stored blocks, packing into pinned staging, enqueueing
  unbounded_ms     the same pose on the unbounded engine (the reference point); ratio = map_ms / unbounded_ms
  resident_ms      the same pose on the streaming engine in resident scope (holes where the map is stored)
  staged_blocks, bytes    drf_render_stats [0], [1]
  equal            depth and colour of the map-scope render equal the unbounded engine's bit for bit
  scan_pose        map scope at the last scan's pose: drf_render_stats must be (0, 0, 0, 0)
  kernels_us       (--merge-kernel-stats) device time per launch of the staged and the resident ray-cast kernels and of
                   k_rs_build / k_rs_clear, from a `rocprofv3 --kernel-trace --stats` summary of this script

Depth bands (drf_set_render_bands; --bands-out profiles/render_bands_time.json): the far pose --bands-pose rendered one pass
with --capacity, banded with the capacity cut to a half, a third and a tenth of the stored blocks that pass staged and to the
smallest capacity the planner accepts (found by bisection: a refused RenderAsync changes nothing), and on the unbounded engine:
medians, passes, largest pass, blocks and bytes staged per leg (a leg the planner refuses is recorded as such).

Run:  rocprofv3 --kernel-trace --stats -d DIR -o rs -- python tools/time_render_scope.py --out profiles/render_scope_time.json
      python tools/rocprof_summary.py DIR/.../rs_results.db > profiles/render_scope_kernel_stats.txt
      python tools/time_render_scope.py --merge-kernel-stats profiles/render_scope_kernel_stats.txt --out profiles/render_scope_time.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from _timing import fusion_options, merge_kernel_stats, room_loop  # noqa: E402


def time_render(f, pose, reps, warmup):
    """(median ms RenderAsync -> GetRenderResult, median ms inside RenderAsync, (bgr, depth) of the last one)."""
    tot, call, img = [], [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        f.RenderAsync([pose])
        t1 = time.perf_counter()
        rb, rd = f.GetRenderResult(copy=False)
        t2 = time.perf_counter()
        if i >= warmup:
            tot.append(1e3 * (t2 - t0))
            call.append(1e3 * (t1 - t0))
        img = (rb[0].copy(), rd[0].copy())
        # the protocol wants a scan between two renders; an all-invalid depth image integrates nothing
        f.IntegrateScanAsync(time_render.blank[0], time_render.blank[1], time_render.scan_pose)
        f.Synchronize()  # the timed render does not queue behind it
    return float(np.median(tot)), float(np.median(call)), img


def add_kernel_stats(res, rows):
    res["kernels_us"] = {name: dict(calls=n, total_us=tot, us_per_call=tot / max(n, 1)) for name, n, tot, _ in rows
                         if "k_raycast" in name or "k_rs_" in name or "k_publish" in name}
    return res["kernels_us"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--depth", type=float, default=2.5)
    ap.add_argument("--margin", type=float, default=0.1)
    ap.add_argument("--num-blocks", type=int, default=400000)
    ap.add_argument("--capacity", type=int, default=32768, help="stage_capacity_blocks of drf_set_render_scope")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--poses", default="300,400,500,600,700", help="frames of the loop whose poses are rendered at the end")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bands-out", default=None, help="run the depth-band legs and write them here")
    ap.add_argument("--bands-pose", type=int, default=300, help="frame of the loop whose pose the depth-band legs render")
    ap.add_argument("--merge-kernel-stats", default=None, help="add the ray-cast kernels of this rocprof summary to --out and exit")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out, add_kernel_stats, indent=1)
    import torch
    assert torch.cuda.is_available(), "tools/time_render_scope.py needs a GPU"
    from tandem_amd._lib import DrError
    from tandem_amd.dr_fusion import DrFusion, RENDER_MAP, RENDER_RESIDENT, streaming_min_radius
    poses, frames = room_loop(args.frames, args.height, args.width)
    bgr, depth = frames["bgr"], frames["depth"]
    opt = fusion_options(frames, args.num_blocks, args.depth, args.height, args.width)
    f, u = DrFusion(opt), DrFusion(opt)
    f.set_streaming(streaming_min_radius(f.options) + args.margin, 0)
    f.set_render_scope(RENDER_MAP, args.capacity)
    loop_stats = np.zeros(4, np.int64)
    for k in range(args.frames):
        for e in (f, u):
            e.IntegrateScanAsync(bgr[k], depth[k], poses[k])
            e.RenderAsync([poses[k]])
            e.GetRenderResult(copy=False)
        loop_stats += np.array(f.render_stats(), np.int64)
    time_render.blank = (np.zeros_like(bgr[0]), np.zeros_like(depth[0]))
    time_render.scan_pose = poses[args.frames - 1]
    del bgr, depth, frames["bgr"], frames["depth"]
    st = f.streaming_stats()
    for e in (f, u):  # leave both where RenderAsync is legal
        e.IntegrateScanAsync(time_render.blank[0], time_render.blank[1], time_render.scan_pose)
        e.Synchronize()
    rows = []
    for k in [int(x) for x in args.poses.split(",")]:
        # alternating: map scope, unbounded, resident scope
        f.set_render_scope(RENDER_MAP, args.capacity)
        map_ms, map_call, map_img = time_render(f, poses[k], args.reps, args.warmup)
        rs = f.render_stats()
        unb_ms, unb_call, unb_img = time_render(u, poses[k], args.reps, args.warmup)
        f.set_render_scope(RENDER_RESIDENT, 0)
        res_ms, _, res_img = time_render(f, poses[k], args.reps, args.warmup)
        equal = bool(np.array_equal(map_img[1].view(np.uint32), unb_img[1].view(np.uint32)) and np.array_equal(map_img[0], unb_img[0]))
        rows.append(dict(pose=k, map_ms=map_ms, map_call_ms=map_call, unbounded_ms=unb_ms, unbounded_call_ms=unb_call, resident_ms=res_ms,
                         ratio=map_ms / unb_ms, staged_blocks=rs[0], bytes=rs[1], whole=rs[2], waited=rs[3], equal=equal,
                         resident_scope_differs=bool(not np.array_equal(res_img[1].view(np.uint32), unb_img[1].view(np.uint32))),
                         hit_pixels=int((unb_img[1] > 0).sum())))
        print(json.dumps(rows[-1]), flush=True)
    f.set_render_scope(RENDER_MAP, args.capacity)
    scan_ms, scan_call, _ = time_render(f, time_render.scan_pose, args.reps, args.warmup)
    scan_stats = f.render_stats()
    unb_scan_ms, _, _ = time_render(u, time_render.scan_pose, args.reps, args.warmup)
    med = lambda key: float(np.median([r[key] for r in rows]))  # noqa: E731
    out = dict(frames=args.frames, height=args.height, width=args.width, voxel_size=0.01, max_sensor_depth=args.depth,
               radius=streaming_min_radius(f.options) + args.margin, resident_blocks=st["resident"], host_blocks=st["host"],
               capacity=args.capacity, reps=args.reps, warmup=args.warmup, loop_render_stats_sum=[int(v) for v in loop_stats],
               poses=rows, map_ms_median=med("map_ms"), map_call_ms_median=med("map_call_ms"), unbounded_ms_median=med("unbounded_ms"),
               resident_ms_median=med("resident_ms"), ratio_median=med("ratio"), staged_blocks_median=med("staged_blocks"),
               all_equal=all(r["equal"] for r in rows),
               scan_pose=dict(map_ms=scan_ms, map_call_ms=scan_call, unbounded_ms=unb_scan_ms, render_stats=list(scan_stats)),
               streaming_stats_after={k: v for k, v in f.streaming_stats().items() if k != "last_scan_us"} ==
               {k: v for k, v in st.items() if k != "last_scan_us"})
    if args.bands_out:
        pose = poses[args.bands_pose]
        unb_ms, _, unb_img = time_render(u, pose, args.reps, args.warmup)
        legs, n = [], None
        def accepted(cap):
            f.set_render_scope(RENDER_MAP, cap)
            try:
                f.RenderAsync([pose])
            except DrError:
                return False
            f.GetRenderResult(copy=False)
            f.IntegrateScanAsync(time_render.blank[0], time_render.blank[1], time_render.scan_pose)
            f.Synchronize()
            return True
        for name, div in (("one_pass", 0), ("half", 2), ("third", 3), ("tenth", 10), ("smallest", -1)):
            if div < 0:
                f.set_render_bands(64)
                lo, hi = 0, n  # lo is refused, hi accepted
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    lo, hi = (lo, mid) if accepted(mid) else (mid, hi)
                cap = hi
            else:
                cap = args.capacity if not div else -(-n // div)
            f.set_render_scope(RENDER_MAP, cap)
            f.set_render_bands(64 if div else 0)
            try:
                ms, call, img = time_render(f, pose, args.reps, args.warmup)
            except DrError as e:  # no plan of bands within this capacity: recorded, not timed
                legs.append(dict(leg=name, capacity=cap, refused=e.code))
                continue
            rs, bs = f.render_stats(), f.render_band_stats()
            n = rs[0] if n is None else n
            legs.append(dict(leg=name, capacity=cap, ms=ms, call_ms=call, ratio_to_unbounded=ms / unb_ms, union_blocks=rs[0], bytes=rs[1],
                             passes=bs[0], largest_pass_blocks=bs[1], staged_blocks=bs[2], banded=bs[3],
                             equal=bool(np.array_equal(img[1].view(np.uint32), unb_img[1].view(np.uint32)) and np.array_equal(img[0], unb_img[0]))))
            print(json.dumps(legs[-1]), flush=True)
        f.set_render_bands(0)
        with open(args.bands_out, "w") as fh:
            json.dump(dict(frames=args.frames, height=args.height, width=args.width, voxel_size=0.01, max_sensor_depth=args.depth, pose=args.bands_pose,
                           reps=args.reps, warmup=args.warmup, unbounded_ms=unb_ms, legs=legs), fh, indent=1)
    f.close()
    u.close()
    print(json.dumps({k: v for k, v in out.items() if k != "poses"}), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
