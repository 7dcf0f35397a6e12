"""Times map-scope mesh extraction (drf_set_mesh_scope(DRF_MESH_MAP)) on the `move` leg of tools/time_fusion_streaming.py:
synth.room loop, 640x480, 1 cm voxels, 2.5 m depth, streaming radius = drf_streaming_min_radius + 0.1 m, 1000 frames.  An
unbounded engine (streaming off) is fed the same frames; at the end both mesh the box that holds the whole map.

Reported (profiles/map_mesh_time.json):
  resident_ms      ExtractMeshAsync -> mesh_num_triangles, resident scope of the streaming engine (median of --reps)
  map_ms           the same in map scope; map_host_ms is the part spent inside ExtractMeshAsync (device sort of the resident
                   keys and their D2H, merge, chunk planning, packing into pinned staging; packing chunk k waits for the copy of
                   chunk k - 2 to leave its buffer)
  map_h2d_ms_est   staged bytes / pinned H2D bandwidth measured here with a 32 MiB torch copy
  mesh_stats       drf_mesh_stats of the map pass: blocks meshed, host blocks uploaded, chunks
  unbounded_ms     the unbounded engine's extraction of the same box; meshes_equal: byte comparison of the two meshes
  map_kernels_us   (--merge-kernel-stats) per-extraction device time of the map pass's kernels, from a
                   `rocprofv3 --kernel-trace --stats` summary of this script (tools/rocprof_summary.py)

Run:  rocprofv3 --kernel-trace --stats -d DIR -o mesh -- python tools/time_map_mesh.py --out profiles/map_mesh_time.json
      python tools/rocprof_summary.py DIR/.../mesh_results.db > profiles/map_mesh_kernel_stats.txt
      python tools/time_map_mesh.py --merge-kernel-stats profiles/map_mesh_kernel_stats.txt --out profiles/map_mesh_time.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from _timing import fusion_options, merge_kernel_stats, room_loop  # noqa: E402


def time_extraction(f, lo, hi, reps):
    """(median ms to the mesh being done, median ms inside ExtractMeshAsync, the last mesh)."""
    tot, call, mesh = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        f.ExtractMeshAsync(lo, hi)
        t1 = time.perf_counter()
        f.mesh_num_triangles()
        t2 = time.perf_counter()
        mesh = f.GetMeshSync()
        tot.append(1e3 * (t2 - t0))
        call.append(1e3 * (t1 - t0))
    return float(np.median(tot)), float(np.median(call)), mesh


def h2d_gbps():
    import torch
    a = torch.empty(32 << 20, dtype=torch.uint8).pin_memory()
    b = torch.empty(32 << 20, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        b.copy_(a, non_blocking=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        b.copy_(a, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    return 10 * (32 << 20) / (e0.elapsed_time(e1) * 1e-3) / 1e9


def add_kernel_stats(res, rows):
    """The per-extraction device time of the map pass (staged k_mc_cells, k_mc_advance) and of the resident pass."""
    staged = resident = 0.0
    calls = {}
    for name, n, tot, _ in rows:
        if "k_mc_cells<" in name and ", true>" in name or "k_mc_advance" in name:
            staged += tot
        elif "k_mc_cells<" in name:
            resident += tot
        if "k_mc_" in name:
            calls[name] = n
    res["map_kernels_us"] = staged / res["reps"]
    # the resident pass runs reps times on the streaming engine and reps times on the unbounded one
    res["resident_kernels_us_both_engines"] = resident / res["reps"]
    res["kernel_calls"] = calls
    return {k: res[k] for k in ("map_kernels_us", "resident_kernels_us_both_engines")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--depth", type=float, default=2.5)
    ap.add_argument("--margin", type=float, default=0.1)
    ap.add_argument("--num-blocks", type=int, default=400000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-kernel-stats", default=None, help="add the mesh kernels of this rocprof summary to --out and exit")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out, add_kernel_stats)
    import torch
    from tandem_amd.dr_fusion import DrFusion, MESH_MAP, MESH_RESIDENT, streaming_min_radius
    poses, frames = room_loop(args.frames, args.height, args.width)
    bgr, depth = frames["bgr"], frames["depth"]
    opt = fusion_options(frames, args.num_blocks, args.depth, args.height, args.width)
    f, u = DrFusion(opt), DrFusion(opt)
    f.set_streaming(streaming_min_radius(f.options) + args.margin, 0)
    for k in range(args.frames):
        for e in (f, u):
            e.IntegrateScanAsync(bgr[k], depth[k], poses[k])
            e.RenderAsync([poses[k]])
            e.GetRenderResult(copy=False)
    del bgr, depth, frames["bgr"], frames["depth"]
    st = f.streaming_stats()
    c = np.array(list(f.export_all_blocks().keys()), np.int64)
    lo = tuple(float(v) for v in (c.min(0) * 8 - 2) * 0.01)
    hi = tuple(float(v) for v in ((c.max(0) + 1) * 8 + 2) * 0.01)
    res_ms, _, res_mesh = time_extraction(f, lo, hi, args.reps)
    res_stats = f.mesh_stats()
    f.set_mesh_scope(MESH_MAP)
    map_ms, map_host_ms, map_mesh = time_extraction(f, lo, hi, args.reps)
    ms = f.mesh_stats()
    f.set_mesh_scope(MESH_RESIDENT)
    unb_ms, _, unb_mesh = time_extraction(u, lo, hi, args.reps)
    same = all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(map_mesh, unb_mesh))
    gbps = h2d_gbps()
    staged_bytes = ms[1] * (4096 + 8) + ms[0] * 8
    out = dict(frames=args.frames, height=args.height, width=args.width, voxel_size=0.01, max_sensor_depth=args.depth,
               radius=streaming_min_radius(f.options) + args.margin, resident_blocks=st["resident"], host_blocks=st["host"],
               box=[lo, hi], reps=args.reps, resident_ms=res_ms, resident_mesh_stats=list(res_stats),
               resident_triangles=int(len(res_mesh[0]) // 3), map_ms=map_ms, map_host_ms=map_host_ms,
               mesh_stats=dict(blocks_meshed=ms[0], host_blocks_uploaded=ms[1], chunks=ms[2]), staged_bytes=staged_bytes,
               h2d_gbps=gbps, map_h2d_ms_est=staged_bytes / (gbps * 1e9) * 1e3, map_triangles=int(len(map_mesh[0]) // 3),
               unbounded_ms=unb_ms, unbounded_triangles=int(len(unb_mesh[0]) // 3), meshes_equal=bool(same),
               streaming_stats_after=f.streaming_stats() == st)
    f.close()
    u.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
