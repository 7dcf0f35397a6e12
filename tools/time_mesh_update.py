"""Times incremental mesh updates (drf_extract_mesh_update_async) against the full extraction (drf_extract_mesh_async) on the
map of tools/time_map_mesh.py: the synth.room loop, 640x480, 1 cm voxels, 2.5 m depth, 1000 frames.  Two engines are fed the
same frames: an unbounded one (resident scope, everything in the pool) and a streaming one at drf_streaming_min_radius + 0.1 m
(map scope, part of the map in the host store).  After the loop, for each engine and for k = 1, 3 and 10 scans between two
updates, --reps rounds of
    update (fetched: the baseline)  ->  k more scans of the loop  ->  full extraction and update, timed, in alternating order
in one process.  Times are host clocks around calls that end in a device synchronise: launch -> size known (`*_ms`, the
extraction with its host part: key sort round trip, selection read-back, chunk planning) and launch -> triangles on the host
(`*_fetch_ms`, which adds the device-to-host copy of what is returned).  Medians of the rounds; the first round of each leg is
a warm-up and is discarded.

Reported per scope and k (profiles/mesh_update_time.json): blocks in scope, blocks meshed again, triangles and bytes returned by
the update and by the full extraction, the times above, and `assembly_equals_full`: the patches of every update of the run,
kept in a MeshPatches store, assemble to the last full extraction byte for byte.
  select_kernel_us  (--merge-kernel-stats) mean device time of k_mu_select, from a `rocprofv3 --kernel-trace --stats` summary
                    of this script (tools/rocprof_summary.py)

Run:  python tools/time_mesh_update.py --out profiles/mesh_update_time.json
      rocprofv3 --kernel-trace --stats -d DIR -o mu -- python tools/time_mesh_update.py --reps 3
      python tools/rocprof_summary.py DIR/.../mu_results.db > profiles/mesh_update_kernel_stats.txt
      python tools/time_mesh_update.py --merge-kernel-stats profiles/mesh_update_kernel_stats.txt --out profiles/mesh_update_time.json"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from _timing import fusion_options, merge_kernel_stats, room_loop  # noqa: E402


def feed(e, frames, poses, k):
    e.IntegrateScanAsync(frames["bgr"][k], frames["depth"][k], poses[k])
    e.RenderAsync([poses[k]])
    e.GetRenderResult(copy=False)


def timed_full(e, lo, hi):
    t0 = time.perf_counter()
    e.ExtractMeshAsync(lo, hi)
    e.mesh_num_triangles()
    t1 = time.perf_counter()
    mesh = e.GetMeshSync()
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t0), mesh


def timed_update(e, lo, hi):
    t0 = time.perf_counter()
    e.ExtractMeshUpdateAsync(lo, hi)
    e.mesh_update_size()
    t1 = time.perf_counter()
    upd = e.GetMeshUpdateSync()
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t0), upd


def run_leg(e, frames, poses, lo, hi, k, reps, cursor, patches):
    """reps + 1 rounds (the first discarded) of: k scans, then the full extraction and the update in alternating order."""
    rec = dict(full_ms=[], full_fetch_ms=[], update_ms=[], update_fetch_ms=[])
    last = None
    for r in range(reps + 1):
        for _ in range(k):
            feed(e, frames, poses, cursor % len(poses))
            cursor += 1
        if r % 2:
            f_ms, f_fetch, mesh = timed_full(e, lo, hi)
            u_ms, u_fetch, upd = timed_update(e, lo, hi)
        else:
            u_ms, u_fetch, upd = timed_update(e, lo, hi)
            f_ms, f_fetch, mesh = timed_full(e, lo, hi)
        st = e.mesh_update_stats()
        assert not st["full"] and st["scans"] == k, st
        patches.apply(upd)
        if r:
            for name, v in (("full_ms", f_ms), ("full_fetch_ms", f_fetch), ("update_ms", u_ms), ("update_fetch_ms", u_fetch)):
                rec[name].append(v)
        nb, nt = len(upd[1]), len(upd[3]) // 3
        last = dict(scans=k, blocks_in_scope=st["scope"], blocks_meshed=st["meshed"], update_triangles=nt,
                    update_bytes=72 * nt + 12 * nb + 8 * (nb + 1), full_triangles=len(mesh[0]) // 3, full_bytes=72 * (len(mesh[0]) // 3),
                    mesh_stats=list(e.mesh_stats()))
    out = dict(last)
    for name, v in rec.items():
        out[name] = float(np.median(v))
        out[name + "_min_max"] = [float(np.min(v)), float(np.max(v))]
    a, b = patches.assemble(), mesh
    out["assembly_equals_full"] = bool(all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b)))
    return out, cursor


def add_kernel_stats(res, rows):
    picked = {name: dict(calls=n, total_us=tot, avg_us=avg) for name, n, tot, avg in rows if re.search(r"k_mu_|k_mc_cells|k_cull", name)}
    res["kernels"] = picked
    sel = [v for k, v in picked.items() if "k_mu_select" in k]
    res["select_kernel_us"] = sel[0]["avg_us"] if sel else None
    return dict(select_kernel_us=res["select_kernel_us"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--depth", type=float, default=2.5)
    ap.add_argument("--margin", type=float, default=0.1)
    ap.add_argument("--num-blocks", type=int, default=400000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scans", default="1,3,10")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-kernel-stats", default=None, help="add the update's kernels of this rocprof summary to --out and exit")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out, add_kernel_stats)
    import torch
    from tandem_amd.dr_fusion import DrFusion, MeshPatches, MESH_MAP, streaming_min_radius
    assert torch.cuda.is_available(), "needs a GPU"
    poses, frames = room_loop(args.frames, args.height, args.width)
    opt = fusion_options(frames, args.num_blocks, args.depth, args.height, args.width)
    f, u = DrFusion(opt), DrFusion(opt)
    f.set_streaming(streaming_min_radius(f.options) + args.margin, 0)
    f.set_mesh_scope(MESH_MAP)
    for k in range(args.frames):
        feed(f, frames, poses, k)
        feed(u, frames, poses, k)
    st = f.streaming_stats()
    c = np.array(list(u.export_blocks().keys()), np.int64)
    lo = tuple(float(v) for v in (c.min(0) * 8 - 2) * 0.01)
    hi = tuple(float(v) for v in ((c.max(0) + 1) * 8 + 2) * 0.01)
    out = dict(frames=args.frames, height=args.height, width=args.width, voxel_size=0.01, max_sensor_depth=args.depth,
               radius=streaming_min_radius(f.options) + args.margin, map_blocks=int(len(c)), resident_blocks=st["resident"],
               host_blocks=st["host"], box=[lo, hi], reps=args.reps, legs=[])
    for scope, e in (("resident", u), ("map", f)):
        patches = MeshPatches()
        t0 = time.perf_counter()
        first = e.GetMeshUpdate(lo, hi)  # the baseline: a full update
        first_ms = 1e3 * (time.perf_counter() - t0)
        assert first[0]
        patches.apply(first)
        cursor = 0
        for k in (int(v) for v in args.scans.split(",")):
            leg, cursor = run_leg(e, frames, poses, lo, hi, k, args.reps, cursor, patches)
            leg.update(scope=scope, first_full_update_fetch_ms=first_ms)
            print(json.dumps(leg), flush=True)
            out["legs"].append(leg)
    out["host_blocks_after"] = f.streaming_stats()["host"]
    out["equal_across_scopes"] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(u.GetMesh(lo, hi), f.GetMesh(lo, hi))))
    f.close()
    u.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
