"""Times drf_locate_system and drf_locate_frame on the map the other DrFusion timing tools work on: the synth.room loop (the room
of the bench's fusion loop) at TANDEM's shape (640x480, 1 cm voxels), --frames frames (default 60) integrated into one engine.  The
frame located is the loop's middle scan: its own depth image, from its own pose moved by 1.5 voxels and turned by 0.3 degrees --
inside the 4-voxel truncation band -- so the refinement should come back to the scan's pose.

Host wall clock (every call returns with the device idle), same box and same session, median over --reps calls (at least 5) after
one warm-up, all runs listed:
  system_s           one DrFusion.locate_system at the start pose with the depth image in host memory (copy, upload, one evaluation)
  system_device_s    the same with the depth image already in device memory
  frame_s            one DrFusion.locate_frame from the start pose, host pointer, with its iterations and status
  frame_device_s     the same with a device pointer
  eval_s             (frame_device_s - system_device_s) / (iterations - 1): what one further evaluation costs (memset, two kernels,
                     read-back, step)
  numpy_eval_s       the numpy restatement of tests/test_map_locate.py for ONE evaluation at the start pose over export_blocks(),
                     measured once.  Its sums and counts are compared bit for bit with locate_system's: identical_bits.
As information: the pose found against the scan's pose (rotation in degrees, translation of the camera centre in voxels), the
overlap valid / samples, and for context drf_align_map's eval_s from profiles/map_align_time.json -- another workload (source voxels
against an uploaded map), so context and not a threshold.
Not measured: the kernels alone (that takes a rocprofv3 --kernel-trace --stats run of this tool, in a run of its own).
One JSON line on stdout; --out writes it, ending with the box's gpu_state.

--scope map (profiles/map_locate_scope_time.json): the locate scope, drf_set_locate_scope(DRF_LOCATE_MAP), on the same loop and
frame, in one engine and session.  One more scan is integrated 30 m along each axis from the room -- beyond what the located
frame's selection reaches -- and streaming is turned on with a radius that evicts nothing.  The four calls are timed in three states:
  a  resident scope, every block in the pool: the existing path, the baseline
  c  map scope, the far scan's blocks in the host store: a non-empty store and an empty selection -- the resident kernel is launched
     (a and c alternate, call by call, so that the box's drift reaches both alike)
  b  map scope, every block in the host store: one staging per call (pack, copy, table), then the staged kernel
Per state the medians and all runs of the four calls and of frame_near_device -- a refinement from a quarter of the start's
offset, which stays within one staging's slack, where the start's own 0.3 degrees move far enough that the second evaluation stages
again (stage_stats says so) -- eval_s as above, eval_near_s the same from frame_near_device (in b: one further evaluation by the
staged kernel and nothing else), and for b the locate_stage_stats and
stage_s = system_device_s(b) - system_device_s(a): what selecting, packing, copying and indexing the staging adds to a call.
Every result of b and c is compared bit for bit with a's.  Not measured: the kernels alone."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from _timing import fusion_options, room_loop  # noqa: E402


def gpu_state():
    """sclk / mclk / power / temperature of GPU 0 as rocm-smi reports them (read only), as bench.py records them."""
    import subprocess
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--showtemp", "--json"], capture_output=True, text=True, timeout=20)
        card = next(iter(json.loads(r.stdout).values()))
        return {k: v for k, v in card.items() if any(w in k.lower() for w in ("sclk", "mclk", "fclk", "power")) or ("temperature" in k.lower() and "edge" in k.lower())}
    except Exception as e:  # noqa: BLE001 -- reporting only
        return dict(error=str(e)[:120])


def start_pose(pose, vs, part=1.0):
    a = np.array([1.0, -2.0, 1.0]) / np.sqrt(6.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(0.3 * part)
    T = np.array(pose, np.float64).reshape(4, 4)
    T[:3, :3] = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)) @ T[:3, :3]
    T[:3, 3] += np.array([1.0, -0.5, 1.0]) * vs * part  # |(1, -0.5, 1)| = 1.5
    return T.astype(np.float32)


def pose_error(T, pose, vs):
    pose = np.asarray(pose, np.float64).reshape(4, 4)
    E = T[:3, :3] @ pose[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(E) - 1.0) / 2.0, -1.0, 1.0)))), float(np.linalg.norm(T[:3, 3] - pose[:3, 3]) / vs)


def timed(call, reps):
    ts = []
    for _ in range(reps + 1):  # the first one is the warm-up
        t0 = time.perf_counter()
        r = call()
        ts.append(time.perf_counter() - t0)
    return r, float(np.median(ts[1:])), [round(x, 6) for x in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num-blocks", type=int, default=400000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-before", action="store_true", help="skip the numpy restatement (and the bit comparison with it)")
    ap.add_argument("--scope", default="resident", choices=("resident", "map"), help="map: the locate scope in three states (see above)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "each figure is the median of at least 5 runs"
    if args.scope == "map":
        return scope_main(args)
    import torch
    assert torch.cuda.is_available(), "time_map_locate.py needs a GPU: a timing taken without one says nothing"
    from tandem_amd.dr_fusion import ALIGN_STATUS, DrFusion
    poses, frames = room_loop(args.frames, args.height, args.width, device="cuda")
    opt = fusion_options(frames, args.num_blocks, 10.0, args.height, args.width)
    vs = float(opt.voxel_size)
    f = DrFusion(opt)
    for k in range(args.frames):
        pose = np.asarray(poses[k], np.float32)
        f.IntegrateScanAsync(frames["bgr"][k], frames["depth"][k], pose)
        f.RenderAsync([pose])
        f.GetRenderResult(copy=False)
    k = args.frames // 2
    depth, pose = np.ascontiguousarray(frames["depth"][k], np.float32), np.asarray(poses[k], np.float32).reshape(4, 4)
    start = start_pose(pose, vs)
    cd = float(np.median(depth[depth > 0]))
    L, d_depth = f._L, C.c_void_p()
    assert L.dr_device_alloc(0, depth.nbytes, C.byref(d_depth)) == 0 and L.dr_memcpy_h2d(d_depth, depth.ctypes.data_as(C.c_void_p), depth.nbytes) == 0
    dptr = int(d_depth.value)
    (sums, counts), system_s, system_all = timed(lambda: f.locate_system(depth, start, centre_depth=cd), args.reps)
    (dsums, dcounts), system_device_s, system_device_all = timed(lambda: f.locate_system(dptr, start, centre_depth=cd), args.reps)
    r, frame_s, frame_all = timed(lambda: f.locate_frame(depth, start, raise_on_failure=False, centre_depth=cd), args.reps)
    rd, frame_device_s, frame_device_all = timed(lambda: f.locate_frame(dptr, start, raise_on_failure=False, centre_depth=cd), args.reps)
    stats = f.locate_stats()
    L.dr_device_free(d_depth)
    assert np.array_equal(sums.view(np.uint64), dsums.view(np.uint64)) and counts == dcounts and np.array_equal(r.T, rd.T)
    eval_s = (frame_device_s - system_device_s) / (r.iterations - 1) if r.iterations > 1 else None
    rot0, tr0 = pose_error(start.astype(np.float64), pose, vs)
    rot, tr = pose_error(r.T, pose, vs)
    out = dict(frames=args.frames, height=args.height, width=args.width, map_blocks=f.stats()["blocks"], located_frame=k, reps=args.reps, centre_depth=cd,
               grid_positions=stats[0], samples=counts[0], valid_at_start=counts[1], unobserved_at_start=counts[2], outside_at_start=counts[3],
               device_bytes=stats[4], system_s=system_s, system_all=system_all, system_device_s=system_device_s, system_device_all=system_device_all,
               frame_s=frame_s, frame_all=frame_all, frame_device_s=frame_device_s, frame_device_all=frame_device_all, iterations=r.iterations,
               status=ALIGN_STATUS[r.status], eval_s=eval_s, valid_at_end=r.valid, cost0=r.cost0, cost=r.cost,
               start_error_rotation_deg=rot0, start_error_translation_voxels=tr0, pose_error_rotation_deg=rot, pose_error_translation_voxels=tr,
               not_measured="the kernels alone; the phases of a call (copy, upload, evaluations) apart")
    try:
        with open(os.path.join(ROOT, "profiles", "map_align_time.json")) as fh:
            out["context_align_map_eval_s"] = json.load(fh)["eval_s"]
    except (OSError, KeyError, ValueError):
        out["context_align_map_eval_s"] = None
    if not args.no_before:
        from test_map_locate import np_locate_system
        blk = f.export_blocks()
        coords = np.array(sorted(blk), np.int64).reshape(-1, 3)
        vox = np.stack([blk[tuple(c)] for c in coords.tolist()])
        cam = {name: getattr(opt, name) for name, _ in opt._fields_}
        t0 = time.perf_counter()
        nsums, ncounts = np_locate_system((coords, vox), cam, depth, start, centre_depth=cd)
        numpy_eval_s = time.perf_counter() - t0
        same = bool(np.array_equal(nsums.view(np.uint64), sums.view(np.uint64))) and ncounts == counts
        assert same, "locate_system and the numpy restatement disagree"
        out.update(numpy_eval_s=numpy_eval_s, identical_bits=same)
    f.close()
    out["gpu_state"] = gpu_state()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


def scope_main(args):
    import torch
    assert torch.cuda.is_available(), "time_map_locate.py needs a GPU: a timing taken without one says nothing"
    from tandem_amd.dr_fusion import ALIGN_STATUS, LOCATE_MAP, LOCATE_RESIDENT, DrFusion, streaming_min_radius
    poses, frames = room_loop(args.frames, args.height, args.width, device="cuda")
    opt = fusion_options(frames, args.num_blocks, 10.0, args.height, args.width)
    vs = float(opt.voxel_size)
    f = DrFusion(opt)
    far = np.eye(4, dtype=np.float32)
    far[:3, 3] = 30.0
    scans = [(k, np.asarray(poses[k], np.float32)) for k in range(args.frames)] + [(0, far @ np.asarray(poses[0], np.float32).reshape(4, 4))]
    for k, pose in scans:
        f.IntegrateScanAsync(frames["bgr"][k], frames["depth"][k], pose)
        f.RenderAsync([pose])
        f.GetRenderResult(copy=False)
    f.set_streaming(max(streaming_min_radius(f.options), 200.0))          # on, and nothing is evicted
    k = args.frames // 2
    depth, pose = np.ascontiguousarray(frames["depth"][k], np.float32), np.asarray(poses[k], np.float32).reshape(4, 4)
    start, near = start_pose(pose, vs), start_pose(pose, vs, 0.25)      # near: the whole refinement stays within one staging's slack
    cd = float(np.median(depth[depth > 0]))
    L, d_depth = f._L, C.c_void_p()
    assert L.dr_device_alloc(0, depth.nbytes, C.byref(d_depth)) == 0 and L.dr_memcpy_h2d(d_depth, depth.ctypes.data_as(C.c_void_p), depth.nbytes) == 0
    dptr = int(d_depth.value)
    calls = dict(system=lambda: f.locate_system(depth, start, centre_depth=cd), system_device=lambda: f.locate_system(dptr, start, centre_depth=cd),
                 frame=lambda: f.locate_frame(depth, start, raise_on_failure=False, centre_depth=cd),
                 frame_device=lambda: f.locate_frame(dptr, start, raise_on_failure=False, centre_depth=cd),
                 frame_near_device=lambda: f.locate_frame(dptr, near, raise_on_failure=False, centre_depth=cd))
    everywhere, far_box = ((-500.0,) * 3, (500.0,) * 3), ((20.0,) * 3, (500.0,) * 3)

    def state(name):
        f.stream_in_region(*everywhere)
        if name == "a":
            f.set_locate_scope(LOCATE_RESIDENT)
        else:
            f.stream_out_region(*(far_box if name == "c" else everywhere))
            f.set_locate_scope(LOCATE_MAP, args.num_blocks)
        return f.streaming_stats()

    def once(name, times, results, stage):
        for call, fn in calls.items():
            t0 = time.perf_counter()
            r = fn()
            times[name][call].append(time.perf_counter() - t0)
            results[name][call] = r
            stage[name][call] = f.locate_stage_stats()

    times = {s: {c: [] for c in calls} for s in "abc"}
    results, stage = {s: {} for s in "abc"}, {s: {} for s in "abc"}
    stored = {}
    for _ in range(args.reps + 1):                                      # the first round is the warm-up; a and c alternate
        for name in "ac":
            stored[name] = state(name)["host"]
            once(name, times, results, stage)
    stored["b"] = state("b")["host"]
    for _ in range(args.reps + 1):
        once("b", times, results, stage)
    L.dr_device_free(d_depth)
    assert stored["a"] == 0 and stored["c"] > 0 and stored["b"] > stored["c"]
    assert all(v == (0, 0, 0, 0) for s in "ac" for v in stage[s].values()), "state c staged something: its selection is not empty"
    assert all(v[0] >= 1 and v[1] > 0 for v in stage["b"].values()) and stage["b"]["frame_near_device"][0] == 1, stage["b"]
    for s in "bc":                                                      # the same bits as the baseline
        for c in ("system", "system_device"):
            assert np.array_equal(results[s][c][0].view(np.uint64), results["a"][c][0].view(np.uint64)) and results[s][c][1] == results["a"][c][1], (s, c)
        for c in ("frame", "frame_device", "frame_near_device"):
            assert np.array_equal(results[s][c].T, results["a"][c].T) and results[s][c].iterations == results["a"][c].iterations, (s, c)
    r, rn = results["a"]["frame"], results["a"]["frame_near_device"]
    out = dict(scope="map", iterations_near=rn.iterations, frames=args.frames, height=args.height, width=args.width, located_frame=k, reps=args.reps, centre_depth=cd, iterations=r.iterations,
               status=ALIGN_STATUS[r.status], samples=results["a"]["system"][1][0], valid_at_start=results["a"]["system"][1][1], identical_bits=True,
               not_measured="the kernels alone; the phases of a staging (selection, packing, copy, table) apart")
    for s, what in (("a", "resident scope, every block resident"), ("c", "map scope, the far scan stored, empty selection"), ("b", "map scope, every block stored")):
        med = {c: float(np.median(times[s][c][1:])) for c in calls}
        out[s] = dict(state=what, stored_blocks=stored[s], stage_stats={c: list(stage[s][c]) for c in calls},
                      eval_s=(med["frame_device"] - med["system_device"]) / (r.iterations - 1) if r.iterations > 1 else None,
                      eval_near_s=(med["frame_near_device"] - med["system_device"]) / (rn.iterations - 1) if rn.iterations > 1 else None,
                      **{c + "_s": med[c] for c in calls}, **{c + "_all": [round(x, 6) for x in times[s][c]] for c in calls})
    out["b"]["stage_s"] = out["b"]["system_device_s"] - out["a"]["system_device_s"]
    f.close()
    out["gpu_state"] = gpu_state()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
