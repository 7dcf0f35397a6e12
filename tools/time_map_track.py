"""Times drf_track_frame on the map the other DrFusion timing tools work on: the synth.room loop (the room of the bench's fusion loop)
at TANDEM's shape (640x480, 1 cm voxels), --frames frames (default 60) integrated into one engine.  The frame tracked is the loop's
middle scan: its own depth image, from its own pose moved by 8 voxels along (1.5, -1.0, 0.8) and turned by 4 degrees about
(1, 2, 3) -- twice the truncation band away, where drf_locate_frame is lost -- with eps_rot 1e-3 and eps_trans 0.02 and every other
option its default.

Host wall clock (every call returns with the device idle), same box and same session, median over --reps calls (at least 3) after
one warm-up, all runs listed:
  frame_s            one DrFusion.track_frame from the start pose, depth image in host memory, with its renders, evaluations, status
  frame_device_s     the same with a device pointer
  one_s              track_frame with max_renders 1, inner_iters 1: one render, one model map, one evaluation
  eval_s             (track_frame with max_renders 1, inner_iters 4  -  one_s) / (its evaluations - 1): one further evaluation
                     (memset, k_track, k_align_fold, read-back, step)
  render_s           (track_frame with max_renders 2, inner_iters 1  -  one_s) - eval_s: one further render (plan, ray-cast,
                     k_track_model)
  locate_after_s     one DrFusion.locate_frame from the pose the tracking ended on, with its iterations, status and pose error
As information: locate_frame alone from the start pose (its status), the pose errors after the tracking and after the
localisation (rotation in degrees, translation of the camera centre in voxels), valid / samples.
--colour adds the same figures for drf_track_colour_frame (the frame's own colour image next to its depth) under "colour", from the same
start in the same session: frame_s, frame_device_s, one_s, eval_s, render_s, the pose error after the tracking, and
eval_ratio = its eval_s / the geometric eval_s -- the colour evaluation gathers three elements per sample where the geometric one
gathers one.
--pyramid adds, under "pyramid", drf_track_pyramid_frame with colour at 1, 3 and 4 levels (device pointers) next to
drf_track_colour_frame from the same start in the same session: the call, where the camera centre ends, the per-level outcomes, one
drf_track_reduce_device call per level 1 to 3, and coarse_round_s, one render + reduction + evaluation at the coarsest level (the
difference of two calls of one render and one evaluation per level, with and without that level).
Not measured: the kernels alone; k_track's fp64 share and the latency of its model gather (that takes counter runs of this tool, in
runs of their own).
One JSON line on stdout; --out writes it, ending with the box's gpu_state."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
from _timing import fusion_options, room_loop  # noqa: E402
from time_map_locate import gpu_state, pose_error, timed  # noqa: E402


def start_pose(pose, vs):
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(4.0)
    T = np.array(pose, np.float64).reshape(4, 4)
    T[:3, :3] = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)) @ T[:3, :3]
    d = np.array([1.5, -1.0, 0.8])
    T[:3, 3] += 8.0 * vs * d / np.linalg.norm(d)
    return T.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num-blocks", type=int, default=400000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--colour", action="store_true", help="also time drf_track_colour_frame")
    ap.add_argument("--pyramid", action="store_true", help="also time drf_track_pyramid_frame at 1, 3 and 4 levels against drf_track_colour_frame")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3, "each figure is the median of at least 3 runs"
    import torch
    assert torch.cuda.is_available(), "time_map_track.py needs a GPU: a timing taken without one says nothing"
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
    o = dict(centre_depth=cd, eps_rot=1e-3, eps_trans=0.02)
    L, d_depth = f._L, C.c_void_p()
    assert L.dr_device_alloc(0, depth.nbytes, C.byref(d_depth)) == 0 and L.dr_memcpy_h2d(d_depth, depth.ctypes.data_as(C.c_void_p), depth.nbytes) == 0
    dptr = int(d_depth.value)

    def track(d, **kw):
        r = f.track_frame(d, start, raise_on_failure=False, **dict(o, **kw))
        return r, f.track_stats()

    def figures(track, d_host, d_dev):
        """the timings of one tracking call: host pointer, device pointer, one render + one evaluation, a further evaluation, a further render"""
        (r, st), frame_s, frame_all = timed(lambda: track(d_host), args.reps)
        (rd, _), frame_device_s, frame_device_all = timed(lambda: track(d_dev), args.reps)
        assert np.array_equal(r.T, rd.T) and r.iterations == rd.iterations
        (r1, st1), one_s, one_all = timed(lambda: track(d_dev, max_renders=1, inner_iters=1), args.reps)
        (r4, st4), four_s, four_all = timed(lambda: track(d_dev, max_renders=1, inner_iters=4), args.reps)
        (r2, st2), two_s, two_all = timed(lambda: track(d_dev, max_renders=2, inner_iters=1), args.reps)
        assert st1[3:5] == (1, 1) and st2[3:5] == (2, 2) and st4[4] == 1
        eval_s = (four_s - one_s) / (st4[3] - 1) if st4[3] > 1 else None
        render_s = (two_s - one_s) - eval_s if eval_s is not None else None
        return r, st, st4, dict(frame_s=frame_s, frame_all=frame_all, frame_device_s=frame_device_s, frame_device_all=frame_device_all, one_s=one_s, one_all=one_all,
                                four_s=four_s, four_all=four_all, two_s=two_s, two_all=two_all, eval_s=eval_s, render_s=render_s)

    r, st, st4, t = figures(track, depth, dptr)
    frame_s, frame_all, frame_device_s, frame_device_all = t["frame_s"], t["frame_all"], t["frame_device_s"], t["frame_device_all"]
    one_s, one_all, four_s, four_all, two_s, two_all, eval_s, render_s = (t[k] for k in ("one_s", "one_all", "four_s", "four_all", "two_s", "two_all", "eval_s", "render_s"))
    colour = None
    if args.colour:
        bgr, d_bgr = np.ascontiguousarray(frames["bgr"][k], np.uint8), C.c_void_p()
        assert L.dr_device_alloc(0, bgr.nbytes, C.byref(d_bgr)) == 0 and L.dr_memcpy_h2d(d_bgr, bgr.ctypes.data_as(C.c_void_p), bgr.nbytes) == 0

        def track_colour(d, **kw):
            b, dd = (int(d_bgr.value), d) if isinstance(d, int) else (bgr, d)
            rc = f.track_colour_frame(b, dd, start, raise_on_failure=False, **dict(o, **kw))
            return rc, f.track_colour_stats()

        rc, stc, stc4, colour = figures(track_colour, depth, dptr)
        L.dr_device_free(d_bgr)
        rotc, trc = pose_error(rc.T, pose, vs)
        colour.update(renders=stc[4], evaluations=stc[3], four_evaluations=stc4[3], status=ALIGN_STATUS[rc.status], device_bytes=stc[5], valid_at_start=rc.valid0,
                      valid_at_end=rc.valid, cost0=rc.cost0, cost=rc.cost, track_error_rotation_deg=rotc, track_error_translation_voxels=trc,
                      eval_ratio=(colour["eval_s"] / eval_s) if colour["eval_s"] and eval_s else None)
    pyramid = None
    if args.pyramid:
        bgr, d_bgr = np.ascontiguousarray(frames["bgr"][k], np.uint8), C.c_void_p()
        assert L.dr_device_alloc(0, bgr.nbytes, C.byref(d_bgr)) == 0 and L.dr_memcpy_h2d(d_bgr, bgr.ctypes.data_as(C.c_void_p), bgr.nbytes) == 0
        bptr = int(d_bgr.value)
        (rc, base_s, base_all) = timed(lambda: f.track_colour_frame(bptr, dptr, start, raise_on_failure=False, **o), args.reps)
        rotc, trc = pose_error(rc.T, pose, vs)
        pyramid = dict(colour_frame_device_s=base_s, colour_frame_device_all=base_all, colour_status=ALIGN_STATUS[rc.status], colour_error_rotation_deg=rotc,
                       colour_error_translation_voxels=trc, levels={}, reduce_s={},
                       not_measured="k_track_reduce alone (the reduce figures are whole calls with their synchronisation); what the unneeded full-resolution rays of "
                                    "a coarse render cost against a render at the level's resolution; counters")
        mj = 5.0 * vs
        d_out, c_out = C.c_void_p(), C.c_void_p()
        assert L.dr_device_alloc(0, depth.nbytes, C.byref(d_out)) == 0 and L.dr_device_alloc(0, bgr.nbytes, C.byref(c_out)) == 0
        for lvl in (1, 2, 3):
            _, s, runs = timed(lambda: f.track_reduce(lvl, mj * (1 << lvl), (bptr, int(c_out.value)), (dptr, int(d_out.value))), args.reps)
            pyramid["reduce_s"][str(lvl)] = dict(s=s, all=runs)
        L.dr_device_free(d_out)
        L.dr_device_free(c_out)
        for levels in (1, 3, 4):
            rp, s, runs = timed(lambda: f.track_pyramid_frame(bptr, dptr, start, raise_on_failure=False, levels=levels, **o), args.reps)
            stp = f.track_pyramid_stats()
            rotp, trp = pose_error(rp.T, pose, vs)
            entry = dict(frame_device_s=s, frame_device_all=runs, status=ALIGN_STATUS[rp.status], evaluations=stp[3], renders=stp[4], device_bytes=stp[5], levels_run=stp[6],
                         levels_abandoned=stp[7], per_level={str(lv): f.track_pyramid_level_stats(lv) for lv in range(levels)}, error_rotation_deg=rotp,
                         error_translation_voxels=trp)
            if levels > 1:  # one coarse round at the coarsest level: (one render and evaluation there and at level 0) - (the same at level 0 alone)
                _, two_l, _ = timed(lambda: f.track_pyramid_frame(bptr, dptr, start, raise_on_failure=False, levels=levels, coarse_renders=1,
                                                                  **dict(o, max_renders=1, inner_iters=1)), args.reps)
                _, two_m, _ = timed(lambda: f.track_pyramid_frame(bptr, dptr, start, raise_on_failure=False, levels=levels - 1, coarse_renders=1,
                                                                  **dict(o, max_renders=1, inner_iters=1)), args.reps)
                entry["coarse_round_s"] = two_l - two_m
            pyramid["levels"][str(levels)] = entry
        L.dr_device_free(d_bgr)
    la, locate_after_s, locate_after_all = timed(lambda: f.locate_frame(dptr, r.T32, raise_on_failure=False, centre_depth=cd), args.reps)
    alone = f.locate_frame(dptr, start, raise_on_failure=False, centre_depth=cd)
    L.dr_device_free(d_depth)
    rot0, tr0 = pose_error(start.astype(np.float64), pose, vs)
    rot, tr = pose_error(r.T, pose, vs)
    rotl, trl = pose_error(la.T, pose, vs)
    out = dict(frames=args.frames, height=args.height, width=args.width, map_blocks=f.stats()["blocks"], tracked_frame=k, reps=args.reps, centre_depth=cd,
               eps_rot=o["eps_rot"], eps_trans=o["eps_trans"], grid_positions=st[0], samples=r.samples, valid_at_start=r.valid0, valid_at_end=r.valid,
               device_bytes=st[5], frame_s=frame_s, frame_all=frame_all, frame_device_s=frame_device_s, frame_device_all=frame_device_all, renders=st[4],
               evaluations=st[3], status=ALIGN_STATUS[r.status], one_s=one_s, one_all=one_all, four_s=four_s, four_all=four_all, four_evaluations=st4[3],
               two_s=two_s, two_all=two_all, eval_s=eval_s, render_s=render_s, cost0=r.cost0, cost=r.cost, locate_after_s=locate_after_s,
               locate_after_all=locate_after_all, locate_after_iterations=la.iterations, locate_after_status=ALIGN_STATUS[la.status],
               locate_alone_status=ALIGN_STATUS[alone.status], locate_alone_valid=alone.valid, start_error_rotation_deg=rot0, start_error_translation_voxels=tr0,
               track_error_rotation_deg=rot, track_error_translation_voxels=tr, locate_error_rotation_deg=rotl, locate_error_translation_voxels=trl,
               not_measured="the kernels alone; k_track's fp64 share and the latency of its model gather; the phases of a render (plan, ray-cast, model map) apart")
    if colour is not None:
        out["colour"] = colour
    if pyramid is not None:
        out["pyramid"] = pyramid
    f.close()
    out["gpu_state"] = gpu_state()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
