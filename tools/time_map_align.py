"""Times drf_align_system and drf_align_map on the maps tools/time_map_merge.py works on: the synth.room loop at TANDEM's shape
(640x480, 1 cm voxels), --frames frames (default 60), split into two sessions of half the frames each.  The second session is
integrated in a world frame of its own: its poses are the loop's moved by the inverse of a known small motion T_known (0.2 degrees
about (1, 2, 3) -- 1.4 voxels at 4 m from the origin -- and (1.5, -1.0, 0.8) voxels: inside the 4-voxel truncation band), so that
p_first = T_known p_second and the registration of the second map to the first from the identity should find T_known.  The two halves of the loop see partly different walls: about a fifth of the second map's
samples have an observed neighbourhood in the first, so the calls run with min_valid = --min-valid (default 0.1).

Host wall clock (every call returns with the device idle), same box and same session, median over --reps calls after one warm-up:
  system_s           one DrFusion.align_system at the identity: validation of both files, both uploads, one evaluation
  align_s            one DrFusion.align_map from the identity, with its iterations and status
  eval_s             (align_s - system_s) / (iterations - 1): what one further evaluation costs (kernels, fold, read-back, step)
  validate_s         drf_map_info of both files: the validation pass both calls start with
  setup_share        (system_s - eval_s) / align_s: the share of a registration taken by validation and upload
  numpy_eval_s       the numpy restatement of tests/test_map_align.py for ONE evaluation at the identity, in batches of --batch source
                     blocks, measured once: what a user had before.  Its sums and counts are compared bit for bit with align_system's.
As information: the pose found against T_known (rotation in degrees, translation in voxels) and the overlap valid / samples.
Not measured: the kernels alone, and the phases of a call apart from the validation.
Files are written through the page cache and read back from it.  One JSON line on stdout; --out writes it."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from _timing import fusion_options, room_loop  # noqa: E402


def known_motion(vs):
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(0.2)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = np.array([1.5, -1.0, 0.8]) * vs
    return T


def numpy_system(src_path, ref_path, T, batch):
    """np_system of tests/test_map_align.py with its per-block half run in batches (the blocks do not depend on each other)."""
    from tandem_amd import map_file
    from test_map_align import np_centre, np_fold, np_options, np_partials
    from test_map_transform import motion, sorted_source
    vs, sc, sv = map_file.read(src_path)
    _, rc, rv = map_file.read(ref_path)
    t0 = time.perf_counter()
    sk, sv = sorted_source(sc, sv)
    rk, rv = sorted_source(rc, rv)
    sc = map_file.unpack_keys(sk).astype(np.int64)
    R, tv = motion(T, vs)
    o = np_options(vs)
    c = np_centre(sc, R, tv)
    parts, counts = [], np.zeros(3, np.int64)
    for at in range(0, len(sc), batch):
        p, sample, valid, _ = np_partials(sc[at:at + batch], sv[at:at + batch], rk, rv, R, tv, c, vs, o)
        parts.append(p)
        counts += (int(sample.sum()), int(valid.sum()), int((sample & ~valid).sum()))
        if (at // batch) % 10 == 9:
            print("numpy route: %d of %d source blocks" % (at + len(p), len(sc)), file=sys.stderr, flush=True)
    sums = np_fold(np.concatenate(parts)) if parts else np.zeros(28)
    return sums, tuple(int(v) for v in counts), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num-blocks", type=int, default=400000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--min-valid", type=float, default=0.1)
    ap.add_argument("--no-before", action="store_true", help="skip the numpy restatement (and the bit comparison with it)")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_map_align.py needs a GPU: a timing taken without one says nothing"
    from tandem_amd.dr_fusion import ALIGN_STATUS, DrFusion, map_info
    poses, frames = room_loop(args.frames, args.height, args.width, device="cuda")
    opt = fusion_options(frames, args.num_blocks, 10.0, args.height, args.width)
    vs = float(opt.voxel_size)
    Tk = known_motion(vs)
    Tk_inv = np.linalg.inv(Tk)
    eye = np.eye(4, dtype=np.float32)
    with tempfile.TemporaryDirectory(dir=args.dir) as work:
        half = args.frames // 2
        paths = []
        for name, ks, S in (("first", range(half), None), ("second", range(half, args.frames), Tk_inv)):
            f = DrFusion(opt)
            for k in ks:
                pose = np.asarray(poses[k], np.float32) if S is None else (S @ np.asarray(poses[k], np.float64)).astype(np.float32)
                f.IntegrateScanAsync(frames["bgr"][k], frames["depth"][k], pose)
                f.RenderAsync([pose])
                f.GetRenderResult(copy=False)
            paths.append(os.path.join(work, name + ".drfmap"))
            f.save_map(paths[-1])
            f.close()
        ref, src = paths
        n_ref, n_src = ((os.path.getsize(p) - 72) // 4104 for p in (ref, src))
        f = DrFusion(opt)
        t0 = time.perf_counter()
        map_info(src)
        map_info(ref)
        validate_s = time.perf_counter() - t0
        sys_t, al_t = [], []
        for _ in range(args.reps + 1):  # the first one is the warm-up
            t0 = time.perf_counter()
            sums, counts = f.align_system(src, ref, eye)
            sys_t.append(time.perf_counter() - t0)
        stats = f.align_stats()
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            r = f.align_map(src, ref, eye, raise_on_failure=False, min_valid=args.min_valid)
            al_t.append(time.perf_counter() - t0)
        f.close()
        system_s, align_s = float(np.median(sys_t[1:])), float(np.median(al_t[1:]))
        eval_s = (align_s - system_s) / (r.iterations - 1) if r.iterations > 1 else None
        E = r.T @ Tk_inv  # the identity if the pose found is T_known
        rot_deg = float(np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))))
        out = dict(frames=args.frames, src_blocks=int(n_src), ref_blocks=int(n_ref), device_bytes=int(stats[5]), reps=args.reps,
                   min_valid=args.min_valid, samples=counts[0], valid_at_identity=counts[1], overlap_at_identity=counts[1] / max(counts[0], 1),
                   validate_s=validate_s, system_s=system_s, system_all=[round(x, 5) for x in sys_t],
                   align_s=align_s, align_all=[round(x, 5) for x in al_t], iterations=r.iterations, status=ALIGN_STATUS[r.status],
                   eval_s=eval_s, setup_share=(system_s - eval_s) / align_s if eval_s is not None else None,
                   valid_at_end=r.valid, cost0=r.cost0, cost=r.cost, known_motion=[float(v) for v in Tk.reshape(16)], pose=[float(v) for v in r.T.reshape(16)],
                   pose_error_rotation_deg=rot_deg, pose_error_translation_voxels=float(np.linalg.norm(E[:3, 3]) / vs),
                   not_measured="the kernels alone; the phases of a call (upload, evaluations) apart from the validation")
        if not args.no_before:
            nsums, ncounts, numpy_eval_s = numpy_system(src, ref, eye, args.batch)
            same = bool(np.array_equal(nsums.view(np.uint64), sums.view(np.uint64))) and ncounts == counts
            assert same, "align_system and the numpy restatement disagree"
            out.update(numpy_eval_s=numpy_eval_s, identical_bits=same, numpy_over_eval=numpy_eval_s / eval_s if eval_s else None)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
