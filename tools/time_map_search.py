"""Times the pose search on the maps its tests work on: the figures of profiles/search_score_time.json and
profiles/search_colour_time.json that an A/B of two builds needs.  One process per run; the library is the one DR_MI355X_LIB names
(default: the tree's product library).

Host wall clock around calls that return with the device idle, two warm-ups, then the median over --reps calls (default 20; the
whole search: --search-reps, default 10), all runs listed:
  score_10648_s, score_colour_10648_s    a score-only drf_search_frame / drf_search_colour_frame (host images, step 4) over the
                                         10 648-candidate lattice of tests/test_map_search.py on the one-scan 96x128 scene
                                         (synth.scene seed 11, oracle-integrated); the two calls alternate, call by call
  score_99144_s, score_colour_99144_s    the same over yaw -32..32 by 4 x pitch -14..14 by 4, half (4, 4, 4): two chunks
  wall_search_colour_s                   the end-to-end drf_search_colour_frame of tests/test_map_search_colour.py: the
                                         oracle-integrated wall at 48x64, 147 candidates, top_k 3, one tracking level
As information: drf_search_stats of each call, and the whole search's status, winner and refined entries.
Not measured: the kernels alone (a rocprofv3 --kernel-trace --stats run of this tool, in a run of its own).
One JSON line on stdout; --out writes it, ending with the box's gpu_state."""
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
from time_map_locate import gpu_state  # noqa: E402


def timed(calls, reps, warmup=2):
    """calls: {name: function}, run in turn in every round.  {name: (last result, median, all runs)}"""
    ts, last = {k: [] for k in calls}, {}
    for _ in range(warmup + reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            last[k] = fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: (last[k], float(np.median(ts[k][warmup:])), [round(x, 7) for x in ts[k]]) for k in calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--search-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5 and args.search_reps >= 5, "each figure is the median of at least 5 runs"
    import torch
    assert torch.cuda.is_available(), "time_map_search.py needs a GPU: a timing taken without one says nothing"
    import test_map_search_colour as SC
    from tandem_amd.dr_fusion import pose_rotations
    from test_fusion_map_file_gpu import engine
    from test_fusion_map_transform_gpu import write
    from test_map_search import SCENE_STEP, VS, scene_anchor, scene_lattice
    from test_map_track import track_scene
    out = dict(reps=args.reps, search_reps=args.search_reps, library=os.environ.get("DR_MI355X_LIB") or "tandem_amd/libdr_mi355x.so",
               not_measured="the kernels alone; the phases of a call (upload, points, score, read-back) apart")
    with tempfile.TemporaryDirectory() as d:
        s = track_scene()
        write(os.path.join(d, "scene.drfmap"), VS, *s["blocks"])
        f = engine(s["cam"])
        f.load_map(os.path.join(d, "scene.drfmap"))
        anchor = scene_anchor(s)[None]
        lattices = {10648: scene_lattice(), 99144: (pose_rotations(np.arange(-32.0, 33.0, 4.0).tolist(), np.arange(-14.0, 15.0, 4.0).tolist()), (4, 4, 4))}
        for n, (rot, half) in lattices.items():
            kw = dict(half=half, top_k=8, score_only=True, score=dict(step=SCENE_STEP))
            stats = {}

            def geometric():
                r = f.search_frame(s["depth"], anchor, rot, **kw)
                stats["score"] = f.search_stats()
                return r

            def colour():
                r = f.search_colour_frame(s["bgr"], s["depth"], anchor, rot, **kw)
                stats["score_colour"] = f.search_stats()
                return r

            for name, (r, med, runs) in timed(dict(score=geometric, score_colour=colour), args.reps).items():
                assert r.n_candidates == n and stats[name][0] == n, (name, r.n_candidates, stats[name])
                out["%s_%d_s" % (name, n)], out["%s_%d_all" % (name, n)], out["%s_%d_stats" % (name, n)] = med, runs, list(stats[name])
        f.close()
        w = SC.integrated_wall()
        write(os.path.join(d, "wall.drfmap"), VS, *w["blocks"])
        f = engine(w["cam"])
        f.load_map(os.path.join(d, "wall.drfmap"))
        kw = dict(SC.WALL_END_TO_END)
        track = dict(kw.pop("track"))
        kw.update(levels=track.pop("levels"), track=track)
        search = lambda: f.search_colour_frame(w["bgr"], w["depth"], SC.wall_anchor()[None], np.eye(3).reshape(1, 9), **kw)  # noqa: E731
        r, med, runs = timed(dict(wall=search), args.search_reps)["wall"]
        out.update(wall_search_colour_s=med, wall_search_colour_all=runs, wall_search_colour_stats=list(f.search_stats()), wall_status=int(r.status),
                   wall_winner=int(r.winner), wall_refined=int(r.refined), wall_winner_candidate=int(r.entries[r.winner].index) if r.winner >= 0 else None)
        f.close()
    out["gpu_state"] = gpu_state()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
