"""Times the search scope (drf_set_search_scope(DRF_SEARCH_MAP)): the figures of profiles/search_scope_time.json.  One process; the
library is the one DR_MI355X_LIB names (default: the tree's product library).

Maps and lattices are those of profiles/search_score_time.json: the one-scan 96x128 scene (synth.scene seed 11, 1 968 blocks) and
the 60-frame room loop at 96x128 (fusion_helpers.room_frames, frame 30 searched), each with the 10 648-candidate lattice of
tests/test_map_search.py and the 99 144-candidate one (two chunks), pixel step 4, the anchor the frame's pose turned and moved as
scene_anchor does.  One engine per map with streaming on and a radius that evicts nothing; a score-only drf_search_frame from a
host image, host wall clock around a call that returns with the device idle, two warm-up rounds, then the median over --reps
rounds (default 20), every run listed.  In every round, in turn:
  a            the resident score, every block in the pool (the parent's score on a pool that holds the map)
  b            the parent's only route for a streamed map, the whole of it timed: drf_stream_in_region of everything, the resident
               score, drf_stream_out_region of everything again
  map_all      map scope, every block stored, the default capacity (if the default refuses the lattice, the size of the store:
               default_capacity says which, 0 being the default)
  map_passes   map scope, every block stored, the largest capacity of union/8, /6, /4, /3, /2 that the plan accepts: about 8 passes
  map_half     map scope, the half x <= median block x stored, the default capacity
all_scores of every state are held to a's, bit for bit.  stage_s of a map-scope state is its median minus a's: what the plan, the
packing, the copy and the staged fetch add to a call.  As information: drf_search_stats and drf_search_stage_stats of each state.
Not measured here: the kernels alone (a rocprofv3 --kernel-trace --stats run of this tool, in a run of its own).
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

EVERYWHERE = ((-500.0, -500.0, -500.0), (500.0, 500.0, 500.0))
STATES = ("a", "b", "map_all", "map_passes", "map_half")


def measure(f, depth, anchor, lattices, cut, reps, warmup=2):
    """f: an engine with streaming on whose blocks are all resident.  {lattice: {state: figures}}"""
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import SEARCH_MAP, SEARCH_RESIDENT
    from test_map_search import SCENE_STEP
    half_region = ((-500.0, -500.0, -500.0), (cut, 500.0, 500.0))
    out = {}
    for n, (rot, half) in lattices.items():
        kw = dict(half=half, top_k=8, score_only=True, score=dict(step=SCENE_STEP), all_scores=True)
        call = lambda: f.search_frame(depth, anchor, rot, **kw)  # noqa: E731
        # the capacity of map_passes: from the union that one pass stages
        f.stream_out_region(*EVERYWHERE)
        f.set_search_scope(SEARCH_MAP, 0)
        default, refused = 0, None                                      # the capacity of map_all and map_half: the default, if it serves
        try:
            call()
        except _lib.DrError as e:
            assert e.code == 5, e
            default, refused = f.streaming_stats()["host"], str(e)
            f.set_search_scope(SEARCH_MAP, default)
            call()
        union = f.search_stage_stats()[2] if f.search_stage_stats()[0] == 1 else f.streaming_stats()["host"]
        capacity = 0
        for part in (8, 6, 4, 3, 2):
            f.set_search_scope(SEARCH_MAP, max(union // part, 1))
            try:
                call()
            except _lib.DrError as e:
                assert e.code == 5, e
                continue
            capacity = max(union // part, 1)
            break
        f.stream_in_region(*EVERYWHERE)
        ts, last, stats = {s: [] for s in STATES}, {}, {}

        def timed(state, fn):
            t0 = time.perf_counter()
            last[state] = fn()
            ts[state].append(time.perf_counter() - t0)
            stats[state] = (list(f.search_stats()), list(f.search_stage_stats()), f.streaming_stats()["host"])

        def route_b():
            f.stream_in_region(*EVERYWHERE)
            r = call()
            f.stream_out_region(*EVERYWHERE)
            return r

        for _ in range(warmup + reps):
            f.set_search_scope(SEARCH_RESIDENT)                         # every block is resident here
            timed("a", call)
            f.stream_out_region(*EVERYWHERE)
            timed("b", route_b)                                         # begins and ends with everything stored
            f.set_search_scope(SEARCH_MAP, default)
            timed("map_all", call)
            if capacity:
                f.set_search_scope(SEARCH_MAP, capacity)
                timed("map_passes", call)
            f.stream_in_region(*EVERYWHERE)
            f.stream_out_region(*half_region)
            f.set_search_scope(SEARCH_MAP, default)
            timed("map_half", call)
            f.stream_in_region(*EVERYWHERE)
        res = dict(union_blocks=int(union), passes_capacity=int(capacity), default_capacity=int(default), default_capacity_refused=refused)
        for s in STATES:
            if not ts[s]:
                continue
            assert last[s].n_candidates == n and np.array_equal(last[s].scores.view(np.uint64), last["a"].scores.view(np.uint64)), (n, s)
            res[s] = dict(s=float(np.median(ts[s][warmup:])), all=[round(x, 7) for x in ts[s]], search_stats=stats[s][0], stage_stats=stats[s][1], stored_blocks=stats[s][2])
        for s in STATES[2:]:
            if s in res:
                res[s]["stage_s"] = res[s]["s"] - res["a"]["s"]
                res[s]["over_a"] = res[s]["s"] / res["a"]["s"]
                res[s]["over_b"] = res[s]["s"] / res["b"]["s"]
        out[str(n)] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3, "each figure is the median of at least 3 runs"
    import torch
    assert torch.cuda.is_available(), "time_search_scope.py needs a GPU: a timing taken without one says nothing"
    import fusion_helpers
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions, pose_rotations, streaming_min_radius
    from test_fusion_map_file_gpu import engine
    from test_fusion_map_transform_gpu import write
    from test_map_search import VS, scene_anchor, scene_lattice
    from test_map_track import track_scene
    lattices = {10648: scene_lattice(), 99144: (pose_rotations(np.arange(-32.0, 33.0, 4.0).tolist(), np.arange(-14.0, 15.0, 4.0).tolist()), (4, 4, 4))}
    out = dict(reps=args.reps, library=os.environ.get("DR_MI355X_LIB") or "tandem_amd/libdr_mi355x.so", states=list(STATES),
               not_measured="the kernels alone; the phases of a staging (plan, packing, copy, table) apart")
    with tempfile.TemporaryDirectory() as d:
        s = track_scene()
        write(os.path.join(d, "scene.drfmap"), VS, *s["blocks"])
        f = engine(s["cam"])
        f.load_map(os.path.join(d, "scene.drfmap"))
        f.set_streaming(max(streaming_min_radius(f.options), 200.0))      # on, and nothing is evicted by itself
        cut = float(np.median(s["blocks"][0][:, 0])) * 8 * VS
        out["scene 96x128"] = dict(blocks=len(s["blocks"][0]), **measure(f, s["depth"], scene_anchor(s)[None], lattices, cut, args.reps))
        f.close()
    fr, frames, H, W = fusion_helpers.room_frames()
    f = DrFusion(DrFusionOptions(**fusion_helpers.options(fr, H, W, VS)))
    for scan in frames:
        fusion_helpers.feed(f, *scan)
    f.set_streaming(max(streaming_min_radius(f.options), 200.0))
    coords = np.array(sorted(f.export_blocks()), np.int64).reshape(-1, 3)
    bgr, depth, pose = frames[30]
    out["room 96x128"] = dict(blocks=len(coords), **measure(f, np.ascontiguousarray(depth, np.float32), scene_anchor(dict(pose=pose))[None], lattices,
                                                           float(np.median(coords[:, 0])) * 8 * VS, args.reps))
    f.close()
    out["gpu_state"] = gpu_state()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
