"""Shared by tools/time_*.py: the synth.room loop the four DrFusion timing tools run on, their engine options, and the merge of a
`rocprofv3 --kernel-trace --stats` summary (tools/rocprof_summary.py) into a tool's JSON result."""
import json
import os
import re

import numpy as np


def room_loop(n, height, width, device="cuda"):
    """The n-frame loop through synth.room: (poses, frames), frames = dict(bgr, depth, fx, fy, cx, cy).  Rendered on the device
    in chunks of 100 and kept in host memory (the operator takes host images)."""
    from synth import room
    poses = room.loop_poses(n, seed=0)
    bgr, depth = [], []
    for i in range(0, n, 100):
        fr = room.render_frames(poses[i:i + 100], height, width, device=device, seed=i)
        bgr.append(fr["bgr"].cpu().numpy())
        depth.append(fr["depth"].cpu().numpy())
    return poses, dict(bgr=np.concatenate(bgr), depth=np.concatenate(depth), fx=fr["fx"], fy=fr["fy"], cx=fr["cx"], cy=fr["cy"])


def fusion_options(frames, num_blocks, max_sensor_depth, height, width):
    """1 cm voxels, one render stream, the intrinsics of `frames`."""
    from tandem_amd.dr_fusion import DrFusionOptions
    return DrFusionOptions(voxel_size=0.01, num_buckets=num_blocks, bucket_size=10, num_blocks=num_blocks, block_size=8,
                           max_sdf_weight=64, truncation_distance=0.04, max_sensor_depth=max_sensor_depth, min_sensor_depth=0.1,
                           num_render_streams=1, fx=frames["fx"], fy=frames["fy"], cx=frames["cx"], cy=frames["cy"],
                           height=height, width=width)


def merge_kernel_stats(path, out, add, indent=None):
    """Reads the kernel rows (name, calls, total us, average us) of the summary at `path`, lets add(result, rows) put what the tool
    reports into the JSON result at `out`, writes it back and prints what add returns."""
    with open(out) as fh:
        res = json.load(fh)
    rows = []
    for line in open(path):
        m = re.match(r"(.*?)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+[\d.]+%$", line.rstrip())
        if m:
            rows.append((m.group(1).strip(), int(m.group(2)), float(m.group(3)), float(m.group(4))))
    shown = add(res, rows)
    res["kernel_stats"] = os.path.basename(path)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(shown, indent=indent))
