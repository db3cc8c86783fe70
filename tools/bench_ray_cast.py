#!/usr/bin/env python3
"""What a virtual scan (csm_ray_cast) costs on the map of bench.py's configs[1] (one 400 x 400 room at 5 cm):
1, 1 000 and --poses poses x 360 beams, range_max 20 m, sub-pixel scale 100, the poses spread over the room.
Two calls alternate in this one process on one library build (box-to-box variance is 8-12 %: only numbers of
one run compare):
  ray_cast        projection + walk + one read-back of the records, host-inclusive wall time;
  host_ray_cast   the sequential restatement, one core, timed on --host-poses poses and scaled.
Median of --repeats, then one more cast with kernel timing on for the split between "cast_project" and
"cast_walk". Per size: cells read per second of the walk kernel, and cells read / cells up to the stop (the
lane waste of one ray per wavefront; 1.0 = every lane of every group held a cell before the stop). The cell
rate of k_ray_walk to compare with is tools/bench_ray_check.py's cells / kernels_ms.ray_walk, from a run in the
same session. One JSON line per measurement, written to --out as well when given."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-poses", type=int, default=200, help="poses the one-core restatement is timed on")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import bench
    from csm_hip import _lib as L, api
    wl = bench.make_workload(0, 1)
    grid, geom = wl["grid"], wl["geom"]
    res, off_x, off_y = geom
    rows, cols = grid.shape
    rng = np.random.RandomState(99)
    n_max = max(args.poses, 1000)
    poses = np.stack([off_x + res * rng.uniform(0.2 * cols, 0.8 * cols, n_max),
                      off_y + res * rng.uniform(0.2 * rows, 0.8 * rows, n_max),
                      rng.uniform(-math.pi, math.pi, n_max)], axis=1)
    angles = -math.pi + 2 * math.pi * np.arange(360) / 360
    prm = api.ray_cast_params(range_max=20.0, subpixel_scale=100)
    lines = []

    def emit(d):
        d["library"] = L.load().csm_version().decode()
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    ctx = api.Context(0)
    ctx.upload_grid(1, grid)
    m = min(args.host_poses, n_max)
    host_ms = []
    for n in sorted({1, 1000, args.poses}):
        sets = [dict(map_id=1, geom=geom, angles=angles, poses=poses[:n])]
        cast = lambda: ctx.ray_cast(sets, params=prm)
        for _ in range(2):
            cast()
        t = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            recs, info = cast()
            t.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()                         # the restatement alternates with the cast
            api.host_ray_cast(grid, geom, angles, poses[:m], params=prm)
            host_ms.append((time.perf_counter() - t0) * 1e3 / m)
        ms = statistics.median(t)
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        cast()
        split = {k: round(ctx.kernel_time(k)[0], 4) for k in ("cast_project", "cast_walk")}
        ctx.enable_kernel_timing(False)
        walk_ms = split["cast_walk"]
        emit(dict(what="cast", entry="ray_cast", poses=n, beams=360, rays=info["rays"], ms=round(ms, 3),
                  rays_per_s=round(1e3 * info["rays"] / ms, 1), device_us=round(info["device_us"], 1),
                  kernels_ms=split, cells_read=info["cells_read"], cells_to_stop=info["cells_to_stop"],
                  cells_read_per_s=round(1e3 * info["cells_read"] / walk_ms, 1) if walk_ms > 0 else None,
                  read_over_to_stop=round(info["cells_read"] / max(info["cells_to_stop"], 1), 4),
                  stopped=int((recs[0]["kind"] != api.CAST_NONE).sum()), host_rays=info["host_rays"]))
    per_pose = statistics.median(host_ms)
    emit(dict(what="host", entry="host_ray_cast", poses_timed=m, ms_per_pose=round(per_pose, 4),
              ms_for_poses={str(n): round(per_pose * n, 1) for n in sorted({1, 1000, args.poses})}))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
