#!/usr/bin/env python3
"""What scoring a scan at many free poses costs (csm_score_pose_sets, csm_pose_set_update): 1 000, 10 000 and
100 000 poses of a 360- and a 1080-beam scan on the map of bench.py's configs[1] (a 400 x 400 room at 5 cm)
and on its likelihood field, the poses a particle cloud around the true pose. Three routes alternate in this
one process after a warm-up (box-to-box variance is 8-12 %: only numbers of one run compare):
  score_pose_sets      the new entry, host-inclusive (upload, kernels, one read-back);
  windows_dev          the only route there was: csm_host_project of every pose on the host, then
                       csm_score_windows_dev with one window of win_x = win_y = 0 per pose, 256 windows per
                       launch chain; timed on the first --old-poses poses and scaled to the set;
  host_score_poses     the restatement on one core, timed on the first --host-poses poses and scaled.
Then csm_pose_set_update on the same set (weights and as many ancestors as poses), and one more update with
kernel timing on for the split between the scoring kernels and the layer-2 chain ("pose_weights",
"pose_resample"). One JSON line per measurement, written to --out as well when given."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")]

KERNELS = ("pose_prep", "pose_score", "pose_rescore", "pose_weights", "pose_resample")


def timed_alternating(fns, repeats, warmup=1):
    """Median wall time (ms) of each of fns, called in turn."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    t = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            t[i].append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(v) for v in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--beams", type=int, nargs="+", default=[360, 1080])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--old-poses", type=int, default=1024, help="poses the windows_dev route is timed on")
    ap.add_argument("--host-poses", type=int, default=256, help="poses the one-core restatement is timed on")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from csm_hip import _lib as L, api, synth
    lines = []

    def emit(d):
        d["library"] = L.load().csm_version().decode()
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    dev = torch.device("cuda:0")
    grid, geom, segs = synth.make_room(1000, rows=400, cols=400, res=0.05)      # bench.make_workload(0, ..)
    ctx = api.Context(0)
    ctx.upload_grid(1, grid)
    ctx.build_pyramid(1, [1, 4])
    ctx.build_likelihood_map(1, 2, sigma=0.05, resolution=geom[0])
    ctx.build_pyramid(2, [1, 4])
    field = ctx.download_level(2, 0)
    truth = (0.11, -0.07, 0.05)
    rng = np.random.RandomState(77)
    for beams in args.beams:
        angles, ranges = synth.cast_scan(segs, truth, n_beams=beams, fov=1.5 * math.pi, max_range=5.7296)
        angles, ranges = np.ascontiguousarray(angles, np.float64), np.ascontiguousarray(ranges, np.float64)
        min_known = api.host_min_known(beams, 0.0)
        for n in args.poses:
            poses = np.asarray(truth) + rng.uniform(-1.0, 1.0, (n, 3)) * (0.25, 0.25, 0.15)
            for map_id, name, cells in ((1, "occupancy", grid), (2, "likelihood_field", field)):
                sets = [dict(map_id=map_id, geom=geom, angles=angles, ranges=ranges, poses=poses)]
                m_old, m_host = min(n, args.old_poses), min(n, args.host_poses)
                out_dev = torch.zeros(m_old * 48, dtype=torch.uint8, device=dev)
                window = ctx.make_window(1, beams, 0, 0, 4, 1, min_known, 0.0)

                def new_route():
                    return ctx.score_pose_sets(sets)

                def old_route():
                    cols, rows = [], []
                    for p in poses[:m_old]:
                        col, row = api.host_project(geom, p, 0.0, 0, angles, ranges)
                        cols.append(torch.from_numpy(col).to(dev))
                        rows.append(torch.from_numpy(row).to(dev))
                    for lo in range(0, m_old, 256):
                        hi = min(lo + 256, m_old)
                        prep = ctx.prepare_windows([map_id] * (hi - lo), [window] * (hi - lo),
                                                   [c.data_ptr() for c in cols[lo:hi]],
                                                   [r.data_ptr() for r in rows[lo:hi]])
                        ctx.score_windows_dev(prep, out_dev.data_ptr() + lo * 48)
                    ctx.synchronize()
                    return out_dev.cpu()

                def host_route():
                    return api.host_score_poses(cells, geom, angles, ranges, poses[:m_host])

                def update():
                    return ctx.pose_set_update(map_id, geom, angles, ranges, poses, 0.02, 0.1, n, 12345)

                new_ms, old_ms, host_ms, upd_ms = timed_alternating((new_route, old_route, host_route, update),
                                                                    args.repeats)
                recs, info = new_route()
                same = bool(np.array_equal(recs[0][:m_host], host_route()))
                ctx.enable_kernel_timing(True)
                ctx.reset_kernel_timing()
                upd = update()
                split = {k: round(ctx.kernel_time(k)[0], 4) for k in KERNELS}
                ctx.enable_kernel_timing(False)
                emit(dict(what="pose_sets", map=name, beams=beams, poses=n, score_pose_sets_ms=round(new_ms, 3),
                          poses_per_s=round(1e3 * n / new_ms), windows_dev_ms_scaled=round(old_ms * n / m_old, 2),
                          windows_dev_poses_timed=m_old, host_score_poses_ms_scaled=round(host_ms * n / m_host, 2),
                          host_poses_timed=m_host, speedup_over_windows_dev=round(old_ms * n / m_old / new_ms, 1),
                          speedup_over_one_core=round(host_ms * n / m_host / new_ms, 1),
                          pose_set_update_ms=round(upd_ms, 3), kernels_ms=split, device_us=round(info["device_us"], 1),
                          uncertain_poses=info["uncertain_poses"], changed_poses=info["changed_poses"],
                          equals_host=same, support=upd["update"]["support"],
                          effective_sample_size=round(api.effective_sample_size(upd["weights"]), 1)))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
