#!/usr/bin/env python3
"""Hill-climbing batches (csm_hill_climbing_batch) of 1080-beam scans, for the
default "ScanMatcherHillClimbing" settings and the frontend's
"FinalScanMatcherHillClimbing" settings. One JSON line per (settings, batch size):
queries/s and cost evaluations/s of the device batch, the replay fraction (passes
whose decisions took the literal sums), the host-fallback count, the "greedy"
kernel time, and the library's host restatement (csm_host_hill_climbing) on one
core, timed on the first min(n, host_queries) queries of the batch.

python tools/bench_hill_climbing.py [--sizes 1,64,256,2048] [--reps 5] [--host-queries 32] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd"))

from csm_hip import api, synth  # noqa: E402

SETTINGS = {
    "ScanMatcherHillClimbing": (0.1, 0.1, 100, 5),
    "FinalScanMatcherHillClimbing": (0.01, 0.01, 5, 2),
}
N_MAPS = 16


def make_queries(ctx, n, offset_scale, seed=0):
    rng = np.random.RandomState(seed)
    maps = []
    for m in range(N_MAPS):
        c = synth.csm_case(4000 + m, rows=400, cols=400, n_beams=1080, fov=1.5 * math.pi, max_range=8.0)
        ctx.upload_grid(90000 + m, c["grid"])
        maps.append(c)
    qs = []
    for i in range(n):
        c = maps[i % N_MAPS]
        init = tuple(np.asarray(c["truth"]) + rng.uniform(-1, 1, 3) * offset_scale)
        qs.append(dict(map_id=90000 + i % N_MAPS, geom=c["geom"], angles=c["angles"], ranges=c["ranges"],
                       rel_pose=(0.05, 0.0, 0.0), init_pose=init, grid=c["grid"]))
    return qs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,256,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-queries", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = api.Context(0)
    lines = []
    for name, hc in SETTINGS.items():
        scale = (0.15, 0.15, 0.05) if hc[2] > 5 else (0.02, 0.02, 0.01)
        for n in [int(s) for s in a.sizes.split(",")]:
            qs = make_queries(ctx, n, np.array(scale), seed=n)
            prep = ctx.prepare_queries(qs)
            out = ctx.hill_climbing_batch(prep, *hc, as_records=True)       # warm-up
            ctx.enable_kernel_timing(True)
            ctx.reset_kernel_timing()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                out = ctx.hill_climbing_batch(prep, *hc, as_records=True)
            dt = (time.perf_counter() - t0) / a.reps
            kms, launches = ctx.kernel_time("greedy")
            ctx.enable_kernel_timing(False)
            evals = sum(o.cost_evaluations for o in out)
            passes = sum(o.iterations + (1 if o.iterations < hc[2] else 0) for o in out)
            replays = sum(o.replays for o in out)
            fallbacks = sum(o.host_path for o in out)
            nh = min(n, a.host_queries)
            t0 = time.perf_counter()
            for q in qs[:nh]:
                api.host_hill_climbing(q["grid"], q["geom"], q["angles"], q["ranges"], q["rel_pose"],
                                       q["init_pose"], *hc)
            host_s = (time.perf_counter() - t0) / nh
            line = dict(settings=name, linear_step=hc[0], angular_step=hc[1], max_iterations=hc[2],
                        max_refinements=hc[3], queries=n, beams=1080,
                        batch_ms=dt * 1e3, kernel_ms=kms / max(launches, 1),
                        queries_per_s=n / dt, cost_evals_per_s=evals / dt,
                        mean_iterations=float(np.mean([o.iterations for o in out])),
                        cost_evals_per_query=evals / n, replay_fraction=replays / max(passes, 1),
                        host_fallbacks=fallbacks,
                        host_ms_per_query=host_s * 1e3, host_ms_batch_estimate=host_s * n * 1e3,
                        speedup_vs_host=host_s * n / dt)
            print(json.dumps(line), flush=True)
            lines.append(line)
            for m in range(N_MAPS):
                ctx.release_grid(90000 + m)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
