#!/usr/bin/env python3
"""PoseGraphOptimizerLM::Optimize with the default settings (ConjugateGradient, or --solver SchurCholesky
for the direct solver on the device; the host yardstick is always the ConjugateGradient restatement
on one core; 10 LM steps at most,
ErrorTolerance 1e-4, Huber 0.01, initial lambda 1e-4) on synthetic graphs (synth.pose_graph_case,
10 scans per local map, 10 % wrong loop edges) of 100 / 1000 / 5000 / 10000 scan nodes. One JSON
line per size: the device call (csm_pose_graph_lm) as kernel time from HIP events and as wall time
of the whole call (structure build, upload, kernel, download), the library's host restatement
(csm_host_pose_graph_lm) on one core, the LM steps and total CG iterations of each, and the largest
pose difference between the two.

python tools/bench_pose_graph.py [--solver ConjugateGradient|SchurCholesky] [--sizes 100,1000,5000,10000]
                                 [--reps 3] [--out FILE] [--append]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd"))

from csm_hip import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,1000,5000,10000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--solver", default="ConjugateGradient", choices=["ConjugateGradient", "SchurCholesky"],
                    help="the device call's solver")
    a = ap.parse_args()
    ctx = api.Context(0)
    lines = []
    for n in [int(s) for s in a.sizes.split(",")]:
        c = synth.pose_graph_case(9000 + n, n_scans=n, wrong_fraction=0.1)
        args = (c["local"], c["scan"], c["edges"], 1e-4)
        kw = dict(solver=a.solver)
        ctx.pose_graph_lm(*args, **kw)                 # warm-up: workspace allocation, code object
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        walls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            dl, ds, di = ctx.pose_graph_lm(*args, **kw)
            walls.append(time.perf_counter() - t0)
        k_ms, launches = ctx.kernel_time("pose_graph")
        ctx.enable_kernel_timing(False)
        t0 = time.perf_counter()
        hl, hs, hi = api.host_pose_graph_lm(*args)
        host_s = time.perf_counter() - t0
        line = dict(solver=a.solver, scan_nodes=n, local_map_nodes=len(c["local"]), edges=len(c["edges"]),
                    loop_edges=sum(e["loop"] for e in c["edges"]), variables=3 * (n + len(c["local"])),
                    device_kernel_ms=k_ms / max(launches, 1), device_call_ms=1e3 * float(np.median(walls)),
                    host_ms=1e3 * host_s, device_steps=di["steps"], host_steps=hi["steps"],
                    device_cg_iterations=di["cg_iterations"], host_cg_iterations=hi["cg_iterations"],
                    device_us_per_cg_iteration=1e3 * (k_ms / max(launches, 1)) / max(di["cg_iterations"], 1),
                    max_pose_diff=float(max(np.abs(dl - hl).max(), np.abs(ds - hs).max())),
                    speedup_vs_host=host_s * 1e3 / (k_ms / max(launches, 1)),
                    call_speedup_vs_host=host_s / float(np.median(walls)))
        print(json.dumps(line), flush=True)
        lines.append(line)
    ctx.close()
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
