#!/usr/bin/env python3
"""Marginal covariances of node pairs (csm_pose_graph_marginals) on synthetic graphs (synth.pose_graph_case,
10 scans per local map, 10 % wrong loop edges; the graphs of tools/bench_pose_graph.py) of 1000 / 5000 /
10000 scan nodes, for three pair lists:
  few    the last scan node against the last local map: a handful of columns (that map and the scan
         node's neighbours)
  last   the last scan node against every local map, the loop search's question: every local map is a
         column, as Sigma_ss and in X[s, s'] of the cross term
  all    every local map node alone: all columns, no scan node
One JSON line per (size, list): the device call as kernel time from HIP events (the chain, and inside it
the factorization and the substitution + pairs) and as wall time of the whole call, next to
csm_host_pose_graph_marginals on one core and next to one SchurCholesky LM step of the same graph on the
device, the three alternating in one process; and the largest |device - host| / sqrt(Sigma_ii Sigma_jj).

python tools/bench_pose_graph_marginals.py [--sizes 1000,5000,10000] [--reps 3] [--no-host-above N]
                                           [--out profiles/pose_graph_marginals_bench.jsonl]"""
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

BLOCKS = ("local_cov", "scan_cov", "cross_cov", "relative_cov")


def _difference(dev, host):
    worst = 0.0
    for d, h in zip(dev, host):
        ds, dt = np.sqrt(np.diag(h["local_cov"])), np.sqrt(np.diag(h["scan_cov"]))
        dr = np.sqrt(np.diag(h["relative_cov"]))
        scales = dict(local_cov=np.outer(ds, ds), scan_cov=np.outer(dt, dt), cross_cov=np.outer(ds, dt),
                      relative_cov=np.outer(dr, dr))
        for k in BLOCKS:
            if h[k].any():
                worst = max(worst, float((np.abs(d[k] - h[k]) / scales[k]).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,5000,10000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host-above", type=int, default=0,
                    help="skip the one-core host restatement for the `all` list above this many scan nodes (0: never)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_marginals_bench.jsonl"))
    a = ap.parse_args()
    ctx = api.Context(0)
    lines = []
    for n in [int(s) for s in a.sizes.split(",")]:
        c = synth.pose_graph_case(9000 + n, n_scans=n, wrong_fraction=0.1)
        nl = len(c["local"])
        graph = (c["local"], c["scan"], c["edges"])
        lists = dict(few=[(nl - 1, n - 1)], last=[(s, n - 1) for s in range(nl)], all=[(s, None) for s in range(nl)])
        for name, pairs in lists.items():
            ctx.pose_graph_marginals(*graph, pairs)         # warm-up: workspace allocation, code object
            ctx.pose_graph_lm(*graph, 1e-4, solver="SchurCholesky", iterations_max=1)
            ctx.enable_kernel_timing(True)
            ctx.reset_kernel_timing()
            walls, lm_walls, host_s = [], [], []
            with_host = name != "all" or not a.no_host_above or n <= a.no_host_above
            for _ in range(a.reps):
                t0 = time.perf_counter()
                dev, info = ctx.pose_graph_marginals(*graph, pairs)
                walls.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                ctx.pose_graph_lm(*graph, 1e-4, solver="SchurCholesky", iterations_max=1)
                lm_walls.append(time.perf_counter() - t0)
                if with_host and len(host_s) < 1:
                    t0 = time.perf_counter()
                    host, _ = api.host_pose_graph_marginals(*graph, pairs)
                    host_s.append(time.perf_counter() - t0)
            k_ms, k_n = ctx.kernel_time("pose_graph_marginals")
            f_ms, f_n = ctx.kernel_time("pose_graph_marginals_factor")
            s_ms, s_n = ctx.kernel_time("pose_graph_marginals_solve")
            lm_ms, lm_n = ctx.kernel_time("pose_graph")
            ctx.enable_kernel_timing(False)
            line = dict(scan_nodes=n, local_map_nodes=nl, edges=len(c["edges"]), pairs_list=name, pairs=len(pairs),
                        columns=info["n_columns"], device_kernel_ms=k_ms / max(k_n, 1),
                        device_factor_ms=f_ms / max(f_n, 1), device_solve_ms=s_ms / max(s_n, 1),
                        device_call_ms=1e3 * float(np.median(walls)),
                        lm_step_kernel_ms=lm_ms / max(lm_n, 1), lm_step_call_ms=1e3 * float(np.median(lm_walls)),
                        host_ms=1e3 * host_s[0] if host_s else None,
                        max_normalised_diff=_difference(dev, host) if host_s else None,
                        all_finite=all(r["finite"] for r in dev))
            print(json.dumps(line), flush=True)
            lines.append(line)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
