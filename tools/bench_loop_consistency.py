#!/usr/bin/env python3
"""What the pairwise consistency of loop edges costs on the device (csm_loop_consistency) and on one host core
(csm_host_loop_consistency): M = 256, 1024, 4096 and 8192 loop edges on a seeded random walk of 10 000 scan
nodes in 1 000 local maps, the edges' noise at their stated covariance, 25 % of them gross outliers (off by 2 to
5 m), gate 11.34, --seeds greedy searches (default 8: from every vertex the selection alone is O(M^3) words on
either side).
The two entries alternate in this one process on one library build (only numbers of one run compare).
Host-inclusive wall time per call through the same Python marshalling (median of --repeats; the host entry runs
--host-repeats times at M >= 4096, where one call takes seconds), then one more device call with kernel timing
on for the two timers apart. Every output of the two entries is compared on every shape. One JSON line per
measurement, written to --out as well when given."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd"), os.path.dirname(os.path.abspath(__file__))]

from bench_loop_search import walk      # noqa: E402

SIGMA = np.array([0.05, 0.05, 0.02])


def loop_edges(poses, local, m, seed=3):
    from csm_hip import api
    rng = np.random.default_rng(seed)
    info = np.diag(1.0 / SIGMA ** 2)
    edges = []
    for k in range(m):
        s, t = int(rng.integers(0, len(local))), int(rng.integers(0, len(poses)))
        z = api.host_inverse_compound(local[s], poses[t]) + SIGMA * rng.normal(size=3)
        if k % 4 == 3:
            a, r = rng.uniform(0.0, 2.0 * math.pi), rng.uniform(2.0, 5.0)
            z[:2] += (r * math.cos(a), r * math.sin(a))
        edges.append(dict(local=s, scan=t, rel=z, info=info, loop=True))
    return api.pose_graph_edges(edges)


def median_ms(fn, repeats):
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 1024, 4096, 8192])
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from csm_hip import _lib as L, api
    lines = []

    def emit(d):
        d["library"] = L.load().csm_version().decode()
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    ctx = api.Context(0)
    poses = walk(10000)
    local = poses[::10].copy()
    for m in args.sizes:
        edges = loop_edges(poses, local, m)
        a = (local, poses, edges, 11.34)
        kw = dict(n_seeds=args.seeds, want_adjacency=True)
        dev = lambda: ctx.loop_consistency(*a, **kw)
        host = lambda: api.host_loop_consistency(*a, **kw)
        d, h = dev(), host()                    # warm-up, and the comparison
        same = all(d[k].tobytes() == h[k].tobytes() for k in ("selected", "degree", "adjacency")) and d["info"] == h["info"]
        host_reps = args.repeats if m < 4096 else args.host_repeats
        dev_t, host_t = [], []
        for r in range(max(args.repeats, host_reps)):   # alternating
            if r < args.repeats:
                dev_t.append(median_ms(dev, 1))
            if r < host_reps:
                host_t.append(median_ms(host, 1))
        dev_ms, host_ms = statistics.median(dev_t), statistics.median(host_t)
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        dev()
        chain_ms = ctx.kernel_time("loop_consistency")[0]
        pairs_ms = ctx.kernel_time("loop_consistency_pairs")[0]
        select_ms = ctx.kernel_time("loop_consistency_select")[0]
        ctx.enable_kernel_timing(False)
        n_pairs = m * (m - 1) // 2
        emit(dict(edges=m, seeds=d["info"]["seeds_run"], pairs=n_pairs, consistent_pairs=d["info"]["consistent_pairs"],
                  clique_size=d["info"]["clique_size"], device_ms=round(dev_ms, 4), chain_ms=round(chain_ms, 4),
                  pairs_kernel_ms=round(pairs_ms, 4), select_kernel_ms=round(select_ms, 4),
                  host_one_core_ms=round(host_ms, 4), host_over_device=round(host_ms / dev_ms, 3),
                  device_pairs_per_s=round(n_pairs / (pairs_ms * 1e-3)), host_pairs_per_s_whole_call=round(n_pairs / (host_ms * 1e-3)),
                  outputs_equal=bool(same)))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
