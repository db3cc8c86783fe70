#!/usr/bin/env python3
"""What the loop search costs on the device (csm_loop_search) and on one host core (csm_host_loop_search), on
a seeded random walk of 10 000 scan nodes in a 40 m box (steps of 0.15 to 0.45 m, local maps of 10 nodes,
travel threshold 10 m, node threshold 2 m):
  online   the last local map's 10 and 50 nodes against 1 000 and 10 000 reference nodes, K = 2 and K = 16,
           every gate measured from the last node's travel distance (LoopSearcherNearest::Search's shape);
  offline  all 10 000 nodes as queries against all nodes before their gate, one_per_map = 1, K = 8.
The two entries alternate in this one process on one library build (box-to-box variance is 8-12 %: only
numbers of one run compare). Host-inclusive wall time per call through the same Python marshalling (median of
--repeats; --offline-repeats for the offline shape), then one more device call with kernel timing on for the
kernel's own time. The records of the two entries are compared on every shape. One JSON line per measurement,
written to --out as well when given."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")]


def timed_alternating(fns, repeats, warmup=2):
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


def walk(n, box=20.0, seed=1):
    rng = np.random.default_rng(seed)
    poses = np.zeros((n, 3))
    turn, step = rng.normal(0.0, 0.25, n), rng.uniform(0.15, 0.45, n)
    heading = 0.0
    for i in range(1, n):
        heading += turn[i]
        nxt = poses[i - 1, :2] + step[i] * np.array([np.cos(heading), np.sin(heading)])
        if np.abs(nxt).max() > box:
            heading += np.pi
            nxt = poses[i - 1, :2] + step[i] * np.array([np.cos(heading), np.sin(heading)])
        poses[i] = (nxt[0], nxt[1], heading)
    return poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--offline-repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from csm_hip import _lib as L, api
    lines = []

    def emit(d):
        d["library"] = L.load().csm_version().decode()
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    ctx = api.Context(0)
    poses = walk(args.nodes + 50)
    shapes = [("online", n_ref, n_q, k, False) for n_ref in sorted({1000, args.nodes}) for n_q in (10, 50)
              for k in (2, 16)]
    shapes.append(("offline", args.nodes, args.nodes, 8, True))
    for what, n_ref, n_q, k, per_map in shapes:
        if what == "online":
            sp = poses[:n_ref + n_q]
            map_index = np.concatenate([np.arange(n_ref) // 10, np.full(n_q, (n_ref + 9) // 10)]).astype(np.int32)
            travel = api.host_travel_distances(sp)
            q = np.arange(n_ref, n_ref + n_q, dtype=np.int32)
            qt = np.full(n_q, travel[-1])
        else:
            sp = poses[:n_ref]
            map_index = (np.arange(n_ref) // 10).astype(np.int32)
            travel = api.host_travel_distances(sp)
            q = np.arange(n_ref, dtype=np.int32)
            qt = travel.copy()
        a = (sp, map_index, travel, q, qt, n_ref, 10.0, 2.0, k, per_map)
        dev = lambda: ctx.loop_search(*a)
        host = lambda: api.host_loop_search(*a)
        reps = args.repeats if what == "online" else args.offline_repeats
        dev_ms, host_ms = timed_alternating((dev, host), reps, warmup=2 if what == "online" else 1)
        drec, dcounts, dinfo = dev()
        hrec, hcounts, hinfo = host()
        same = drec.tobytes() == hrec.tobytes() and dcounts.tobytes() == hcounts.tobytes() and dinfo == hinfo
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        dev()
        kernel_ms = ctx.kernel_time("loop_search")[0]
        ctx.enable_kernel_timing(False)
        emit(dict(what=what, ref_nodes=n_ref, queries=n_q, k=k, one_per_map=int(per_map),
                  pairs_evaluated=dinfo["pairs_evaluated"], pairs_eligible=dinfo["pairs_eligible"],
                  records=int(dcounts.sum()), device_ms=round(dev_ms, 4), kernel_ms=round(kernel_ms, 4),
                  host_one_core_ms=round(host_ms, 4), host_over_device=round(host_ms / dev_ms, 3),
                  records_equal=bool(same)))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
