#!/usr/bin/env python3
"""What the free-space check of loop candidates (csm_ray_check_batch) costs next to the search whose poses it
checks, on the maps of bench.py's configs[2] (256 candidate submaps of one room family, one 1080-beam query
scan): 1 and --queries queries, each checked at the pose the search found for it. Three calls alternate in
this one process on one library build (box-to-box variance is 8-12 %: only numbers of one run compare):
  ray_check_batch              projection + walk + one read-back, per_beam off;
  correlative_match_batch      the search of the same queries (2.5 m x 2.5 m x 0.5 rad, L = 4);
  host_ray_check               the sequential restatement, one core, one query after the other.
Host-inclusive wall time per call (median of --repeats), then one more check with kernel timing on for the
split between "ray_project" and "ray_walk". One JSON line per measurement, written to --out as well when
given."""
import argparse
import json
import os
import statistics
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-queries", type=int, default=8, help="queries the one-core restatement is timed on")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bench
    from csm_hip import _lib as L, api
    rx, ry, rt = bench.LOOP_PARAMS[:3]
    low = 4
    lines = []

    def emit(d):
        d["library"] = L.load().csm_version().decode()
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    ctx = api.Context(0)
    queries, _ = bench.make_loop_queries(ctx, 0, args.queries)
    grids = {q["map_id"]: ctx.download_level(q["map_id"], 0) for q in queries[:args.host_queries]}
    prm = api.ray_check_params(usable_range_min=0.01, usable_range_max=20.0, subpixel_scale=100, end_tolerance=1)
    for n in sorted({1, args.queries}):
        prep = ctx.prepare_queries(queries[:n])
        found = ctx.correlative_match_batch(prep, rx, ry, rt, low, 0.0, 0.0)
        poses = [s["estimated_pose"] for s in found]
        checked = ctx.prepare_queries([dict(q, init_pose=p) for q, p in zip(queries[:n], poses)])
        check = lambda: ctx.ray_check_batch(checked, params=prm)
        match = lambda: ctx.correlative_match_batch(prep, rx, ry, rt, low, 0.0, 0.0, as_records=True)
        check_ms, match_ms = timed_alternating((check, match), args.repeats)
        records = check()
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        check()
        split = {k: round(ctx.kernel_time(k)[0], 4) for k in ("ray_project", "ray_walk")}
        ctx.enable_kernel_timing(False)
        emit(dict(what="batch", queries=n, beams=int(prep.arr[0].scan.n_points), entry="ray_check_batch",
                  ms=round(check_ms, 3), queries_per_s=round(1e3 * n / check_ms, 1),
                  ratio_to_match=round(check_ms / match_ms, 4), kernels_ms=split,
                  cells=sum(r["cells"] for r in records), walked=sum(r["walked"] for r in records),
                  blocked=sum(r["blocked"] for r in records), host_beams=sum(r["host_beams"] for r in records)))
        emit(dict(what="batch", queries=n, entry="correlative_match_batch", ms=round(match_ms, 3)))
    m = min(args.host_queries, args.queries)
    t0 = time.perf_counter()
    for q, p in zip(queries[:m], poses[:m]):
        api.host_ray_check(grids[q["map_id"]], q["geom"], q["angles"], q["ranges"], q["rel_pose"], p, params=prm)
    host_ms = (time.perf_counter() - t0) * 1e3 / m
    emit(dict(what="host", entry="host_ray_check", queries_timed=m, ms_per_query=round(host_ms, 3),
              ms_for_batch=round(host_ms * args.queries, 1)))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
