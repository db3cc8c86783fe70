#!/usr/bin/env python3
"""What the K best poses cost next to the single best one, on bench.py's configs[1] workload (1080 beams,
400 x 400 map at 5 cm, 4 m x 4 m x 60 deg, L = 4: 867,888 candidates per window). Two comparisons, both
sides in this one process on one library build:

  single: correlative_peaks (k_max 4 and 16) against correlative_match with CSM_TUNE_NO_TWO_PHASE
          (the exhaustive search the peaks are selected from), one window per call;
  batch:  correlative_peaks_batch against correlative_match_batch with CSM_TUNE_NO_BOUND_PASS
          (the exact kernel on every candidate block), 256 queries per call.

Host-inclusive wall time per call (median of --repeats), then one more call of each with kernel timing
on for the per-kernel split. One JSON line per measurement, appended to --out as well."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")]

KERNELS = ("project", "bin", "score_coarse", "score_fine", "finalize", "peaks_coarse", "peaks_select")


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def kernel_split(ctx, fn):
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_timing()
    fn()
    out = {k: round(ctx.kernel_time(k)[0], 4) for k in KERNELS}
    ctx.enable_kernel_timing(False)
    return {k: v for k, v in out.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--excl", type=int, nargs=3, default=(3, 3, 2), help="exclusion radii x y theta, search steps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peaks_bench.jsonl"))
    args = ap.parse_args()
    import bench
    from csm_hip import _lib as L, api
    wl = bench.make_workload(0, args.queries)
    rx, ry, rt, low = wl["params"]
    lines = []

    def emit(d):
        d["library"] = L.load().csm_version().decode()
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    # one window per call
    ctx = api.Context(0, tuning_off=L.TUNE_NO_TWO_PHASE)
    ctx.upload_grid(1, wl["grid"])
    s = wl["scans"][0]
    one = (1, wl["geom"], s["angles"], s["ranges"], s["rel_pose"], s["init_pose"], rx, ry, rt, low)
    match = lambda: ctx.correlative_match(*one)
    base_ms = timed(match, args.repeats)
    emit(dict(what="single", entry="correlative_match, CSM_TUNE_NO_TWO_PHASE", ms=round(base_ms, 4),
              candidates=match()["candidates"], kernels_ms=kernel_split(ctx, match)))
    for k_max in (4, 16):
        peaks = lambda: ctx.correlative_peaks(*one, k_max, tuple(args.excl))
        ms = timed(peaks, args.repeats)
        emit(dict(what="single", entry="correlative_peaks", k_max=k_max, excl=list(args.excl), ms=round(ms, 4),
                  ratio_to_match=round(ms / base_ms, 3), n_peaks=len(peaks()), kernels_ms=kernel_split(ctx, peaks)))
    ctx.close()

    # the batch
    ctx = api.Context(0, tuning_off=L.TUNE_NO_BOUND_PASS)
    ctx.upload_grid(1, wl["grid"])
    prep = ctx.prepare_queries([dict(map_id=1, geom=wl["geom"], angles=q["angles"], ranges=q["ranges"],
                                     rel_pose=q["rel_pose"], init_pose=q["init_pose"]) for q in wl["scans"]])
    match = lambda: ctx.correlative_match_batch(prep, rx, ry, rt, low, 0.0, 0.0, as_records=True)
    base_ms = timed(match, args.repeats)
    emit(dict(what="batch", queries=args.queries, entry="correlative_match_batch, CSM_TUNE_NO_BOUND_PASS",
              ms=round(base_ms, 3), kernels_ms=kernel_split(ctx, match)))
    for k_max in (4, 16):
        peaks = lambda: ctx.correlative_peaks_batch(prep, rx, ry, rt, low, k_max, tuple(args.excl), as_records=True)
        ms = timed(peaks, args.repeats)
        emit(dict(what="batch", queries=args.queries, entry="correlative_peaks_batch", k_max=k_max,
                  excl=list(args.excl), ms=round(ms, 3), ratio_to_match=round(ms / base_ms, 3),
                  n_peaks_total=int(sum(peaks()[1])), kernels_ms=kernel_split(ctx, peaks)))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
