#!/usr/bin/env python3
"""What the motion prior costs next to the entries that existed before it, on bench.py's configs[1]
workload (1080 beams, 400 x 400 map at 5 cm, 4 m x 4 m x 60 deg, L = 4: 867,888 candidates per window), a
batch of --queries windows through three calls that alternate in this one process on one library build
(box-to-box variance is 8-12 %: only numbers of one run compare):
  correlative_match_prior_batch      exact scores + dump, coarse count, ONE pass that keeps both winners;
  correlative_peaks_batch(k_max = 1) the same volume plus one selection round: the yardstick;
  correlative_match_batch            the reference's search (bound pass, no dump): what a caller pays today.

Host-inclusive wall time per call (median of --repeats), then one more call of each with kernel timing on
for the per-kernel split: "prior_select" (k_prior_argmax + k_prior_pick) is to be read against
"peaks_select" (k_peaks_argmax + k_peaks_pick); both stream the same 6 bytes per candidate once. One JSON
line per measurement, written to --out as well when given."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")]

KERNELS = ("project", "bin", "score_coarse", "score_fine", "finalize", "peaks_coarse", "peaks_select", "prior_select")


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
    ap.add_argument("--information", type=float, nargs=3, default=(2.0, 2.0, 40.0),
                    help="diagonal of the prior's information matrix (x, y, theta), score units")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import bench
    from csm_hip import _lib as L, api
    wl = bench.make_workload(0, args.queries)
    rx, ry, rt, low = wl["params"]
    lam = np.diag(args.information)
    lines = []

    def emit(d):
        d["library"] = L.load().csm_version().decode()
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    ctx = api.Context(0)
    ctx.upload_grid(1, wl["grid"])
    prep = ctx.prepare_queries([dict(map_id=1, geom=wl["geom"], angles=q["angles"], ranges=q["ranges"],
                                     rel_pose=q["rel_pose"], init_pose=q["init_pose"]) for q in wl["scans"]])
    lams = [lam] * prep.n
    prior = lambda: ctx.correlative_match_prior_batch(prep, rx, ry, rt, low, lams, as_records=True)
    peaks = lambda: ctx.correlative_peaks_batch(prep, rx, ry, rt, low, 1, as_records=True)
    match = lambda: ctx.correlative_match_batch(prep, rx, ry, rt, low, 0.0, 0.0, as_records=True)
    prior_ms, peaks_ms, match_ms = timed_alternating((prior, peaks, match), args.repeats)
    rate = lambda ms: round(1e3 * prep.n / ms, 1)
    out = prior()
    moved = sum(bytes(o.prior.best) != bytes(o.prior.unweighted) for o in out)
    emit(dict(what="batch", queries=prep.n, entry="correlative_match_prior_batch", information=list(args.information),
              ms=round(prior_ms, 3), windows_per_s=rate(prior_ms), ratio_to_peaks=round(prior_ms / peaks_ms, 3),
              ratio_to_match=round(prior_ms / match_ms, 3), winners_moved=int(moved),
              kernels_ms=kernel_split(ctx, prior)))
    emit(dict(what="batch", queries=prep.n, entry="correlative_peaks_batch", k_max=1, ms=round(peaks_ms, 3),
              windows_per_s=rate(peaks_ms), kernels_ms=kernel_split(ctx, peaks)))
    emit(dict(what="batch", queries=prep.n, entry="correlative_match_batch", ms=round(match_ms, 3),
              windows_per_s=rate(match_ms), kernels_ms=kernel_split(ctx, match)))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
