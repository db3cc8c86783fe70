#!/usr/bin/env python3
"""csm_construct_maps_from_scans (one call for N maps) against the loop of
csm_construct_map_from_scans calls it replaces: N = 1, 16 and 256 maps of 10 scans x
1080 beams, both forms alternating in one process, warmed up, the median of the
repetitions. The ctypes arguments are built once, so only the library calls are
timed. At N = 1 two interleaved series of the single call show the spread the
batch call's median has to stay within. The 256-map case runs a second time with
the scans that overlapping local maps have in common shared (the same arrays), so
scan_bytes_uploaded shows what the de-duplication saves.

python tools/bench_map_batch.py [reps]      one JSON line per case"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd"))

from csm_hip import _lib as L, api, synth  # noqa: E402

POOL, SCANS, WINDOW, BEAMS = 8, 15, 10, 1080


def make_jobs(pool, n_maps, shared, keep):
    """n_maps local maps: map i is a window of 10 of the 15 scans of trajectory i % 8, starting at scan 0 or 5
    (neighbouring local maps overlap by half). shared: maps hold the very arrays of the pool."""
    jobs = (L.MapBuildJob * n_maps)()
    for i in range(n_maps):
        case = pool[i % POOL]
        first = 5 * ((i // POOL) % 2)
        nodes = case["nodes"][first:first + WINDOW]
        arr = (L.ScanNode * WINDOW)()
        for k, nd in enumerate(nodes):
            a, r = nd["angles"], nd["ranges"]
            if not shared:
                a, r = a.copy(), r.copy()
            keep += [a, r]
            arr[k].global_pose[:] = [nd["pose"][0] + 1e-3 * (i // POOL), nd["pose"][1], nd["pose"][2]]
            arr[k].scan.angles = a.ctypes.data_as(C.POINTER(C.c_double))
            arr[k].scan.ranges = r.ctypes.data_as(C.POINTER(C.c_double))
            arr[k].scan.n_points = a.size
            arr[k].scan.relative_sensor_pose[:] = list(nd["rel_pose"])
            arr[k].min_range, arr[k].max_range = nd["min_range"], nd["max_range"]
        keep.append(arr)
        s = case["shape"]
        jobs[i].map_id = 1000 + i
        jobs[i].shape = L.MapShape(s["res"], s["off_x"], s["off_y"], s["rows"], s["cols"], s["log2_block"])
        jobs[i].global_map_pose[:] = list(nodes[0]["pose"])
        jobs[i].nodes = arr
        jobs[i].n_nodes = WINDOW
    return jobs


def run_case(ctx, pool, n_maps, shared, reps):
    lib, keep = ctx.lib, []
    jobs = make_jobs(pool, n_maps, shared, keep)
    prm = L.MapBuilderParams(0.01, 20.0, 0.62, 0.46, 100)
    binfo, info = L.MapBatchInfo(), L.MapBuildInfo()
    ctx._check(lib.csm_construct_maps_from_scans(ctx._ctx, jobs, n_maps, C.byref(prm), None, C.byref(binfo)))
    # every repetition rebuilds the maps in the frames the first build left: the same work each time
    frames = [L.MapShape.from_buffer_copy(jobs[i].shape) for i in range(n_maps)]
    shapes = (L.MapShape * n_maps)()
    single_args = [(jobs[i].map_id, C.byref(shapes[i]), C.cast(jobs[i].global_map_pose, C.c_void_p), jobs[i].nodes)
                   for i in range(n_maps)]

    single, prm_ref, info_ref = lib.csm_construct_map_from_scans, C.byref(prm), C.byref(info)

    def reset():
        for i in range(n_maps):
            jobs[i].shape = frames[i]
            shapes[i] = frames[i]

    def batch():
        reset()
        t0 = time.perf_counter()
        rc = lib.csm_construct_maps_from_scans(ctx._ctx, jobs, n_maps, C.byref(prm), None, C.byref(binfo))
        dt = time.perf_counter() - t0
        ctx._check(rc)
        return dt

    def loop():
        reset()
        t0 = time.perf_counter()
        for map_id, shape, pose, nodes in single_args:
            rc = single(ctx._ctx, map_id, shape, pose, nodes, WINDOW, prm_ref, info_ref)
            if rc:
                ctx._check(rc)
        return time.perf_counter() - t0

    for _ in range(3):
        loop()
        batch()
    series = {"loop": [], "loop_again": [], "batch": []}
    for _ in range(reps):
        series["loop"].append(loop())
        if n_maps == 1:
            series["loop_again"].append(loop())
        series["batch"].append(batch())
    med = {k: statistics.median(v) * 1e3 for k, v in series.items() if v}
    out = dict(maps=n_maps, shared_scans=bool(shared), reps=reps, loop_ms=med["loop"], batch_ms=med["batch"],
               speedup=med["loop"] / med["batch"], batch_ms_per_map=med["batch"] / n_maps,
               batch_min_ms=min(series["batch"]) * 1e3, loop_min_ms=min(series["loop"]) * 1e3,
               chunks=binfo.chunks, scan_bytes_uploaded=binfo.scan_bytes_uploaded,
               batch_host_us=binfo.host_us, batch_device_us=binfo.device_us,
               rays=sum(jobs[i].info.rays for i in range(n_maps)),
               cell_updates=sum(jobs[i].info.cell_updates for i in range(n_maps)))
    if n_maps == 1:
        out["loop_again_ms"] = med["loop_again"]
        out["single_call_spread_ms"] = abs(med["loop"] - med["loop_again"])
        out["gate"] = "batch within the single call's spread: %s" % (
            med["batch"] <= max(med["loop"], med["loop_again"]) + out["single_call_spread_ms"])
    else:
        out["gate"] = "batch below the loop: %s" % (med["batch"] < med["loop"])
    for i in range(n_maps):
        ctx.release_grid(1000 + i)
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    if reps < 20:
        raise SystemExit("at least 20 repetitions")
    pool = [synth.map_case(100 + p, n_scans=SCANS, n_beams=BEAMS) for p in range(POOL)]
    for case in pool:
        for nd in case["nodes"]:
            nd["angles"] = np.ascontiguousarray(nd["angles"], np.float64)
            nd["ranges"] = np.ascontiguousarray(nd["ranges"], np.float64)
    ctx = api.Context(0)
    for n_maps, shared, r in ((1, False, max(reps, 200)), (16, False, max(reps, 50)), (256, False, reps),
                              (256, True, reps)):
        print(json.dumps(run_case(ctx, pool, n_maps, shared, r)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
