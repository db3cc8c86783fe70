#!/usr/bin/env python3
"""What the loop search by appearance costs on the device (csm_scan_descriptors, csm_appearance_search) and on
one host core (csm_host_scan_descriptors, csm_host_appearance_search), on the random-walk graph of
tools/bench_loop_search.py (10 000 scan nodes in a 40 m box, local maps of 10 nodes, travel threshold 10 m) with
a scan of 1080 beams synthesised per node (csm_hip.synth.cast_scan against the box's walls and a few boxes in
it), descriptors of 20 rings x 64 sectors over 0.5 .. 20 m:
  build    the descriptors of all scans in one call;
  online   the last local map's 10 and 50 nodes against 1 000 and 10 000 reference nodes, K = 2 and K = 16, every
           gate measured from the last node's travel distance, max_distance open (every pair is scored at every
           shift);
  offline  all 10 000 nodes as queries against all nodes before their gate, one record per map, K = 8, with
           --offline-max-distance as the gate (pairs whose ring distance exceeds it are not scored at any shift,
           on either side).
The two entries alternate in this one process on one library build after a warm-up; host-inclusive wall time
per call through the same Python marshalling, median of --repeats (the offline host call runs once: it takes
a minute or more); then one more device call with kernel timing on for the kernels' own time. The records of
the two entries are compared on every shape. One JSON line per measurement, written to --out as well when
given."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd"), os.path.join(ROOT, "tools")]

from bench_loop_search import timed_alternating, walk      # noqa: E402

SHAPE, RANGE = (20, 64), (0.5, 20.0)
U32_MAX = 0xffffffff


def world(box=20.0, n_boxes=16, seed=2):
    from csm_hip import synth
    rng = np.random.default_rng(seed)
    segs = synth._segments_of_box(-box - 1.0, -box - 1.0, box + 1.0, box + 1.0)
    for _ in range(n_boxes):
        cx, cy = rng.uniform(-box, box, 2)
        w, h = rng.uniform(1.0, 5.0, 2)
        segs += synth._segments_of_box(cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)
    return np.asarray(segs, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--offline-max-distance", type=int, default=400)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from csm_hip import _lib as L, api, synth
    lines = []

    def emit(d):
        d["library"] = L.load().csm_version().decode()
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    ctx = api.Context(0)
    poses = walk(args.nodes + 50)
    segs = world()
    scans = [synth.cast_scan(segs, p, n_beams=args.beams, max_range=25.0) for p in poses]
    angles, ranges, offsets = api.ragged_scans(scans)

    build = (angles, ranges, offsets, SHAPE[0], SHAPE[1], RANGE[0], RANGE[1])
    dev_ms, host_ms = timed_alternating((lambda: ctx.scan_descriptors(*build), lambda: api.host_scan_descriptors(*build)),
                                        args.repeats, warmup=1)
    desc, used = ctx.scan_descriptors(*build)
    hdesc, hused = api.host_scan_descriptors(*build)
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_timing()
    ctx.scan_descriptors(*build)
    kernel_ms = ctx.kernel_time("scan_descriptors")[0]
    ctx.enable_kernel_timing(False)
    emit(dict(what="build", scans=len(scans), beams=int(offsets[-1]), beams_used=int(used.sum()),
              device_ms=round(dev_ms, 4), kernel_ms=round(kernel_ms, 4), host_one_core_ms=round(host_ms, 4),
              host_over_device=round(host_ms / dev_ms, 3),
              descriptors_equal=bool(desc.tobytes() == hdesc.tobytes() and used.tobytes() == hused.tobytes())))

    shapes = [("online", n_ref, n_q, k, False, U32_MAX) for n_ref in sorted({1000, args.nodes}) for n_q in (10, 50)
              for k in (2, 16)]
    shapes.append(("offline", args.nodes, args.nodes, 8, True, args.offline_max_distance))
    for what, n_ref, n_q, k, per_map, gate in shapes:
        if what == "online":
            n = n_ref + n_q
            map_index = np.concatenate([np.arange(n_ref) // 10, np.full(n_q, (n_ref + 9) // 10)]).astype(np.int32)
            travel = api.host_travel_distances(poses[:n])
            q = np.arange(n_ref, n, dtype=np.int32)
            qt = np.full(n_q, travel[-1])
        else:
            n = n_ref
            map_index = (np.arange(n) // 10).astype(np.int32)
            travel = api.host_travel_distances(poses[:n])
            q = np.arange(n, dtype=np.int32)
            qt = travel.copy()
        a = (desc[:n], map_index, travel, q, qt, n_ref, 10.0, gate, 0, k, per_map)
        dev = lambda: ctx.appearance_search(*a)
        host = lambda: api.host_appearance_search(*a)
        if what == "online":
            dev_ms, host_ms = timed_alternating((dev, host), args.repeats, warmup=1)
            hrec, hcounts, hinfo = host()
        else:
            dev_ms, = timed_alternating((dev,), args.repeats, warmup=1)
            t0 = time.perf_counter()
            hrec, hcounts, hinfo = host()
            host_ms = (time.perf_counter() - t0) * 1e3
        drec, dcounts, dinfo = dev()
        same = drec.tobytes() == hrec.tobytes() and dcounts.tobytes() == hcounts.tobytes() and dinfo == hinfo
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        dev()
        kernel_ms = ctx.kernel_time("appearance_search")[0]
        ctx.enable_kernel_timing(False)
        emit(dict(what=what, ref_nodes=n_ref, queries=n_q, k=k, one_per_map=int(per_map), max_distance=gate,
                  pairs_evaluated=dinfo["pairs_evaluated"], pairs_eligible=dinfo["pairs_eligible"],
                  records=int(dcounts.sum()), upload_bytes=int(desc[:n].nbytes + 12 * n + 12 * n_q),
                  device_ms=round(dev_ms, 4), kernel_ms=round(kernel_ms, 4), host_one_core_ms=round(host_ms, 4),
                  host_over_device=round(host_ms / dev_ms, 3), records_equal=bool(same)))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
