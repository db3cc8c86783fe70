#!/usr/bin/env python3
"""What a distance field costs to build. Shapes: 1 and 256 resident maps of 400 x 400 cells (synthetic rooms)
at R = 16 and R = 255; one 2000 x 2000 room at R = 255; one 400 x 400 map with a single obstacle in a corner
(the longest search of the row pass). Three timings alternate in this one process on one library build, round
by round:

  device:      build_distance_maps, all maps on one launch chain;
  host:        the route it replaces -- download_level, csm_host_distance_map, upload_grid per map;
  likelihood:  for scale, build_likelihood_maps at R = 16 on the same maps.

Host-inclusive wall time per call ending in a synchronise (median of the rounds), plus the two kernels' own
times from one more device build with kernel timing on. Every device result is compared with the host route's
cells, and the run ends with an error where they differ. One JSON line per measurement, written to --out as well. Only numbers of one run compare."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")]

RES = 0.05
DISTINCT = 8            # rooms generated; the maps cycle through them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2, help="rounds that also time the host route")
    ap.add_argument("--skip-large", action="store_true", help="leave the 2000 x 2000 map out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.host_rounds < 1 or args.rounds < args.host_rounds:
        ap.error("--host-rounds must be 1 .. --rounds: every device result is compared with the host route's cells")
    import numpy as np
    from csm_hip import _lib as L, api, synth
    rooms = [synth.make_room(40 + k, 400, 400, RES)[0] for k in range(DISTINCT)]
    single = np.zeros((400, 400), np.uint16)
    single[399, 399] = 50000
    shapes = [("rooms", 1, rooms, (16, 255)), ("rooms", 256, rooms, (16, 255)), ("single_obstacle", 1, [single], (255,))]
    if not args.skip_large:
        shapes.append(("room2000", 1, [synth.make_room(77, 2000, 2000, 0.025)[0]], (255,)))
    lines = []

    def emit(d):
        d["library"] = L.load().csm_version().decode()
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    ctx = api.Context(0)
    lf_table = api.host_likelihood_kernel(16 * RES / 3.0, RES, 16)
    for what, n, grids, radii in shapes:
        srcs = [1000 + i for i in range(n)]
        dsts = [100000 + i for i in range(n)]
        host_dsts = [200000 + i for i in range(n)]
        lf_dsts = [300000 + i for i in range(n)]
        for i, s in enumerate(srcs):
            ctx.upload_grid(s, grids[i % len(grids)])
        rows, cols = grids[0].shape
        obstacles = sum(int((grids[i % len(grids)] >= 32768).sum()) for i in range(n)) / (n * float(rows * cols))
        for R in radii:
            table = api.host_distance_kernel(R * RES / 3.0, RES, R)
            t = dict(device=[], host=[], likelihood=[])

            def device():
                ctx.build_distance_maps(srcs, dsts, radius=R, table=table)          # returns when built

            def host():
                for s, d in zip(srcs, host_dsts):
                    ctx.upload_grid(d, api.host_distance_map(ctx.download_level(s, 0), radius=R, table=table))

            def likelihood():
                ctx.build_likelihood_maps(srcs, lf_dsts, radius=16, kernel=lf_table)

            def equal():                # the device's cells against the host route's (built in round 0)
                return all((ctx.download_level(d, 0) == ctx.download_level(h, 0)).all()
                           for d, h in zip(dsts, host_dsts))

            same = True
            device()                    # warm-up: workspaces, code object
            likelihood()
            for rnd in range(args.rounds):
                for name, fn in (("device", device), ("host", host), ("likelihood", likelihood)):
                    if name == "host" and rnd >= args.host_rounds:
                        continue
                    t0 = time.perf_counter()
                    fn()
                    t[name].append((time.perf_counter() - t0) * 1e3)
                same = same and equal()         # outside the timed parts: this round's device result
            ctx.enable_kernel_timing(True)
            ctx.reset_kernel_timing()
            device()
            columns_ms, rows_ms = ctx.kernel_time("distance_columns")[0], ctx.kernel_time("distance_rows")[0]
            ctx.enable_kernel_timing(False)
            same = same and equal()
            med = {k: round(statistics.median(v), 4) for k, v in t.items() if v}
            emit(dict(what="distance_field", shape=what, maps=n, rows=rows, cols=cols, radius=R,
                      obstacle_share=round(obstacles, 6), device_ms=med["device"], host_route_ms=med.get("host"),
                      likelihood_r16_ms=med["likelihood"], columns_kernel_ms=round(columns_ms, 4),
                      rows_kernel_ms=round(rows_ms, 4), device_ms_all=[round(v, 4) for v in t["device"]],
                      host_equals_device=same))
            if not same:
                sys.exit("bench_distance: the device build of %s (%d maps, R = %d) was not compared equal to the "
                         "host route's cells" % (what, n, R))
        for m in srcs + dsts + host_dsts + lf_dsts:
            if ctx.has_grid(m):
                ctx.release_grid(m)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
