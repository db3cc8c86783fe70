#!/usr/bin/env python3
"""What a likelihood field costs to build, for 1 and 256 resident maps of 400 x 400 cells (synthetic rooms,
about 1.3 % obstacle cells) at R in {3, 6, 16}. Three timings alternate in this one process on one library
build, round by round:

  device:  build_likelihood_maps, all maps in one launch;
  host:    the route it replaces -- download_level, csm_host_likelihood_map, upload_grid per map;
  pyramid: for scale, build_pyramids (box-max 4) on the same maps, freshly uploaded outside the timed part.

Host-inclusive wall time per call ending in a synchronise (median of the rounds), plus the kernel's own
time from one more device build with kernel timing on. One JSON line per measurement, written to --out as
well."""
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
    ap.add_argument("--maps", type=int, nargs="+", default=(1, 256))
    ap.add_argument("--radii", type=int, nargs="+", default=(3, 6, 16))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2, help="rounds that also time the host route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_bench.jsonl"))
    args = ap.parse_args()
    from csm_hip import _lib as L, api, synth
    rooms = [synth.make_room(40 + k, 400, 400, RES)[0] for k in range(DISTINCT)]
    lines = []

    def emit(d):
        d["library"] = L.load().csm_version().decode()
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    ctx = api.Context(0)
    for n in args.maps:
        srcs = [1000 + i for i in range(n)]
        dsts = [100000 + i for i in range(n)]
        host_dsts = [200000 + i for i in range(n)]
        pyr = [300000 + i for i in range(n)]
        for i, s in enumerate(srcs):
            ctx.upload_grid(s, rooms[i % DISTINCT])
        obstacles = sum(int((rooms[i % DISTINCT] >= 32768).sum()) for i in range(n)) / (n * 400.0 * 400.0)
        for R in args.radii:
            sigma = R * RES / 3.0
            table = api.host_likelihood_kernel(sigma, RES, R)
            t = dict(device=[], host=[], pyramid=[])

            def device():
                ctx.build_likelihood_maps(srcs, dsts, radius=R, kernel=table)      # returns when built

            def host():
                for s, d in zip(srcs, host_dsts):
                    ctx.upload_grid(d, api.host_likelihood_map(ctx.download_level(s, 0), radius=R, kernel=table))

            def pyramid():
                ctx.build_pyramids(pyr, [1, 4])
                ctx.synchronize()

            device()                    # warm-up: workspaces, code object
            for rnd in range(args.rounds):
                for name, fn in (("device", device), ("host", host), ("pyramid", pyramid)):
                    if name == "host" and rnd >= args.host_rounds:
                        continue
                    if name == "pyramid":
                        for i, p in enumerate(pyr):         # levels that exist are kept: start from bare maps
                            ctx.upload_grid(p, rooms[i % DISTINCT])
                    t0 = time.perf_counter()
                    fn()
                    t[name].append((time.perf_counter() - t0) * 1e3)
            same = t["host"] and all((ctx.download_level(d, 0) == ctx.download_level(h, 0)).all()
                                     for d, h in zip(dsts[:4], host_dsts[:4]))
            ctx.enable_kernel_timing(True)
            ctx.reset_kernel_timing()
            device()
            kernel_ms = ctx.kernel_time("likelihood")[0]
            ctx.enable_kernel_timing(False)
            med = {k: round(statistics.median(v), 4) for k, v in t.items() if v}
            emit(dict(what="likelihood_field", maps=n, rows=400, cols=400, radius=R, sigma=round(sigma, 5),
                      obstacle_share=round(obstacles, 5), device_ms=med["device"], host_route_ms=med.get("host"),
                      pyramid_ms=med["pyramid"], kernel_ms=round(kernel_ms, 4),
                      device_ms_all=[round(v, 4) for v in t["device"]], host_equals_device=bool(same)))
        for m in srcs + dsts + host_dsts + pyr:
            if ctx.has_grid(m):
                ctx.release_grid(m)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
