"""What the projection certificate DECIDES, per family of kernels that project a beam:
which entries, poses, beams or queries the device hands to the host. tests/golden/make_certificate_records.py
records these decisions with the library of the commit it runs on, tests/test_gpu_certificate_records.py
recomputes them with the built library and compares: exact lists, exact integers.

Inputs are csm_hip.synth with fixed seeds. Every family has a generic frame, a frame with everything on exact
multiples of the resolution (hit points on cell edges: nothing there can be certified) and a far frame
(offsets around 1e3 m, headings around 1e2 rad, as in tests/test_gpu_projection.py)."""
import math

import numpy as np

from csm_hip import _lib as L, api, synth

N_BEAMS = 360
WIN_THETA = 4                         # 9 theta slices
N_POSES = 64
BASE = 8700                           # 8700 .. 8709: this module's map ids
FRAMES = ("generic", "aligned", "far")
MAP_CAP_MAX = 64                      # one scan of 64 beams: no list is longer


def frame(name):
    """dict(grid, geom, angles, ranges, rel_pose, pose): one scan at a map-local robot pose."""
    if name == "generic":
        c = synth.csm_case(610, n_beams=N_BEAMS)
        geom, pose = c["geom"], c["init_pose"]
    elif name == "aligned":
        c = synth.csm_case(611, n_beams=N_BEAMS, origin="aligned", truth=(0.0, 0.0, 0.0),
                           init_error=(0.05, -0.10, 0.0))
        geom, pose = c["geom"], c["init_pose"]
    else:
        c = synth.csm_case(612, n_beams=N_BEAMS)
        shift, turn = (1037.0, -1989.0), -101.0
        geom = (c["geom"][0], c["geom"][1] + shift[0], c["geom"][2] + shift[1])
        pose = (c["init_pose"][0] + shift[0], c["init_pose"][1] + shift[1], c["init_pose"][2] + turn)
    return dict(name=name, grid=c["grid"], geom=geom, angles=c["angles"], ranges=c["ranges"],
                rel_pose=(0.0, 0.0, 0.0), pose=tuple(float(v) for v in pose))


def poses_of(f):
    """N_POSES sensor poses around the frame's pose; in the aligned frame the second half sits on the cell
    lattice with the heading of the scan, so that axis-parallel beams end on cell edges."""
    rng = np.random.RandomState(620 + FRAMES.index(f["name"]))
    p = np.asarray(f["pose"]) + rng.uniform(-0.3, 0.3, (N_POSES, 3)) * (1.0, 1.0, 0.2)
    if f["name"] == "aligned":
        half = N_POSES // 2
        res = f["geom"][0]
        p[half:, 0] = rng.randint(-6, 7, N_POSES - half) * res
        p[half:, 1] = rng.randint(-6, 7, N_POSES - half) * res
        p[half:, 2] = 0.0
    return p


def _query(f, map_id):
    return dict(map_id=map_id, geom=f["geom"], angles=f["angles"], ranges=f["ranges"], rel_pose=f["rel_pose"],
                init_pose=f["pose"])


def _ints(a):
    return [int(v) for v in a]


def map_case():
    """One map of one 64-beam scan: the sensor and the walls in x on multiples of the resolution (a beam that
    ends on them cannot be certified, nor can the axis-parallel ones), the walls in y off them."""
    y = 1.5013
    segs = [(-2.0, -y, 2.0, -y), (2.0, -y, 2.0, y), (2.0, y, -2.0, y), (-2.0, y, -2.0, -y)]
    pose = (0.0, 0.0, 0.0)
    angles, ranges = synth.cast_scan(segs, pose, 64, 2 * math.pi, 10.0)
    nodes = [dict(pose=pose, angles=angles, ranges=ranges, rel_pose=(0.0, 0.0, 0.0), min_range=0.0, max_range=9.0)]
    return dict(nodes=nodes, map_pose=(0.0, 0.0, 0.0),
                shape=dict(res=0.25, off_x=0.0, off_y=0.0, rows=8, cols=8, log2_block=2))


def _device_projection(case, cap):
    ctx = api.Context(0, map_uncertain_cap=cap)
    try:
        _, info = ctx.construct_map_from_scans(BASE + 9, case["shape"], case["map_pose"], case["nodes"])
        ctx.release_grid(BASE + 9)
    finally:
        ctx.close()
    return int(info["device_projection"])


def record_map_build():
    """The least capacity of the uncertified-beam list at which the build keeps the device's hit points,
    stepping up from 1, and what one less gives."""
    case = map_case()
    below = None
    for cap in range(1, MAP_CAP_MAX + 1):
        dp = _device_projection(case, cap)
        if dp == 1:
            return dict(least_cap=cap, device_projection_below=below)
        below = dp
    return dict(least_cap=None, device_projection_below=below)


def record(ctx):
    """Every family's decisions on context `ctx` (the map build opens contexts of its own)."""
    frames = [frame(n) for n in FRAMES]
    doc = {"project_scan": {}, "pose_sets": {}, "ray_check": {}, "greedy_cost": {}, "hill_climbing": {}}
    for i, f in enumerate(frames):
        ctx.upload_grid(BASE + i, f["grid"])
    try:
        for f in frames:
            _, _, step_theta = api.host_search_step(f["geom"][0], f["ranges"])
            col, _, unc, count = ctx.project_scan(f["geom"], f["pose"], step_theta, WIN_THETA, f["angles"],
                                                  f["ranges"])
            doc["project_scan"][f["name"]] = dict(entries=int(col.size), count=int(count),
                                                  uncertified=sorted(_ints(unc)))
        sets = [dict(map_id=BASE + i, geom=f["geom"], angles=f["angles"], ranges=f["ranges"], poses=poses_of(f))
                for i, f in enumerate(frames)]
        for f, s in zip(frames, sets):
            recs, info = ctx.score_pose_sets([s])
            doc["pose_sets"][f["name"]] = dict(
                uncertain_poses=info["uncertain_poses"],
                flagged=_ints(np.nonzero(recs[0]["flags"] & L.POSE_UNCERTAIN)[0]))
        queries = [_query(f, BASE + i) for i, f in enumerate(frames)]
        for f, r in zip(frames, ctx.ray_check_batch(queries)):
            doc["ray_check"][f["name"]] = dict(host_beams=int(r["host_beams"]))
        fields = ("host_path", "replays", "cost_evaluations", "iterations", "refinements")
        for f, r in zip(frames, ctx.greedy_cost_covariance_batch(queries, [f["pose"] for f in frames])):
            doc["greedy_cost"][f["name"]] = {k: int(r[k]) for k in fields}
        for f, r in zip(frames, ctx.hill_climbing_batch(queries)):
            doc["hill_climbing"][f["name"]] = {k: int(r[k]) for k in fields}
    finally:
        for i in range(len(frames)):
            if ctx.has_grid(BASE + i):
                ctx.release_grid(BASE + i)
    doc["map_build"] = {"aligned": record_map_build()}
    return doc
