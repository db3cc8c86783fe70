"""Case table of the many-map builder (csm_construct_maps_from_scans): inputs on
synth.map_case that between them reach every path of the build chain, each with the
property it is in the table for. tests/test_cpu_map_batch_cases.py proves the
properties with the literal CPU builder; tests/test_gpu_map_batch.py runs the cases
alone, mixed in one call, chunked, and against the loop of single calls.

The builder settings are shared by a batch, so a case that needs its own usable
range carries it in its nodes' max_range: the builder uses min(usable_range_max,
node max_range) per node (grid_map_builder.cpp:606-607), so the rays are the same."""
import math

import numpy as np

from csm_hip import synth


def _limited(case, max_range):
    """The case with every node's usable range capped at max_range."""
    case = dict(case)
    case["nodes"] = [dict(nd, max_range=max_range) for nd in case["nodes"]]
    return case


def _reshaped(case, log2_block, off_x, off_y):
    """A frame left behind by earlier builds: another block size, offsets off the block lattice
    (as tests/test_gpu_map_build.py::test_map_randomised)."""
    shape = dict(case["shape"])
    n = 1 << log2_block
    shape["log2_block"] = log2_block
    shape["rows"] = shape["cols"] = -(-int(math.ceil(1.0 / shape["res"])) // n) * n
    shape["off_x"], shape["off_y"] = off_x, off_y
    return dict(case, shape=shape)


def _one_usable():
    case = synth.map_case(10, n_scans=1, n_beams=64)
    second = float(np.sort(np.asarray(case["nodes"][0]["ranges"]))[1])
    return _limited(case, second)          # r >= max_range is unusable: only the smallest range stays


def _aligned():
    """Sensors and walls on exact multiples of the resolution: hit points on cell edges, which the
    device cannot certify (tests/test_gpu_map_build.py::test_map_aligned_geometry)."""
    segs = [(-2.0, -1.5, 2.0, -1.5), (2.0, -1.5, 2.0, 1.5), (2.0, 1.5, -2.0, 1.5), (-2.0, 1.5, -2.0, -1.5)]
    nodes = []
    for pose in [(0.0, 0.0, 0.0), (0.25, 0.0, math.pi / 2), (0.25, 0.25, math.pi / 4)]:
        angles, ranges = synth.cast_scan(segs, pose, 720, 2 * math.pi, 10.0)
        nodes.append(dict(pose=pose, angles=angles, ranges=ranges, rel_pose=(0.0, 0.0, 0.0),
                          min_range=0.0, max_range=9.0))
    return dict(nodes=nodes, map_pose=(0.0, 0.0, 0.0),
                shape=dict(res=0.25, off_x=0.0, off_y=0.0, rows=8, cols=8, log2_block=2))


def _shared_pair():
    """Two local maps over the same scan arrays (consecutive local maps share their overlapped
    scans) under different map poses."""
    a = synth.map_case(16, n_scans=5, n_beams=360)
    p = a["nodes"][2]["pose"]
    b = dict(a, map_pose=(p[0] + 0.013, p[1] - 0.027, p[2] + 0.4))
    return a, b


# name -> (builder, property the oracle must show); property keys: shape (rows, cols), rays, updates,
# saturated, saturated_min, updates_min, beams, has_65535, all_zero
CASES = {
    "one_scan": (lambda: synth.map_case(0, n_scans=1, n_beams=90), dict(shape=(304, 272), rays=89)),
    "ten": (lambda: synth.map_case(3, n_scans=10, n_beams=360), dict(rays=3590, saturated=96)),
    "saturate": (lambda: synth.map_case(5, n_scans=30, n_beams=720, step=0.0),
                 dict(updates_min=2600000, saturated=11305, has_65535=True)),
    "tiny": (lambda: synth.map_case(8, n_scans=2, n_beams=64, max_range=3.0, res=0.2),
             dict(shape=(48, 48), rays=5)),
    "one_usable": (_one_usable, dict(rays=1, updates=22)),
    "none_usable": (lambda: _limited(synth.map_case(9, n_scans=2, n_beams=64), 0.02),
                    dict(shape=(48, 48), rays=0, all_zero=True)),
    "none_usable_one_node": (lambda: _limited(synth.map_case(9, n_scans=1, n_beams=64), 0.02),
                             dict(shape=(48, 48), rays=0, all_zero=True)),
    # ... and the first scan's beams at 0 and +-pi / 2 run along cell edges of the fresh frame
    "odd": (lambda: synth.map_case(12, n_scans=7, n_beams=181), dict(beams=1267, uncertain_min=2)),
    "fine": (lambda: synth.map_case(7, n_scans=3, n_beams=500, res=0.025, max_range=12.0), dict(beams=1500)),
    # sensor offset, range noise, other block sizes, offsets off the block lattice
    "blocks_of_4": (lambda: _reshaped(synth.map_case(14, n_scans=4, n_beams=181, rel_pose=(0.1, -0.05, 0.02),
                                                     noise=0.01), 2, 0.0137, -0.0219), dict(beams=724)),
    "blocks_of_32": (lambda: _reshaped(synth.map_case(15, n_scans=3, n_beams=360, rel_pose=(-0.12, 0.07, -0.3),
                                                      noise=0.01), 5, -3.2137, 4.8219), dict(beams=1080)),
    # hit points exactly on cell edges: beams the device projection cannot certify
    "aligned": (_aligned, dict(beams=2160, uncertain_min=2)),
    "shared_a": (lambda: _shared_pair()[0], dict(beams=1800)),
    "shared_b": (lambda: _shared_pair()[1], dict(beams=1800)),
}


def build(names=None):
    """[(name, case)] in table order; the shared pair is built once so that both jobs hold the very
    same angle and range arrays."""
    pair = _shared_pair()
    out = []
    for name, (make, _) in CASES.items():
        if names is not None and name not in names:
            continue
        out.append((name, pair[0] if name == "shared_a" else pair[1] if name == "shared_b" else make()))
    return out


# the cases that take two csm_update_map_with_scan calls after their build (test_updates_onto_batch_built_maps)
UPDATED = ("tiny", "odd", "blocks_of_4")


def update_nodes(case):
    """The nodes of the two updates: the map's own first node (its scan is in the map, so it fits and
    nothing is resized), then that node 3 m further along x (Expand must grow the map)."""
    nd = case["nodes"][0]
    return [nd, dict(nd, pose=(nd["pose"][0] + 3.0, nd["pose"][1], nd["pose"][2]))]


def edge_beams(case, subpixel=100):
    """Usable beams of the case whose hit point, computed as the builder's host path computes it, lies
    on a cell edge of the map's frame before the call (at the cell or the sub-pixel resolution) or
    closer to one than 1.4e-11 / resolution cells. The device certifies a beam only if it stays farther
    from the edge than its margin, which is never below 64 * 2.3e-16 * 1e3 / resolution (csm_certify.hpp,
    direct_margin): these beams it can never certify. cos(pi / 2) = 6e-17 puts a beam there as surely
    as sin(0) = 0 does."""
    shape, mp = case["shape"], case["map_pose"]
    count = 0
    for nd in case["nodes"]:
        # Compound(global pose, relative sensor pose), then InverseCompound(map pose, .)
        gp, rp = nd["pose"], nd["rel_pose"]
        gx = gp[0] + math.cos(gp[2]) * rp[0] - math.sin(gp[2]) * rp[1]
        gy = gp[1] + math.sin(gp[2]) * rp[0] + math.cos(gp[2]) * rp[1]
        dx, dy = gx - mp[0], gy - mp[1]
        x = math.cos(mp[2]) * dx + math.sin(mp[2]) * dy
        y = -math.sin(mp[2]) * dx + math.cos(mp[2]) * dy
        th = gp[2] + rp[2] - mp[2]
        for a, r in zip(np.asarray(nd["angles"], float), np.asarray(nd["ranges"], float)):
            if r >= min(20.0, nd["max_range"]) or r <= max(0.01, nd["min_range"]):
                continue
            hx, hy = x + r * math.cos(th + a), y + r * math.sin(th + a)
            on_edge = False
            for h, off in ((hx, shape["off_x"]), (hy, shape["off_y"])):
                for res in (shape["res"], shape["res"] / subpixel):
                    q = (h - off) / res
                    on_edge |= min(q - math.floor(q), math.ceil(q) - q) <= 1.4e-11 / res
            count += on_edge
    return count
