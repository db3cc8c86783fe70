"""Case table of the global map builder (csm_construct_global_map): inputs on
synth.map_case, each with the property it is in the table for and, per rank setting,
the rank paths it must reach. tests/test_cpu_global_map_cases.py proves the properties
with the literal CPU builder and a numpy count of the hits per cell;
tests/test_gpu_global_map.py runs the cases and asserts from csm_global_map_info that
the paths were taken."""
import math

import numpy as np

import map_batch_cases as MB
from csm_hip import synth

# (rank_direct_max, rank_tile); (0, 0) = the library's defaults, 32 and 4096
RANKS = [(0, 0), (2, 4), (8, 16), (1, 64)]
DEFAULTS = (32, 4096)

# name -> (builder, property). Property keys as tests/map_batch_cases.py, plus max_hits_min (some cell
# has at least that many hits), above (n, at least so many cells with more than n hits) and paths:
# rank setting -> the paths ("direct", "sorted", "tiled") that at least three cells each take.
ALL = ("direct", "sorted", "tiled")
CASES = {
    "ten": (lambda: synth.map_case(3, n_scans=10, n_beams=360),
            dict(rays=3590, max_hits_min=20,
                 paths={(0, 0): ("direct",), (2, 4): ALL, (8, 16): ALL, (1, 64): ("direct", "sorted")})),
    "saturate": (lambda: synth.map_case(5, n_scans=30, n_beams=720, step=0.0),
                 dict(rays=21570, max_hits_min=150, has_65535=True,
                      paths={(0, 0): ("direct", "sorted"), (2, 4): ALL, (8, 16): ALL, (1, 64): ALL})),
    "revisit": (lambda: synth.map_case(1, n_scans=120, n_beams=1080, step=0.0),
                dict(max_hits_min=1000, above=(256, 100),
                     paths={(0, 0): ("direct", "sorted"), (8, 16): ALL})),
    "one_scan": (MB.CASES["one_scan"][0], dict(MB.CASES["one_scan"][1], paths={rk: ("direct",) for rk in RANKS})),
    "none_usable": (MB.CASES["none_usable"][0], dict(MB.CASES["none_usable"][1], paths={rk: () for rk in RANKS})),
    "odd": (MB.CASES["odd"][0],
            dict(MB.CASES["odd"][1], paths={(0, 0): ("direct",), (2, 4): ALL, (8, 16): ("direct", "sorted"),
                                            (1, 64): ("direct", "sorted")})),
}

# the cases that run under every rank setting in one part, and under the three part cuts
SMALL = ("ten", "saturate", "one_scan", "none_usable", "odd")
CUT = ("ten", "saturate", "odd")
# ... of which these have, under (2, 4), cells that are sorted in every single node (odd: 181 beams, none)
NODE_LONG = ("ten", "saturate")


def build(names=None):
    return [(name, make()) for name, (make, _) in CASES.items() if names is None or name in names]


def beams(case):
    return [len(nd["ranges"]) for nd in case["nodes"]]


def hits_per_cell(case, shape, usable_min=0.01, usable_max=20.0):
    """Hit points per cell of the built map (shape = the frame after the build), projected with numpy:
    good to a few hits at cell edges. Returns the sorted counts of the cells with hits."""
    mp = case["map_pose"]
    cells = []
    for nd in case["nodes"]:
        gp, rp = nd["pose"], nd["rel_pose"]
        gx = gp[0] + math.cos(gp[2]) * rp[0] - math.sin(gp[2]) * rp[1]
        gy = gp[1] + math.sin(gp[2]) * rp[0] + math.cos(gp[2]) * rp[1]
        dx, dy = gx - mp[0], gy - mp[1]
        x = math.cos(mp[2]) * dx + math.sin(mp[2]) * dy
        y = -math.sin(mp[2]) * dx + math.cos(mp[2]) * dy
        th = gp[2] + rp[2] - mp[2]
        a, r = np.asarray(nd["angles"], float), np.asarray(nd["ranges"], float)
        ok = ~((r >= min(usable_max, nd["max_range"])) | (r <= max(usable_min, nd["min_range"])))
        col = np.floor((x + r[ok] * np.cos(th + a[ok]) - shape["off_x"]) / shape["res"]).astype(np.int64)
        row = np.floor((y + r[ok] * np.sin(th + a[ok]) - shape["off_y"]) / shape["res"]).astype(np.int64)
        cells.append(row * shape["cols"] + col)
    if not cells:
        return np.zeros(0, np.int64)
    _, counts = np.unique(np.concatenate(cells), return_counts=True)
    return np.sort(counts)


def paths_taken(counts, rank):
    """Cells per rank path for the hit counts `counts` under a rank setting."""
    direct_max, tile = rank if rank != (0, 0) else DEFAULTS
    counts = np.asarray(counts)
    return dict(direct=int(((counts >= 1) & (counts <= direct_max)).sum()),
                sorted=int(((counts > direct_max) & (counts <= tile)).sum()),
                tiled=int((counts > tile).sum()))
