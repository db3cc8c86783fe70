"""Window shapes for the three units that read a window's whole score volume (peaks, volume covariance,
motion prior): the inputs of tests/test_gpu_volume_shapes.py that the CPU suite checks too
(tests/test_cpu_volume_shape_cases.py). Every case names a synthetic map + scan, a search range, the
coarse stride L and the properties of its window it is in the table for; the windows and every expected
result come from the references (peaks_reference, volume_reference, prior_reference), computed once per
process and shared. Pure numpy and the CPU oracle; no GPU.

A property is a statement about the reference's window shape (nt, nx, ny) and total = nt nx ny:
  one          total == 1
  nxc1, nyc1   nx // L == 1, ny // L == 1 (the axis is one coarse node)
  nt1          nt == 1
  row<256      nx ny < 256: a stride of 256 candidates carries into theta
  ny<4         ny < 4: a run of 4 candidates wraps through x
  <256 >256 <1024 >1024 <8192 >8192    total on that side of the kernels' strides and chunk size
  mod1 mod2 mod3                         total % 4
  capped       total > 256 * 8192: the cap of workgroups per window bites
  nodes>65536  more coarse nodes than one trip of the known-count kernel covers
  no_band      the closed form reports no edge-band contact
  ties         the winner's key is shared by more than 1000 candidates
  elig         a known-rate threshold takes the node of a threshold-0 peak out"""
import functools
import math

import numpy as np

import peaks_reference as PR
import prior_reference as P
import volume_reference as VR
from csm_hip import synth
from oracle import oracle as O

K_MAX, EXCL = 4, (1, 1, 1)          # a small exclusion box: tiny windows run out of candidates
TAUS = (0.005, 0.02)
LAMBDA_NAMES = ("diag", "full", "indef")


def sym(xx, yy, tt, xy=0.0, xt=0.0, yt=0.0):
    return np.array([[xx, xy, xt], [xy, yy, yt], [xt, yt, tt]], np.float64)


# tests/test_gpu_prior.py's matrices (that file imports the GPU fixtures; this one must not)
LAMBDAS = dict(diag=sym(2.0, 2.0, 40.0), full=sym(3.0, 2.0, 60.0, 1.0, 4.0, -3.0), indef=sym(1.5, 1.5, 20.0, 2.5))


def uniform_case():
    """tests/test_gpu_peaks.py's _uniform_case: every known cell the same value."""
    grid = np.zeros((96, 96), np.uint16)
    grid[8:88, 8:88] = 30000
    grid[30:40, 50:70] = 0
    n = 90
    ang = -math.pi + 2 * math.pi * np.arange(n) / n
    rng = np.full(n, 1.1)
    rng[::3] = 1.4
    rng[0] = 1.5
    return dict(grid=grid, geom=(0.05, -2.4 + 0.0137, -2.4 - 0.0219), angles=ang, ranges=rng,
                rel_pose=(0.0, 0.0, 0.0), init_pose=(0.31, -0.2, 0.1))


MAKERS = dict(
    beams360=lambda: synth.csm_case(2),                                     # 400 x 400, 360 beams
    unknown360=lambda: synth.csm_case(32, interior_unknown=0.25, rel_pose=(0.04, -0.02, 0.01)),
    big120=lambda: synth.csm_case(71, rows=640, cols=640, n_beams=120),
    uniform=uniform_case,
    # 1.6 m cells: the same search range in metres is a window of a few cells (the mixed batch)
    coarse_short=lambda: synth.csm_case(81, rows=24, cols=24, res=1.6, n_beams=90, max_range=1.0,
                                        init_error=(0.9, -0.7, 0.3), n_boxes=0),
    coarse_long=lambda: synth.csm_case(81, rows=24, cols=24, res=1.6, n_beams=90, max_range=20.0,
                                       init_error=(0.9, -0.7, 0.02), n_boxes=0),
)


@functools.lru_cache(maxsize=None)
def scan_case(maker):
    return MAKERS[maker]()


def _case(name, maker, cells, L, props, elig=False, metres=None):
    """cells = (wx, wy, wt): the window in search steps each side; metres: the range as given instead."""
    return dict(name=name, maker=maker, cells=cells, metres=metres, L=L, props=frozenset(props.split()), elig=elig)


def _tiny():
    """The issue's five shapes, (0, 0, 0), (0, 0.3, 0), (0.3, 0, 2 st), (0.1, 0.1, 2 st), (0.35, 0.2, 6 st) at
    0.05 m cells, over L: windows of (0, 0, 0), (0, 3, 0), (3, 0, 1), (1, 1, 1) and (4, 2, 3) steps."""
    out = []
    for L in (1, 2, 3, 4, 8):
        one = "one nt1 nxc1 nyc1" if L == 1 else "nt1 nxc1 nyc1"
        out.append(_case("point_L%d" % L, "beams360", (0, 0, 0), L, one + " row<256 <256" + (" ny<4" if L < 4 else "")))
        out.append(_case("ycol_L%d" % L, "beams360", (0, 3, 0), L, "nt1 nxc1 row<256 <256"))
        out.append(_case("xrow_L%d" % L, "beams360", (3, 0, 1), L, "nyc1 row<256 <256" + (" ny<4" if L < 4 else "")))
        out.append(_case("cube_L%d" % L, "beams360", (1, 1, 1), L,
                         "row<256 <256" + (" ny<4" if L in (1, 3) else "") + (" nxc1 nyc1" if L >= 3 else "")))
        out.append(_case("slab_L%d" % L, "beams360", (4, 2, 3), L, "row<256" + (" nyc1" if L == 8 else "")))
    # a known-rate threshold that bites on tiny L > 1 windows
    out.append(_case("slab_elig_L2", "unknown360", (4, 2, 3), 2, "row<256 elig", elig=True))
    out.append(_case("slab_elig_L4", "unknown360", (4, 2, 3), 4, "row<256 elig", elig=True))
    return out


MID = [
    # total = nt * nx * ny, just below and just above the strides 256 and 1024 and the chunk 8192
    _case("mid_255", "beams360", (2, 8, 1), 1, "<256 mod3 row<256"),                   # 3 x 5 x 17
    _case("mid_252", "beams360", (2, 2, 3), 2, "<256 row<256"),                        # 7 x 6 x 6
    _case("mid_261", "beams360", (14, 0, 4), 1, ">256 <1024 mod1 row<256 ny<4 nyc1"),  # 9 x 29 x 1
    _case("mid_270", "beams360", (1, 2, 7), 3, ">256 <1024 mod2 row<256"),             # 15 x 3 x 6
    _case("mid_1023", "beams360", (5, 15, 1), 1, "<1024 >256 mod3"),                   # 3 x 11 x 31
    _case("mid_1025", "beams360", (2, 2, 20), 1, ">1024 <8192 mod1 row<256"),          # 41 x 5 x 5
    _case("mid_1026", "beams360", (1, 2, 28), 3, ">1024 <8192 mod2 row<256"),          # 57 x 3 x 6
    _case("mid_8151", "beams360", (6, 9, 16), 1, "<8192 >1024 mod3 row<256"),          # 33 x 13 x 19
    _case("mid_8190", "beams360", (2, 7, 45), 3, "<8192 >1024 mod2 row<256"),          # 91 x 6 x 15
    _case("mid_8211", "beams360", (8, 11, 10), 1, ">8192 mod3"),                       # 21 x 17 x 23
    _case("mid_8400", "beams360", (9, 9, 10), 2, ">8192"),                             # 21 x 20 x 20
]

LARGE = [
    _case("big_L1", "big120", None, 1, "capped no_band >8192", metres=(6.4, 6.4, 1.15)),
    _case("big_L2", "big120", None, 2, "capped no_band >8192 nodes>65536", metres=(6.4, 6.4, 1.15)),
    _case("big_L3", "big120", None, 3, "capped no_band >8192 nodes>65536", metres=(6.4, 6.4, 1.15)),
    _case("big_ties_L2", "uniform", None, 2, "capped ties >8192 nodes>65536", metres=(6.4, 6.4, 4.3)),
]

# the mixed batch: one search range for every query, windows that differ through the maps' cell size
BATCH_RANGE, BATCH_L = (6.4, 6.4, 1.15), 2
BATCH = [
    _case("batch_short", "coarse_short", None, BATCH_L, "<256 row<256", metres=BATCH_RANGE),
    _case("batch_long", "coarse_long", None, BATCH_L, ">256 <1024 row<256", metres=BATCH_RANGE),
]

TINY = _tiny()
CASES = TINY + MID + LARGE
BY_NAME = {c["name"]: c for c in CASES + BATCH}
assert len(BY_NAME) == len(CASES) + len(BATCH)
NAMES = [c["name"] for c in CASES]


def search_range(c):
    """(rx, ry, rt) of a case: `cells` search steps each side (half the range is a quarter of a step short
    of them, so that no rounding of range / step decides), or the range in metres and radians as given."""
    if c["metres"] is not None:
        return c["metres"]
    case = scan_case(c["maker"])
    steps = O.search_step(case["geom"][0], case["ranges"])
    return tuple((2 * w - 0.5) * s if w else 0.0 for w, s in zip(c["cells"], steps))


@functools.lru_cache(maxsize=None)
def volume(name):
    """(case, prior_reference.volume of it): the oracle's dumps and the window, with the case's known-rate
    threshold. Computed once, shared, never changed."""
    c = BY_NAME[name]
    case = scan_case(c["maker"])
    rng = search_range(c)
    thr = 0.0
    if c["elig"]:       # tests/test_gpu_peaks.py's rule: the smallest rate among the nodes of the threshold-0 peaks
        ref0, _, win = PR.peaks(case, *rng, c["L"], K_MAX, EXCL)
        _, _, _, CK = O.csm_closed_form(case, *rng, c["L"], dump=True)
        wx, wy, wt = win["win"]
        thr = min(int(CK[r["best_theta"] + wt, (r["best_x"] + wx) // c["L"], (r["best_y"] + wy) // c["L"]])
                  for r in ref0) / float(len(case["angles"]))
    return case, P.volume(case, *rng, c["L"], 0.0, thr)


def shape_of(name):
    return volume(name)[1]["win"]["shape"]


def known_thr(name):
    return volume(name)[1]["known_thr"]


@functools.lru_cache(maxsize=None)
def peaks(name, k_max=K_MAX, excl=EXCL):
    """peaks_reference.select on the shared volume: the records, best first."""
    case, v = volume(name)
    wx, wy, wt = v["win"]["win"]
    return PR.select(v["S"], v["K"], v["CK"], v["L"], case["grid"], v["win"]["col"], v["win"]["row"], wx, wy, wt,
                     k_max, excl, v["score_thr"], v["known_thr"])


@functools.lru_cache(maxsize=None)
def summary(name, tau):
    """volume_reference.summary's dict on the shared volume (the same calls, without a second oracle run)."""
    case, v = volume(name)
    win = v["win"]
    wx, wy, wt = win["win"]
    best = peaks(name, 1, (0, 0, 0))
    m = VR.moments_of(v["S"], v["K"], v["CK"], v["L"], best[0] if best else None, wx, wy, wt, len(case["angles"]), tau,
                      v["known_thr"])
    if not m["best"]["found"]:
        return dict(moments=m, mean_offset=[0.0] * 3, sensor_covariance=[0.0] * 9, covariance=[0.0] * 9,
                    estimated_pose=None)
    _, est = PR.poses_of(m["best"], win, case["rel_pose"])
    mean, scov, cov = VR.covariance(m, win["steps"], est, case["rel_pose"])
    return dict(moments=m, mean_offset=mean, sensor_covariance=scov, covariance=cov, estimated_pose=est)


@functools.lru_cache(maxsize=None)
def prior(name, lam):
    """(prior_reference's result dict, clamped candidates) of the shared volume under LAMBDAS[lam]."""
    case, v = volume(name)
    return P.prior(v, case, LAMBDAS[lam])
