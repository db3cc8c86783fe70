"""The beam-count ladder of the window chains, without a GPU: the size rules that switch a chain at a
beam count, restated in plain Python, the rungs they imply (the last n on one side, the first on the
other), what k_binj makes of a pair of slices (records, entries per tile), and the case families of
test_gpu_beam_ladder.py with the premises that file relies on. Shared by test_cpu_beam_ladder_cases.py
and test_gpu_beam_ladder.py; nothing here touches a GPU.

The rules (csm_joint_kernels.hip: binj_hash_size, binj_lds_bytes; csm_plan.hip: bin_hash_size;
csm_batch.hip / csm_window.hip: joint lists when binj_lds_bytes <= 150 KiB; csm_device.hpp: kJRec,
kMaxPoints, kMaxMult, kTile) are RESTATED, not read from the library: test_cpu_beam_ladder_cases.py holds
the literal rungs they must give, and test_gpu_beam_ladder.py pins the joint / per-slice switch to its
rung through bound_pass_stats()."""
import math

import numpy as np

from csm_hip import synth

import unit_bound_cases as U

K_TILE = 64                     # endpoint tiles of the frame
K_JREC = 256                    # entries per record of a joint list
K_MAX_MULT = 15                 # beams per entry of a merged list
K_MAX_POINTS = 10240            # beams per scan
JOINT_LDS_LIMIT = 150 * 1024    # k_binj's tables must fit: joint lists, else per-slice lists for the whole group
CBX, CBY = 84, 48               # the fine plan's candidate block (columns; rows unless a family says otherwise)


# ---- the size rules ----

def binj_hash_size(n):
    """Slots of k_binj's table for a pair of slices of n beams each: 4/3 of the 2 n beams, in 64s."""
    h = ((8 * n + 2) // 3 + 63) & ~63
    return max(h, 512)


def binj_lds_bytes(tiles, n, hash_size):
    """k_binj's LDS: 20 bytes per tile (an even number of tiles), 12 per slot, 2 per beam of the pair."""
    ntp = (tiles + 1) & ~1
    return 20 * ntp + 12 * hash_size + 2 * (2 * n) + 16


def bin_hash_size(n):
    """Slots of k_bin's table (per-slice lists): a power of two, load <= 2/3, at most 16384."""
    h = 1024
    while 2 * h < 3 * n and h < 16384:
        h <<= 1
    return h


def slot_product_below_2_31(n):
    """k_binj's slot = (18 bits of hash x table size) >> 18: the product stays below 2^31 up to here."""
    return ((1 << 18) - 1) * binj_hash_size(n) < 1 << 31


def joint_lists(tiles, n):
    return binj_lds_bytes(tiles, n, binj_hash_size(n)) <= JOINT_LDS_LIMIT


def _switches(rule):
    """[(last n, first n)] for every n in 1 .. kMaxPoints - 1 at which rule(n) != rule(n + 1)."""
    return [(n, n + 1) for n in range(1, K_MAX_POINTS) if rule(n) != rule(n + 1)]


def rungs(tiles):
    """The ladder on maps of `tiles` endpoint tiles: per threshold, the pairs (last n on this side, first n
    on the other); computed from the rules above."""
    return {
        "binj_slot_product": _switches(slot_product_below_2_31),
        "joint_lists": _switches(lambda n: joint_lists(tiles, n)),
        "bin_hash_size": _switches(bin_hash_size),
        "max_points": [(K_MAX_POINTS, K_MAX_POINTS + 1)],
    }


def ladder(tiles):
    """Every beam count of rungs(tiles) that a scan may have, ascending."""
    return sorted({n for pairs in rungs(tiles).values() for pair in pairs for n in pair if n <= K_MAX_POINTS})


def tiles_of(shape, w):
    """Endpoint tiles of window w's frame on a grid of `shape` (csm_plan.hip: window_frame)."""
    rows, cols = shape
    x_lo, y_lo = -w["wx"], -w["wy"]
    x_hi, y_hi = x_lo + w["nx"] - 1, y_lo + w["ny"] - 1
    return -(-(cols - x_lo + x_hi) // K_TILE) * -(-(rows - y_lo + y_hi + 1) // K_TILE)


# ---- what k_binj makes of a pair of slices ----

def joint_list_stats(window, shape=None, pair=0):
    """The joint list of slices 2 pair, 2 pair + 1 of a window from unit_bound_cases.window_of, as k_binj
    builds it: the frame is (row + y_hi + shift, col + x_hi), shift = (ny - 1) & 1; tiles are 64 x 64; a
    cell of the table is (row pair, column); a cell has ceil(max of its four beam counts (slice x row
    parity) / 15) entries; a tile of e entries has ceil(e / 256) records. Beams outside the frame (below 0;
    past the grid's `shape` where given) are in no list. A premise check for the cases below, not a
    reference for results.

    Returns records (of the pair), tiles (with a beam), max_entries (in one tile), max_records (of one
    tile), max_beams (the greatest of the four counts of any cell)."""
    x_hi, y_hi = -window["wx"] + window["nx"] - 1, -window["wy"] + window["ny"] - 1
    shift = (window["ny"] - 1) & 1
    cells = {}
    for sl, t in enumerate(range(2 * pair, min(2 * pair + 2, window["col"].shape[0]))):
        ry, cx = window["row"][t].astype(np.int64) + y_hi, window["col"][t].astype(np.int64) + x_hi
        ok = (ry >= 0) & (cx >= 0)
        if shape is not None:
            ok &= (ry <= shape[0] - 1 + window["wy"] + y_hi) & (cx <= shape[1] - 1 + window["wx"] + x_hi)
        rr = ry[ok] + shift
        keys, counts = np.unique(np.stack([rr >> 1, cx[ok], rr & 1]), axis=1, return_counts=True)
        for (rp, c, odd), m in zip(keys.T.tolist(), counts.tolist()):
            cells.setdefault((rp, c), [0, 0, 0, 0])[2 * sl + odd] = m
    entries = {}
    for (rp, c), four in cells.items():
        tile = (rp // (K_TILE // 2), c // K_TILE)
        entries[tile] = entries.get(tile, 0) + -(-max(four) // K_MAX_MULT)
    records = {tile: -(-e // K_JREC) for tile, e in entries.items()}
    return dict(records=sum(records.values()), tiles=len(entries), max_entries=max(entries.values(), default=0),
                max_records=max(records.values(), default=0),
                max_beams=max((max(four) for four in cells.values()), default=0))


# ---- case families ----

class Family:
    """Windows of one shape: make(seed, n_beams) -> case, the window (half ranges, L), the rows of a
    candidate block as the fine plan cuts this window, and the seeds / beam counts the GPU test runs."""

    def __init__(self, name, make, seeds, beams, rx, ry, rt, Lr=4, cby=CBY):
        self.name, self.make, self.seeds, self.beams = name, make, tuple(seeds), tuple(beams)
        self.rx, self.ry, self.rt, self.Lr, self.cby = rx, ry, rt, Lr, cby
        self._cases, self._premises = {}, {}

    def case(self, seed, n):
        if (seed, n) not in self._cases:
            self._cases[seed, n] = self.make(seed, n)
        return self._cases[seed, n]

    def premises(self, oracle, seed, n, score_thr=0.0, known_thr=0.0):
        """select_rounds' restatement of the coarse-first chain plus joint_list_stats of pair 0 and the
        endpoint tiles of the frame, computed once per (seed, beams, thresholds)."""
        key = (seed, n, score_thr, known_thr)
        if key not in self._premises:
            case = self.case(seed, n)
            sel = U.select_rounds(case, oracle, self.rx, self.ry, self.rt, self.Lr, CBX, self.cby, score_thr, known_thr)
            sel["lists"] = joint_list_stats(sel["window"], case["grid"].shape)
            sel["tiles"] = tiles_of(case["grid"].shape, sel["window"])
            self._premises[key] = sel
        return self._premises[key]


def _small(seed, n, init_error=(0.06, -0.04, 0.05)):
    """_small of test_gpu_coarse_first.py (a scan of the room's middle, +-4 x +-4 candidates) at n beams"""
    return synth.csm_case(seed, rows=96, cols=96, n_beams=n, max_range=1.2, init_error=init_error)


def _tall(seed, n):
    """_tall of test_gpu_coarse_first.py (+-4 x +-41 candidates, the sensor high in the map) at n beams"""
    return synth.csm_case(seed, rows=96, cols=96, n_beams=n, max_range=1.0, init_error=(0.06, -0.04, 0.05),
                          truth=(0.05, 1.3, 0.2))


def _wide(seed, n):
    """A 270 deg scan over 5 m in a 256 x 256 map: the pair's beams end in more than 8 tiles"""
    return synth.csm_case(seed, rows=256, cols=256, n_beams=n, max_range=5.0, fov=1.5 * math.pi,
                          init_error=(0.06, -0.04, 0.02))


def _noisy(seed, n, sigma=0.07):
    """A room scan over 3 m in a 192 x 192 map whose ranges carry Gaussian noise of 7 cm: the walls smear
    over several cells and one endpoint tile of the pair holds more than kJRec entries, yet the scan still
    matches its room well enough for the level to leave units out (scattered returns match nothing: every
    unit would be scored)."""
    c = synth.csm_case(seed, rows=192, cols=192, n_beams=n, max_range=3.0, init_error=(0.06, -0.04, 0.02))
    r = np.clip(c["ranges"] + sigma * np.random.RandomState(seed).randn(n), 0.2, 3.0)
    r[int(np.argmax(c["ranges"]))] = 3.0          # the longest beam sets the angular step
    c["ranges"] = r
    return c


def _small_far(seed, n):
    """_small started too far off: nothing in its window reaches the score threshold"""
    return _small(seed, n, init_error=(0.3, 0.3, 0.5))


def _reach(seed, n, init_error=(0.03, -0.02, 0.03)):
    """The queries of test_gpu_coarse_first.py's thresholded batch (1.6 m: the scan reaches the walls and
    passes LoopDetectorCorrelative's thresholds) at n beams"""
    return synth.csm_case(seed, rows=96, cols=96, n_beams=n, max_range=1.6, init_error=init_error)


def _reach_far(seed, n):
    return _reach(seed, n, init_error=(0.3, 0.3, 0.5))


RT80 = math.radians(80)
RUNG_BEAMS = (3072, 3073, 4248, 4249)          # both sides of the slot-product rung and of the joint-list rung
FAMILIES = {f.name: f for f in (
    Family("rungs_small", _small, (21, 25), RUNG_BEAMS, 0.4, 0.4, RT80),
    Family("rungs_tall", _tall, (21, 23), RUNG_BEAMS, 0.4, 4.1, RT80, cby=42),
    Family("many_records", _wide, (70, 75), (1080,), 0.4, 0.4, math.radians(20)),
    Family("split_tile", _noisy, (404, 411), (4248,), 0.4, 0.4, math.radians(30)),
    # the thresholded batches: queries that cannot be found at all, and queries of which some are found
    Family("rungs_small_far", _small_far, (27,), (3073, 4248), 0.4, 0.4, RT80),
    Family("rungs_reach", _reach, (50, 51, 52), (3073, 4248), 0.4, 0.4, math.radians(60)),
    Family("rungs_reach_far", _reach_far, (55,), (3073, 4248), 0.4, 0.4, math.radians(60)),
)}


# ---- the window every chain scores candidate by candidate ----

PAIR_RX, PAIR_RY, PAIR_RT, PAIR_L = 0.45, 4.05, math.radians(0.3), 4      # test_gpu_pair_window.py's 3 x 12 x 84 window
PAIR_SHAPE = (3, 12, 84)


def pair_window_case(n, saturated):
    """The window of test_gpu_pair_window.py (200 x 200 map, beams of at most 1.2 m) cast with n beams, on
    the room's grid or on a grid of 65535 throughout."""
    case = synth.csm_case(17, rows=200, cols=200, n_beams=n, max_range=1.2)
    if saturated:
        case["grid"] = np.full_like(case["grid"], 65535)
    return case


# ---- near ties at the joint limit ----

TIE_RX, TIE_RY, TIE_RT, TIE_L = 4.0, 2.6, math.radians(6), 4
TIE_BEAMS = 4248


def near_tie_case(kind):
    """The `checker` and `noise` landscapes of test_gpu_bound_pass.py::test_near_tie_landscapes under a scan
    of 4248 beams of at most 2.5 m (no candidate brings a beam to the map's edge: no edge band), on a 200 x 200
    map (20 endpoint tiles: the joint lists still fit) and a window of 7 slices x 84 x 56 candidates. 84 columns
    are the widest candidate block, which is 48 rows high at most: 4 pairs of slices x 2 row blocks = 8 units,
    below the 16 from which the batch would score the level first, so the packed-fp32 bound pass runs, with the
    widest slack it has."""
    seed = {"checker": 42, "noise": 43}[kind]
    case = synth.csm_case(seed, rows=200, cols=200, n_beams=TIE_BEAMS, max_range=2.5)
    rr, cc = np.indices(case["grid"].shape)
    if kind == "checker":
        case["grid"] = np.where((rr + cc) & 1, 40000, 40001).astype(np.uint16)
    else:
        case["grid"] = (50000 + np.random.RandomState(seed).randint(-2, 3, case["grid"].shape)).astype(np.uint16)
    return case
