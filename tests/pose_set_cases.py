"""Case builders of the pose sets' second round (tests/test_cpu_pose_sets_cases.py proves their conditions
without a GPU, tests/test_gpu_pose_sets_edges.py runs them on the device). Plain numpy: no GPU and no library
call in here.

Cell picking. Geometry (2^-4, -2, -1.5), a 48 x 64 map, every pose at a cell centre with theta = 0 exactly,
every beam at angle 0.0 exactly with range m 2^-4: cos 0 = 1 and sin 0 = 0 on host and device alike, so beam m
of the pose at cell (row, col) hits cell (row, col + m) by exact dyadic arithmetic, half a cell from every
edge (the certificate's margin there is about 1e-11 of a cell: no such pose is marked). A test asks for a run
of cell values per pose, the builder writes the runs into the grid and puts the poses on them, and the
expected (S, K) is read from the wanted runs, with no projection code in between. Poses that ask for the same
run share its cells: exact ties.

Forced marks. A pose whose x is exactly col 2^-4 - 2 under a scan whose first range is 0.0 has hx = x and an
integral cell coordinate, whatever its heading and the other beams: the certificate must mark it, the host
projects it and k_pose_rescore scores it.

Generic sets come from the seeds of pose_set_reference (make_scan, make_poses), with the frame, the heading
range, the angle scale and the resolution as parameters."""
import numpy as np

import pose_set_reference as R

RES = 2.0 ** -4
G = (RES, -2.0, -1.5)
ROWS, COLS = 48, 64
MAX_POSES = 1 << 18


def cell_picking(runs, seed=0):
    """runs: (n_poses, n_beams) wanted cell values, or (n_poses,) for one beam of range 0. Distinct runs get
    distinct slots of n_beams cells of one row, in a seeded order (neighbouring slots hold unrelated values);
    cells no run uses stay 0. Returns the case with its expected S and K."""
    runs = np.asarray(runs, dtype=np.int64)
    runs = runs.reshape(-1, 1) if runs.ndim == 1 else runs
    n, nb = runs.shape
    assert 1 <= nb <= COLS and runs.min() >= 0 and runs.max() <= 65535
    uniq, inv = np.unique(runs, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    per_row = COLS // nb
    assert len(uniq) <= ROWS * per_row, "more distinct runs than the map has slots"
    slot = np.random.RandomState(4000 + seed).permutation(ROWS * per_row)[:len(uniq)]
    srow, scol = slot // per_row, (slot % per_row) * nb
    grid = np.zeros((ROWS, COLS), np.uint16)
    for m in range(nb):
        grid[srow, scol + m] = uniq[:, m]
    poses = np.stack([(scol[inv] + 0.5) * RES - 2.0, (srow[inv] + 0.5) * RES - 1.5, np.zeros(n)], axis=1)
    return dict(geom=G, grid=grid, angles=np.zeros(nb), ranges=np.arange(nb) * RES, poses=poses,
                S=runs.sum(axis=1), K=(runs != 0).sum(axis=1), n_points=nb)


def force(poses, indices):
    """A copy of `poses` (geometry G) with x of the listed poses moved onto the nearest cell edge."""
    p = np.array(poses, dtype=np.float64).reshape(-1, 3)
    idx = np.asarray(indices, dtype=np.int64)
    p[idx, 0] = np.round((p[idx, 0] + 2.0) / RES) * RES - 2.0
    return p


def forced_scan(seed, n_points, r_lo=0.2, r_hi=1.5):
    angles, ranges = R.make_scan(seed, n_points, r_lo, r_hi)
    ranges[0] = 0.0
    return angles, ranges


def generic(seed, n_points, n_poses, geom=R.GEOM, theta_half=np.pi, angle_scale=1.0, scale=1.0, shape=(R.ROWS, R.COLS)):
    """A generic set around the centre of a `shape` map in frame `geom`: headings uniform in +-theta_half, beam
    angles times angle_scale, lengths (pose spread, ranges) times `scale` (the resolution over 0.05)."""
    res, off_x, off_y = geom
    centre = (off_x + 0.5 * shape[1] * res, off_y + 0.5 * shape[0] * res)
    angles, ranges = R.make_scan(seed, n_points)
    poses = R.make_poses(seed, n_poses, 1.0 * scale, 0.8 * scale, centre=centre)
    poses[:, 2] *= theta_half / np.pi
    return dict(geom=geom, angles=angles * angle_scale, ranges=ranges * scale, poses=poses)


# ---- rescore ----

MANY_FIXES = (0, 1, 7, 8, 9, 10, 11, 12, 13, 40, 41, 63, 64, 65, 128, 150, 191, 192, 255, 256, 257, 298, 299)


def many_fixes_case():
    """65 beams x 300 poses, 23 forced: 0 and 299, neighbours, seven in a row (with four wavefronts to a
    workgroup of k_pose_rescore: six workgroups, the last with three fixes)."""
    angles, ranges = forced_scan(41, 65)
    assert len(MANY_FIXES) == 23
    return dict(geom=G, grid=R.make_map(41), angles=angles, ranges=ranges,
                poses=force(R.make_poses(41, 300), MANY_FIXES), forced=MANY_FIXES)


def three_sets_case():
    """Sets of 65, 1100, 65 (the first scan again) and 3 beams on two maps, empty sets between them, forced
    poses in each: fixes of one batch with different n_points, so hit_at is not a multiple of anything."""
    grids = [R.make_map(42), R.make_map(43, 40, 72)]
    a65, r65 = forced_scan(42, 65)
    a1100, r1100 = forced_scan(43, 1100, 0.2, 1.2)
    a3, r3 = forced_scan(44, 3)
    plan = [(0, a65, r65, 70, (0, 33, 69)), (1, a3, r3, 0, ()), (1, a1100, r1100, 9, (2, 3, 8)),
            (0, a65, r65, 0, ()), (1, a65, r65, 130, (1, 64, 129)), (0, a3, r3, 5, (0, 4))]
    sets = []
    for k, (m, a, r, n, forced) in enumerate(plan):
        poses = force(R.make_poses(50 + k, n, 0.9, 0.7), forced) if n else np.zeros((0, 3))
        sets.append(dict(map=m, geom=G, angles=a, ranges=r, poses=poses, forced=forced))
    return grids, sets


def two_batches_case():
    """65536 beams x 129 poses, all forced: 129 x 2 x 65536 x 4 B of indices is one 512 KiB over the 64 MiB a
    batch of k_pose_rescore stages, so 128 + 1. Ranges in [0, 1], the first 0: every beam stays inside."""
    angles, ranges = forced_scan(45, 65536, 0.0, 1.0)
    return dict(geom=G, grid=R.make_map(45), angles=angles, ranges=ranges,
                poses=force(R.make_poses(45, 129, 0.5, 0.3), range(129)), forced=tuple(range(129)))


# ---- weights and resampling: cell picking, one beam of range 0 unless said ----

TILE_SHAPES = (1023, 1024, 1025, 2049, 3073, 5000)


def tile_shape_case(n):
    """n poses over 1200 distinct values. At temperature 0.3 every weight is above 2^24 e^-3.4, so the prefix
    sums pass 2^32 within the first tile (by design, not by accident)."""
    rng = np.random.RandomState(6000 + n)
    pool = rng.choice(65536, 1200, replace=False)
    return cell_picking(rng.choice(pool, n), seed=n)


TIE_N = 3073
TIE_FIRST = (0, 63, 64, 1023, 1024, 2048, TIE_N - 1)


def tie_case(first):
    """Two values only. The greater one is held by pose `first`, by every 61st pose after it and by the last
    pose: holders in different wavefronts and tiles, the first of them the answer (alone when it is the last)."""
    vals = np.full(TIE_N, 20000)
    vals[first::61] = 60000
    vals[TIE_N - 1] = 60000
    return cell_picking(vals, seed=first)


ZERO_N = 3300
ZERO_LAYOUTS = dict(
    runs=(0, 1, 63, 128, 1000, 1023, 2048, 2049, ZERO_N - 1),     # poses 64..127 and 1024..2047 weigh nothing
    last=(ZERO_N - 1,),
    first=(0,),
)
ZERO_TEMPERATURE = 2e-4


def zero_runs_case(layout):
    """Value 1 everywhere (known, eligible, 65534 values = 3.3e7 keys below the top: far outside the table at
    temperature 2e-4), 65535 and 65435 in turn on the listed poses (key differences 0 and 49900: weights
    2^24 and about 8e3)."""
    vals = np.full(ZERO_N, 1)
    weighted = np.array(ZERO_LAYOUTS[layout])
    vals[weighted] = np.where(np.arange(weighted.size) % 2 == 0, 65535, 65435)
    c = cell_picking(vals, seed=len(layout))
    c["weighted"] = weighted
    return c


ELIGIBILITY_THRESHOLDS = ((0.0, 1), (0.5, 5), (0.875, 8), (1.0, 9))       # (threshold, min_known of 8 beams)


def eligibility_case():
    """8 beams, 45 poses with K = 0 .. 8 in turn. Poses with K = 4 sit on cells of 65535 (key 4 x 32268 +
    499 x 262140, the greatest by far), the others on small values: from min_known = 5 on, the greatest key
    belongs to an ineligible pose."""
    rng = np.random.RandomState(6100)
    runs = np.zeros((45, 8), np.int64)
    for i in range(45):
        k = i % 9
        at = rng.permutation(8)[:k]
        runs[i, at] = 65535 if k == 4 else rng.randint(50, 400, k)
    return cell_picking(runs, seed=8)


def limit_case(unique_last):
    """2^18 poses on one cell (all weights 2^24, m0 = 2^42); with unique_last the last pose on a greater one."""
    vals = np.full(MAX_POSES, 30000)
    if unique_last:
        vals[-1] = 30001
    return cell_picking(vals, seed=18)


# ---- accumulator limits ----

FULL_S, FULL_K = 65536 * 65535, 65536
ACC_TEMPERATURE = 2e-4                # bins of 2^23 keys at 65536 beams: one hit of the lowered cell is 3.3e7 keys
LOWERED = (24, 58)                    # a cell only the seventh pose reaches (x >= 1.625: the six stay below 1.5)


def accumulator_case():
    """A map of 65535 everywhere under 65536 beams with ranges in [0, 1]: six generic poses within 0.5 / 0.3 m
    of the centre have every beam inside, S = 0xFFFF0000. grid_low has cell LOWERED set to 1 and a seventh pose
    0.65 m to its left, whose beams reach it."""
    angles, ranges = R.make_scan(46, 65536, 0.0, 1.0)
    poses = R.make_poses(46, 6, 0.5, 0.3)
    grid = np.full((ROWS, COLS), 65535, np.uint16)
    low = grid.copy()
    low[LOWERED] = 1
    seventh = np.array([[0.97875, 0.02, 0.7]])
    return dict(geom=G, grid=grid, grid_low=low, angles=angles, ranges=ranges, poses=poses,
                poses7=np.concatenate([poses, seventh]))


# ---- frames and headings ----

def _centred(res):
    return (res, -0.5 * R.COLS * res, -0.5 * R.ROWS * res)


def frame_cases():
    """name -> generic case with its grid, for 65 and 360 beams x 257 poses."""
    out = {}
    for nb in (65, 360):
        seed = 700 + nb
        variants = dict(
            theta_1e2=dict(theta_half=1e2),
            theta_1e4=dict(theta_half=1e4),
            angles_x40=dict(angle_scale=40.0),
            far_1e4=dict(geom=(0.05, 1e4, -1e4)),
            far_odd=dict(geom=(0.05, -3333.3, 7777.7)),
            res_0p1=dict(geom=_centred(0.1), scale=2.0),
            res_0p03=dict(geom=_centred(0.03), scale=0.6),
            res_third=dict(geom=_centred(1.0 / 3.0), scale=(1.0 / 3.0) / 0.05),
        )
        for k, (name, kw) in enumerate(variants.items()):
            c = generic(seed + k, nb, 257, **kw)
            c["grid"] = R.make_map(seed + k)
            out["%s_%d" % (name, nb)] = c
        c = generic(seed + 20, nb, 257)
        c["ranges"][::7] = 0.0
        c["ranges"][3::11] *= -1.0
        c["grid"] = R.make_map(seed + 20)
        out["zero_negative_%d" % nb] = c
    return out


# ---- set layout ----

LAYOUTS = {8: (0, 5003, 0, 1, 11400, 7, 0), 16: (9001, 0, 23800, 3)}


def layout_case(group_poses):
    """Sets of the listed sizes over two maps (the second in a frame of its own) and scans of 3 to 5 beams, the
    first scan used by every third set. group_poses is what the call's total makes the host choose:
    min(16, max(4, total / 2048)) rounded down to a multiple of 4."""
    sizes = LAYOUTS[group_poses]
    total = sum(sizes)
    assert min(16, max(4, total // 2048)) // 4 * 4 == group_poses
    grids = [R.make_map(47), R.make_map(48, 40, 72)]
    geoms = [R.GEOM, (0.04, -1.3, -0.9)]
    scans = [R.make_scan(47 + j, 3 + j) for j in range(3)]
    sets = []
    for k, n in enumerate(sizes):
        a, r = scans[k % 3]
        m = k % 2
        half = (1.0, 0.8) if m == 0 else (0.9, 0.5)
        centre = (0.0, 0.0) if m == 0 else (-1.3 + 0.5 * 72 * 0.04, -0.9 + 0.5 * 40 * 0.04)
        poses = R.make_poses(80 + 10 * group_poses + k, n, *half, centre=centre) if n else np.zeros((0, 3))
        sets.append(dict(map=m, geom=geoms[m], angles=a, ranges=r, poses=poses))
    return grids, sets
