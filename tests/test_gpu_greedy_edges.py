"""The greedy-endpoint cost / covariance batch and the hill-climbing matcher on the device
(csm_greedy_cost_covariance_batch, csm_hill_climbing_batch) where test_gpu_hill_climbing.py does not
look: every setting of tests/test_cpu_greedy.py's CASES (kernel sizes up to 8, thresholds on and past
the table's values, denormal and -0.0 tables, zero / negative / overflowing scaling), kernel windows
across every map edge, beam counts around the wave, the workgroup and the LDS-to-scratch switch, the
host fallback of uncertified queries, and maps with unallocated blocks. Every result is compared with
`==` (covariances with np.array_equal) against the Python literal (tests/greedy_literal.py) or, where
that would be slow, against the host restatement, which test_cpu_greedy.py pins to the literal at
the same settings. Each call runs in a default context and in one with literal sums only
(TUNE_GREEDY_LITERAL_SUMS); the two agree bit for bit. Measured: the file takes about ten seconds on
one MI355X, nearly all of it in the Python literal and the host restatement."""
import math

import numpy as np
import pytest

import cost_edge_cases as CE
import greedy_edge_cases as GE
import greedy_literal as GL
from csm_hip import _lib as L
from csm_hip import api, synth
from greedy_edge_cases import CASES

pytestmark = pytest.mark.gpu

FIELDS = ("normalized_initial_cost", "normalized_cost", "sensor_pose", "best_sensor_pose", "estimated_pose",
          "iterations", "refinements", "diff_translation", "diff_rotation")


@pytest.fixture(scope="module")
def ctxs(gpu_ctx):
    lit = api.Context(0, tuning_off=L.TUNE_GREEDY_LITERAL_SUMS)
    yield gpu_ctx, lit
    lit.close()


def _bits(r):
    v = [r["normalized_initial_cost"], r["normalized_cost"], r["diff_translation"], r["diff_rotation"]]
    v += r["sensor_pose"] + r["best_sensor_pose"] + r["estimated_pose"] + list(np.ravel(r["covariance"]))
    return np.array(v, np.float64).tobytes(), (r["iterations"], r["refinements"], r["host_path"])


def _same_as(got, want, where=""):
    for key in FIELDS:
        assert got[key] == want[key], (where, key, got[key], want[key])
    assert np.array_equal(got["covariance"], want["covariance"], equal_nan=True), \
        (where, got["covariance"], want["covariance"])


def _upload(ctxs, map_id, grid):
    for ctx in ctxs:
        ctx.upload_grid(map_id, grid)


def _release(ctxs, map_ids):
    for ctx in ctxs:
        for m in map_ids:
            if ctx.has_grid(m):
                ctx.release_grid(m)


def _hill(ctxs, qs, hc, prm):
    """hill_climbing_batch in both contexts: bit-identical results; in the literal-sums context every
    device query replays each decision. Returns the default context's results."""
    a, b = (ctx.hill_climbing_batch(qs, *hc, greedy=prm) for ctx in ctxs)
    for i, (x, y) in enumerate(zip(a, b)):
        assert _bits(x) == _bits(y), i
        if not y["host_path"]:
            assert y["replays"] == y["iterations"] + (y["iterations"] < hc[2]), (i, y)
    return a


def _cost(ctxs, qs, poses, prm):
    a, b = (ctx.greedy_cost_covariance_batch(qs, np.asarray(poses, np.float64), greedy=prm) for ctx in ctxs)
    for i, (x, y) in enumerate(zip(a, b)):
        assert _bits(x) == _bits(y), i
    return a


def _want_hill(q, hc, prm, literal=True, alloc=None):
    if literal:
        return GL.optimize_pose(q["grid"], q["geom"], q["angles"], q["ranges"], q["rel_pose"], q["init_pose"],
                                *hc, prm, alloc=alloc)
    return api.host_hill_climbing(q["grid"], q["geom"], q["angles"], q["ranges"], q["rel_pose"], q["init_pose"],
                                  *hc, greedy=prm)


def _check_cost(got, q, pose, prm, literal=True, alloc=None, where=""):
    n = len(q["angles"])
    if literal:
        lit = GL.Greedy(**prm)
        c = lit.cost(q["grid"], q["geom"], q["angles"], q["ranges"], tuple(pose), alloc)
        cov = lit.covariance(q["grid"], q["geom"], q["angles"], q["ranges"], tuple(pose), alloc)
    else:
        c, cov = api.host_greedy_cost(q["grid"], q["geom"], q["angles"], q["ranges"], pose, prm, covariance=True)
    assert got["normalized_cost"] == c / n and got["normalized_initial_cost"] == c / n, (where, got, c / n)
    assert got["best_sensor_pose"] == list(pose), where
    assert np.array_equal(got["covariance"], cov, equal_nan=True), (where, got["covariance"], cov)


# ---------------------------------------------------------------- 1. settings sweep


@pytest.mark.parametrize("seed,greedy,hc,opts", CASES)
def test_settings_sweep_equals_literal(ctxs, seed, greedy, hc, opts):
    grid, c, init = GE.case(seed, **opts)
    prm = GE.settings(greedy)
    mid = 91000 + seed
    _upload(ctxs, mid, grid)
    q = dict(map_id=mid, geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
             init_pose=init, grid=grid)
    sensor = api.host_compound(init, c["rel_pose"])
    poses = [sensor, sensor + (0.021, -0.013, 0.007)]
    try:
        got = _hill(ctxs, [q], hc, prm)[0]
        cost = _cost(ctxs, [q, q], poses, prm)
    finally:
        _release(ctxs, [mid])
    assert got["host_path"] == 0 and all(r["host_path"] == 0 for r in cost)
    _same_as(got, _want_hill(q, hc, prm), seed)
    for p, r in zip(poses, cost):
        _check_cost(r, q, p, prm, where=seed)
    if seed == 36:
        assert got["normalized_cost"] == -math.inf and np.isnan(got["covariance"]).any()


# ---------------------------------------------------------------- 2. map edges


EDGE_MAPS = {
    # rows, cols (pitch != cols / pitch == cols), resolution, offset shift (m)
    "ragged_203x317": (203, 317, 0.05, (0.0, 0.0)),
    "wide_96x152_coarse": (96, 152, 0.1, (0.0377, -0.0519)),
}


@pytest.mark.parametrize("k", [0, 1, 3, 8])
@pytest.mark.parametrize("name", list(EDGE_MAPS))
def test_kernel_windows_across_every_edge(ctxs, name, k):
    rows, cols, res, shift = EDGE_MAPS[name]
    grid, geom, _ = synth.make_room(60 + list(EDGE_MAPS).index(name), rows, cols, res)
    grid = GE.ringed(grid, rows)
    geom = (geom[0], geom[1] + shift[0], geom[2] + shift[1])
    prm = GE.settings(dict(kernel_size=k))
    ext_x, ext_y = cols * res, rows * res
    reach = 0.8 * max(ext_x, ext_y)
    spots = [(fx, fy) for fx in (0.03, 0.5, 0.97) for fy in (0.03, 0.5, 0.97)] + \
            [(-0.1, 0.5), (1.1, 0.5), (0.5, -0.1), (0.5, 1.1), (-0.1, -0.1), (1.1, 1.1), (1.1, -0.1), (-0.1, 1.1)]
    rng = np.random.RandomState(rows + cols + k)
    mid = 92000 + 10 * list(EDGE_MAPS).index(name) + k
    qs, poses = [], []
    seen = {kind: dict(left=0, right=0, below=0, above=0) for kind in ("hit", "missed")}
    for i, (fx, fy) in enumerate(spots):
        pose = (geom[1] + fx * ext_x, geom[2] + fy * ext_y, 0.3 * i)
        angles = np.linspace(-math.pi, math.pi, 360, endpoint=False)
        ranges = rng.uniform(0.05, reach, angles.size)
        qs.append(dict(map_id=mid, geom=geom, angles=angles, ranges=ranges, rel_pose=(0.0, 0.0, 0.0),
                       init_pose=pose, grid=grid))
        poses.append(pose)
        for kind, sides in GE.straddles(geom, grid.shape, pose, angles, ranges, max(k, 1),
                                        prm["hit_and_missed_dist"]).items():
            for side, v in sides.items():
                seen[kind][side] += v
    # kernel windows of hit and of missed points lie across each of the four edges
    assert all(v > 0 for sides in seen.values() for v in sides.values()), seen
    hc = (0.05, 0.05, 5, 1)
    _upload(ctxs, mid, grid)
    try:
        got = _hill(ctxs, qs, hc, prm)
        cost = _cost(ctxs, qs, poses, prm)
    finally:
        _release(ctxs, [mid])
    literal = k <= 3
    for i, q in enumerate(qs):
        assert got[i]["host_path"] == 0 and cost[i]["host_path"] == 0
        _same_as(got[i], _want_hill(q, hc, prm, literal), (name, k, i))
        _check_cost(cost[i], q, poses[i], prm, literal, where=(name, k, i))


# ---------------------------------------------------------------- 3. beam counts


_BEAM_CASES = {}


def _beam_query(n, map_id, seed=0):
    key = (n, seed)
    if key not in _BEAM_CASES:
        c = synth.csm_case(4000 + seed + n % 89, rows=240, cols=260, n_beams=n, fov=1.5 * math.pi,
                           max_range=5.0, rel_pose=(0.03, -0.01, 0.005))
        init = tuple(np.asarray(c["truth"]) + (0.06, -0.05, 0.02))
        _BEAM_CASES[key] = dict(geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
                                init_pose=init, grid=c["grid"])
    return dict(_BEAM_CASES[key], map_id=map_id)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 10240])
def test_beam_counts_around_wave_workgroup_and_scratch(ctxs, n, k):
    prm = GE.settings(dict(kernel_size=k))
    hc = (0.1, 0.1, 100, 5)
    mid = 93000 + n
    q = _beam_query(n, mid)
    _upload(ctxs, mid, q["grid"])
    sensor = api.host_compound(q["init_pose"], q["rel_pose"])
    try:
        got = _hill(ctxs, [q], hc, prm)[0]
        cost = _cost(ctxs, [q], [sensor], prm)[0]
    finally:
        _release(ctxs, [mid])
    literal = n <= 257
    assert got["host_path"] == 0 and cost["host_path"] == 0
    _same_as(got, _want_hill(q, hc, prm, literal), (n, k))
    _check_cost(cost, q, sensor, prm, literal, where=(n, k))


def test_more_than_10240_beams_is_einval(ctxs):
    q = _beam_query(10241, 93100)
    _upload(ctxs, 93100, q["grid"])
    try:
        for ctx in ctxs:
            for call in (lambda: ctx.hill_climbing_batch([q]),
                         lambda: ctx.greedy_cost_covariance_batch([q], np.zeros(3))):
                with pytest.raises(api.CsmError) as e:
                    call()
                assert e.value.code == L.CSM_EINVAL
    finally:
        _release(ctxs, [93100])


MIXED_BEAMS = [64, 4097, 300, 5003, 1, 10240, 700, 4096, 2000, 4097, 257]


def _mixed_batch():
    """Queries of MIXED_BEAMS beams over three maps (ids 93200-93202); returns (queries, grids)."""
    rng = np.random.RandomState(12)
    maps = [synth.csm_case(4100 + m, rows=240, cols=260, n_beams=8, max_range=5.0) for m in range(3)]
    qs = []
    for i, n in enumerate(MIXED_BEAMS):
        m = maps[i % 3]
        angles, ranges = synth.cast_scan(m["segs"], m["truth"], n, 1.5 * math.pi, 5.0)
        init = tuple(np.asarray(m["truth"]) + rng.uniform(-0.1, 0.1, 3) * (1, 1, 0.3))
        qs.append(dict(map_id=93200 + i % 3, geom=m["geom"], angles=angles, ranges=ranges,
                       rel_pose=(0.03, 0.0, 0.0), init_pose=init, grid=m["grid"]))
    return qs, [m["grid"] for m in maps]


@pytest.mark.parametrize("k", [1, 3])
def test_mixed_lds_and_scratch_batch(ctxs, k):
    """LDS-sized and scratch-sized scans (4097, 5003, 10240: scratch strides that are and are not
    multiples of 16, at per-query offsets) in one batch over three maps: each result equals the same
    query run alone and the host restatement."""
    prm = GE.settings(dict(kernel_size=k))
    hc = (0.1, 0.1, 100, 5)
    qs, grids = _mixed_batch()
    for m in range(3):
        _upload(ctxs, 93200 + m, grids[m])
    try:
        poses = [api.host_compound(q["init_pose"], q["rel_pose"]) for q in qs]
        got = _hill(ctxs, qs, hc, prm)
        cost = _cost(ctxs, qs, poses, prm)
        alone = [_hill(ctxs, [q], hc, prm)[0] for q in qs]
        alone_cost = [_cost(ctxs, [q], [p], prm)[0] for q, p in zip(qs, poses)]
    finally:
        _release(ctxs, [93200, 93201, 93202])
    for i, q in enumerate(qs):
        assert got[i]["host_path"] == 0
        assert _bits(got[i]) == _bits(alone[i]) and _bits(cost[i]) == _bits(alone_cost[i]), i
        _same_as(got[i], _want_hill(q, hc, prm, literal=False), i)
        _check_cost(cost[i], q, poses[i], prm, literal=False, where=i)


# ---------------------------------------------------------------- 4. host fallback


def test_uncertified_queries_take_the_host_path(ctxs):
    """(a) a hit coordinate exactly on a cell edge at the start pose; (b) a certified start whose first
    +x candidate puts one there (the search breaks mid-way); both in one batch with device queries,
    on a shared map and on maps of their own, with a scan over 4096 beams among them."""
    grid, geom, segs = GE.edge_map(61)
    grid2, _, segs2 = GE.edge_map(62)
    hc = (GE.EDGE_STEP, 0.05, 10, 2)
    prm = GE.settings({})
    a_pose, b_pose = GE.start_on_edge(), GE.first_move_on_edge()
    rng = np.random.RandomState(6)

    def query(mid, g, pose, n, edge):
        room = segs2 if g is grid2 else segs
        if edge:
            angles, ranges = GE.edge_scan(room, pose, n)
        else:
            angles, ranges = synth.cast_scan(room, pose, n, 1.5 * math.pi, 5.0)
        return dict(map_id=mid, geom=geom, angles=angles, ranges=ranges, rel_pose=(0.0, 0.0, 0.0), init_pose=pose,
                    grid=g)

    def device_pose():
        return (1.0 + rng.uniform(-0.3, 0.3), 0.2 + rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2))

    qs = [query(94000, grid, device_pose(), 360, False), query(94000, grid, a_pose, 360, True),
          query(94000, grid, device_pose(), 4500, False), query(94000, grid, b_pose, 720, True),
          query(94001, grid, a_pose, 1080, True), query(94002, grid2, b_pose, 360, True),
          query(94002, grid2, device_pose(), 1080, False)]
    intended = [0, 1, 0, 1, 1, 1, 0]
    _upload(ctxs, 94000, grid)
    _upload(ctxs, 94001, grid)
    _upload(ctxs, 94002, grid2)
    try:
        got = _hill(ctxs, qs, hc, prm)
        alone = [_hill(ctxs, [q], hc, prm)[0] for q in qs[1:4:2]]
        poses = [q["init_pose"] for q in qs]
        cost = _cost(ctxs, qs, poses, prm)
    finally:
        _release(ctxs, [94000, 94001, 94002])
    assert [g["host_path"] for g in got] == intended
    assert [g["host_path"] for g in alone] == [1, 1]
    # the cost batch evaluates the start and its +-res neighbours only: (a) alone is uncertified
    assert [c["host_path"] for c in cost] == [0, 1, 0, 0, 1, 0, 0]
    for i, q in enumerate(qs):
        _same_as(got[i], _want_hill(q, hc, prm), i)
        _check_cost(cost[i], q, poses[i], prm, where=i)


# ---------------------------------------------------------------- 5. both decision forms


def test_interval_and_replayed_decisions_both_occur(ctxs):
    """The default context decides from interval bounds where they are apart (replays == 0 after
    iterations) and replays the literal sums where they are not: both happen on the sweep, edge and
    beam-count inputs above (their parity is checked there)."""
    trusted = replayed = 0
    results = []
    for seed, greedy, hc, opts in CASES:
        grid, c, init = GE.case(seed, **opts)
        ctxs[0].upload_grid(95000, grid)
        q = dict(map_id=95000, geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
                 init_pose=init)
        results.append(ctxs[0].hill_climbing_batch([q], *hc, greedy=GE.settings(greedy))[0])
    ctxs[0].release_grid(95000)
    qs, grids = _mixed_batch()
    for m in range(3):
        ctxs[0].upload_grid(93200 + m, grids[m])
    try:
        results += ctxs[0].hill_climbing_batch(qs, greedy=GE.settings({}))
    finally:
        _release(ctxs[:1], [93200, 93201, 93202])
    for r in results:
        assert r["host_path"] == 0
        trusted += r["iterations"] > 0 and r["replays"] == 0
        replayed += r["replays"] > 0
    assert trusted > 0 and replayed > 0, (trusted, replayed)


# ---------------------------------------------------------------- 6. maps with allocation


@pytest.mark.parametrize("log2_block", [3, 4, 5])
def test_missing_blocks_read_zero(ctxs, log2_block):
    """csm_upload_grid_blocks with blocks left out, known cells in them included: the device reads 0
    there, as the literal does with the bitmap (and the cells kept)."""
    bs = 1 << log2_block
    br, bc = -(-200 // bs), -(-240 // bs)
    c = synth.csm_case(4600 + log2_block, rows=br * bs, cols=bc * bs, n_beams=720, fov=1.5 * math.pi,
                       max_range=5.0)
    grid = c["grid"]
    rng = np.random.RandomState(log2_block)
    mask = (rng.rand(br, bc) < 0.7).astype(np.uint8)
    blocks = [grid[r * bs:(r + 1) * bs, k * bs:(k + 1) * bs].copy() if mask[r, k] else None
              for r in range(br) for k in range(bc)]
    dropped = np.kron(mask, np.ones((bs, bs), np.uint8)) == 0
    assert grid[dropped].any()                     # known cells left out with their blocks
    mid = 96000 + log2_block
    for ctx in ctxs:
        ctx.upload_grid_blocks(mid, blocks, br, bc, log2_block)
    hc = (0.05, 0.05, 20, 2)
    qs = [dict(map_id=mid, geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
               init_pose=tuple(np.asarray(c["truth"]) + rng.uniform(-0.08, 0.08, 3) * (1, 1, 0.3)), grid=grid)
          for _ in range(4)]
    poses = [api.host_compound(q["init_pose"], q["rel_pose"]) for q in qs]
    differ = 0
    try:
        cells = ctxs[0].download_level(mid, 0)
        assert not cells[dropped].any() and np.array_equal(cells[~dropped], grid[~dropped])
        for k in (1, 3):
            prm = GE.settings(dict(kernel_size=k))
            got = _hill(ctxs, qs, hc, prm)
            cost = _cost(ctxs, qs, poses, prm)
            for i, q in enumerate(qs):
                assert got[i]["host_path"] == 0
                w = _want_hill(q, hc, prm, alloc=(mask, log2_block))
                _same_as(got[i], w, (k, i))
                _check_cost(cost[i], q, poses[i], prm, alloc=(mask, log2_block), where=(k, i))
                lit = GL.Greedy(**prm)
                differ += lit.cost(grid, q["geom"], q["angles"], q["ranges"], tuple(poses[i])) != \
                    lit.cost(grid, q["geom"], q["angles"], q["ranges"], tuple(poses[i]), (mask, log2_block))
    finally:
        _release(ctxs, [mid])
    assert differ > 0        # the missing blocks change what the scans read


def test_device_built_maps_equal_literal_with_allocation(ctxs, oracle):
    """Maps the device built itself (a fresh construct, the frontend's rebuilt latest map, a local map
    grown by updates), with scans whose kernel windows (k = 1, 3) reach unknown cells and unallocated
    blocks: equal to the literal on the oracle's cells and tracked allocation."""
    hc = (0.05, 0.05, 20, 2)
    unalloc = unknown = checked = 0

    def check(grid, alloc, log2_block, queries, where):
        nonlocal unalloc, unknown, checked
        qs = [dict(q, map_id=97000, grid=grid) for q in queries]
        poses = [api.host_compound(q["init_pose"], q["rel_pose"]) for q in qs]
        for k in (1, 3):
            prm = GE.settings(dict(kernel_size=k))
            got = _hill(ctxs, qs, hc, prm)
            cost = _cost(ctxs, qs, poses, prm)
            for i, q in enumerate(qs):
                assert got[i]["host_path"] == 0
                _same_as(got[i], _want_hill(q, hc, prm, alloc=(alloc, log2_block)), (where, k, i))
                _check_cost(cost[i], q, poses[i], prm, alloc=(alloc, log2_block), where=(where, k, i))
                u, z = GE.window_reads(grid, alloc, log2_block, q["geom"], poses[i], q["angles"], q["ranges"], k,
                                       prm["hit_and_missed_dist"])
                unalloc += u
                unknown += z
                checked += 1

    try:
        for log2_block in (3, 4):
            w = CE.fresh_construct(oracle, log2_block)
            for ctx in ctxs:
                shape, _ = ctx.construct_map_from_scans(97000, w["shape0"], w["map_pose"], w["nodes"])
                assert shape == w["shape"]
            assert np.array_equal(ctxs[0].download_level(97000, 0), w["grid"])
            check(w["grid"], w["alloc"], log2_block, w["queries"][:3], ("fresh", log2_block))
            _release(ctxs, [97000])
        shapes = [None, None]
        for f in CE.frontend_frames(oracle, 4):
            for j, ctx in enumerate(ctxs):
                shapes[j], _ = ctx.construct_map_from_scans(97000, shapes[j] or f["before"], f["map_pose"],
                                                            f["window"])
                assert shapes[j] == f["shape"], f["k"]
            if f["k"] % 6 == 1:
                assert np.array_equal(ctxs[0].download_level(97000, 0), f["grid"])
                check(f["grid"], f["alloc"], 4, [f["query"]], ("frontend", f["k"]))
        _release(ctxs, [97000])
        steps = list(CE.local_map_steps(oracle, 3))
        for ctx in ctxs:
            ctx.upload_grid(97000, np.zeros((steps[0]["before"]["rows"], steps[0]["before"]["cols"]), np.uint16))
        for s in steps:
            for ctx in ctxs:
                shape, _ = ctx.update_map_with_scan(97000, s["before"], s["map_pose"], s["node"],
                                                    usable_range_max=6.0)
                assert shape == s["shape"], s["k"]
            if s["query"] is not None and s["k"] % 2 == 0:
                check(s["grid"], s["alloc"], 3, [s["query"]], ("local", s["k"]))
    finally:
        _release(ctxs, [97000])
    assert checked >= 20 and unalloc > 0 and unknown > 0, (checked, unalloc, unknown)
