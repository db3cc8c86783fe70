"""GPU parity of the three map builders on cells whose value depends on the order of their hits and misses
(tests/map_rank_cases.py; the cases' properties are proven in tests/test_cpu_map_rank_cases.py). Every build
is compared with oracle.construct_map cell for cell and counter for counter, every target cell with the
value of its planned sequence (k hits, the miss block, n - k hits: another interval for the block is another
value), and the global builder's counts of hit cells per rank path with the exact counts from the
sequences. A hit ranked wrongly (map_rank_ray, k_gmap_rank_sort), a miss put into the wrong interval
(map_miss) or an interval counter read wrongly (map_apply_hit_cell) changes a target."""
import numpy as np
import pytest

import global_map_cases as GM
import map_rank_cases as MR
from csm_hip import api
from test_gpu_global_map import _check

pytestmark = pytest.mark.gpu

BASE = 9800                          # 9800 .. 9899: this file's map ids

SWEEP = ["sweep_%d" % b for b in range(MR.SWEEP_BUILDS)]
WALKS = ["walks_%d" % s for s in MR.WALK_SCALES]
RANK_KEYS = ("direct_cells", "sorted_cells", "tiled_cells", "max_hits_per_cell")


@pytest.fixture(scope="module")
def cases():
    return dict(MR.build())


@pytest.fixture(scope="module")
def wanted(oracle, cases):
    """The oracle's (shape, grid, stats) of every case, computed once and never changed."""
    out = {}
    for name, case in cases.items():
        shape, grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"], **MR.oracle_kw(case))
        grid.setflags(write=False)
        out[name] = (shape, grid, stats)
    return out


@pytest.fixture(scope="module")
def target_values():
    """(n, k) -> the value of the planned sequence, through oracle.bayes_update."""
    memo = {}

    def value(n, k):
        if (n, k) not in memo:
            memo[(n, k)] = int(MR.values_by_block_position(n)[k]) if k is not None else MR.value_of(MR.planned(n, k))
        return memo[(n, k)]
    return value


def _global(ctx, map_id, case, rank=(0, 0), limit=0):
    return ctx.construct_global_map(map_id, case["shape"], case["map_pose"], case["nodes"], scratch_limit_bytes=limit,
                                    rank_direct_max=rank[0], rank_tile=rank[1], **MR.build_kw(case))


def _check_targets(ctx, map_id, case, shape, value, tag):
    got = ctx.download_level(map_id, 0)
    for T, n, k in case["targets"]:
        x, y = MR.in_frame(T, shape)
        assert got[y, x] == value(n, k), (case["name"], tag, "target", T, "hits", n, "block after", k,
                                          int(got[y, x]), value(n, k))


def _check_build(ctx, map_id, case, shape, info, want, value, tag):
    _check(ctx, map_id, shape, info, want, (case["name"], tag))
    assert info["device_projection"] == 1, (case["name"], tag)
    _check_targets(ctx, map_id, case, shape, value, tag)


def _check_rank_info(ginfo, case, shape, rank, parts=None):
    want = MR.rank_info(case, shape, rank, parts)
    assert {key: ginfo[key] for key in RANK_KEYS} == want, (case["name"], rank, ginfo)


# ---- the global builder ----

@pytest.mark.parametrize("rank", GM.RANKS, ids=lambda rk: "rank_%d_%d" % rk)
@pytest.mark.parametrize("name", SWEEP)
def test_global_sweep_under_every_rank_setting(gpu_ctx, cases, wanted, target_values, name, rank):
    """Every n in 1 .. 50 with every block position: n % 4 for the uint4 groups of the interval counters,
    every padded sort size up to 64, and n, n +- 1 around both splits of the small settings."""
    case = cases[name]
    shape, info, ginfo = _global(gpu_ctx, BASE, case, rank)
    _check_build(gpu_ctx, BASE, case, shape, info, wanted[name], target_values, rank)
    assert ginfo["parts"] == 1 and ginfo["beams"] == sum(GM.beams(case))
    _check_rank_info(ginfo, case, shape, rank)
    gpu_ctx.release_grid(BASE)


@pytest.mark.parametrize("name", ["boundaries_default", "largest_tile", "all_pairs"])
def test_global_rank_boundaries(gpu_ctx, cases, wanted, target_values, name):
    """The default splits 32 | 33 and 4096 | 4097 (a last tile of one entry); the largest tile, 16384
    entries in 64 KB of dynamic LDS, full and with one entry more; and the job whose hit cells and long
    cells together are its rays. The case's own settings, and where they are the defaults, (0, 0) too."""
    case = cases[name]
    settings = [case["rank"]] + ([(0, 0)] if case["rank"] == GM.DEFAULTS else [])
    for rank in settings:
        shape, info, ginfo = _global(gpu_ctx, BASE, case, rank)
        _check_build(gpu_ctx, BASE, case, shape, info, wanted[name], target_values, rank)
        assert ginfo["parts"] == 1 and ginfo["beams"] == sum(GM.beams(case))
        _check_rank_info(ginfo, case, shape, rank)
        if name == "all_pairs":
            assert ginfo["direct_cells"] == 0 and 2 * ginfo["sorted_cells"] == info["rays"] == ginfo["beams"]
        gpu_ctx.release_grid(BASE)


@pytest.mark.parametrize("name", ["two_nodes"] + SWEEP)
def test_global_parts_give_the_same_bytes(gpu_ctx, cases, wanted, target_values, name):
    """One part against one node per part. two_nodes: a target's hits lie in the first and the last part
    and its miss block in the part between them, so a part starts from the cells the one before left
    (keep_cells) on cells that take hits and on cells that take misses only."""
    case = cases[name]
    rank = (2, 4)
    shape, info, ginfo = _global(gpu_ctx, BASE, case, rank, 0)
    assert ginfo["parts"] == 1
    _check_build(gpu_ctx, BASE, case, shape, info, wanted[name], target_values, "one part")
    whole = gpu_ctx.download_level(BASE, 0)
    shape2, info2, ginfo2 = _global(gpu_ctx, BASE + 1, case, rank, 1)
    assert ginfo2["parts"] == len(case["nodes"]), ginfo2
    _check_build(gpu_ctx, BASE + 1, case, shape2, info2, wanted[name], target_values, "one node per part")
    assert np.array_equal(gpu_ctx.download_level(BASE + 1, 0), whole)
    for key in ("rays", "cell_updates", "saturated_reads", "first_known_row", "first_known_col"):
        assert info2[key] == info[key], (name, key)
    _check_rank_info(ginfo, case, shape, rank)
    _check_rank_info(ginfo2, case, shape, rank, [[k] for k in range(len(case["nodes"]))])
    gpu_ctx.release_grid(BASE)
    gpu_ctx.release_grid(BASE + 1)


# ---- the single and the batch builder ----

@pytest.mark.parametrize("name", SWEEP + ["two_nodes"] + WALKS)
def test_single_builder(gpu_ctx, cases, wanted, target_values, name):
    case = cases[name]
    shape, info = gpu_ctx.construct_map_from_scans(BASE, case["shape"], case["map_pose"], case["nodes"],
                                                   **MR.build_kw(case))
    _check_build(gpu_ctx, BASE, case, shape, info, wanted[name], target_values, "single")
    gpu_ctx.release_grid(BASE)


def _jobs(names, cases):
    return [dict(map_id=BASE + 10 + i, shape=cases[n]["shape"], map_pose=cases[n]["map_pose"], nodes=cases[n]["nodes"])
            for i, n in enumerate(names)]


@pytest.mark.parametrize("limit", [0, 1], ids=["one_chunk", "one_job_per_chunk"])
@pytest.mark.parametrize("scale", MR.WALK_SCALES)
def test_batch_builder(gpu_ctx, cases, wanted, target_values, scale, limit):
    """All cases of one sub-pixel scale in one call: in one chunk, and under a limit that gives every job
    a chunk of its own."""
    names = [n for n in SWEEP + ["two_nodes"] + WALKS if cases[n]["subpixel_scale"] == scale]
    names = names + names[-1:] if len(names) == 1 else names         # the scale-1 walks twice: two maps in the chunk
    jobs = _jobs(names, cases)
    results, binfo = gpu_ctx.construct_maps_from_scans(jobs, scratch_limit_bytes=limit, **MR.build_kw(cases[names[0]]))
    assert binfo["chunks"] == (1 if limit == 0 else len(jobs)), binfo
    for job, name, (shape, info, status) in zip(jobs, names, results):
        assert status == 0, name
        _check_build(gpu_ctx, job["map_id"], cases[name], shape, info, wanted[name], target_values, ("batch", limit))
        gpu_ctx.release_grid(job["map_id"])


@pytest.mark.parametrize("scale", MR.WALK_SCALES)
def test_walks_on_the_global_builder(gpu_ctx, cases, wanted, target_values, scale):
    """The closed form of the walk without a clip window (map_walk_ray), which the ray check never runs."""
    case = cases["walks_%d" % scale]
    for limit in (0, 1):
        shape, info, ginfo = _global(gpu_ctx, BASE, case, (2, 4), limit)
        _check_build(gpu_ctx, BASE, case, shape, info, wanted[case["name"]], target_values, ("global", limit))
        assert ginfo["parts"] == (1 if limit == 0 else len(case["nodes"]))
        gpu_ctx.release_grid(BASE)


# ---- updates ----

def test_updates_start_from_the_cells_of_the_build_before(gpu_ctx, oracle, cases, wanted, target_values):
    """two_nodes node by node: a build from the first node (a target's first k hits), an update with the
    node of the miss blocks, an update with the last node (the other n - k hits): the start value of a
    cell that takes hits is what the call before left. No update resizes the map."""
    case = cases["two_nodes"]
    kw, okw = MR.build_kw(case), MR.oracle_kw(case)
    want_shape, want_grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"][:1], **okw)
    shape, info = gpu_ctx.construct_map_from_scans(BASE, case["shape"], case["map_pose"], case["nodes"][:1], **kw)
    _check(gpu_ctx, BASE, shape, info, (want_shape, want_grid, stats), "two_nodes, node 0")
    assert shape == wanted["two_nodes"][0]
    for k, node in enumerate(case["nodes"][1:], 1):
        want_shape, want_grid, stats = oracle.update_map(want_shape, want_grid, case["map_pose"], node, **okw)
        shape2, info = gpu_ctx.update_map_with_scan(BASE, shape, case["map_pose"], node, **kw)
        assert shape2 == shape == want_shape, k
        _check(gpu_ctx, BASE, shape2, info, (want_shape, want_grid, stats), "two_nodes, node %d" % k)
        assert info["device_projection"] == 1
    assert np.array_equal(want_grid, wanted["two_nodes"][1])
    _check_targets(gpu_ctx, BASE, case, shape, target_values, "updates")
    gpu_ctx.release_grid(BASE)
