"""GPU parity of csm_construct_global_map (one map of many scans, cast in parts, long hit
lists sorted) against the literal CPU builder, and its equivalence with
csm_construct_map_from_scans on the same job: cells, geometry, counters and every piece
of state a later call reads, for every rank setting and part cut. Cases:
tests/global_map_cases.py (their properties are proven in
tests/test_cpu_global_map_cases.py). The parity is against oracle.construct_map, this
project's restatement of the reference's builder."""
import math

import numpy as np
import pytest

import global_map_cases as GM
from csm_hip import _lib as L, api

pytestmark = pytest.mark.gpu

G, S = 9500, 9600            # map ids: the global entry's, the single entry's


@pytest.fixture(scope="module")
def cases():
    return dict(GM.build(GM.SMALL))


@pytest.fixture(scope="module")
def wanted(oracle, cases):
    """The oracle's (shape, grid, stats) of every small case, computed once and never changed."""
    out = {}
    for name, case in cases.items():
        shape, grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"])
        grid.setflags(write=False)
        out[name] = (shape, grid, stats)
    return out


def _global(ctx, map_id, case, rank=(0, 0), limit=0):
    return ctx.construct_global_map(map_id, case["shape"], case["map_pose"], case["nodes"],
                                    scratch_limit_bytes=limit, rank_direct_max=rank[0], rank_tile=rank[1])


def _check(ctx, map_id, shape, info, want, name):
    want_shape, want_grid, stats = want
    assert shape == want_shape, name
    got = ctx.download_level(map_id, 0)
    assert got.shape == want_grid.shape, name
    bad = np.argwhere(got != want_grid)
    assert bad.size == 0, (name, len(bad), bad[:5], got[tuple(bad[0])], want_grid[tuple(bad[0])])
    assert info["rays"] == stats["rays"], name
    assert info["cell_updates"] == stats["updates"], name
    assert info["saturated_reads"] == stats["oob_reads"], name
    ys, xs = np.nonzero(want_grid)
    first = (ys.min(), xs.min()) if ys.size else want_grid.shape
    assert (info["first_known_row"], info["first_known_col"]) == first, name
    assert ctx.debug_grid_known(map_id) == tuple(first), name


def _check_paths(ginfo, prop, rank, name):
    for path in prop["paths"].get(rank, ()):
        assert ginfo[path + "_cells"] > 0, (name, rank, path, ginfo)
    if "paths" in prop and rank in prop["paths"] and not prop["paths"][rank]:
        assert ginfo["direct_cells"] + ginfo["sorted_cells"] + ginfo["tiled_cells"] == 0
    assert ginfo["max_hits_per_cell"] >= prop.get("max_hits_min", 0), (name, ginfo)


def _local(map_pose, pose):
    c, s_ = math.cos(map_pose[2]), math.sin(map_pose[2])
    dx, dy = pose[0] - map_pose[0], pose[1] - map_pose[1]
    return (c * dx + s_ * dy, -s_ * dx + c * dy, pose[2] - map_pose[2])


def _query(map_id, case, shape):
    """The case's last scan from a pose a little off the true one, map-local."""
    nd = case["nodes"][-1]
    init = _local(case["map_pose"], (nd["pose"][0] + 0.08, nd["pose"][1] - 0.06, nd["pose"][2] + 0.015))
    return dict(map_id=map_id, geom=(shape["res"], shape["off_x"], shape["off_y"]), angles=nd["angles"],
                ranges=nd["ranges"], rel_pose=nd["rel_pose"], init_pose=init)


def _match(ctx, q):
    s = ctx.correlative_match(q["map_id"], q["geom"], q["angles"], q["ranges"], q["rel_pose"], q["init_pose"],
                              0.5, 0.5, 0.2, 4, 0.0, 0.0)
    return (s["pose_found"], s["estimated_pose"], s["best_sensor_pose"], s["raw"])


def _same_allocation(ctx, case, shape, id_a, id_b):
    """The cost / covariance reads the block allocation the build carried: bit-equal on both maps."""
    qa, qb = _query(id_a, case, shape), _query(id_b, case, shape)
    ca = ctx.cost_covariance_batch([qa], [qa["init_pose"]], 1e4)[0]
    cb = ctx.cost_covariance_batch([qb], [qb["init_pose"]], 1e4)[0]
    for key in ("normalized_cost", "covariance", "hessian"):
        assert np.array_equal(ca[key], cb[key], equal_nan=True), key


@pytest.mark.parametrize("rank", GM.RANKS, ids=lambda rk: "rank_%d_%d" % rk)
@pytest.mark.parametrize("name", GM.SMALL)
def test_every_case_every_rank_in_one_part(gpu_ctx, cases, wanted, name, rank):
    case, prop = cases[name], GM.CASES[name][1]
    shape, info, ginfo = _global(gpu_ctx, G, case, rank)
    _check(gpu_ctx, G, shape, info, wanted[name], name)
    assert ginfo["parts"] == 1 and ginfo["beams"] == sum(GM.beams(case))
    _check_paths(ginfo, prop, rank, name)
    # ... and what the single entry leaves under another id
    shape_s, info_s = gpu_ctx.construct_map_from_scans(S, case["shape"], case["map_pose"], case["nodes"])
    assert shape_s == shape
    for key in ("rays", "cell_updates", "saturated_reads", "first_known_row", "first_known_col", "device_projection"):
        assert info[key] == info_s[key], (name, key)
    assert np.array_equal(gpu_ctx.download_level(G, 0), gpu_ctx.download_level(S, 0))
    assert gpu_ctx.debug_grid_known(G) == gpu_ctx.debug_grid_known(S)
    _same_allocation(gpu_ctx, case, shape, G, S)
    gpu_ctx.release_grid(G)
    gpu_ctx.release_grid(S)


def _planned_limit(case, n_cells):
    """A limit that holds a quarter of the beams and one node more: 3 to 5 parts."""
    beams = GM.beams(case)
    limit = api.host_map_batch_plan([sum(beams) // 4 + max(beams)], [n_cells], 0)[1][0]
    parts = len(api.host_global_map_parts(beams, n_cells, limit)[1])
    assert 3 <= parts <= 5, parts
    return limit, parts


@pytest.mark.parametrize("cut", ["one_part", "one_node_per_part", "planned"])
@pytest.mark.parametrize("name", GM.CUT)
def test_part_cuts_give_the_same_bytes(gpu_ctx, cases, wanted, name, cut):
    """(2, 4): every part takes all three rank paths. `saturate` reads saturated cells across parts,
    `odd` has uncertain beams patched in the bounds phase and again when their part is cast."""
    case, prop = cases[name], GM.CASES[name][1]
    rank = (2, 4)
    shape, info, ginfo = _global(gpu_ctx, G, case, rank, 1 << 40)
    assert ginfo["parts"] == 1
    whole = gpu_ctx.download_level(G, 0)
    n_cells = shape["rows"] * shape["cols"]
    if cut == "one_part":
        limit, parts = 0, 1
    elif cut == "one_node_per_part":
        limit, parts = 1, len(case["nodes"])
    else:
        limit, parts = _planned_limit(case, n_cells)
    assert parts == len(api.host_global_map_parts(GM.beams(case), n_cells, limit)[1])
    shape2, info2, ginfo2 = _global(gpu_ctx, G + 1, case, rank, limit)
    assert ginfo2["parts"] == parts, ginfo2
    _check(gpu_ctx, G + 1, shape2, info2, wanted[name], name)
    assert np.array_equal(gpu_ctx.download_level(G + 1, 0), whole)
    for key in ("rays", "cell_updates", "saturated_reads", "first_known_row", "first_known_col"):
        assert info2[key] == info[key], (name, key)
    _check_paths(ginfo, prop, rank, name)
    # every part, even of one node, has short and (NODE_LONG) long cells: proven on the CPU. The hit
    # cells are counted per part: never fewer than in one part, and no list longer
    assert ginfo2["direct_cells"] > 0, ginfo2
    assert ginfo2["sorted_cells"] + ginfo2["tiled_cells"] > 0 or name not in GM.NODE_LONG, ginfo2
    assert ginfo2["direct_cells"] + ginfo2["sorted_cells"] + ginfo2["tiled_cells"] >= \
        ginfo["direct_cells"] + ginfo["sorted_cells"] + ginfo["tiled_cells"]
    assert ginfo2["max_hits_per_cell"] <= ginfo["max_hits_per_cell"]
    _same_allocation(gpu_ctx, case, shape, G, G + 1)
    gpu_ctx.release_grid(G)
    gpu_ctx.release_grid(G + 1)


@pytest.mark.parametrize("cap", [1, 3])
def test_parts_under_a_small_uncertain_cap(cases, wanted, cap):
    """With room for `cap` uncertain beams a part with more of them is projected on the host, on its
    own and in both phases; the map is the same."""
    small = api.Context(0, map_uncertain_cap=cap)
    try:
        for limit in (0, 1):
            shape, info, ginfo = _global(small, G, cases["odd"], (2, 4), limit)
            _check(small, G, shape, info, wanted["odd"], "odd")
            assert ginfo["parts"] == (1 if limit == 0 else len(cases["odd"]["nodes"]))
            if cap == 1 and limit == 0:
                assert info["device_projection"] == 0      # at least two uncertain beams: proven on the CPU
    finally:
        small.close()


@pytest.fixture(scope="module")
def revisit(oracle):
    case = dict(GM.build(["revisit"]))["revisit"]
    shape, grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"])
    grid.setflags(write=False)
    return case, (shape, grid, stats)


@pytest.mark.parametrize("rank", [(0, 0), (8, 16)], ids=lambda rk: "rank_%d_%d" % rk)
def test_revisited_room(gpu_ctx, revisit, rank):
    """120 scans from one pose: lists of more than 1000 hits, longer than any small tile, and at the
    defaults the split between counted and sorted cells."""
    case, want = revisit
    prop = GM.CASES["revisit"][1]
    shape, info, ginfo = _global(gpu_ctx, G, case, rank)
    _check(gpu_ctx, G, shape, info, want, "revisit")
    _check_paths(ginfo, prop, rank, "revisit")
    assert ginfo["max_hits_per_cell"] >= 1000 and ginfo["beams"] == 120 * 1080
    if rank == (8, 16):
        assert ginfo["tiled_cells"] >= 100          # every cell above 256 hits, at least
    else:
        assert ginfo["sorted_cells"] >= 100 and ginfo["tiled_cells"] == 0
    gpu_ctx.release_grid(G)


def test_the_map_is_usable(gpu_ctx, cases):
    case = cases["ten"]
    shape, _, _ = _global(gpu_ctx, G, case, (8, 16), 1)
    shape_s, _ = gpu_ctx.construct_map_from_scans(S, case["shape"], case["map_pose"], case["nodes"])
    assert shape == shape_s
    got, want = _match(gpu_ctx, _query(G, case, shape)), _match(gpu_ctx, _query(S, case, shape))
    assert got[0] == 1 and got == want
    gpu_ctx.release_grid(G)
    gpu_ctx.release_grid(S)


def test_refusals_leave_a_resident_map_alone(gpu_ctx, cases):
    old = np.arange(32 * 32, dtype=np.uint16).reshape(32, 32)
    gpu_ctx.upload_grid(G, old)
    case = cases["ten"]
    kw = dict(map_id=G, shape=case["shape"], map_pose=case["map_pose"], nodes=case["nodes"])
    for bad in (dict(scratch_limit_bytes=-1), dict(rank_tile=3), dict(rank_tile=24), dict(rank_tile=2),
                dict(rank_tile=1 << 15), dict(rank_direct_max=-1), dict(subpixel_scale=0), dict(nodes=[])):
        with pytest.raises(api.CsmError) as err:
            gpu_ctx.construct_global_map(**dict(kw, **bad))
        assert err.value.code == L.CSM_EINVAL, bad
        assert np.array_equal(gpu_ctx.download_level(G, 0), old), bad
    # refused after the projection, as the single call refuses it: all usable beams point along +x
    angles, ranges = np.array([0.0, 0.0, 0.0]), np.array([2.0, 3.0, 1.5])
    shape = dict(res=0.05, off_x=0.0, off_y=0.0, rows=32, cols=32, log2_block=4)
    along_x = dict(pose=(0.3, 0.2, 0.0), angles=angles, ranges=ranges, rel_pose=(0.0, 0.0, 0.0),
                   min_range=0.0, max_range=10.0)
    far = [dict(along_x, angles=np.array([0.3, 1.1, 2.0])),
           dict(along_x, pose=(1000.3, 1000.2, 0.0), angles=np.array([0.3, 1.1, 2.0]))]
    for nodes in ([along_x], [along_x, along_x], far):
        messages = []
        for call in (gpu_ctx.construct_global_map, gpu_ctx.construct_map_from_scans):
            with pytest.raises(api.CsmError) as err:
                call(G, shape, (0.0, 0.0, 0.0), nodes)
            assert err.value.code == L.CSM_EINVAL
            messages.append(str(err.value))
            assert np.array_equal(gpu_ctx.download_level(G, 0), old)
        assert messages[0] == messages[1]
    # one node per part: the same refusals
    with pytest.raises(api.CsmError):
        gpu_ctx.construct_global_map(G, shape, (0.0, 0.0, 0.0), [along_x, along_x], scratch_limit_bytes=1)
    assert np.array_equal(gpu_ctx.download_level(G, 0), old)
    gpu_ctx.release_grid(G)


def test_rebuild_over_a_larger_map_with_levels(oracle, cases, wanted):
    """An id that holds a larger map with box-max levels and a phase-major copy is rebuilt from a small
    job: context A by the single entry, context B by the global one in parts. Levels built afterwards,
    a match and the cost (which reads the carried block allocation) are the same, and the cells are the
    oracle's: nothing stale is read."""
    big = cases["ten"]
    small = dict(cases["odd"], nodes=[dict(nd, max_range=3.0) for nd in cases["odd"]["nodes"][:3]])
    a = api.Context(0, tuning_off=L.TUNE_FORCE_TWO_PHASE)
    b = api.Context(0, tuning_off=L.TUNE_FORCE_TWO_PHASE)
    try:
        shape_a, _ = a.construct_map_from_scans(G, big["shape"], big["map_pose"], big["nodes"])
        shape_b, _, _ = _global(b, G, big)
        assert shape_a == shape_b == wanted["ten"][0]
        for ctx in (a, b):
            ctx.build_pyramid(G, [1, 4])
            assert _match(ctx, _query(G, big, shape_a))[0] == 1       # leaves a phase-major copy
        # the small job, in the frame the first build left
        job = dict(small, shape=shape_a)
        want_shape, want_grid, stats = oracle.construct_map(job["shape"], job["map_pose"], job["nodes"])
        assert want_grid.size < wanted["ten"][1].size
        shape_a2, info_a = a.construct_map_from_scans(G, job["shape"], job["map_pose"], job["nodes"])
        shape_b2, info_b, ginfo = _global(b, G, job, (2, 4), 1)
        assert ginfo["parts"] == len(job["nodes"])
        assert shape_a2 == shape_b2 == want_shape
        _check(b, G, shape_b2, info_b, (want_shape, want_grid, stats), "odd over ten")
        for ctx in (a, b):
            with pytest.raises(api.CsmError) as err:       # the box-max level is behind the new cells
                ctx.download_level(G, 1)
            assert err.value.code == L.CSM_ENOENT
            ctx.build_pyramid(G, [1, 4])
        for level in (0, 1):
            assert np.array_equal(a.download_level(G, level), b.download_level(G, level)), level
        qa = _query(G, job, want_shape)
        assert _match(a, qa) == _match(b, qa)
        ca = a.cost_covariance_batch([qa], [qa["init_pose"]], 1e4)[0]
        cb = b.cost_covariance_batch([qa], [qa["init_pose"]], 1e4)[0]
        for key in ("normalized_cost", "covariance", "hessian"):
            assert np.array_equal(ca[key], cb[key], equal_nan=True), key
    finally:
        a.close()
        b.close()


def test_host_projection_gives_the_same(cases, wanted):
    host = api.Context(0, tuning_off=L.TUNE_MAP_HOST_PROJECTION)
    try:
        for name in ("ten", "odd", "none_usable"):
            for limit in (0, 1):
                shape, info, ginfo = _global(host, G, cases[name], (8, 16), limit)
                _check(host, G, shape, info, wanted[name], name)
                assert info["device_projection"] == 0
    finally:
        host.close()


def test_live_bytes_return():
    case = dict(GM.build(["ten"]))["ten"]
    before = api.debug_live_bytes()
    ctx = api.Context(0)
    try:
        _global(ctx, G, case, (2, 4), 1)
        _global(ctx, G, case)
        assert api.debug_live_bytes()[0] > before[0]
    finally:
        ctx.close()
    assert api.debug_live_bytes() == before
