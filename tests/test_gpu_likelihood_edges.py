"""GPU parity of the likelihood-field build at the numbers its index arithmetic branches on
(tests/likelihood_reference.py, EDGE_CASES): discs whose rim holds off-axis cells, tables that are not the
monotone Gaussian, halos holding exactly (2R + 1)^2 obstacles and one more, maps of one row, one column and
one cell, the value 65535, other thresholds, the dense path on partial tiles and pad columns. Then what the
host keeps beside the cells: the first known row and column of every built field (csm_debug_grid_known), a
batch whose tallest and widest maps are different maps, and a search near a map's low edge, where those
counters decide the result. Bar: equality of bytes, integers and double bits; nothing has a tolerance."""
import ctypes as C
import math

import numpy as np
import pytest

import likelihood_reference as LR
from csm_hip import _lib as Lb, api, synth
from test_gpu_likelihood import _strip

pytestmark = pytest.mark.gpu

SRC, DST, REF = 8300, 8301, 8302                 # 8300 .. 8399: this file's ids
RANGE = (1.0, 1.0, math.radians(10))


def _id(case):
    return "%s-R%d-%s-%d" % case


def _release(ctx, ids):
    for m in ids:
        if ctx.has_grid(m):
            ctx.release_grid(m)


@pytest.mark.parametrize("keep_unknown", [False, True])
@pytest.mark.parametrize("case", LR.EDGE_CASES, ids=_id)
def test_cells_equal_the_reference(gpu_ctx, case, keep_unknown):
    name, R, kind, occ = case
    g, t, want = LR.edge_expected(name, R, kind, occ, keep_unknown)
    try:
        gpu_ctx.upload_grid(SRC, g)
        gpu_ctx.build_likelihood_map(SRC, DST, radius=R, occupied_min=occ, keep_unknown=keep_unknown, kernel=t)
        got = gpu_ctx.download_level(DST, 0)
        assert np.array_equal(gpu_ctx.download_level(SRC, 0), g)            # the source is not touched
    finally:
        _release(gpu_ctx, (SRC, DST))
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("keep_unknown", [False, True])
@pytest.mark.parametrize("case", LR.ALL_CASES, ids=_id)
def test_counters_equal_the_first_known_cell_of_the_reference(gpu_ctx, case, keep_unknown):
    name, R, kind, occ = case
    g, t, want = LR.edge_expected(name, R, kind, occ, keep_unknown)
    try:
        gpu_ctx.upload_grid(SRC, g)
        gpu_ctx.build_likelihood_map(SRC, DST, radius=R, occupied_min=occ, keep_unknown=keep_unknown, kernel=t)
        gpu_ctx.upload_grid(REF, want)
        built, uploaded, source = (gpu_ctx.debug_grid_known(m) for m in (DST, REF, SRC))
    finally:
        _release(gpu_ctx, (SRC, DST, REF))
    assert built == LR.first_known(want)
    assert uploaded == LR.first_known(want)
    assert source == LR.first_known(g)
    if name == "all_unknown":
        assert built == g.shape == (20, 33)


def test_the_hook_refuses_a_map_that_is_not_resident(gpu_ctx):
    assert not gpu_ctx.has_grid(8399)
    with pytest.raises(api.CsmError) as err:
        gpu_ctx.debug_grid_known(8399)
    assert err.value.code == Lb.CSM_ENOENT
    out = (C.c_int32 * 2)(-7, -7)
    assert gpu_ctx.lib.csm_debug_grid_known(gpu_ctx._ctx, 8399, out) == Lb.CSM_ENOENT
    assert list(out) == [-7, -7]
    assert gpu_ctx.lib.csm_debug_grid_known(gpu_ctx._ctx, 8399, None) == Lb.CSM_EINVAL
    assert gpu_ctx.lib.csm_debug_grid_known(None, 8399, out) == Lb.CSM_EINVAL


# one_cell first and lineNx1 second: the tallest map alone sets the launch's row tiles, line1xN (fifth) alone
# its column tiles, and neither is the first or the last job
BATCH = ["one_cell", "lineNx1", "dense64", "all_unknown", "line1xN", "switch_16_plus", "low_known", "random37x53"]


@pytest.mark.parametrize("R,kind,keep_unknown", [(16, "ramp", False), (5, "gauss", True)])
def test_batch_of_eight_shapes_equals_eight_single_calls(gpu_ctx, R, kind, keep_unknown):
    n = len(BATCH)
    srcs, dsts, singles = [[8310 + 10 * k + i for i in range(n)] for k in range(3)]
    t = LR.table_of(kind, R)
    kw = dict(radius=R, kernel=t, keep_unknown=keep_unknown)
    shapes = [LR.grid_of(name).shape for name in BATCH]
    assert max(s[0] for s in shapes) == shapes[1][0] == 200 and sorted(s[0] for s in shapes)[-2] <= 65
    assert max(s[1] for s in shapes) == shapes[4][1] == 200 and sorted(s[1] for s in shapes)[-2] <= 130
    try:
        for s, name in zip(srcs, BATCH):
            gpu_ctx.upload_grid(s, LR.grid_of(name))
        for s, d in zip(srcs, singles):
            gpu_ctx.build_likelihood_map(s, d, **kw)
        one = [gpu_ctx.download_level(d, 0) for d in singles]
        for order in (list(range(n)), list(reversed(range(n)))):
            # the second call rebuilds every destination, in the same ids, from the reversed list
            gpu_ctx.build_likelihood_maps([srcs[i] for i in order], [dsts[i] for i in order], **kw)
            for i, name in enumerate(BATCH):
                want = LR.edge_expected(name, R, kind, 32768, keep_unknown)[2]
                cells = gpu_ctx.download_level(dsts[i], 0)
                assert np.array_equal(cells, want), (name, order[0], np.argwhere(cells != want)[:8])
                assert np.array_equal(cells, one[i]), (name, order[0])
                assert gpu_ctx.debug_grid_known(dsts[i]) == LR.first_known(want), (name, order[0])
                assert gpu_ctx.debug_grid_known(singles[i]) == LR.first_known(want), (name, order[0])
                assert np.array_equal(gpu_ctx.download_level(srcs[i], 0), LR.grid_of(name))
    finally:
        _release(gpu_ctx, srcs + dsts + singles)


# ---- maps whose cells begin at the low edge: the counters decide the edge-band flag and the literal redo ----

LOW_EDGE = [(50, 4), (51, 4), (52, 5), (53, 8), (54, 3), (55, 4), (56, 2), (57, 6)]     # test_gpu_edge.py's
_band = {}           # (seed, keep_unknown) -> FLAG_EDGE_BAND of the match on the uploaded reference field


def _low_edge_case(seed):
    return synth.csm_case(seed, rows=256, cols=288, origin="low_edge", half_x=5.2, half_y=4.4,
                          init_error=(0.23, 0.19, 0.03))


def _low_edge_field(case, keep_unknown):
    return LR.likelihood_map(case["grid"], LR.table_of("gauss", 3), 3, 32768, keep_unknown)


@pytest.mark.parametrize("keep_unknown", [False, True])
@pytest.mark.parametrize("seed,Lr", LOW_EDGE)
def test_low_edge_field_matches_like_an_upload_and_like_the_oracle(gpu_ctx, oracle, seed, Lr, keep_unknown):
    case = _low_edge_case(seed)
    want = _low_edge_field(case, keep_unknown)
    scan = (case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"])
    try:
        gpu_ctx.upload_grid(SRC, case["grid"])
        gpu_ctx.build_likelihood_map(SRC, DST, radius=3, keep_unknown=keep_unknown, kernel=LR.table_of("gauss", 3))
        gpu_ctx.upload_grid(REF, want)
        assert gpu_ctx.debug_grid_known(DST) == gpu_ctx.debug_grid_known(REF) == LR.first_known(want)
        got = _strip(gpu_ctx.correlative_match(DST, *scan, *RANGE, Lr))
        ref = _strip(gpu_ctx.correlative_match(REF, *scan, *RANGE, Lr))
    finally:
        _release(gpu_ctx, (SRC, DST, REF))
    _band[(seed, keep_unknown)] = bool(ref["raw"]["flags"] & Lb.FLAG_EDGE_BAND)
    assert got == ref                                                    # flags among them
    lit = oracle.csm(dict(case, grid=want), *RANGE, Lr)
    raw = got["raw"]
    assert got["pose_found"] == lit["found"], (raw, lit)
    assert (raw["best_x"], raw["best_y"], raw["best_theta"]) == (lit["bestX"], lit["bestY"], lit["bestT"]), (raw, lit)
    assert raw["score"] == lit["scoreMax"]
    assert got["estimated_pose"] == lit["estimatedPose"]


def test_low_edge_fields_reach_the_edge_band(gpu_ctx):
    """The sixteen runs above are about the counters only if some of them depend on the counters: at least
    one match on an UPLOADED reference field (the route not under test) must raise the edge-band flag. Runs
    the matches it has no flag of yet, so that it also holds on its own."""
    for seed, Lr in LOW_EDGE:
        for keep_unknown in (False, True):
            if (seed, keep_unknown) in _band:
                continue
            case = _low_edge_case(seed)
            try:
                gpu_ctx.upload_grid(REF, _low_edge_field(case, keep_unknown))
                m = gpu_ctx.correlative_match(REF, case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                                              case["init_pose"], *RANGE, Lr)
            finally:
                _release(gpu_ctx, (REF,))
            _band[(seed, keep_unknown)] = bool(m["raw"]["flags"] & Lb.FLAG_EDGE_BAND)
    print("edge band on the uploaded field:", sorted(k for k, v in _band.items() if v))
    assert any(_band.values())
