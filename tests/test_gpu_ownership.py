"""Every device and pinned buffer of a context is owned (DevBuf / PinBuf in csm_internal.hpp): the
library's own live-byte counters (csm_debug_live_bytes) return to where they were once the maps
are released and the context is closed. The counters are process-wide and the card is shared, so
device-wide free memory would not show this."""
import math

import numpy as np
import pytest

from csm_hip import api, synth

pytestmark = pytest.mark.gpu

CSM = (1.0, 1.0, math.radians(10), 4, 0.0, 0.0)
BNB = (2.5, 2.5, 0.5, 2, 0.3, 0.5)


def _every_family(ctx, case, mids):
    """matcher, batches, cost, hill climbing on the given maps; a map build and a pose graph."""
    args = (case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"])
    for m in mids:
        ctx.correlative_match(m, *args, *CSM)
    qs = [dict(map_id=m, geom=case["geom"], angles=case["angles"], ranges=case["ranges"],
               rel_pose=case["rel_pose"], init_pose=case["init_pose"]) for m in mids]
    ctx.correlative_match_batch(qs, *CSM[:4], 0.0, 0.0)
    ctx.bnb_match_batch(qs, *BNB)
    poses = np.array([api.host_compound(q["init_pose"], q["rel_pose"]) for q in qs])
    ctx.cost_covariance_batch(qs, poses, 1e4)
    ctx.greedy_cost_covariance_batch(qs, poses)
    ctx.hill_climbing_batch(qs)
    built = synth.map_case(950, n_scans=4)
    ctx.construct_map_from_scans(99, built["shape"], built["map_pose"], built["nodes"])
    g = synth.pose_graph_case(951, n_scans=20)
    ctx.pose_graph_lm(g["local"], g["scan"], g["edges"], 1e-4)


def test_release_and_close_return_every_byte():
    case = synth.csm_case(11, rows=256, cols=256)
    grid = case["grid"]
    k = 4
    blocks = [grid[r * 16:(r + 1) * 16, c * 16:(c + 1) * 16].copy() for r in range(16) for c in range(16)]
    before = api.debug_live_bytes()
    ctx = api.Context(0)
    try:
        ctx.upload_grid(1, grid)
        ctx.upload_grid_blocks(2, [b if b.any() else None for b in blocks], 16, 16, k)
        _every_family(ctx, case, (1, 2))
        for m in (1, 2, 99):
            ctx.release_grid(m)
        # the workspaces have their size now: a map's whole footprint goes with release_grid
        mark = api.debug_live_bytes()
        ctx.upload_grid(1, grid)
        assert api.debug_live_bytes()[0] > mark[0]
        _every_family(ctx, case, (1,))
        ctx.release_grid(99)
        ctx.release_grid(1)
        assert api.debug_live_bytes() == mark
    finally:
        ctx.close()
    assert api.debug_live_bytes() == before
