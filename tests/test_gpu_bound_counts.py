"""The beam counts of the packed-fp32 bound pass (csm_joint_kernels.hip: count as scalar FMA
operand): an entry's four 4-bit counts multiply the pre-scaled key copy as fp32 denormals straight
from the entry word. Small cases built so that every count 1 .. 15, a cell split into two entries,
an entry with all four (row parity x slice) counts and an entry with a single count occur -- asserted
from the host projection -- on a map whose cells include 1 and 65535, through csm_score_windows_dev
and its fp32 key dump (as tests/test_gpu_headline.py) and through csm_bnb_match_batch.

Bounds: |fp32 key - key| <= (n + 3) 2^-24 key for n beams; a flushed denormal
count would show as a dumped 0 where the exact key is not 0."""
import math

import numpy as np
import pytest
import torch

from csm_hip import _lib as L, api, synth

pytestmark = pytest.mark.gpu

ROWS = COLS = 96
RES = 0.05
LR = 4
# (row offset, column offset, beams) of the cells the near beams end in, relative to the sensor's cell.
# Column +3 holds three vertically adjacent cells: whichever parity the frame gives the rows, two of them
# share a pair row. Every other cell has no hit neighbour above or below.
TRIPLE = [(-1, 3, 5), (0, 3, 6), (1, 3, 7)]
LONE = [(-6, -6, 1), (-6, -3, 3), (-6, 0, 4), (-6, 5, 8), (-3, -5, 9), (-3, -1, 10), (-3, 6, 11),
        (3, -6, 12), (3, -2, 13), (3, 6, 14), (6, -4, 17)]
N_FAR = 10
FAR_RANGE = 2.0            # 40 cells: sets the angular step, so that near beams keep their cell in neighbouring slices


def _case(seed):
    rng = np.random.RandomState(seed)
    _, geom, _ = synth.make_room(seed, rows=ROWS, cols=COLS, res=RES)
    grid = rng.randint(2, 65535, (ROWS, COLS)).astype(np.uint16)
    pick = rng.rand(ROWS, COLS)
    grid[pick < 0.25] = 0
    grid[(pick >= 0.25) & (pick < 0.35)] = 1
    grid[(pick >= 0.35) & (pick < 0.45)] = 65535
    res, off_x, off_y = geom[0], geom[1], geom[2]
    sr, sc = ROWS // 2, COLS // 2
    x0, y0, th0 = off_x + (sc + 0.5) * res, off_y + (sr + 0.5) * res, 0.3
    angles, ranges = [], []
    for dr, dc, m in TRIPLE + LONE:
        a, r = math.atan2(dr * res, dc * res) - th0, math.hypot(dr * res, dc * res)
        angles += [a] * m
        ranges += [r] * m
    for k in range(N_FAR):
        angles.append(-2.0 + 0.41 * k)
        ranges.append(FAR_RANGE - 0.013 * k)
    # beams of one cell follow each other: the batch entries merge beams (and run the bound pass) where
    # neighbouring beams mostly share cells
    angles, ranges = np.asarray(angles), np.asarray(ranges)
    assert 96 <= len(angles) <= 160
    return dict(grid=grid, geom=geom, angles=angles, ranges=ranges, rel_pose=(0.0, 0.0, 0.0),
                init_pose=(x0, y0, th0), truth=(x0, y0, th0))


def _entry_counts(col, row, parity):
    """[(e0, o0, e1, o1)] of every (pair row, column) the slice pairs hit, rows paired as (r + parity) >> 1."""
    nt = col.shape[0]
    out = []
    for t0 in range(0, nt, 2):
        cells = {}
        for s, t in enumerate(range(t0, min(t0 + 2, nt))):
            for r, c in zip(row[t].tolist(), col[t].tolist()):
                v = cells.setdefault(((r + parity) >> 1, c), [0, 0, 0, 0])
                v[2 * s + ((r + parity) & 1)] += 1
        out += [tuple(v) for v in cells.values()]
    return out


@pytest.fixture(scope="module")
def case():
    return _case(7)


def test_case_reaches_every_count_path(case):
    """From the host projection alone: the scan does what the GPU tests below rely on."""
    sx, sy, st = api.host_search_step(case["geom"][0], case["ranges"])
    wt = api.host_window(0.07, st)
    col, row = api.host_project(case["geom"], case["init_pose"], st, wt, case["angles"], case["ranges"])
    assert col.shape[0] % 2 == 1 and col.shape[0] >= 5       # the last pair holds one slice
    for parity in (0, 1):
        ent = _entry_counts(col, row, parity)
        nibbles = set()
        for e in ent:
            for b in e:
                while b > 0:                                  # a cell with more than 15 beams: 15 + the rest
                    nibbles.add(min(b, 15))
                    b -= min(b, 15)
        assert nibbles >= set(range(1, 16)), sorted(nibbles)
        assert any(max(e) > 15 for e in ent)                  # split into two entries
        assert any(min(e) > 0 for e in ent)                   # all four counts in one entry
        assert any(sum(1 for b in e if b) == 1 for e in ent)  # a single count
    assert {1, 65535} <= set(np.unique(case["grid"]).tolist())


def _run(ctx, case, rx, ry, rt, n_copies=2):
    dev = torch.device("cuda", 0)
    sx, sy, st = api.host_search_step(case["geom"][0], case["ranges"])
    wx, wy, wt = api.host_window(rx, sx), api.host_window(ry, sy), api.host_window(rt, st)
    col, row = api.host_project(case["geom"], case["init_pose"], st, wt, case["angles"], case["ranges"])
    n = len(case["angles"])
    ctx.upload_grid(9, case["grid"])
    ctx.build_pyramid(9, [1, LR])
    w = ctx.make_window(2 * wt + 1, n, wx, wy, LR, 1, api.host_min_known(n, 0.0), 0.0)
    c_d, r_d = torch.from_numpy(col).to(dev), torch.from_numpy(row).to(dev)
    out = torch.zeros(n_copies * 48, dtype=torch.uint8, device=dev)
    prepared = ctx.prepare_windows([9] * n_copies, [w] * n_copies, [c_d.data_ptr()] * n_copies,
                                   [r_d.data_ptr()] * n_copies)
    nx, ny = -(-(2 * wx + 1) // LR) * LR, -(-(2 * wy + 1) // LR) * LR
    fkeys = torch.zeros((2 * wt + 1) * nx * ny, dtype=torch.float32, device=dev)
    ctx.score_windows_dump_dev(prepared, out.data_ptr(), None, None, [fkeys.data_ptr()] + [0] * (n_copies - 1))
    torch.cuda.synchronize(dev)
    final = []
    for k in range(n_copies):
        r = L.Result.from_buffer_copy(out.cpu().numpy()[48 * k:48 * (k + 1)].tobytes())
        if r.flags & (L.FLAG_EDGE_BAND | L.FLAG_KEY_TIE):      # finished by the exact single-window paths
            d = ctx.score_window(9, w, col, row)
            final.append((d["found"], d["best_x"], d["best_y"], d["best_theta"], d["score"]))
        else:
            final.append((r.found, r.best_x, r.best_y, r.best_theta, r.score))
    ctx.release_grid(9)
    return final, fkeys.cpu().numpy(), (wx, wy, nx, ny)


def _range_of(w):          # a search range (full width) whose window is +-w cells, clear of the rounding
    return (2 * w - 0.5) * RES


# +-4 and +-6 cells: one candidate block; 12 x 84 candidates: two row blocks of 48 = 6 lane groups x R = 8,
# the second with 36 rows = 6 x R = 6 -- the R = 8 launch and the R = 6 tail launch both run
WINDOWS = [("pm4", _range_of(4), _range_of(4), (4, 4, 12, 12)), ("pm6", _range_of(6), _range_of(6), (6, 6, 16, 16)),
           ("both_launches", _range_of(4), _range_of(41), (4, 41, 12, 84))]


@pytest.mark.parametrize("name,rx,ry,shape", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_counts_as_denormal_operands(case, oracle, name, rx, ry, shape):
    dev = torch.device("cuda", 0)
    rt = 0.07
    outs, keys = [], None
    for off in (0, L.TUNE_NO_BOUND_PASS):
        ctx = api.Context(0, tuning_off=off)
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        final, fk, got_shape = _run(ctx, case, rx, ry, rt)
        ctx.close()
        assert got_shape == shape
        outs.append(final)
        if off == 0:
            keys = fk
    lit = oracle.csm(case, rx, ry, rt, LR)
    want = (lit["found"], lit["bestX"], lit["bestY"], lit["bestT"], lit["scoreMax"])
    assert outs[0] == outs[1]
    assert all(f == want for f in outs[0]), (outs[0], want)
    _, oS, oK, _ = oracle.csm_closed_form(case, rx, ry, rt, LR, dump=True)
    key = 32268.0 * oK.astype(np.float64) + 499.0 * oS.astype(np.float64)
    got = keys.astype(np.float64).reshape(key.shape)
    n = len(case["angles"])
    err = np.abs(got - key)
    print(name, "max rel err", float((err / np.maximum(key, 1.0)).max()), "bound", (n + 3) * 2.0 ** -24,
          "zero keys", int((got == 0).sum()), "of", got.size, "exact zero", int((key == 0).sum()))
    assert not np.any((got == 0) & (key != 0))                # no flushed denormal
    assert np.all(err <= (n + 3) * 2.0 ** -24 * key), float((err / np.maximum(key, 1.0)).max())
    assert float(err.max()) > 0.0                             # it IS an approximation
    assert float(key.max()) > 2.0 ** 24


def test_bnb_leaf_pass(case, oracle, gpu_ctx):
    """The <124, 6> leaf pass of branch and bound (two exact rounds behind the bound pass) on the same map
    and scan, from two initial poses."""
    qs, cases = [], []
    for i, shift in enumerate([(0.0, 0.0, 0.0), (0.21, -0.13, 0.05)]):
        c = dict(case)
        c["init_pose"] = tuple(np.asarray(case["truth"]) + np.asarray(shift))
        cases.append(c)
        qs.append(dict(map_id=1500, geom=c["geom"], angles=c["angles"], ranges=c["ranges"],
                       rel_pose=c["rel_pose"], init_pose=c["init_pose"]))
    gpu_ctx.upload_grid(1500, case["grid"])
    rx, ry, rt, H, thr = 2.5, 2.5, 0.5, 2, (0.2, 0.5)
    gpu_ctx.bound_pass_stats()
    outs = gpu_ctx.bnb_match_batch(qs, rx, ry, rt, H, thr[0], thr[1])
    scored, skipped = gpu_ctx.bound_pass_stats()
    # the bound pass ran: only behind it does the exact kernel count its blocks (with two row blocks per
    # slice pair and a second round, it may well end up scoring every one of them)
    assert scored > 0, (scored, skipped)
    for c, o in zip(cases, outs):
        want = oracle.bnb(c, rx, ry, rt, H, thr[0], thr[1])
        raw = o["raw"]
        assert o["pose_found"] == want["found"] == 1, (raw, want)
        if raw["flags"] == 0:
            assert (raw["best_x"], raw["best_y"], raw["best_theta"]) == (want["bestX"], want["bestY"], want["bestT"])
            assert raw["score"] == want["scoreMax"]
        assert o["estimated_pose"] == want["estimatedPose"]
    gpu_ctx.release_grid(1500)
