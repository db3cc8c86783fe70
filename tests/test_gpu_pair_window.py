"""GPU parity of what the four pair-row scoring bodies share (PairWindow, flush_flags / flush_packed:
csm_score_common.hpp), on ONE small window that takes every body through the shared branches:

  3 theta slices          the last pair of slices holds one slice;
  12 x 84 candidates      L = 4: one block column, row blocks of 48 and 36 -- in the R = 8 launch the last
                          block has waves without a candidate inside the window, and the R = 6 tail launch
                          has a block that starts behind the last row and leaves at once;
  200 beams over 270 deg  on a 200 x 200 grid; record boxes start on odd and on even columns (checked
                          below on the host), so both column-parity shifts of the lane address occur.

Five runs: the batch chain by default (fp32 bound pass + exact list kernel), without the bound pass
(k_score_joint_batch), without joint lists (k_score_pairs2_batch), with one slice per workgroup
(k_score_pairs_batch), and the single-window dump path (k_score_pairs) with and without the lane table.
Every run's S and K of EVERY candidate equal the oracle's closed form; the fp32 keys of the default run
obey the bound pass's proven error |key32 - key| <= (n + 3) 2^-24 key. A second window of 4000 beams at
1.2 m on a saturated grid puts heavy entries at chunk ends of both gathers that flush."""
import math

import numpy as np
import pytest
import torch

from csm_hip import _lib as L, api, synth

pytestmark = pytest.mark.gpu

LR = 4
RX, RY, RT = 0.45, 4.05, math.radians(0.3)        # half ranges over the 5 cm step: windows of 5, 41, 1
NX, NY, NT = 12, 84, 3


def _make(case, oracle):
    res = case["geom"][0]
    sx, sy, st = api.host_search_step(res, case["ranges"])
    wx, wy, wt = api.host_window(RX, sx), api.host_window(RY, sy), api.host_window(RT, st)
    assert (wx, wy, wt) == (5, 41, 1)
    sensor = api.host_compound(case["init_pose"], case["rel_pose"])
    col, row = api.host_project(case["geom"], sensor, st, wt, case["angles"], case["ranges"])
    _, S, K, _ = oracle.csm_closed_form(case, RX, RY, RT, LR, dump=True)
    assert S.shape == K.shape == (NT, NX, NY)
    return dict(case=case, win=(wx, wy, wt), col=col, row=row, n=len(case["angles"]), S=S, K=K)


@pytest.fixture(scope="module")
def room(oracle):
    w = _make(synth.csm_case(31, rows=200, cols=200, n_beams=200, fov=1.5 * math.pi), oracle)
    # not an all-unknown window, and known counts that differ between candidates
    assert int(w["K"].max()) > w["n"] // 2 and int(w["K"].min()) < int(w["K"].max())
    assert int(w["S"].max()) > 0
    # Record boxes: k_bin / k_binj cut the frame (row + y_hi + shift, col + x_hi) into 64 x 64 tiles and a
    # record's window starts at its tile's least column; the parity of that column + x_lo is the shift.
    wx, wy, _ = w["win"]
    x_lo, y_lo = -wx, -wy
    x_hi, y_hi = x_lo + NX - 1, y_lo + NY - 1
    shift = (y_lo + y_hi) & 1
    for sl in ([0], [1], [2], [0, 1]):              # per-slice lists, and the joint list of the first pair
        cc = np.concatenate([w["col"][t] for t in sl]) + x_hi
        rr = np.concatenate([w["row"][t] for t in sl]) + y_hi + shift
        ok = (cc >= 0) & (rr >= 0)
        tile = (rr[ok] // 64) * 1024 + cc[ok] // 64
        starts = {int(cc[ok][tile == t].min()) - x_hi + x_lo for t in np.unique(tile)}
        assert {s & 1 for s in starts} == {0, 1}, sl
    return w


@pytest.fixture(scope="module")
def saturated(oracle):
    case = synth.csm_case(17, rows=200, cols=200, n_beams=4000, max_range=1.2)
    case["grid"] = np.full_like(case["grid"], 65535)
    w = _make(case, oracle)
    dup = np.unique(np.stack([w["col"][1], w["row"][1]]), axis=1, return_counts=True)[1]
    assert int(dup.max()) > 15                      # entries of the full multiplicity
    assert int(w["K"].max()) == w["n"] and int(w["S"].max()) == 65535 * w["n"]
    return w


def _batch(w, tuning_off, want_f32=False):
    """The window twice through csm_score_windows_dump_dev; returns the dumps of both copies."""
    dev = torch.device("cuda", 0)
    ctx = api.Context(0, tuning_off=tuning_off)
    try:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        ctx.upload_grid(1, w["case"]["grid"])
        ctx.build_pyramid(1, [1, LR])
        wx, wy, wt = w["win"]
        win = ctx.make_window(2 * wt + 1, w["n"], wx, wy, LR, 1, api.host_min_known(w["n"], 0.0), 0.0)
        c_d, r_d = torch.from_numpy(w["col"]).to(dev), torch.from_numpy(w["row"]).to(dev)
        nw, size = 2, NT * NX * NY
        out = torch.zeros(nw * 48, dtype=torch.uint8, device=dev)
        ds = [torch.zeros(size, dtype=torch.int32, device=dev) for _ in range(nw)]
        dk = [torch.zeros(size, dtype=torch.int16, device=dev) for _ in range(nw)]
        df = [torch.zeros(size, dtype=torch.float32, device=dev) for _ in range(nw)] if want_f32 else None
        prepared = ctx.prepare_windows([1] * nw, [win] * nw, [c_d.data_ptr()] * nw, [r_d.data_ptr()] * nw)
        ctx.bound_pass_stats()
        ctx.score_windows_dump_dev(prepared, out.data_ptr(), [t.data_ptr() for t in ds], [t.data_ptr() for t in dk],
                                   [t.data_ptr() for t in df] if want_f32 else None)
        torch.cuda.synchronize(dev)
        stats = ctx.bound_pass_stats()
    finally:
        ctx.close()
    S = [t.cpu().numpy().view(np.uint32).reshape(NT, NX, NY) for t in ds]
    K = [t.cpu().numpy().view(np.uint16).reshape(NT, NX, NY) for t in dk]
    F = [t.cpu().numpy().reshape(NT, NX, NY) for t in df] if want_f32 else None
    return S, K, F, stats


BATCH_RUNS = [("default", 0), ("no_bound_pass", L.TUNE_NO_BOUND_PASS), ("no_joint", L.TUNE_NO_JOINT),
              ("one_slice", L.TUNE_NO_JOINT | L.TUNE_NO_TWO_SLICES)]


@pytest.mark.parametrize("name,tuning_off", BATCH_RUNS, ids=[r[0] for r in BATCH_RUNS])
def test_batch_bodies_every_candidate(room, name, tuning_off):
    S, K, F, (scored, skipped) = _batch(room, tuning_off, want_f32=name == "default")
    for k in range(2):
        assert np.array_equal(S[k], room["S"]), (name, k)
        assert np.array_equal(K[k], room["K"]), (name, k)
    if name != "default":
        assert scored == skipped == 0               # no bound pass in these chains
        return
    # dumps ask for every block: the list kernel scored all of them after the fp32 pass
    assert scored > 0 and skipped == 0, (scored, skipped)
    key = 32268.0 * room["K"].astype(np.float64) + 499.0 * room["S"].astype(np.float64)
    for k in range(2):
        err = np.abs(F[k].astype(np.float64) - key)
        assert np.all(err <= (room["n"] + 3) * 2.0 ** -24 * key + 1e-9), (k, float(err.max()))
    assert float(np.abs(F[0].astype(np.float64) - key).max()) > 0.0      # it IS an approximation


@pytest.mark.parametrize("tuning_off", [0, L.TUNE_NO_LANE_MAP], ids=["lane_table", "threads_in_order"])
def test_single_window_body_every_candidate(room, tuning_off):
    ctx = api.Context(0, tuning_off=tuning_off)
    try:
        ctx.upload_grid(1, room["case"]["grid"])
        ctx.build_pyramid(1, [1, LR])
        wx, wy, wt = room["win"]
        win = ctx.make_window(2 * wt + 1, room["n"], wx, wy, LR, 1, api.host_min_known(room["n"], 0.0), 0.0)
        _, S, K, _ = ctx.score_window(1, win, room["col"], room["row"], dump=True)
    finally:
        ctx.close()
    assert np.array_equal(S, room["S"]) and np.array_equal(K, room["K"])


@pytest.mark.parametrize("name,tuning_off", BATCH_RUNS[1:3], ids=[r[0] for r in BATCH_RUNS[1:3]])
def test_flush_rule_heavy_entries_at_chunk_ends(saturated, name, tuning_off):
    """4000 beams at 1.2 m, every cell 65535: up to 70 beams per cell, entries of the full multiplicity.

    [no_bound_pass] is also the first test of the joint path above 3072 beams per scan: there k_binj's hash
    table has more than 8192 slots, and a signed shift of the slot product used to throw every cell whose
    product reached 2^31 out of the table (K = 3127 / 3139 / 3151 instead of 4000 for every candidate of
    slice 0 / 1 / 2, S = 65535 K; 3000 beams were exact)."""
    S, K, _, _ = _batch(saturated, tuning_off)
    for k in range(2):
        assert np.array_equal(K[k], saturated["K"]), (name, k)
        assert np.array_equal(S[k], saturated["S"]), (name, k)
